"""GPU tests of the pose graph's robust loss (slslam_solver_options.po_huber_delta: the reference's robustify ? new HuberLoss(0.001) : NULL,
src/po_problem.cpp:27,55) and of the per-edge report (slslam_po_edge_report, slslam_po_batch_get_edge_report), against the CPU reference of
tests/po_robust_reference.py (the oracle's LM loop, residual functor and Huber loss).  Needs a real MI355X.

Shapes: k_po_linearise packs 5 edges of 12 lanes per wave.  The two "corrupted" graphs have E = 26 (last wave: one edge) and E = 63 (last
wave: three); E = 1, 5, 10 are one lane group, one full wave, two full waves.  Tolerances against the reference are those of
tests/test_gpu_po.py against the oracle (cost 1e-8, radius 1e-5, final cost 1e-7, initial cost 1e-12, poses 1e-6), here held on EVERY
record of the trace; between two device paths those of tests/test_gpu_po.py and tests/test_gpu_po_batch.py (1e-9 on the poses).
A record whose reference cost lies below 1e-12 of the initial cost is rounding noise of a tree-shaped graph that can be met exactly
(its cost is ~1e-18): there, as in test_po_structured_factorisation_topologies, costs and the iteration a tolerance fires at are not
comparable and only the poses are."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_robust_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
REF_DELTA = 0.001                                    # the reference's HuberLoss(0.001)


# ---------------------------------------------------------------------------------------------- graphs
def _corrupt(g, e=None):
    """One loop constraint off by (1.5, 0, -1) m and 0.4 rad: the first loop edge unless an edge is named."""
    g = dict(g, constraints=np.array(g["constraints"], dtype=np.float64).copy())
    if e is None:
        e = int(np.nonzero(np.asarray(g["pose_index_2"]) - np.asarray(g["pose_index_1"]) > 1)[0][0])
    g["constraints"][e, 3:6] += (1.5, 0.0, -1.0)
    g["constraints"][e, 1] += 0.4
    return g, e


def _chain(seed, n):
    """A chain without loops, its free poses perturbed (a tree: every constraint can be met exactly)."""
    g = synth.make_pose_graph(seed, num_poses=n, num_loops=0)
    rng = np.random.default_rng(seed)
    return dict(g, parameters=g["parameters"] + rng.normal(0, 2e-3, g["parameters"].shape) * (np.arange(len(g["parameters"])) >= 6))


def _consistent():
    """Twelve poses on a line, no rotation, steps of 0.5 m, two loops; constraints from the poses.  Every operation of the functor is exact
    on these numbers (zero angle-axis vectors take the first-order branches, the translations are multiples of 0.5), so Te == 0 and
    s == 0 EXACTLY on every edge: sqrt(s) must not be divided by."""
    n = 12
    x = np.zeros((n, 6)); x[:, 3] = 0.5 * np.arange(n)
    pairs = sorted([(k, k + 1) for k in range(n - 1)] + [(2, 9), (1, 10)])
    cons = np.zeros((len(pairs), 6)); cons[:, 3] = [0.5 * (b - a) for a, b in pairs]
    return dict(num_poses=n, pose_index_1=np.array([p[0] for p in pairs], np.int32), pose_index_2=np.array([p[1] for p in pairs], np.int32),
                constraints=cons, parameters=x.reshape(-1))


def _one_edge(t):
    """Two poses at the origin, one edge whose constraint is a translation t along x: Te = (0, 0, 0, t, 0, 0) exactly, s = t * t."""
    cons = np.zeros((1, 6)); cons[0, 3] = t
    return dict(num_poses=2, pose_index_1=np.array([0], np.int32), pose_index_2=np.array([1], np.int32), constraints=cons, parameters=np.zeros(12))


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name in ("c24", "c60", "clean24", "clean60"):
        g = synth.make_pose_graph(7, *((24, 3) if name.endswith("24") else (60, 4)))
        return (g, -1) if name.startswith("clean") else _corrupt(g)
    if name == "gauge24":                            # the gauge edge itself (edge 0: pose1 is constant, only J2 enters)
        return _corrupt(synth.make_pose_graph(7, 24, 3), 0)
    if name == "e1":                                 # two poses, one edge, off by 0.5 m
        g = synth.make_pose_graph(27, num_poses=2, num_loops=0)
        g = dict(g, constraints=g["constraints"].copy()); g["constraints"][0, 3] += 0.5
        return g, 0
    if name == "e5":
        return _chain(31, 6), -1
    if name == "e10":
        return _chain(32, 11), -1
    if name == "consistent":
        return _consistent(), -1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name, delta):
    """The CPU reference's solve of a graph: computed once, shared, never modified."""
    x, s, t = ref.po_solve(_graph(name)[0], delta)
    x.setflags(write=False)
    return x, s, t


# ---------------------------------------------------------------------------------------------- comparisons
def _against_reference(label, got, want):
    (x1, s1, t1), (x0, s0, t0) = got, want
    floor = 1e-12 * s0["initial_cost"]
    noise = any(r["cost"] < floor for r in t0)
    print("%s: steps %d+%d / %d+%d, term %d / %d, cost %.12e -> %.12e / %.12e -> %.12e, max |dx| %.3e%s" % (
        label, s1["num_successful_steps"], s1["num_unsuccessful_steps"], s0["num_successful_steps"], s0["num_unsuccessful_steps"],
        s1["termination_type"], s0["termination_type"], s1["initial_cost"], s1["final_cost"], s0["initial_cost"], s0["final_cost"],
        np.abs(x1 - x0).max(), "  (reaches rounding noise)" if noise else ""))
    for a, b in zip(t0, t1):
        print("   it %2d valid %d/%d ok %d/%d cost rel %.2e radius rel %.2e" % (
            a["iteration"], a["step_is_valid"], b["step_is_valid"], a["step_is_successful"], b["step_is_successful"],
            abs(a["cost"] - b["cost"]) / max(abs(a["cost"]), 1e-300), abs(a["trust_region_radius"] - b["trust_region_radius"]) / a["trust_region_radius"]))
    assert abs(s0["initial_cost"] - s1["initial_cost"]) <= 1e-12 * s0["initial_cost"]
    assert s0["num_free_parameters"] == s1["num_free_parameters"] and s0["num_residual_blocks"] == s1["num_residual_blocks"]
    for a, b in zip(t0, t1):
        if a["cost"] < floor:
            break
        assert a["iteration"] == b["iteration"]
        assert a["step_is_valid"] == b["step_is_valid"] and a["step_is_successful"] == b["step_is_successful"], a["iteration"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * abs(a["cost"]) + 1e-18, a["iteration"]
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-5 * a["trust_region_radius"], a["iteration"]
    assert np.abs(x1 - x0).max() < 1e-6
    if noise:
        assert s1["final_cost"] < floor and s0["final_cost"] < floor
        return
    assert len(t0) == len(t1)
    for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type"):
        assert s0[k] == s1[k], k
    assert abs(s0["final_cost"] - s1["final_cost"]) <= 1e-7 * s0["final_cost"]


def _report_against_reference(label, g, x, delta, sq, w):
    """sq_norm and weight within 1e-10 relative of the reference at the same parameters - as far as fp64 knows sq_norm.  Te is a difference
    of quantities of the size of the poses (several metres here), so each of its components carries an absolute rounding error of a few
    eps max|x|, whatever its own size: d = 8 eps max(1, max|x|) ~ 1e-14, and s = |Te|^2 inherits 2 sqrt(s) d + d^2.  That term is
    below 1e-10 s for every edge with a real residual (s above 1e-8 .. 3e-7 on these graphs; 1e-14 of the false loop closure's s) and is what decides for the
    edges a solve meets to rounding noise: the free tail behind the last loop closure (s ~ 1e-18 .. 1e-20) and dead-reckoned odometry
    edges (s ~ 1e-31).  The reference does not know those to 1e-10 either: one ulp on its own inputs moves edges 24, 25 of the 24-pose
    graph by 7e-10 and 3e-8 relative, edges 60 .. 62 of the 60-pose graph by 5e-8 .. 1e-6; the device differs from it there by 3e-8 and
    1e-6, and by at most 2e-11 on every other edge.  The weights need no such term."""
    sq0, w0 = ref.edge_report(g, x, delta)
    d = 8 * np.finfo(float).eps * max(1.0, np.abs(x).max())
    rel = np.abs(sq - sq0) / np.maximum(sq0, 1e-300)
    real = sq0 * 1e-10 >= 2 * np.sqrt(sq0) * d
    print("%s: report vs reference: sq_norm rel %.2e over the %d edges with s > %.1e, worst |d sq_norm| / allowed %.3f, weight rel %.2e" % (
        label, rel[real].max(initial=0.0), int(real.sum()), (2e10 * d) ** 2,
        (np.abs(sq - sq0) / (1e-10 * sq0 + 2 * np.sqrt(sq0) * d + d * d)).max(), np.abs(w / w0 - 1).max()))
    assert (np.abs(sq - sq0) <= 1e-10 * sq0 + 2 * np.sqrt(sq0) * d + d * d).all()
    assert (np.abs(w - w0) <= 1e-10 * w0).all()


def _same_decisions(sa, sb, ta, tb):
    for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert len(ta) == len(tb)
    for a, b in zip(ta, tb):
        assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * abs(a["cost"]) + 1e-18
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-5 * a["trust_region_radius"]


def _batch(hip, graphs, **opt):
    b = hip.POBatch()
    for g in graphs:
        b.add(g)
    b.finalize(**opt)
    return b


def _results(b, n):
    return [(b.parameters(i), b.summary(i), b.trace(i), b.edge_report(i)) for i in range(n)]


# ---------------------------------------------------------------------------------------------- A. trace parity
@pytest.mark.parametrize("delta", [REF_DELTA, 0.05])
@pytest.mark.parametrize("name", ["c24", "c60"])
def test_trace_parity_with_reference(hip, name, delta):
    g, _ = _graph(name)
    _against_reference("%s delta %g" % (name, delta), hip.po_solve(g, po_huber_delta=delta), _reference(name, delta))


# ---------------------------------------------------------------------------------------------- B. every factor path
def test_every_factor_path(hip):
    g, _ = _graph("c24")
    want = _reference("c24", REF_DELTA)
    xs, ss, ts = hip.po_solve(g, po_huber_delta=REF_DELTA)
    xd, sd, td = hip.po_solve(g, po_huber_delta=REF_DELTA, po_dense_factor=1)
    _against_reference("structured", (xs, ss, ts), want)
    _against_reference("dense", (xd, sd, td), want)
    print("structured vs dense: max |dx| %.3e" % np.abs(xs - xd).max())
    assert np.abs(xs - xd).max() < 1e-9                                  # same system, different elimination order
    # only the factor is single precision: the stated tolerance of test_po_fp32_factorisation_tolerance
    x32, s32, _ = hip.po_solve(g, po_huber_delta=REF_DELTA, po_factor_fp32=1)
    print("fp32 factor: cost %.9e vs %.9e, max |dx| %.3e, steps %d vs %d" % (s32["final_cost"], ss["final_cost"], np.abs(x32 - xs).max(),
                                                                                s32["num_successful_steps"], ss["num_successful_steps"]))
    assert s32["termination_type"] in (0, 2, 3) and s32["num_successful_steps"] >= 1
    assert abs(s32["initial_cost"] - ss["initial_cost"]) <= 1e-13 * ss["initial_cost"]
    assert abs(s32["final_cost"] - ss["final_cost"]) <= 1e-4 * ss["final_cost"]
    assert np.abs(x32 - xs).max() < 1e-4
    # the batched path
    (xb, sb, tb), = hip.po_solve_batch([g], po_huber_delta=REF_DELTA)
    _against_reference("batch", (xb, sb, tb), want)
    _same_decisions(ss, sb, ts, tb)
    assert np.abs(xb - xs).max() < 1e-9


# ---------------------------------------------------------------------------------------------- C. boundaries
@pytest.mark.parametrize("name", ["e1", "e5", "e10", "gauge24"])
def test_small_shapes_and_gauge_edge(hip, name):
    """E = 1 (s > a^2 on the only edge), one and two full waves, and the corrupted gauge edge, whose pose1 is constant: only J2 enters
    the system but the corrector still applies."""
    g, bad = _graph(name)
    x0 = np.asarray(g["parameters"], np.float64).reshape(-1)
    sq0, w0 = ref.edge_report(g, x0, REF_DELTA)
    assert (w0 < 1).all() if name != "gauge24" else w0[bad] < 1e-3       # the loss is active where the case says so
    _report_against_reference(name + " at the start", g, x0, REF_DELTA, *hip.po_edge_report(g, None, REF_DELTA))
    got = hip.po_solve(g, po_huber_delta=REF_DELTA)
    _against_reference(name, got, _reference(name, REF_DELTA))
    assert np.array_equal(got[0][:6], x0[:6])                            # pose1 of edge 0 stays put
    if name == "gauge24":                                                # (a tree's solution is rounding noise on every edge)
        _report_against_reference(name, g, got[0], REF_DELTA, *hip.po_edge_report(g, got[0], REF_DELTA))


def test_consistent_graph_has_zero_cost_and_no_division(hip):
    g, _ = _graph("consistent")
    x0, s0, t0 = hip.po_solve(g)
    x1, s1, t1 = hip.po_solve(g, po_huber_delta=REF_DELTA)
    print("consistent: cost %r / %r, term %d / %d, steps %d+%d / %d+%d" % (s1["initial_cost"], s0["initial_cost"], s1["termination_type"], s0["termination_type"],
          s1["num_successful_steps"], s1["num_unsuccessful_steps"], s0["num_successful_steps"], s0["num_unsuccessful_steps"]))
    assert s1["initial_cost"] == 0.0 and s1["final_cost"] == 0.0 and np.isfinite(x1).all()
    for k in ("termination_type", "num_successful_steps", "num_unsuccessful_steps"):
        assert s0[k] == s1[k], k
    assert len(t0) == len(t1) and x1.tobytes() == np.asarray(g["parameters"], np.float64).tobytes()
    sq, w = hip.po_edge_report(g, x1, REF_DELTA)
    assert (sq == 0.0).all() and (w == 1.0).all()
    # constraints from the true poses of a curved loop: s ~ 1e-30, every edge an inlier
    gl = synth.make_pose_graph(4, num_poses=30, num_loops=2)
    truth = gl["true_parameters"].reshape(-1, 6)
    cons = []
    for a, b in zip(gl["pose_index_1"], gl["pose_index_2"]):
        Ra, ta = synth.wt_to_rt(truth[a]); Rb, tb = synth.wt_to_rt(truth[b])
        cons.append(synth.rt_to_wt(Rb @ Ra.T, tb - (Rb @ Ra.T) @ ta))
    gl = dict(gl, constraints=np.array(cons), parameters=gl["true_parameters"])
    x, s, _ = hip.po_solve(gl, po_huber_delta=REF_DELTA)
    sq, w = hip.po_edge_report(gl, x, REF_DELTA)
    assert s["initial_cost"] < 1e-25 and np.abs(x - gl["true_parameters"]).max() < 1e-12 and sq.max() < 1e-25 and (w == 1.0).all()


def test_threshold_between_inlier_and_outlier(hip):
    """s just below and just above a^2, with a = 0.5 and t = a (1 -+ 2^-30): s = t * t is exact to the last bit on both sides."""
    a = 0.5
    for t, inlier in ((a * (1 - 2.0 ** -30), True), (a * (1 + 2.0 ** -30), False)):
        g = _one_edge(t)
        s = t * t
        assert (s < a * a) == inlier and s != a * a
        sq, w = hip.po_edge_report(g, None, a)
        sq0, w0 = ref.edge_report(g, g["parameters"], a)
        assert abs(sq[0] - s) <= 1e-15 * s and abs(sq0[0] - s) <= 1e-15 * s and (sq[0] < a * a) == inlier
        _, summ, _ = hip.po_solve(g, po_huber_delta=a, max_num_iterations=0)
        want_cost = 0.5 * s if inlier else 0.5 * (2 * a * np.sqrt(s) - a * a)
        print("t = a %s 2^-30: weight %.17g (reference %.17g), cost %.17g (expected %.17g)" % ("-" if inlier else "+", w[0], w0[0], summ["initial_cost"], want_cost))
        assert (w[0] == 1.0) if inlier else (w[0] < 1.0 and abs(w[0] - a / np.sqrt(s)) <= 1e-15)
        assert abs(w[0] - w0[0]) <= 1e-10
        assert abs(summ["initial_cost"] - want_cost) <= 1e-12 * want_cost
        _against_reference("threshold", hip.po_solve(g, po_huber_delta=a), ref.po_solve(g, a))


# ---------------------------------------------------------------------------------------------- D. off means off
def test_off_means_off(hip):
    """po_huber_delta = 0 is the code as it was: the LBA loss's huber_delta stays ignored, bit for bit.  (E = 5: one wave, so the order
    of the fp64 atomic sums - the only thing that can differ between two runs of a larger graph - is fixed.)"""
    g, _ = _graph("e5")
    xa, sa, ta = hip.po_solve(g, po_huber_delta=0.0, huber_delta=1.0 / 406.05)
    xb, sb, tb = hip.po_solve(g, po_huber_delta=0.0, huber_delta=0.0)
    xc, sc, tc = hip.po_solve(g)
    assert xa.tobytes() == xb.tobytes() == xc.tobytes() and sa == sb == sc and ta == tb == tc
    # a loss no edge reaches: every block is an inlier, the decisions are those without a loss
    for name in ("c24", "e10"):
        g, _ = _graph(name)
        x0, s0, t0 = hip.po_solve(g)
        x1, s1, t1 = hip.po_solve(g, po_huber_delta=1e6)
        print("%s, delta 1e6 vs 0: max |dx| %.3e" % (name, np.abs(x0 - x1).max()))
        if name == "c24":
            _same_decisions(s0, s1, t0, t1)
        assert np.abs(x0 - x1).max() < 1e-9
        assert (hip.po_edge_report(g, x1, 1e6)[1] == 1.0).all()


# ---------------------------------------------------------------------------------------------- E. edge report
@pytest.mark.parametrize("name", ["c24", "c60"])
def test_edge_report(hip, name):
    g, bad = _graph(name)
    x, _, _ = hip.po_solve(g, po_huber_delta=REF_DELTA)
    sq, w = hip.po_edge_report(g, x, REF_DELTA)
    _report_against_reference(name, g, x, REF_DELTA, sq, w)
    print("%s: bad edge %d weight %.4e, smallest other %.4e (ratio %.4f)" % (name, bad, w[bad], np.delete(w, bad).min(), w[bad] / np.delete(w, bad).min()))
    assert int(np.argmin(w)) == bad and w[bad] < 0.1 * np.delete(w, bad).min()
    # without a loss every weight is 1 and the norms are the same
    sqn, wn = hip.po_edge_report(g, x, 0.0)
    assert sqn.tobytes() == sq.tobytes() and (wn == 1.0).all()
    # either output may be NULL
    L = hip.lib()
    i1, i2, cons, xx = hip._po_arrays(g, x)
    cg = hip.POGraph(int(g["num_poses"]), len(i1), hip._ip(i1), hip._ip(i2), hip._dp(cons), hip._dp(xx))
    only_sq, only_w = np.zeros(len(i1)), np.zeros(len(i1))
    assert L.slslam_po_edge_report(C.byref(cg), REF_DELTA, hip._dp(only_sq), None) == 0
    assert L.slslam_po_edge_report(C.byref(cg), REF_DELTA, None, hip._dp(only_w)) == 0
    assert L.slslam_po_edge_report(C.byref(cg), REF_DELTA, None, None) == 0
    assert only_sq.tobytes() == sq.tobytes() and only_w.tobytes() == w.tobytes()
    # the batch getter is the one-shot call at the batch's parameters and delta
    b = _batch(hip, [g], po_huber_delta=REF_DELTA)
    try:
        b.solve(); b.download()
        xb = b.parameters(0)
        sqb, wb = b.edge_report(0)
        sq1, w1 = hip.po_edge_report(g, xb, REF_DELTA)
        assert sqb.tobytes() == sq1.tobytes() and wb.tobytes() == w1.tobytes()
        assert L.slslam_po_batch_get_edge_report(b._h, 0, None, hip._dp(only_w)) == 0 and only_w.tobytes() == wb.tobytes()
        assert L.slslam_po_batch_get_edge_report(b._h, 0, None, None) == 0
        b.reset()
        with pytest.raises(hip.SlslamError) as ei:                       # as slslam_po_batch_get_parameters: no results after a reset
            b.edge_report(0)
        assert ei.value.status == 5
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- F. it does what it is for
@pytest.mark.parametrize("name", ["24", "60"])
def test_robust_solve_survives_a_false_loop_closure(hip, name):
    clean, _ = _graph("clean" + name)
    g, _ = _graph("c" + name)
    xc = hip.po_solve(clean)[0].reshape(-1, 6)
    worst = {}
    for delta in (0.0, REF_DELTA):
        x = hip.po_solve(g, po_huber_delta=delta)[0].reshape(-1, 6)
        worst[delta] = np.linalg.norm(x[:, 3:] - xc[:, 3:], axis=1).max()
    print("%s poses: worst translation distance from the clean solution %.4f m plain, %.4f m robust" % (name, worst[0.0], worst[REF_DELTA]))
    assert worst[REF_DELTA] < 0.1 * worst[0.0]


# ---------------------------------------------------------------------------------------------- G. batch
def test_batch_mixed_set(hip):
    names = ["c24", "c60", "consistent", "e1"]
    graphs = [_graph(n)[0] for n in names]
    b = _batch(hip, graphs, po_huber_delta=REF_DELTA)
    alone = _batch(hip, graphs[:1], po_huber_delta=REF_DELTA)
    try:
        b.solve(); b.download()
        first = _results(b, len(graphs))
        for n, g, (x, s, t, (sq, w)) in zip(names, graphs, first):
            x1, s1, t1 = hip.po_solve(g, po_huber_delta=REF_DELTA)       # the criterion of tests/test_gpu_po_batch.py::_against_oneshot
            print("%s vs one-shot: %d+%d steps, max |dx| %.3e" % (n, s["num_successful_steps"], s["num_unsuccessful_steps"], np.abs(x - x1).max()))
            if n != "e1":                                                # (a tree that reaches rounding noise: the poses alone)
                _same_decisions(s1, s, t1, t)
            assert np.abs(x - x1).max() < 1e-9, n
            sq1, w1 = hip.po_edge_report(g, x, REF_DELTA)
            assert sq.tobytes() == sq1.tobytes() and w.tobytes() == w1.tobytes(), n
        assert (first[2][3][1] == 1.0).all() and (first[2][3][0] == 0.0).all() and first[2][1]["final_cost"] == 0.0
        # a graph's result does not depend on its company
        alone.solve(); alone.download()
        (xa, sa, ta, _), = _results(alone, 1)
        _same_decisions(sa, first[0][1], ta, first[0][2])
        assert np.abs(xa - first[0][0]).max() < 1e-9
        # reset + solve reproduces the first result
        b.reset(); b.solve(); b.download()
        for n, (x, s, t, (sq, w)), (x2, s2, t2, (sq2, w2)) in zip(names, first, _results(b, len(graphs))):
            for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type"):
                assert s[k] == s2[k] or n == "e1", (n, k)
            assert np.abs(x - x2).max() < 1e-9 and np.abs(w - w2).max() < 1e-9, n
    finally:
        b.close()
        alone.close()

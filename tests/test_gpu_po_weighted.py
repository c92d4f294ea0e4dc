"""GPU tests of the pose graph's per-edge square-root information matrices (slslam_po_graph.sqrt_information: blocks whitened by W_e before
the loss) in slslam_po_solve, slslam_po_edge_report, slslam_po_covariance and the batch, against the CPU reference of
tests/po_weighted_reference.py (the oracle's LM loop, residual functor and Huber loss; the numpy covariance).  Needs a real MI355X.

Graphs: those of tests/test_gpu_po_robust.py (k_po_linearise packs 5 edges of 12 lanes per wave: E = 1, 5, 10 are one lane group, one and
two full waves; E = 26 and 63 end in a wave of one and of three edges) and e6, a 7-pose chain whose second wave holds one edge.  Weights:
synth.make_edge_information - W_e = R_e diag(s_e) T_e, full, NOT symmetric, O(1): a transposed or column-major read is another problem
(tests/test_po_weighted_cpu.py holds the reference to that), the conditioning is that of the unweighted graphs.
Tolerances against the reference are exactly those tests/test_gpu_po_robust.py holds against its reference, on EVERY record of the trace
(cost 1e-8, radius 1e-5, final cost 1e-7, initial cost 1e-12, poses 1e-6, and its rounding-noise floor for trees); between two device
paths 1e-9 on the poses."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402
import po_weighted_reference as wref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 0.05
K = 100.0                                            # tests/test_gpu_po_covariance.py's factor on the reference's yardstick y
COV_OK = 0
SMALL_W = 0.01                                       # test I: the false loop closure's W = SMALL_W * I


@functools.lru_cache(maxsize=None)
def _graph(name):
    return wref.weighted(name)


@functools.lru_cache(maxsize=None)
def _reference(name, delta):
    """The CPU reference's solve of a weighted graph: computed once, shared, never modified."""
    x, s, t = wref.po_solve(_graph(name)[0], delta)
    x.setflags(write=False)
    return x, s, t


# ---------------------------------------------------------------------------------------------- comparisons (tests/test_gpu_po_robust.py's)
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
    """tests/test_gpu_po_robust.py's allowance - 1e-10 relative plus what the absolute rounding error d = 8 eps max(1, max |x|) of every
    component of Te does to s - with d multiplied by max_e ||W_e||_inf: a component of W_e Te is a sum of six components of Te times
    entries of W_e, so it carries at most ||W_e||_inf d."""
    sq0, w0 = wref.edge_report(g, x, delta)
    d = 8 * np.finfo(float).eps * max(1.0, np.abs(x).max()) * np.abs(g["sqrt_information"]).sum(axis=2).max()
    allowed = 1e-10 * sq0 + 2 * np.sqrt(sq0) * d + d * d
    print("%s: report vs reference: worst |d sq_norm| / allowed %.3f, weight rel %.2e, d %.2e" % (
        label, (np.abs(sq - sq0) / allowed).max(), np.abs(w / w0 - 1).max(), d))
    assert (np.abs(sq - sq0) <= allowed).all()
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


def _unweighted(g):
    return {k: v for k, v in g.items() if k != "sqrt_information"}


# ---------------------------------------------------------------------------------------------- A. trace parity
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("name", ["c24", "c60"])
def test_trace_parity_with_reference(hip, name, delta):
    g, _ = _graph(name)
    _against_reference("%s delta %g" % (name, delta), hip.po_solve(g, po_huber_delta=delta), _reference(name, delta))


# ---------------------------------------------------------------------------------------------- B. boundaries
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("name", ["e1", "e5", "e6", "e10", "gauge24"])
def test_small_shapes_and_gauge_edge(hip, name, delta):
    """One lane group, one full wave, a second wave of one edge, two full waves, and the weighted gauge edge (pose1 constant: only W J2
    enters the system, W Te still enters the cost)."""
    g, _ = _graph(name)
    x0 = np.asarray(g["parameters"], np.float64).reshape(-1)
    got = hip.po_solve(g, po_huber_delta=delta)
    _against_reference("%s delta %g" % (name, delta), got, _reference(name, delta))
    assert np.array_equal(got[0][:6], x0[:6])                            # pose1 of edge 0 stays put
    _report_against_reference(name + " at the start", g, x0, delta, *hip.po_edge_report(g, None, delta))


# ---------------------------------------------------------------------------------------------- C. off means off
def test_off_means_off(hip):
    """No weights is the code as it was, however "no weights" is said (E = 5: one wave, so the order of the fp64 atomic sums is fixed)."""
    g = _unweighted(_graph("e5")[0])
    assert "sqrt_information" not in g
    xa, sa, ta = hip.po_solve(g)
    xb, sb, tb = hip.po_solve(dict(g, sqrt_information=None))
    assert xa.tobytes() == xb.tobytes() and sa == sb and ta == tb
    i1, i2, cons, xx = hip._po_arrays(g)
    cg = hip.POGraph(int(g["num_poses"]), len(i1), hip._ip(i1), hip._ip(i2), hip._dp(cons), hip._dp(xx))     # six positional arguments
    assert not cg.sqrt_information
    o, s, tr, n = hip.default_options(), hip.Summary(), (hip.Iteration * 64)(), C.c_int(0)
    assert hip.lib().slslam_po_solve(C.byref(cg), C.byref(o), C.byref(s), tr, 64, C.byref(n)) == 0
    assert xx.tobytes() == xa.tobytes() and hip._summary_dict(s) == sa and hip._trace_list(tr, n.value) == ta
    # identity matrices take the whitening kernels and give the same solve
    g, _ = _graph("c24")
    g0 = _unweighted(g)
    x0, s0, t0 = hip.po_solve(g0)
    x1, s1, t1 = hip.po_solve(dict(g0, sqrt_information=np.tile(np.eye(6), (len(g0["pose_index_1"]), 1, 1))))
    print("c24, identity matrices vs NULL: max |dx| %.3e" % np.abs(x0 - x1).max())
    _same_decisions(s0, s1, t0, t1)
    assert np.abs(x0 - x1).max() < 1e-9


# ---------------------------------------------------------------------------------------------- D. scale
def test_twice_the_identity_is_four_times_the_cost(hip):
    g = _unweighted(_graph("c24")[0])
    g2 = dict(g, sqrt_information=np.tile(2.0 * np.eye(6), (len(g["pose_index_1"]), 1, 1)))
    _, s1, _ = hip.po_solve(g, max_num_iterations=0)
    _, s2, _ = hip.po_solve(g2, max_num_iterations=0)
    sq1, _ = hip.po_edge_report(g)
    sq2, _ = hip.po_edge_report(g2)
    print("initial cost %.17g / %.17g = %.17g; sq_norm ratio - 4: %.2e" % (s2["initial_cost"], s1["initial_cost"], s2["initial_cost"] / s1["initial_cost"],
                                                                          np.abs(sq2 / sq1 - 4.0).max()))
    assert abs(s2["initial_cost"] - 4.0 * s1["initial_cost"]) <= 1e-14 * 4.0 * s1["initial_cost"]
    assert (np.abs(sq2 - 4.0 * sq1) <= 1e-14 * 4.0 * sq1).all()


# ---------------------------------------------------------------------------------------------- E. edge report
def test_edge_report(hip):
    g, _ = _graph("c24")
    x, _, _ = hip.po_solve(g, po_huber_delta=DELTA)
    sq, w = hip.po_edge_report(g, x, DELTA)
    _report_against_reference("c24", g, x, DELTA, sq, w)
    assert (w < 1.0).any() and (w == 1.0).any()                          # the loss is active on some edges and not on others
    sq_plain, _ = hip.po_edge_report(_unweighted(g), x, DELTA)
    assert np.abs(sq / sq_plain - 1).max() > 0.1                         # |W_e Te|^2 is not |Te|^2
    # either output may be NULL
    L = hip.lib()
    cg, keep = hip._po_graph(g, x)
    E = len(keep[0])
    only_sq, only_w = np.zeros(E), np.zeros(E)
    assert L.slslam_po_edge_report(C.byref(cg), DELTA, hip._dp(only_sq), None) == 0
    assert L.slslam_po_edge_report(C.byref(cg), DELTA, None, hip._dp(only_w)) == 0
    assert L.slslam_po_edge_report(C.byref(cg), DELTA, None, None) == 0
    assert only_sq.tobytes() == sq.tobytes() and only_w.tobytes() == w.tobytes()
    # the batch getter is the one-shot call at the batch's parameters and delta
    b = _batch(hip, [g], po_huber_delta=DELTA)
    try:
        b.solve(); b.download()
        xb = b.parameters(0)
        sqb, wb = b.edge_report(0)
        sq1, w1 = hip.po_edge_report(g, xb, DELTA)
        assert sqb.tobytes() == sq1.tobytes() and wb.tobytes() == w1.tobytes()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- F. every factor path
def test_every_factor_path(hip):
    g, _ = _graph("c24")
    want = _reference("c24", DELTA)
    xs, ss, ts = hip.po_solve(g, po_huber_delta=DELTA)
    xd, sd, td = hip.po_solve(g, po_huber_delta=DELTA, po_dense_factor=1)
    _against_reference("structured", (xs, ss, ts), want)
    _against_reference("dense", (xd, sd, td), want)
    print("structured vs dense: max |dx| %.3e" % np.abs(xs - xd).max())
    assert np.abs(xs - xd).max() < 1e-9
    x32, s32, _ = hip.po_solve(g, po_huber_delta=DELTA, po_factor_fp32=1)
    print("fp32 factor: cost %.9e vs %.9e, max |dx| %.3e, steps %d vs %d" % (s32["final_cost"], ss["final_cost"], np.abs(x32 - xs).max(),
                                                                                s32["num_successful_steps"], ss["num_successful_steps"]))
    assert s32["termination_type"] in (0, 2, 3) and s32["num_successful_steps"] >= 1
    assert abs(s32["initial_cost"] - ss["initial_cost"]) <= 1e-13 * ss["initial_cost"]
    assert abs(s32["final_cost"] - ss["final_cost"]) <= 1e-4 * ss["final_cost"]
    assert np.abs(x32 - xs).max() < 1e-4
    (xb, sb, tb), = hip.po_solve_batch([g], po_huber_delta=DELTA)
    _against_reference("batch", (xb, sb, tb), want)
    _same_decisions(ss, sb, ts, tb)
    assert np.abs(xb - xs).max() < 1e-9


# ---------------------------------------------------------------------------------------------- G. covariance
def test_covariance(hip):
    """H = J^T J of the whitened J: one-shot and batch against the weighted numpy covariance, within K * y of
    tests/test_gpu_po_covariance.py; and further than that from the unweighted covariance."""
    g, _ = _graph("c24")
    x = _reference("c24", 0.0)[0]
    N = int(g["num_poses"])
    pairs = [(int(a), int(b)) for a, b in zip(g["pose_index_1"], g["pose_index_2"]) if b - a > 1] + [(1, N - 1), (2, 2), (0, N - 1)]
    ref = wref.covariance(g, x, 0.0)
    cp0, cq0 = cref.blocks(ref, N, pairs)
    top = np.abs(ref["sigma"]).max()

    def deviation(label, got):
        nonlocal ref, cp0, cq0, top
        st, cp, cq = got
        d = max(np.abs(cp - cp0).max(), np.abs(cq - cq0).max()) / top
        print("%s: n %d pivot %.3e  y %.3e  d %.3e  d / y %.3f" % (label, ref["n"], ref["pivot"], ref["y"], d, d / ref["y"]))
        assert st == COV_OK
        return d

    assert deviation("one-shot", hip.po_covariance(g, pairs, 0.0, params=x)) <= K * ref["y"]
    plain = hip.po_covariance(_unweighted(g), pairs, 0.0, params=x)
    assert deviation("the unweighted covariance", plain) > K * ref["y"]
    b = _batch(hip, [g, _unweighted(g)])
    try:
        b.set_covariance_pairs(0, pairs); b.set_covariance_pairs(1, pairs)
        b.solve(); b.covariance(); b.download()                          # at the poses the batch's own solve reached
        xb = b.parameters(0)
        ref = wref.covariance(g, xb, 0.0)
        cp0, cq0 = cref.blocks(ref, N, pairs)
        top = np.abs(ref["sigma"]).max()
        assert deviation("batch", b.get_covariance(0)) <= K * ref["y"]
        st1, cp1, cq1 = b.get_covariance(1)                              # its unweighted neighbour is not whitened
        _, cp2, cq2 = hip.po_covariance(_unweighted(g), pairs, 0.0, params=b.parameters(1))
        assert st1 == COV_OK and max(np.abs(cp1 - cp2).max(), np.abs(cq1 - cq2).max()) <= K * ref["y"] * np.abs(cp2).max()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- H. mixed batch
def test_mixed_batch(hip):
    graphs = [_graph("c24")[0], _unweighted(_graph("c24")[0]), _graph("e1")[0], _unweighted(_graph("c60")[0])]
    names = ["c24 weighted", "c24", "e1 weighted", "c60"]
    b = _batch(hip, graphs, po_huber_delta=DELTA)
    alone = _batch(hip, graphs[:1], po_huber_delta=DELTA)
    try:
        b.solve(); b.download()
        alone.solve(); alone.download()
        for i, (n, g) in enumerate(zip(names, graphs)):
            x, s, t = b.parameters(i), b.summary(i), b.trace(i)
            x1, s1, t1 = hip.po_solve(g, po_huber_delta=DELTA)
            print("%s vs one-shot: %d+%d steps, max |dx| %.3e" % (n, s["num_successful_steps"], s["num_unsuccessful_steps"], np.abs(x - x1).max()))
            if not n.startswith("e1"):                                   # (a tree that reaches rounding noise: the poses alone)
                _same_decisions(s1, s, t1, t)
            assert np.abs(x - x1).max() < 1e-9, n
            sq, w = b.edge_report(i)
            sq1, w1 = hip.po_edge_report(g, x, DELTA)
            assert sq.tobytes() == sq1.tobytes() and w.tobytes() == w1.tobytes(), n
        _same_decisions(alone.summary(0), b.summary(0), alone.trace(0), b.trace(0))
        assert np.abs(alone.parameters(0) - b.parameters(0)).max() < 1e-9
        assert np.abs(b.parameters(0) - b.parameters(1)).max() > 1e-6    # the weights were used, and only where given
    finally:
        b.close()
        alone.close()


# ---------------------------------------------------------------------------------------------- I. what the feature is for
@pytest.mark.parametrize("name", ["24", "60"])
def test_a_small_weight_discounts_a_false_loop_closure(hip, name):
    """No loss; the false loop closure gets W = 0.01 I, every other edge the identity.  The worst translation distance from the clean
    solution falls below 0.1 of the unweighted solve's.  The CPU reference alone gives ratios 0.028 (24 poses, 2.59 m unweighted) and
    0.018 (60 poses, 1.46 m) - and 0.087 / 0.047 at W = 0.1 I, 0.027 / 0.017 at 0.03 I.  The ratio does not go to zero with w: its floor
    is the distance between the clean solution and the solution with the edge REMOVED (W = 0: 0.0284 / 0.0181 - the clean graph has a
    correct constraint there, the discounted one has none), which 0.01 I has reached; in between, the remnant of the false pull happens to
    offset a little of that distance, hence 0.027 at 0.03 I."""
    clean, _ = wref.graph("clean" + name)
    g, bad = wref.graph("c" + name)
    W = np.tile(np.eye(6), (len(g["pose_index_1"]), 1, 1))
    W[bad] *= SMALL_W
    xc = hip.po_solve(clean)[0].reshape(-1, 6)
    xp = hip.po_solve(g)[0].reshape(-1, 6)
    xw = hip.po_solve(dict(g, sqrt_information=W))[0].reshape(-1, 6)
    worst_plain = np.linalg.norm(xp[:, 3:] - xc[:, 3:], axis=1).max()
    worst_weighted = np.linalg.norm(xw[:, 3:] - xc[:, 3:], axis=1).max()
    print("%s poses: worst translation distance from the clean solution %.4f m unweighted, %.4f m with the edge at %g I (ratio %.4f)" % (
        name, worst_plain, worst_weighted, SMALL_W, worst_weighted / worst_plain))
    assert worst_weighted < 0.1 * worst_plain


# ---------------------------------------------------------------------------------------------- J. the C++ mirror
def test_cxx_mirror_solves_with_the_weights(hip, tmp_path):
    """POProblem::set_sqrt_information + ceres::Solve (tests/host_cxx/po_weighted_mirror.cpp) give what capi.po_solve gives."""
    host, libdir = os.path.join(ROOT, "slslam_amd", "host"), os.path.join(ROOT, "slslam_amd", "_lib")
    subprocess.check_call(["make", "-s", "-C", host])
    exe = os.path.join(ROOT, "tests", "_build", "po_weighted_mirror")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "host_cxx", "po_weighted_mirror.cpp"),
                           "-L", libdir, "-lslslam_host", "-lslslam_hip", "-Wl,-rpath," + libdir])
    g, _ = _graph("c24")
    E = len(g["pose_index_1"])
    for weighted in (1, 0):
        path = tmp_path / ("graph%d.txt" % weighted)
        rows = ["%d %d %d" % (int(g["num_poses"]), E, weighted)] + ["%d %d" % (a, b) for a, b in zip(g["pose_index_1"], g["pose_index_2"])]
        vals = [np.asarray(g["constraints"]).reshape(-1), np.asarray(g["parameters"]).reshape(-1)] + ([g["sqrt_information"].reshape(-1)] if weighted else [])
        rows += ["%.17g" % v for a in vals for v in a]
        path.write_text("\n".join(rows) + "\n")
        p = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        x = np.array([float(v) for v in p.stdout.split()])
        x1, _, _ = hip.po_solve(g if weighted else _unweighted(g), max_num_iterations=10)
        print("C++ mirror, weighted %d: max |dx| against capi.po_solve %.3e" % (weighted, np.abs(x - x1).max()))
        assert x.shape == x1.shape and np.abs(x - x1).max() < 1e-9

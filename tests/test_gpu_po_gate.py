"""Edge statistics under posterior covariances on the device (include/slslam_hip.h: slslam_po_edge_statistics, slslam_po_gate,
slslam_po_batch_gate / _get_gate; capi.lba_odometry_edges; POProblem::gate) against the numpy reference of tests/po_gate_reference.py.
Needs a real MI355X.

Every deviation d (relative to the quantity's top, tests/po_gate_reference.py) is held to K * y with y the reference's own yardstick
and K = 100, the bound of tests/test_gpu_po_covariance.py.  Each comparison prints d / y per quantity; the worst measured on the
MI355X are listed in profiles/po_gate_bench.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402
import po_gate_reference as gref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 100.0
REF_DELTA = 0.001
COV_OK, COV_SINGULAR = 0, 1
INVALID = 1
CHI2_6_95, CHI2_6_99 = 12.6, 16.8
GRAPHS = [(4, 1), (12, 2), (24, 3)]


@functools.lru_cache(maxsize=None)
def _solved(shape):
    """(graph, the oracle's solved poses, its summary): computed once, shared, never modified."""
    from oracle import pyoracle
    g = synth.make_pose_graph(7, *shape)
    x, s, _ = pyoracle.po_solve(g, linear_solver=2)
    x.setflags(write=False)
    return g, x, s


def _item(got, k):
    return {q: got[q][k] for q in gref.QUANTITIES}


def _hold(label, got, refs):
    """Device results (dict of arrays) against one reference per item: statuses equal, singular items zero but for the error, the
    others within K * y per quantity.  Returns the worst d / y per quantity."""
    worst = dict.fromkeys(gref.QUANTITIES, 0.0)
    for k, ref in enumerate(refs):
        assert got["status"][k] == ref["status"], (label, k)
        if ref["status"] != COV_OK:
            assert not got["cov"][k].any() and not got["sqrt_information"][k].any() and got["mahalanobis2"][k] == 0.0, (label, k)
            assert np.abs(got["error"][k] - ref["error"]).max() <= K * np.finfo(np.float64).eps * max(1.0, np.abs(ref["error"]).max()), (label, k)
            continue
        assert ref["pivot"] >= 1e3 * gref.PIVOT_MIN, (label, k, ref["pivot"])      # well conditioned, as tests/test_po_gate_cpu.py holds its cases
        for q, r in gref.deviations(ref, _item(got, k)).items():
            worst[q] = max(worst[q], r)
    print("%s: worst d / y  " % label + "  ".join("%s %.3f" % (q, worst[q]) for q in gref.QUANTITIES))
    for q in gref.QUANTITIES:
        assert worst[q] <= K, (label, q)
    return worst


# ---------------------------------------------------------------------------------------------- the primitive
@pytest.mark.parametrize("n", [1, 5, 6, 65])
def test_primitive_matches_reference(hip, n):
    items = gref.primitive_items(n)
    arrays = {k: items[k] for k in ("cov_aa", "cov_bb", "cov_ab", "cov_meas")}
    got = hip.po_edge_statistics(items["pose_a"], items["pose_b"], items["constraints"], sigma2=items["sigma2"], **arrays)
    refs = gref.primitive_reference(items)
    _hold("primitive n %d" % n, got, refs)
    assert [int(s) for s in got["status"]] == [int(s) for s in items["singular"]]
    for k in range(n):
        if items["singular"][k]:
            continue
        S, W = got["cov"][k], got["sqrt_information"][k]
        assert (S == S.T).all() and not np.triu(W, 1).any()
        st, W_host = hip.po_sqrt_information(S)                      # the rule the definition names, on the device's own S
        assert st == COV_OK and np.abs(W - W_host).max() <= K * refs[k]["y"]["sqrt_information"] * np.abs(W_host).max(), k
        # W^T W S = I up to the conditioning of S scaled to unit diagonal: eps over its smallest pivot
        assert np.abs(W.T @ W @ S - np.eye(6)).max() <= K * np.finfo(np.float64).eps / refs[k]["pivot"], k
    # every optional block NULL except R: S = R
    only_r = hip.po_edge_statistics(items["pose_a"], items["pose_b"], items["constraints"], cov_meas=items["cov_meas"], sigma2=items["sigma2"])
    _hold("primitive n %d, R alone" % n, only_r, gref.primitive_reference(items, use=("cov_meas",)))
    good = ~items["singular"]
    assert (only_r["cov"][good] == np.tril(items["cov_meas"][good]) + np.transpose(np.tril(items["cov_meas"][good], -1), (0, 2, 1))).all()
    assert (only_r["error"] == got["error"]).all()
    again = hip.po_edge_statistics(items["pose_a"], items["pose_b"], items["constraints"], sigma2=items["sigma2"], **arrays)
    assert all((again[q] == got[q]).all() for q in got)               # no atomics: the same bits


# ---------------------------------------------------------------------------------------------- one graph
def _gate_both_ways(hip, label, g, x, cand, delta):
    """The device's gate against the reference fed the device's OWN Sigma blocks (the new kernel alone), then end to end."""
    pairs = list(zip(cand["pose_a"], cand["pose_b"]))
    cs, got = hip.po_gate(g, cand, delta, params=x)
    assert cs == COV_OK
    st, cp, cq = hip.po_covariance(g, pairs, delta, params=x)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    _, refs = gref.gate(g, x, cand, delta, blocks=(st, cp[a], cp[b], cq))
    w1 = _hold(label + ", device Sigma", got, refs)
    _, refs = gref.gate(g, x, cand, delta)
    w2 = _hold(label + ", end to end", got, refs)
    return got, w1, w2


@pytest.mark.parametrize("delta", [0.0, REF_DELTA])
@pytest.mark.parametrize("shape", GRAPHS)
def test_gate_matches_reference(hip, shape, delta):
    g, x, _ = _solved(shape)
    cand = gref.graph_candidates(g, x)
    got, _, _ = _gate_both_ways(hip, "gate N %d loops %d delta %g" % (shape + (delta,)), g, x, cand, delta)
    # the candidate that touches the constant pose: S = sigma2 Jb Sbb Jb^T + R
    b = cand["pose_b"][0]
    _, cp, _ = hip.po_covariance(g, [], delta, params=x)
    ref = gref.edge_statistics(x.reshape(-1, 6)[cand["pose_a"][0]], x.reshape(-1, 6)[b], cand["constraints"][0], None, cp[b], None, cand["cov_meas"][0], cand["sigma2"])
    assert max(gref.deviations(ref, _item(got, 0)).values()) <= K


def test_gate_honours_edge_weights(hip):
    g, x, _ = _solved((24, 3))
    gw = dict(g, sqrt_information=synth.make_edge_information(7, g))
    cand = gref.graph_candidates(g, x)
    got, _, _ = _gate_both_ways(hip, "gate N 24 loops 3 weighted", gw, x, cand, 0.0)
    _, plain = hip.po_gate(g, cand, 0.0, params=x)
    assert np.abs(got["mahalanobis2"] - plain["mahalanobis2"]).max() > 1e-3 * plain["mahalanobis2"].max()


def _cut_chain():
    g = synth.make_pose_graph(7, 12, 0)
    keep = [e for e, (a, b) in enumerate(zip(g["pose_index_1"], g["pose_index_2"])) if (a, b) != (5, 6)]
    return dict(g, pose_index_1=g["pose_index_1"][keep], pose_index_2=g["pose_index_2"][keep], constraints=g["constraints"][keep])


def test_singular_graph_makes_every_candidate_singular(hip):
    g = _cut_chain()
    x = np.asarray(g["parameters"], dtype=np.float64)
    cand = dict(pose_a=[1, 7, 0], pose_b=[2, 8, 11], constraints=np.zeros((3, 6)) + 0.01, cov_meas=np.tile(np.eye(6), (3, 1, 1)), sigma2=1.0)
    cs, got = hip.po_gate(g, cand, 0.0)
    assert cs == COV_SINGULAR
    cs0, refs = gref.gate(g, x, cand)
    assert cs0 == COV_SINGULAR
    _hold("the 12-pose chain cut at (5, 6)", got, refs)
    assert (got["status"] == COV_SINGULAR).all() and got["error"].any()


# ---------------------------------------------------------------------------------------------- the scenario the feature exists for
def test_gate_separates_a_false_loop_closure(hip):
    g, x, s = _solved((24, 3))
    cand = gref.scenario(g, x, s["final_cost"])
    cs, got = hip.po_gate(g, cand, 0.0, params=x)
    _, refs = gref.gate(g, x, cand)
    _hold("scenario", got, refs)
    good, bad = got["mahalanobis2"]
    print("scenario: sigma2 %.3e  m2 consistent %.3f (reference %.3f)  corrupted %.3e (reference %.3e)" % (
        cand["sigma2"], good, refs[0]["mahalanobis2"], bad, refs[1]["mahalanobis2"]))
    assert cs == COV_OK and good < CHI2_6_95 and bad > CHI2_6_99
    # what consistency_broken() thresholds comes from the same call
    assert np.linalg.norm(got["error"][1][:3]) > 0.3 and np.linalg.norm(got["error"][1][3:]) > 1.0


# ---------------------------------------------------------------------------------------------- the batch
def test_batch_matches_one_graph_calls(hip):
    graphs = [_solved(s)[0] for s in GRAPHS]
    b = hip.POBatch()
    try:
        for g in graphs:
            b.add(g)
        b.finalize()
        b.solve(); b.download()
        xs = [b.parameters(i) for i in range(3)]
        cands = [None, gref.graph_candidates(graphs[1], xs[1]), gref.graph_candidates(graphs[2], xs[2])]
        cands[1] = {k: (v[:1] if k != "sigma2" else v) for k, v in cands[1].items()}
        cands[2] = {k: (list(v) * 2)[:7] if k != "sigma2" else v for k, v in cands[2].items()}
        assert len(cands[1]["pose_a"]) == 1 and len(cands[2]["pose_a"]) == 7
        pairs = [[(1, 3)], [(1, 11), (11, 1)], []]
        for i in range(3):
            b.set_covariance_pairs(i, pairs[i])
            b.set_candidates(i, cands[i])
        with pytest.raises(hip.SlslamError) as ei:            # no gate call yet
            b.get_gate(1)
        assert ei.value.status == INVALID
        b.covariance(); b.download()
        plain = [b.get_covariance(i) for i in range(3)]
        with pytest.raises(hip.SlslamError) as ei:            # a covariance call is not a gate call
            b.get_gate(1)
        assert ei.value.status == INVALID
        before = b.covariance_stats()
        b.gate(); b.download()
        first = [b.get_gate(i) for i in range(3)]
        stats = b.covariance_stats()
        b.gate(); b.download()
        assert b.covariance_stats() == dict(calls=stats["calls"] + 1, allocations=stats["allocations"])      # the second call allocates nothing
        assert stats["calls"] == before["calls"] + 1
        assert len(first[0]["status"]) == 0
        for i in range(3):                                     # get_covariance after gate == after covariance (the same launches, the same order
            st, cp, cq = b.get_covariance(i)                   # of work items: only the atomic sums of the linearisation can differ)
            top = np.abs(plain[i][1]).max()
            assert st == plain[i][0] and cq.shape == plain[i][2].shape
            ref = cref.covariance(graphs[i], xs[i], 0.0)
            assert np.abs(cp - plain[i][1]).max() <= K * ref["y"] * top
            assert len(pairs[i]) == 0 or np.abs(cq - plain[i][2]).max() <= K * ref["y"] * top
        for i in (1, 2):
            _, refs = gref.gate(graphs[i], xs[i], cands[i])
            _hold("batch graph %d" % i, b.get_gate(i), refs)
            _, one = hip.po_gate(graphs[i], cands[i], 0.0, params=xs[i])
            _hold("batch graph %d, the one-graph call" % i, one, refs)
        # validity: a solve, a reset, a replaced candidate list
        b.gate(); b.solve(); b.download()
        with pytest.raises(hip.SlslamError):
            b.get_gate(1)
        b.gate(); b.download()
        assert (b.get_gate(2)["status"] == COV_OK).all()
        b.set_candidates(2, cands[1])
        with pytest.raises(hip.SlslamError):
            b.get_gate(2)
        b.gate(); b.download()
        assert len(b.get_gate(2)["status"]) == 1
        b.reset()
        with pytest.raises(hip.SlslamError):
            b.get_gate(2)
    finally:
        b.close()


def test_graph_without_edges(hip):
    """No edge, so no free pose: every Sigma block is zero and S = R - through the one-graph call and in a batch beside a solved graph."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-0.5, 0.5, (3, 3)), rng.uniform(-2, 2, (3, 3))], axis=1)
    g0 = dict(num_poses=3, pose_index_1=np.zeros(0, np.int32), pose_index_2=np.zeros(0, np.int32), constraints=np.zeros((0, 6)), parameters=x.reshape(-1))
    sd = np.array([2e-3] * 3 + [1e-2] * 3)
    cand = dict(pose_a=[0, 2], pose_b=[1, 0], constraints=np.array([gref.relative_pose(x[0], x[1]) + sd, gref.relative_pose(x[2], x[0]) - sd]),
                cov_meas=np.tile(np.diag(sd * sd), (2, 1, 1)), sigma2=1.0)
    refs = [gref.edge_statistics(x[a], x[b], cand["constraints"][k], None, None, None, cand["cov_meas"][k], 1.0) for k, (a, b) in enumerate(zip(cand["pose_a"], cand["pose_b"]))]
    cs, got = hip.po_gate(g0, cand)
    assert cs == COV_OK
    _hold("one graph without edges", got, refs)
    assert (got["cov"] == cand["cov_meas"]).all()
    no_r = dict(cand, cov_meas=None)                             # nothing at all to weigh the error with: singular, error written
    cs, got = hip.po_gate(g0, no_r)
    assert cs == COV_OK and (got["status"] == COV_SINGULAR).all() and not got["cov"].any() and got["error"].any()
    g1, x1, _ = _solved((4, 1))
    c1 = gref.graph_candidates(g1, x1)
    b = hip.POBatch()
    try:
        b.add(g0); b.add(g1, x1)
        b.finalize()
        b.set_candidates(0, cand); b.set_candidates(1, c1)
        b.gate(); b.download()
        _hold("batch: the graph without edges", b.get_gate(0), refs)
        _hold("batch: its neighbour", b.get_gate(1), gref.gate(g1, x1, c1)[1])
        st, cp, cq = b.get_covariance(0)
        assert st == COV_OK and not cp.any()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------- odometry edges of an LBA window
def test_lba_odometry_edges(hip):
    w = synth.make_window(11, num_lines=40, num_kf=4, num_free=3)
    x, s, _ = hip.lba_solve(w)
    cov = hip.lba_covariance(w, params=x, with_lines=False)
    st, free, cc = cov[0], [int(c) for c in cov[1]], cov[2]
    assert st == COV_OK and len(free) == 3
    const = next(c for c in range(4) if c not in free)
    cams = x[:24].reshape(4, 6)
    pairs = [(free[0], free[1]), (free[1], free[2]), (free[2], free[0]), (const, free[0]), (free[1], const)]
    sigma2 = 0.5
    cons, got = hip.lba_odometry_edges(cov, cams, pairs, sigma2)
    refs = []
    for k, (a, b) in enumerate(pairs):
        blk = lambda p, q: cc[6 * free.index(p):6 * free.index(p) + 6, 6 * free.index(q):6 * free.index(q) + 6] if p in free and q in free else None  # noqa: E731
        assert np.abs(gref.residual(cams[a], cams[b], cons[k])).max() < 1e-12      # C = T_b o T_a^-1 meets its own edge
        refs.append(gref.edge_statistics(cams[a], cams[b], cons[k], blk(a, a), blk(b, b), blk(a, b), None, sigma2))
    # (the error of an exactly met edge is rounding alone: only cov and sqrt_information are held; m2 of rounding noise means nothing)
    for k, ref in enumerate(refs):
        assert got["status"][k] == COV_OK == ref["status"] and ref["pivot"] >= 1e3 * gref.PIVOT_MIN, (k, ref["pivot"])
        d = gref.deviations(ref, _item(got, k))
        print("odometry edge %s: d / y cov %.3f sqrt_information %.3f" % (pairs[k], d["cov"], d["sqrt_information"]))
        assert d["cov"] <= K and d["sqrt_information"] <= K, k
        assert np.abs(got["error"][k]).max() < 1e-12
    _, both_const = hip.lba_odometry_edges(cov, cams, [(const, const)], sigma2)
    assert both_const["status"][0] == COV_SINGULAR and not both_const["sqrt_information"].any()


# ---------------------------------------------------------------------------------------------- the C++ mirror
def test_cxx_mirror_gates(hip, tmp_path):
    """POProblem::gate (tests/host_cxx/po_gate_mirror.cpp) returns what slslam_po_gate returns for the arrays it forwards."""
    host, libdir = os.path.join(ROOT, "slslam_amd", "host"), os.path.join(ROOT, "slslam_amd", "_lib")
    subprocess.check_call(["make", "-s", "-C", host])
    exe = os.path.join(ROOT, "tests", "_build", "po_gate_mirror")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I", host, "-o", exe, os.path.join(ROOT, "tests", "host_cxx", "po_gate_mirror.cpp"),
                           "-L", libdir, "-lslslam_host", "-lslslam_hip", "-Wl,-rpath," + libdir])
    g, x, _ = _solved((12, 2))
    W = synth.make_edge_information(7, g)
    cand = gref.graph_candidates(g, x)
    E, M = len(g["pose_index_1"]), len(cand["pose_a"])
    for weighted, robust in ((1, 1), (0, 0)):
        path = tmp_path / ("gate%d.txt" % weighted)
        rows = ["%d %d %d %d %d" % (int(g["num_poses"]), E, weighted, robust, M)] + ["%d %d" % (a, b) for a, b in zip(g["pose_index_1"], g["pose_index_2"])]
        vals = [np.asarray(g["constraints"]).reshape(-1), np.asarray(x).reshape(-1)] + ([W.reshape(-1)] if weighted else [])
        rows += ["%.17g" % v for a in vals for v in a]
        rows += ["%d %d" % (a, b) for a, b in zip(cand["pose_a"], cand["pose_b"])]
        rows += ["%.17g" % v for a in (cand["constraints"].reshape(-1), cand["cov_meas"].reshape(-1)) for v in a] + ["%.17g" % cand["sigma2"]]
        path.write_text("\n".join(rows) + "\n")
        p = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        m2 = np.array([float(v) for v in p.stdout.split()])
        _, want = hip.po_gate(dict(g, sqrt_information=W) if weighted else g, cand, REF_DELTA if robust else 0.0, params=x)
        assert m2.shape == (M,) and np.abs(m2 - want["mahalanobis2"]).max() <= 1e-9 * want["mahalanobis2"].max()
        gm = dict(g, sqrt_information=W) if weighted else g
        _hold("mirror graph, weighted %d robust %d" % (weighted, robust), want, gref.gate(gm, x, cand, REF_DELTA if robust else 0.0)[1])

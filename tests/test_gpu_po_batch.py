"""GPU tests of the pose-graph batch (include/slslam_hip.h: slslam_po_batch_*): many graphs through one launch sequence must give
what slslam_po_solve gives each of them, and agree with the oracle's envelope Cholesky.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest

from slslam_amd import synth

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4


def _trace_parity(t0, t1, n=None, tol=1e-8):
    assert len(t0) == len(t1)
    for a, b in list(zip(t0, t1))[:n]:
        assert a["iteration"] == b["iteration"] and a["step_is_successful"] == b["step_is_successful"]
        assert abs(a["cost"] - b["cost"]) <= tol * abs(a["cost"]) + 1e-18
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-5 * a["trust_region_radius"]


def _add_edges(g, pairs, rng):
    """extra edges between existing poses, constraints from the true poses + a little noise"""
    truth = g["true_parameters"].reshape(-1, 6)
    ed = {(int(a), int(b)): c for a, b, c in zip(g["pose_index_1"], g["pose_index_2"], g["constraints"])}
    for a, b in pairs:
        a, b = (a, b) if a < b else (b, a)
        if (a, b) in ed:
            continue
        Ra, ta = synth.wt_to_rt(truth[a]); Rb, tb = synth.wt_to_rt(truth[b])
        Rrel = synth.rodrigues(rng.normal(0, 1e-3, 3)) @ Rb @ Ra.T
        ed[(a, b)] = synth.rt_to_wt(Rrel, tb - (Rb @ Ra.T) @ ta + rng.normal(0, 2e-3, 3))
    keys = sorted(ed)
    return dict(g, pose_index_1=np.array([k[0] for k in keys], dtype=np.int32), pose_index_2=np.array([k[1] for k in keys], dtype=np.int32),
                constraints=np.array([ed[k] for k in keys]))


def _no_edges():
    return dict(num_poses=3, pose_index_1=np.zeros(0, np.int32), pose_index_2=np.zeros(0, np.int32),
                constraints=np.zeros((0, 6)), parameters=np.arange(18.0))


def _unreferenced():
    g = synth.make_pose_graph(4, num_poses=30, num_loops=2)
    return dict(g, num_poses=31, parameters=np.concatenate([g["parameters"], np.arange(6.0)]))


def _mixed_set():
    gs = [synth.make_pose_graph(s, num_poses=n, num_loops=l) for s, n, l in [(1, 12, 1), (2, 40, 3), (3, 75, 4), (7, 260, 8), (25, 120, 2)]]
    rng = np.random.default_rng(11)                 # hub, dense_loops, three_levels, ring of test_po_structured_factorisation_topologies
    gs.append(_add_edges(synth.make_pose_graph(24, num_poses=40, num_loops=0), [(10, k) for k in (15, 20, 25, 30, 35, 39)], rng))
    gs.append(_add_edges(synth.make_pose_graph(26, num_poses=60, num_loops=0), [(i, i + 7) for i in range(1, 50, 3)], rng))
    gs.append(_add_edges(synth.make_pose_graph(28, num_poses=300, num_loops=0), [(4, 296), (2, 298)], rng))
    gs.append(_add_edges(synth.make_pose_graph(22, num_poses=30, num_loops=0), [(1, 29)], rng))
    gs.append(synth.make_pose_graph(21, num_poses=50, num_loops=0))      # a tree whose start is exact
    gs.append(_no_edges())
    gs.append(_unreferenced())
    return gs


def _config5():
    return [synth.make_pose_graph(s, num_poses=260, num_loops=8) for s in range(100, 164)]


def _against_oneshot(hip, graphs, results):
    for i, (g, (x, s, t)) in enumerate(zip(graphs, results)):
        x1, s1, t1 = hip.po_solve(g)
        for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks"):
            assert s[k] == s1[k], (i, k, s[k], s1[k])
        d = np.abs(x - x1).max() if len(x) else 0.0
        print("graph %d vs one-shot: %d+%d steps, max |dx| %.3e" % (i, s["num_successful_steps"], s["num_unsuccessful_steps"], d))
        assert d < 1e-9, i
        _trace_parity(t1, t)


def _against_oracle(oracle, graphs, results):
    for i, (g, (x, s, t)) in enumerate(zip(graphs, results)):
        x0, s0, t0 = oracle.po_solve(g, linear_solver=2)
        d = np.abs(x - x0).max() if len(x) else 0.0
        big = int(g["num_poses"]) == 260
        cost_tol, pose_tol = (1e-6, 1e-5) if big else (1e-7, 1e-6)
        print("graph %d vs oracle: steps %d+%d / %d+%d, term %d / %d, cost %.9e / %.9e, max |dx| %.3e" % (
            i, s["num_successful_steps"], s["num_unsuccessful_steps"], s0["num_successful_steps"], s0["num_unsuccessful_steps"],
            s["termination_type"], s0["termination_type"], s["final_cost"], s0["final_cost"], d))
        assert d < pose_tol, i
        if s0["initial_cost"] < 1e-20:              # the exact tree (and the graph without edges): cost and poses alone
            assert s["final_cost"] < 1e-20 and s0["final_cost"] < 1e-20, i
            continue
        assert s["num_successful_steps"] == s0["num_successful_steps"], i
        assert s["num_unsuccessful_steps"] == s0["num_unsuccessful_steps"], i
        assert s["termination_type"] == s0["termination_type"], i
        assert abs(s["final_cost"] - s0["final_cost"]) <= cost_tol * s0["final_cost"], i


@pytest.fixture(scope="module")
def mixed(hip):
    graphs = _mixed_set()
    return graphs, hip.po_solve_batch(graphs)


@pytest.fixture(scope="module")
def config5(hip):
    graphs = _config5()
    return graphs, hip.po_solve_batch(graphs)


def test_mixed_batch_matches_oneshot(hip, mixed):
    _against_oneshot(hip, *mixed)


def test_mixed_batch_matches_oracle(oracle, mixed):
    _against_oracle(oracle, *mixed)


def test_config5_batch_matches_oracle(oracle, config5):
    _against_oracle(oracle, *config5)


def test_config5_batch_matches_oneshot(hip, config5):
    _against_oneshot(hip, *config5)


def test_result_does_not_depend_on_company(hip):
    g7 = synth.make_pose_graph(7, num_poses=260, num_loops=8)
    (xa, sa, ta), = hip.po_solve_batch([g7])
    others = _config5()
    graphs = others[:32] + [g7] + others[32:63]
    assert len(graphs) == 64
    xb, sb, tb = hip.po_solve_batch(graphs)[32]
    for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type"):
        assert sa[k] == sb[k], k
    assert np.abs(xa - xb).max() < 1e-9


def test_edge_cases(hip):
    ge, gu = _no_edges(), _unreferenced()
    res = hip.po_solve_batch([ge, synth.make_pose_graph(2, num_poses=40, num_loops=3), gu])
    x, s, t = res[0]
    assert x.tobytes() == ge["parameters"].tobytes() and s["termination"] == "FUNCTION_TOLERANCE" and t == []
    assert s["num_free_parameters"] == 0 and s["num_residual_blocks"] == 0
    x, s, t = res[2]
    assert x[-6:].tobytes() == np.arange(6.0).tobytes() and s["num_free_parameters"] == 6 * 29
    # zero iterations: the initial parameters, bit for bit
    graphs = [synth.make_pose_graph(s_, num_poses=n, num_loops=l) for s_, n, l in [(1, 12, 1), (7, 260, 8)]]
    for g, (x, s, t) in zip(graphs, hip.po_solve_batch(graphs, max_num_iterations=0)):
        assert x.tobytes() == np.asarray(g["parameters"], np.float64).tobytes()
    # a consistent graph (constraints from the true poses): nothing to do
    g = synth.make_pose_graph(4, num_poses=30, num_loops=2)
    truth = g["true_parameters"].reshape(-1, 6)
    cons = []
    for a, b in zip(g["pose_index_1"], g["pose_index_2"]):
        Ra, ta = synth.wt_to_rt(truth[a]); Rb, tb = synth.wt_to_rt(truth[b])
        Rrel = Rb @ Ra.T
        cons.append(synth.rt_to_wt(Rrel, tb - Rrel @ ta))
    g0 = dict(g, constraints=np.array(cons), parameters=g["true_parameters"])
    (x, s, t), _ = hip.po_solve_batch([g0, g])
    assert s["final_cost"] < 1e-25 and np.abs(x - g["true_parameters"]).max() < 1e-12
    # the dense and fp32 factorisations have no batch form
    for opt in ({"po_dense_factor": 1}, {"po_factor_fp32": 1}):
        b = hip.POBatch()
        b.add(g)
        with pytest.raises(hip.SlslamError) as ei:
            b.finalize(**opt)
        assert ei.value.status == UNSUPPORTED
        b.close()


def test_reuse_and_streams(hip):
    graphs = _mixed_set()[:9] + _config5()[:8]
    b = hip.POBatch()
    for g in graphs:
        b.add(g)
    b.finalize()
    runs = []
    rt = ctypes.CDLL("libamdhip64.so")
    stream = ctypes.c_void_p()
    assert rt.hipStreamCreate(ctypes.byref(stream)) == 0
    try:
        for st in (None, None, stream.value, stream.value):
            b.reset(st); b.solve(st); b.download(st)
            runs.append([(b.parameters(i), b.summary(i), b.trace(i)) for i in range(len(graphs))])
    finally:
        b.close()
        assert rt.hipStreamDestroy(stream) == 0
    for r in runs[1:]:
        for i, ((x0, s0, _), (x1, s1, _)) in enumerate(zip(runs[0], r)):
            for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type"):
                assert s0[k] == s1[k], (i, k)
            assert np.abs(x0 - x1).max() < 1e-9, i

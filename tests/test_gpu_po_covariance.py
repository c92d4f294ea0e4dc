"""Posterior covariances of pose graphs on the device (include/slslam_hip.h: slslam_po_covariance, slslam_po_batch_covariance /
_get_covariance) against the numpy reference of tests/po_covariance_reference.py.  Needs a real MI355X.

Shapes (seed 7): the smallest at which the 64 x 64 blocking can go wrong - n = 18 is one partial block, 66 one block plus two rows,
138 partial, 192 exactly three blocks, 354 six blocks.  The deviation of a graph is d = max |Sigma_dev - Sigma_ref| / max |Sigma_ref|
over every block asked for, held to K * y with y the reference's own yardstick (its two routes' difference and what +-1 ulp on J's
entries does to it), computed here per graph and printed.  K is the next power of ten above the worst d / y measured on the MI355X
(profiles/po_covariance_bench.txt lists the ratios per graph): the worst is 19.3 - the 4-pose graph under po_huber_delta 0.001,
d = 1.2e-14, where the weight sqrt(delta / sqrt(s)) of a whole 6 x 12 block carries the rounding of s, a coherent error that independent
+-1 ulp on 18 columns understates - and at most 7.9 elsewhere, so K = 100."""
import functools
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402

pytestmark = pytest.mark.gpu
K = 100.0
REF_DELTA = 0.001
SHAPES = [(4, 1), (12, 2), (24, 3), (33, 2), (60, 4)]
COV_OK, COV_SINGULAR = 0, 1
INVALID = 1


# ---------------------------------------------------------------------------------------------- graphs and references
@functools.lru_cache(maxsize=None)
def _solved(shape):
    """(graph, the oracle's solved poses): computed once, shared, never modified."""
    from oracle import pyoracle
    g = synth.make_pose_graph(7, *shape)
    x, _, _ = pyoracle.po_solve(g, linear_solver=2)
    x.setflags(write=False)
    return g, x


def _pairs(g):
    """The loop closures' endpoints, (first free, last free), one a == b, one pair that touches the constant pose."""
    N = int(g["num_poses"])
    loops = [(int(a), int(b)) for a, b in zip(g["pose_index_1"], g["pose_index_2"]) if b - a > 1]
    return loops + [(1, N - 1), (N - 1, 1), (2, 2), (0, N - 1)]


def _cut_chain():
    g = synth.make_pose_graph(7, 12, 0)
    keep = [e for e, (a, b) in enumerate(zip(g["pose_index_1"], g["pose_index_2"])) if (a, b) != (5, 6)]
    return dict(g, pose_index_1=g["pose_index_1"][keep], pose_index_2=g["pose_index_2"][keep], constraints=g["constraints"][keep])


def _corrupt(g):
    """tests/test_gpu_po_robust.py's corruption: the first loop constraint off by (1.5, 0, -1) m and 0.4 rad."""
    g = dict(g, constraints=np.array(g["constraints"], dtype=np.float64).copy())
    e = int(np.nonzero(np.asarray(g["pose_index_2"]) - np.asarray(g["pose_index_1"]) > 1)[0][0])
    g["constraints"][e, 3:6] += (1.5, 0.0, -1.0)
    g["constraints"][e, 1] += 0.4
    return g


def _deviation(label, got, g, x, delta, pairs):
    """Holds (status, cov_poses, cov_pairs) to the reference at x; returns (d, y, reference)."""
    st, cp, cq = got
    ref = cref.covariance(g, x, delta)
    cp0, cq0 = cref.blocks(ref, int(g["num_poses"]), pairs)
    top = np.abs(ref["sigma"]).max()
    d = max(np.abs(cp - cp0).max(), np.abs(cq - cq0).max() if len(pairs) else 0.0) / top
    print("%s: n %d pivot %.3e  y %.3e (r %.2e c %.2e)  d %.3e  d / y %.3f" % (label, ref["n"], ref["pivot"], ref["y"], ref["r"], ref["c"], d, d / ref["y"]))
    assert st == COV_OK
    assert d <= K * ref["y"], label
    return d, ref["y"], ref


# ---------------------------------------------------------------------------------------------- 1, 2: one graph
@pytest.mark.parametrize("delta", [0.0, REF_DELTA])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_shot_matches_reference(hip, shape, delta):
    g, x = _solved(shape)
    pairs = _pairs(g)
    got = hip.po_covariance(g, pairs, delta, params=x)
    _, y, ref = _deviation("N %d loops %d delta %g" % (shape + (delta,)), got, g, x, delta, pairs)
    st, cp, cq = got
    top = np.abs(ref["sigma"]).max()
    N = shape[0]
    # structure: (a, b) against (b, a); symmetric, positive definite marginals; exact zeros at and with the constant pose
    ia, ib = pairs.index((1, N - 1)), pairs.index((N - 1, 1))
    assert np.abs(cq[ia] - cq[ib].T).max() <= K * y * top
    assert not cp[0].any() and not cq[pairs.index((0, N - 1))].any()
    assert np.abs(cq[pairs.index((2, 2))] - cp[2]).max() <= K * y * top
    for k in range(1, N):
        assert np.abs(cp[k] - cp[k].T).max() <= K * y * top, k
        assert np.linalg.eigvalsh(0.5 * (cp[k] + cp[k].T)).min() > 0.0, k


def test_unreferenced_pose_is_zero(hip):
    g, x = _solved((12, 2))
    gu = dict(g, num_poses=13, parameters=np.concatenate([x, np.arange(6.0)]))
    pairs = [(1, 12), (12, 12), (12, 0), (1, 11)]
    st, cp, cq = hip.po_covariance(gu, pairs)
    assert st == COV_OK
    assert not cp[12].any() and not cp[0].any() and not cq[:3].any()
    _deviation("12 / 2 with a thirteenth pose no edge references", (st, cp[:12], cq[3:]), g, x, 0.0, [(1, 11)])


# ---------------------------------------------------------------------------------------------- 3: the robust point
def test_robust_point(hip):
    g = _corrupt(synth.make_pose_graph(7, 24, 3))
    x, s, _ = hip.po_solve(g, po_huber_delta=REF_DELTA)
    pairs = _pairs(g)
    got = hip.po_covariance(g, pairs, REF_DELTA, params=x)
    _, y, ref = _deviation("corrupted 24 / 3 at the robust solution", got, g, x, REF_DELTA, pairs)
    plain = hip.po_covariance(g, pairs, 0.0, params=x)
    top = np.abs(ref["sigma"]).max()
    change = max(np.abs(got[1] - plain[1]).max(), np.abs(got[2] - plain[2]).max()) / top
    print("the down-weighted edge changes Sigma by %.3e of max |Sigma| (K y = %.3e)" % (change, K * y))
    assert plain[0] == COV_OK and change > K * y


# ---------------------------------------------------------------------------------------------- 4 - 6: the batch
@pytest.fixture(scope="module")
def batch(hip):
    """The five graphs and the singular one in one batch: solve -> covariance -> download.  Different pair lists; graph 1 has none."""
    graphs = [_solved(s)[0] for s in SHAPES] + [_cut_chain()]
    pair_lists = [_pairs(g) for g in graphs]
    pair_lists[1] = []
    pair_lists[5] = [(1, 2), (7, 8), (2, 9)]
    b = hip.POBatch()
    for g in graphs:
        b.add(g)
    b.set_covariance_pairs(0, pair_lists[0])                # before finalize
    b.finalize()
    for i in range(1, 6):
        b.set_covariance_pairs(i, pair_lists[i])
    b.solve(); b.covariance(); b.download()
    yield b, graphs, pair_lists
    b.close()


def test_batch_matches_reference(hip, batch):
    b, graphs, pair_lists = batch
    for i in range(5):
        x = b.parameters(i)
        _deviation("batch graph %d" % i, b.get_covariance(i), graphs[i], x, 0.0, pair_lists[i])
    st, cp, cq = b.get_covariance(5)
    assert st == COV_SINGULAR and not cp.any() and not cq.any() and cq.shape == (3, 6, 6)
    st1, cp1, cq1 = hip.po_covariance(graphs[5], pair_lists[5])
    assert st1 == COV_SINGULAR and not cp1.any() and not cq1.any()


def test_covariance_leaves_the_solve_alone(hip, oracle):
    graphs = [_solved(s)[0] for s in SHAPES[1:4]]
    b = hip.POBatch()
    for g in graphs:
        b.add(g)
        b.set_covariance_pairs(len(b) - 1, _pairs(g))
    b.finalize()
    try:
        def results():
            return [(b.parameters(i).tobytes(), sorted(b.summary(i).items()), b.trace(i), b.edge_report(i)[0].tobytes()) for i in range(len(graphs))]
        b.solve(); b.download()
        before = results()
        b.covariance(); b.download()
        assert results() == before
        assert b.get_covariance(0)[0] == COV_OK
        b.reset(); b.solve(); b.download()
        x, s, _ = b.parameters(1), b.summary(1), b.trace(1)
        x0, s0, _ = oracle.po_solve(graphs[1], linear_solver=2)          # tests/test_gpu_po_batch.py's tolerances against the oracle
        assert np.abs(x - x0).max() < 1e-6
        for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type"):
            assert s[k] == s0[k], k
        assert abs(s["final_cost"] - s0["final_cost"]) <= 1e-7 * s0["final_cost"]
    finally:
        b.close()


def test_states_and_stats(hip):
    g, _ = _solved((12, 2))
    g2, _ = _solved((24, 3))
    b = hip.POBatch()
    b.add(g); b.add(g2)
    b.set_covariance_pairs(0, [(1, 11)])
    b.finalize()
    try:
        b.solve(); b.download()
        with pytest.raises(hip.SlslamError) as ei:            # no covariance call yet
            b.get_covariance(0)
        assert ei.value.status == INVALID
        b.covariance(); b.download()
        first = b.get_covariance(0)
        stats = b.covariance_stats()
        assert stats["calls"] == 1 and stats["allocations"] >= 1
        b.covariance(); b.download()
        again = b.get_covariance(0)
        assert b.covariance_stats() == dict(calls=2, allocations=stats["allocations"])
        for got in (first, again):
            _deviation("12 / 2 in a batch of two", got, g, b.parameters(0), 0.0, [(1, 11)])
        b.covariance(); b.solve(); b.download()              # a solve enqueued behind the covariance call
        with pytest.raises(hip.SlslamError) as ei:
            b.get_covariance(0)
        assert ei.value.status == INVALID
        longer = [(1, 11), (11, 1), (3, 4), (5, 5)]
        b.set_covariance_pairs(0, longer)
        b.covariance(); b.download()
        _deviation("longer pair list", b.get_covariance(0), g, b.parameters(0), 0.0, longer)
        _deviation("its neighbour", b.get_covariance(1), g2, b.parameters(1), 0.0, [])
        assert b.covariance_stats()["calls"] == 4
    finally:
        b.close()

"""GPU tests: the descriptor matcher (slslam_descriptor_matcher_*, slslam_match_descriptors; csrc/descriptor_match.h) against its numpy
reference (tests/descriptor_match_reference.py, which tests/test_descriptor_match_cpu.py pins by hand).

Every integer output must be equal and best_distance / second_distance must match bit for bit: the kernel evaluates the contract's float
chain in the contract's order without contraction, and the reductions are minima and counts."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as R  # noqa: E402
from test_descriptor_match_cpu import HAND, SEQ_MAX_DISTANCE, SEQ_RATIO, check_hand, shuffled_sequence  # noqa: E402
from test_place_cpu import SEQ, seq_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

INT_KEYS = ("match", "best", "num_admissible", "best_query")
FLOAT_KEYS = ("best_distance", "second_distance")
NS = [1, 63, 64, 65, 130]                # the edges of a wave of query descriptors
MS = [1, 7, 8, 9, 64, 65, 200]           # the edges of a group of eight keyframe descriptors, and of the finish kernel's wave


def same(got, ref):
    assert got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["num_matched"] == ref["num_matched"]
    for k in INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    for k in FLOAT_KEYS:
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k


def same_bytes(a, b):
    assert a["status"] == b["status"] and a["num_matched"] == b["num_matched"]
    for k in INT_KEYS + FLOAT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def unit(rng, n, D):
    d = rng.standard_normal((n, D))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def make_views(seed, ns, ms, D, noise=0.05):
    """keyframes of ms descriptors and query frames of ns, all noisy views of the same max(ns + ms) unit descriptors, the queries shuffled"""
    rng = np.random.default_rng(np.random.SeedSequence([16, int(seed)]))
    base = unit(rng, max(ns + ms), D)

    def view(rows):
        d = base[rows] + noise * rng.standard_normal((len(rows), D))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return [view(rng.permutation(len(base))[:n]) for n in ns], [view(np.arange(m)) for m in ms]


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed_on_the_device(hip, name):
    q, k, ratio, max_distance, want = HAND[name]
    check_hand(hip.match_descriptors(np.array(q, np.float32), np.array(k, np.float32), ratio, max_distance), want)


# ---- shapes: every n against every m in one call per D.  D = 1: every descriptor is +1 or -1, every r is 0 or 2 - nothing but ties.
@pytest.mark.parametrize("D", [1, 16, 72, 128])
def test_shapes(hip, D):
    queries, keyframes = make_views(100 + D, NS, MS, D)
    m = hip.DescriptorMatcher(D, max_keyframes=len(MS), max_descriptors=200, max_frames=len(NS), max_candidates=len(MS))
    store = R.Store()
    for k in keyframes:
        assert m.insert(k)["id"] == store.insert(k)[1]
    call = [(q, list(range(len(MS)))) for q in queries]
    for ratio, max_distance in ((1.2, 0.9), (1.0, float("inf"))):
        got, ref = m.run(call, ratio, max_distance), store.run(call, ratio, max_distance)
        for gf, rf in zip(got, ref):
            for g, r in zip(gf, rf):
                same(g, r)
        if D >= 16 and ratio > 1.0:                               # (the case is not an empty one, and not everything is admissible)
            big = ref[NS.index(130)][MS.index(200)]
            assert big["num_matched"] >= 100 and 0 < big["num_admissible"].min() and big["num_admissible"].max() < 200
    same_bytes(hip.match_descriptors(queries[3], keyframes[5], 1.2, 0.9), got_first(m, queries[3], 5))
    m.close()


def got_first(m, q, kid):
    return m.run([(q, [kid])], 1.2, 0.9)[0][0]


def test_duplicated_descriptors(hip):
    """every descriptor twice on both sides: ties everywhere, and r <= 0 between copies"""
    rng = np.random.default_rng(31)
    base = unit(rng, 40, 72).astype(np.float32)
    k = np.concatenate([base, base])
    q = k[rng.permutation(80)]
    ref = R.match(q, k, 1.5, 0.25)
    assert (np.abs(ref["best_distance"]) <= 1e-6).all() and (ref["best_distance"] < 0).any() and (ref["num_admissible"] == 2).all()
    assert (ref["best"] < 40).all() and np.array_equal(ref["best_distance"].view(np.uint32), ref["second_distance"].view(np.uint32))
    same(hip.match_descriptors(q, k, 1.5, 0.25), ref)
    ref1 = R.match(q, k, 1.0, 0.25)
    assert ref1["num_matched"] == 40                                                # (mutual alone: the lowest index on both sides)
    same(hip.match_descriptors(q, k, 1.0, 0.25), ref1)


def test_nothing_admissible(hip):
    (q,), (k,) = make_views(41, [65], [70], 16)
    for max_distance in (-1.0, float("-inf")):
        got = hip.match_descriptors(q, k, 1.5, max_distance)
        same(got, R.match(q, k, 1.5, max_distance))
        assert got["status"] == "OK" and got["num_matched"] == 0 and (got["best"] == -1).all() and (got["best_query"] == -1).all()
        assert np.isinf(got["best_distance"]).all() and (got["num_admissible"] == 0).all()


def test_mixed_statuses_in_one_call(hip):
    queries, keyframes = make_views(42, [65, 9, 30], [64, 10], 16)
    nan = queries[1].copy()
    nan[4, 3] = np.nan
    empty = np.zeros((0, 16), np.float32)
    m = hip.DescriptorMatcher(16, max_keyframes=4, max_descriptors=65, max_frames=5, max_candidates=3)
    store = R.Store()
    for k in keyframes:
        m.insert(k), store.insert(k)
    call = [(queries[0], [0, -1, 1]), (empty, [0]), (nan, [1, -1]), (queries[2], []), (queries[2], [-1, 1])]
    got, ref = m.run(call, 1.2, 0.9), store.run(call, 1.2, 0.9)
    assert [[g["status"] for g in gf] for gf in got] == [["OK", "EMPTY", "OK"], ["EMPTY"], ["INVALID_DESCRIPTOR"] * 2, [], ["EMPTY", "OK"]]
    for gf, rf in zip(got, ref):
        for g, r in zip(gf, rf):
            same(g, r)
            assert g["candidate"] == r["candidate"]
    assert len(got[2][0]["best_query"]) == 10 and (got[2][0]["best_query"] == -1).all() and (got[2][0]["match"] == -1).all()
    # before anything is inserted every candidate is -1
    m0 = hip.DescriptorMatcher(16, max_keyframes=4, max_descriptors=65, max_frames=5, max_candidates=3)
    g = m0.run([(queries[0], [-1])])[0][0]
    assert g["status"] == "EMPTY" and (g["match"] == -1).all() and len(g["best_query"]) == 0
    m0.close()
    m.close()


# ---- a pair's bytes do not depend on the call
def test_independent_of_the_call(hip):
    ns = [130, 64, 1, 77, 65, 12, 63, 128]
    queries, keyframes = make_views(43, ns, [200, 9, 65], 72)
    m = hip.DescriptorMatcher(72, max_keyframes=3, max_descriptors=200, max_frames=8, max_candidates=3)
    for k in keyframes:
        m.insert(k)
    alone = m.run([(queries[0], [0])], 1.2, 0.9)[0][0]
    among = m.run([(q, [2, 0, 1]) for q in queries[1:5]] + [(queries[0], [1, 0, 2])] + [(q, [0, 1, 2]) for q in queries[5:]], 1.2, 0.9)
    assert sum(len(a) for a in among) == 24
    same_bytes(alone, among[4][1])
    same_bytes(alone, hip.match_descriptors(queries[0], keyframes[0], 1.2, 0.9))
    same(among[7][2], R.match(queries[7], keyframes[2], 1.2, 0.9))
    assert alone["num_matched"] > 60
    m.close()


# ---- buffers persist; the store's ids
def test_reuse_growth_and_refused_inserts(hip):
    queries, keyframes = make_views(44, [60, 64, 33], [64, 20, 64], 16)
    m = hip.DescriptorMatcher(16, max_keyframes=3, max_descriptors=64, max_frames=2, max_candidates=2)
    assert m.stats() == {"calls": 0, "allocations": 0} and m.size() == 0
    assert m.insert(keyframes[0]) == {"status": "OK", "id": 0}
    assert m.stats() == {"calls": 1, "allocations": 1}                             # the store
    bad = keyframes[1].copy()
    bad[19, 15] = np.inf
    assert m.insert(bad) == {"status": "INVALID_DESCRIPTOR", "id": -1}
    assert m.insert(np.zeros((0, 16), np.float32)) == {"status": "EMPTY", "id": -1}
    assert m.size() == 1
    assert m.insert(keyframes[1]) == {"status": "OK", "id": 1}                     # a refused insert leaves the ids unchanged
    r1 = m.run([(queries[0], [0, 1]), (queries[1], [1, 0])], 1.2, 0.9)
    assert m.stats() == {"calls": 5, "allocations": 2}                             # the run's blocks
    r2 = m.run([(queries[1], [1, 0]), (queries[0], [0, 1])], 1.2, 0.9)
    assert m.insert(keyframes[2]) == {"status": "OK", "id": 2}
    r3 = m.run([(queries[0], [0])], 1.2, 0.9)
    assert m.stats() == {"calls": 8, "allocations": 2}                             # a run that fits allocates nothing
    r4 = m.run([(queries[0], [0, 1]), (queries[2], [2]), (queries[1], [1, 2]), (queries[0], [2, 0]), (queries[1], [0, 1])], 1.2, 0.9)
    # (five frames where two were declared: larger blocks)
    assert m.stats() == {"calls": 9, "allocations": 3}
    for x, y in ((r1[0][0], r2[1][0]), (r1[1][1], r2[0][1]), (r1[0][0], r3[0][0]), (r1[0][1], r4[0][1])):
        same_bytes(x, y)
    same(r4[2][1], R.match(queries[1], keyframes[2], 1.2, 0.9))
    same(r1[0][1], R.match(queries[0], keyframes[1], 1.2, 0.9))
    with pytest.raises(hip.SlslamError) as ei:                                    # the store is full
        m.insert(keyframes[0])
    assert ei.value.status == 5 and m.size() == 3
    for call in ([(queries[0], [3])], [(queries[0], [0, 1, 2])], [(np.zeros((65, 16), np.float32), [0])]):
        with pytest.raises(hip.SlslamError) as ei:
            m.run(call)
        assert ei.value.status == 1
    assert m.stats() == {"calls": 9, "allocations": 3}
    m.close()


# ---- the loop-closure chain: the recogniser names a keyframe, the matcher pairs the features
def test_place_sequence_end_to_end(hip):
    """the CPU test's place sequence, the rows of every revisit frame shuffled: PlaceDB, PlaceFilter and DescriptorMatcher are fed the same
    keyframes; at every reported loop the candidates are the reported keyframe and its two neighbours"""
    K, L, D = SEQ["tree"]
    _, nodes, _ = seq_inputs()
    s, frames, perms = shuffled_sequence()
    tree = hip.VocTree(K, L, D, nodes)
    db = hip.PlaceDB(tree, max_docs=80, max_words=32, max_frames=1, recent=SEQ["recent"], num_avg_words=SEQ["navg"])
    flt = hip.PlaceFilter(**SEQ["filt"])
    dm = hip.DescriptorMatcher(D, max_keyframes=80, max_descriptors=32, max_frames=1, max_candidates=3)
    store = R.Store()
    loops = 0
    for i, fr in enumerate(frames):
        loop, kf, _ = hip.place_candidates(db, flt, fr)
        assert dm.insert(fr) == {"status": "OK", "id": i} and store.insert(fr) == ("OK", i)
        if not loop:
            continue
        loops += 1
        cands = [kf - 1, kf, kf + 1]
        c, res = hip.loop_matches(dm, fr, cands, SEQ_RATIO, SEQ_MAX_DISTANCE)
        rc, ref = R.loop_matches(store, fr, cands, SEQ_RATIO, SEQ_MAX_DISTANCE)
        assert c == rc == int(s["place"][i])                       # (first pass: keyframe id = place)
        same(res, ref)
        assert res["num_matched"] == len(fr) and np.array_equal(res["match"], perms[i])
    assert loops > 0 and dm.size() == db.size()["inserted"] == len(frames)
    for h in (dm, flt, db, tree):
        h.close()


def test_end_to_end_recovers_the_pose(hip):
    """a stereo pair whose current frame comes in shuffled order with descriptors attached, 140 common lines and 10 more on either side:
    descriptors -> matches -> matched_trials -> the pose of the id-paired call (the pattern of tests/test_gpu_line_match.py)"""
    n, o = 140, 10
    pair = synth.make_ransac_pair(8100, num_lines=n + 2 * o, outlier_frac=0.0, num_trials=1)
    dp = synth.make_descriptor_pair(8100, n=n, dim=72, noise=0.03, outliers=o)
    qid, kid = dp["query_id"].copy(), dp["keyframe_id"].copy()
    qid[qid < 0] = n + np.arange(o)                                # (the lines only one side sees)
    kid[kid < 0] = n + o + np.arange(o)
    frame = dict(observations=pair["obs1"][qid], lines=pair["lines"][kid])
    ref = R.match(dp["query"], dp["keyframe"], 1.5, 0.25)
    assert np.array_equal(ref["match"], dp["truth"])               # (the condition on the input)
    got = hip.match_descriptors(dp["query"], dp["keyframe"], 1.5, 0.25)
    same(got, ref)
    tr = hip.matched_trials(frame, got, pair["obs0"][kid], num_trials=1001)
    ids = qid[got["match"] >= 0]                                   # the same pairs by landmark id
    assert len(ids) == n and np.array_equal(kid[tr["line_index"]], ids)
    by_id = dict(obs0=pair["obs0"][ids], obs1=pair["obs1"][ids], lines=pair["lines"][ids], samples=tr["samples"])
    est = hip.PoseEstimator(max_frames=2, max_lines=n)
    a, b = est.run([{k: tr[k] for k in ("obs0", "obs1", "lines", "samples")}, by_id])
    est.close()
    assert a["status"] == "OK" and b["status"] == "OK"
    assert np.abs(a["pose"] - b["pose"]).max() < 1e-10             # (tests/test_gpu_pose_estimator.py: _same_frame)
    assert a["num_inliers"] == b["num_inliers"] and np.array_equal(a["mask"], b["mask"])

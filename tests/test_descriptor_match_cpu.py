"""The descriptor matcher without a device (include/slslam_hip.h: slslam_descriptor_matcher_*, slslam_match_descriptors): hand-computed
cases that pin the numpy reference (tests/descriptor_match_reference.py), every argument check of the C ABI (made before a device is
asked for), SLSLAM_ERR_NO_DEVICE on a machine without one, and the property of the synthetic place sequence that the GPU end-to-end test
relies on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as R  # noqa: E402
from test_place_cpu import SEQ, seq_inputs  # noqa: E402

INVALID_ARGUMENT, NO_DEVICE, STATE = 1, 2, 5
EPS = np.float32(2.0 ** -12)                                    # (1, EPS) . (1, EPS) = 1 + 2^-24: every product and difference is exact
SEQ_RATIO, SEQ_MAX_DISTANCE = 1.5, 0.25

# Hand-computed pairs, also run on the device by tests/test_gpu_descriptor_match.py: (q, k, ratio, max_distance, expected fields)
INF = float("inf")
HAND = {
    # r = (1 - 1 * 1) - 0 * 0 = 0 exactly
    "zero": ([[1, 0]], [[1, 0]], 1.5, INF,
             dict(best=[0], best_distance=[0.0], second_distance=[INF], num_admissible=[1], best_query=[0], match=[0])),
    # two equal keyframe descriptors and two equal query descriptors: every r is 0, the lowest index wins on both sides; query 0 is
    # matched (0 * 1.5 <= 0), query 1 is not mutual
    "tie": ([[1, 0], [1, 0]], [[1, 0], [1, 0]], 1.5, INF,
            dict(best=[0, 0], best_distance=[0.0, 0.0], second_distance=[0.0, 0.0], num_admissible=[2, 2], best_query=[0, 0], match=[0, -1])),
    # r(q1, k1) = (1 - 1) - EPS * EPS = -2^-24, below the 0 of the three other pairs: the order of the floats, not of their bits
    "negative": ([[1, 0], [1, EPS]], [[1, 0], [1, EPS]], 1.5, INF,
                 dict(best=[0, 1], best_distance=[0.0, -2.0 ** -24], second_distance=[0.0, 0.0], num_admissible=[2, 2], best_query=[0, 1],
                      match=[0, 1])),
    # D = 1: r = 1 - 0.75 = 0.25 and 1 - 0.5 = 0.5; 0.25 * 2 <= 0.5 holds at equality ...
    "ratio_equal": ([[1]], [[0.75], [0.5]], 2.0, INF,
                    dict(best=[0], best_distance=[0.25], second_distance=[0.5], num_admissible=[2], best_query=[0, 0], match=[0])),
    # ... and fails one ulp of the ratio above it
    "ratio_above": ([[1]], [[0.75], [0.5]], float(np.nextafter(2.0, 3.0)), INF,
                    dict(best=[0], best_distance=[0.25], second_distance=[0.5], num_admissible=[2], best_query=[0, 0], match=[-1])),
    # r = 0.25 is not < 0.25 ...
    "max_distance_equal": ([[1]], [[0.75], [0.5]], 1.0, 0.25,
                           dict(best=[-1], best_distance=[INF], second_distance=[INF], num_admissible=[0], best_query=[-1, -1], match=[-1])),
    # ... and is below the next double
    "max_distance_above": ([[1]], [[0.75], [0.5]], 1.0, float(np.nextafter(0.25, 1.0)),
                           dict(best=[0], best_distance=[0.25], second_distance=[INF], num_admissible=[1], best_query=[0, -1], match=[0])),
}


def check_hand(got, want):
    assert got["status"] == "OK"
    for key, v in want.items():
        a = np.asarray(got[key])
        if key.endswith("distance"):
            assert a.dtype == np.float32 and a.view(np.uint32).tolist() == np.array(v, dtype=np.float32).view(np.uint32).tolist(), key
        else:
            assert a.tolist() == v, key
    assert got["num_matched"] == sum(1 for x in want["match"] if x >= 0)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed(name):
    q, k, ratio, max_distance, want = HAND[name]
    check_hand(R.match(np.array(q, np.float32), np.array(k, np.float32), ratio, max_distance), want)


def test_reference_statuses():
    k = np.array([[1, 0]], np.float32)
    assert R.match(np.zeros((0, 2), np.float32), k)["status"] == "EMPTY"
    assert R.match(k, None)["status"] == "EMPTY"
    bad = R.match(np.array([[1, 0], [np.nan, 0]], np.float32), k)
    assert bad["status"] == "INVALID_DESCRIPTOR" and bad["best"].tolist() == [-1, -1] and bad["best_query"].tolist() == [-1]
    assert R.match(np.array([[np.inf, 0]], np.float32), None)["status"] == "INVALID_DESCRIPTOR"
    s = R.Store()
    assert s.insert(np.zeros((0, 2))) == ("EMPTY", -1) and s.insert([[np.nan, 1]]) == ("INVALID_DESCRIPTOR", -1)
    assert s.insert(k) == ("OK", 0) and s.insert(k) == ("OK", 1)


def test_make_descriptor_pair():
    p = synth.make_descriptor_pair(5, n=40, dim=16, noise=0.02, outliers=7)
    q, k, t = p["query"], p["keyframe"], p["truth"]
    assert q.shape == k.shape == (47, 16) and q.dtype == np.float32
    assert np.allclose(np.linalg.norm(q, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(k, axis=1), 1, atol=1e-6)
    assert (t >= 0).sum() == 40 and sorted(t[t >= 0].tolist()) == sorted(np.nonzero(p["keyframe_id"] >= 0)[0].tolist())
    assert np.array_equal(p["query_id"][t >= 0], p["keyframe_id"][t[t >= 0]]) and (p["query_id"][t < 0] == -1).all()
    assert not np.array_equal(p["query_id"], p["keyframe_id"])                # (each view has its own order)
    ref = R.match(q, k, 1.5, 0.25)
    assert np.array_equal(ref["match"][t >= 0], t[t >= 0]) and (ref["match"][t < 0] == -1).all()


# ---- the C ABI's argument checks: made before a device is asked for, so they hold on every machine
def _result():
    b = {"match": np.full(4, -7, np.int32), "best_query": np.full(4, -7, np.int32)}
    return capi.DescriptorResult(-7, -7, -7, capi._ip(b["match"]), None, None, None, None, capi._ip(b["best_query"])), b


def _untouched(r, b):
    return (r.status, r.num_matched, r.num_keyframe_descriptors) == (-7, -7, -7) and (b["match"] == -7).all() and (b["best_query"] == -7).all()


def test_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    good = (2, 4, 4, 2, 3)                                      # D, max_keyframes, max_descriptors, max_frames, max_candidates
    for i, bad in ((0, 0), (0, 129), (1, 0), (2, 0), (2, 513), (3, 0), (4, 0), (4, 9)):
        args = list(good)
        args[i] = bad
        assert L.slslam_descriptor_matcher_create(-1, *args, C.byref(h)) == INVALID_ARGUMENT, args
    assert L.slslam_descriptor_matcher_create(-1, *good, None) == INVALID_ARGUMENT
    assert L.slslam_descriptor_matcher_create(-1, 128, 1, 512, 1, 8, C.byref(h)) == 0      # the limits themselves; no device is touched
    n = C.c_int(-1)
    assert L.slslam_descriptor_matcher_size(h, C.byref(n)) == 0 and n.value == 0
    assert L.slslam_descriptor_matcher_size(None, C.byref(n)) == INVALID_ARGUMENT
    assert L.slslam_descriptor_matcher_stats(None, None, None) == INVALID_ARGUMENT
    L.slslam_descriptor_matcher_destroy(h)
    L.slslam_descriptor_matcher_destroy(None)


def test_insert_and_run_arguments():
    L = capi.lib()
    h = C.c_void_p()
    assert L.slslam_descriptor_matcher_create(-1, 2, 4, 4, 2, 3, C.byref(h)) == 0
    d = np.array([[1, 0], [0, 1], [1, 0], [0, 1], [1, 0]], np.float32)
    st, kid = C.c_int(-7), C.c_int(-7)
    for n, ptr in ((-1, capi._fp(d)), (5, capi._fp(d)), (2, None)):
        assert L.slslam_descriptor_matcher_insert(h, n, ptr, C.byref(st), C.byref(kid)) == INVALID_ARGUMENT
    assert L.slslam_descriptor_matcher_insert(None, 2, capi._fp(d), C.byref(st), C.byref(kid)) == INVALID_ARGUMENT
    assert (st.value, kid.value) == (-7, -7)

    none, zero, two = np.array([-1, -1, -1, -1], np.int32), np.array([0], np.int32), np.array([-2], np.int32)
    Q = capi.DescriptorQuery

    def run(queries, ratio=1.5, max_distance=1.0, num_pairs=None, out=True, frames=None):
        qs = (Q * max(len(queries), 1))(*queries)
        r, b = _result()
        rc = L.slslam_descriptor_matcher_run(h, len(queries) if frames is None else frames, qs if queries else None, ratio, max_distance,
                                             sum(q.num_candidates for q in queries) if num_pairs is None else num_pairs,
                                             C.byref(r) if out else None)
        assert _untouched(r, b)
        return rc

    ok = Q(2, capi._fp(d), 1, capi._ip(none))
    bad = [
        run([ok], frames=-1),                                               # negative counts
        run([ok], num_pairs=-1),
        run([Q(-1, capi._fp(d), 1, capi._ip(none))]),
        run([Q(2, capi._fp(d), -1, capi._ip(none))]),
        run([Q(2, None, 1, capi._ip(none))]),                               # a missing array
        run([Q(2, capi._fp(d), 1, None)]),
        run([ok], out=False),
        L.slslam_descriptor_matcher_run(h, 1, None, 1.5, 1.0, 0, None),
        run([Q(5, capi._fp(d), 1, capi._ip(none))]),                        # n > max_descriptors
        run([Q(2, capi._fp(d), 4, capi._ip(none))]),                        # more candidates than max_candidates
        run([Q(2, capi._fp(d), 1, capi._ip(zero))]),                        # a candidate outside [-1, inserted): nothing is inserted
        run([Q(2, capi._fp(d), 1, capi._ip(two))]),
        run([ok, ok], num_pairs=1),                                         # a wrong num_pairs
        run([ok], num_pairs=2),
        run([ok], ratio=float("nan")),                                      # NaN
        run([ok], max_distance=float("nan")),
        L.slslam_descriptor_matcher_run(None, 0, None, 1.5, 1.0, 0, None),
    ]
    assert bad == [INVALID_ARGUMENT] * len(bad)
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_descriptor_matcher_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)

    # the one-shot call
    r, b = _result()
    f = capi._fp(d)
    for args in ((0, 1, f, 1, f), (129, 1, f, 1, f), (2, -1, f, 1, f), (2, 513, f, 1, f), (2, 1, f, -1, f), (2, 1, f, 513, f),
                 (2, 1, None, 1, f), (2, 1, f, 1, None)):
        assert L.slslam_match_descriptors(*args, 1.5, 1.0, C.byref(r)) == INVALID_ARGUMENT, args[:2]
    assert L.slslam_match_descriptors(2, 1, f, 1, f, float("nan"), 1.0, C.byref(r)) == INVALID_ARGUMENT
    assert L.slslam_match_descriptors(2, 1, f, 1, f, 1.5, float("nan"), C.byref(r)) == INVALID_ARGUMENT
    assert L.slslam_match_descriptors(2, 1, f, 1, f, 1.5, 1.0, None) == INVALID_ARGUMENT
    assert _untouched(r, b)

    if capi.device_count() == 0:                                # every compute entry point says so, and leaves its outputs alone
        assert L.slslam_descriptor_matcher_insert(h, 2, f, C.byref(st), C.byref(kid)) == NO_DEVICE and (st.value, kid.value) == (-7, -7)
        assert run([ok]) == NO_DEVICE
        assert run([]) == NO_DEVICE
        assert L.slslam_match_descriptors(2, 1, f, 1, f, 1.5, 1.0, C.byref(r)) == NO_DEVICE and _untouched(r, b)
        m = capi.DescriptorMatcher(2, max_keyframes=2, max_descriptors=4, max_frames=1, max_candidates=1)
        for call in (lambda: m.insert(d[:2]), lambda: m.run([(d[:2], [-1])]), lambda: capi.match_descriptors(d[:2], d[:2])):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert m.size() == 0 and m.stats() == {"calls": 0, "allocations": 0}
        m.close()
    L.slslam_descriptor_matcher_destroy(h)


# ---- the place sequence: what the GPU end-to-end test relies on, on the reference alone
def shuffled_sequence():
    """SEQ's frames with the rows of every revisit frame in a shuffled order; perm[i][a] = the row of the first-pass keyframe's frame
    that row a of revisit frame i shows."""
    _, _, s = seq_inputs()
    frames, perms = list(s["frames"]), {}
    for i in range(s["first_pass"], len(frames)):
        perms[i] = np.random.default_rng(np.random.SeedSequence([15, i])).permutation(len(frames[i])).astype(np.int32)
        frames[i] = np.ascontiguousarray(frames[i][perms[i]])
    return s, frames, perms


def test_place_sequence_matches_on_the_reference():
    s, frames, perms = shuffled_sequence()
    total = wrong = 0
    neighbours = []
    least = 0.0
    for i, perm in perms.items():
        kf = int(s["place"][i])                                 # (first pass: keyframe id = place)
        r = R.match(frames[i], frames[kf], SEQ_RATIO, SEQ_MAX_DISTANCE)
        total += len(perm)
        wrong += int((r["match"] != perm).sum())
        least = min(least, float(r["best_distance"].min()))
        for nb in (kf - 1, kf + 1):
            neighbours.append(R.match(frames[i], frames[nb], SEQ_RATIO, SEQ_MAX_DISTANCE)["num_matched"])
    assert (total, wrong) == (450, 0)
    assert max(neighbours) <= 2
    assert -1e-6 < least < 0.25

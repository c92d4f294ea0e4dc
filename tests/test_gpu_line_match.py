"""GPU tests: the line matcher (slslam_line_matcher_*, slslam_match_lines; csrc/line_match.h) against its numpy reference
(tests/line_match_reference.py, which tests/test_line_match_cpu.py pins to the oracle's ransac_score) and against the oracle itself.

best_error and second_error are compared bit for bit and every integer output exactly: the kernel evaluates the reference's float / double
mix without contraction, and the reductions are minima and counts.  With extents a pair's decision also hangs on the interval [lo, hi] of
the segment contract, which the device reproduces to 1e-9 (tests/test_gpu_lba_segments.py), not to the bit: every test with extents asserts
on the CPU reference that no decision lies within 1e-6 of its boundary - a property of the input."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_match_reference as M  # noqa: E402
from test_line_match_cpu import END_TO_END_SEED, oracle_pairs  # noqa: E402

pytestmark = pytest.mark.gpu

THR = 5.0 / 406.05
TILE = M.TILE
INT_KEYS = ("match", "best_line", "num_admissible", "best_observation")


def same(got, ref):
    assert got["status"] == ref["status"], (got["status"], ref["status"])
    assert got["num_matched"] == ref["num_matched"]
    for k in INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    for k in ("best_error", "second_error"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k


def clear_of_boundary(ref):
    g = ref["gap"][np.isfinite(ref["gap"])]
    assert g.size == 0 or g.min() >= 1e-6, g.min()


def same_bytes(a, b):
    assert a["status"] == b["status"] and a["num_matched"] == b["num_matched"]
    for k in INT_KEYS + ("best_error", "second_error"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- shapes: the edges of a wave (observations) and of the LDS line tile
@pytest.mark.parametrize("L", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("K", [1, 63, 64, 65])
def test_shapes(hip, oracle, K, L):
    fr = M.make_frame(7000 + 10 * K + L, K, L, extents=True)
    plain = {k: v for k, v in fr.items() if k != "extents"}
    ref = M.match(plain)
    got = hip.match_lines(plain)
    same(got, ref)
    assert np.array_equal(got["num_admissible"], oracle_pairs(oracle, plain, THR).sum(axis=1))
    if min(K, L) >= 63:
        assert ref["num_matched"] >= min(K, L) // 4                        # (the case is not an empty one)
    refx = M.match(fr, margin=0.05)
    clear_of_boundary(refx)
    same(hip.match_lines(fr, margin=0.05), refx)


def test_admissible_set_is_the_oracles(hip, oracle):
    """Every pair on its own: one frame per map line, so that num_admissible is the pair's bit"""
    fr = M.make_frame(7100, 65, TILE + 1)
    bits = oracle_pairs(oracle, fr, THR)
    m = hip.LineMatcher(max_frames=TILE + 1, max_observations=65, max_lines=1)
    got = m.run([dict(pose=fr["pose"], observations=fr["observations"], lines=fr["lines"][l:l + 1]) for l in range(TILE + 1)])
    m.close()
    assert bits.sum() >= 40
    assert np.array_equal(np.stack([g["num_admissible"] for g in got], axis=1).astype(bool), bits)
    for thr in (1e-3, 0.05):                                               # (and the whole frame at other thresholds)
        assert np.array_equal(hip.match_lines(fr, error_thr=thr)["num_admissible"], oracle_pairs(oracle, fr, thr).sum(axis=1))


def mixed_frames():
    bad = M.make_frame(7203, 30, 70)
    bad["pose"] = bad["pose"].copy()
    bad["pose"][7] = np.inf
    e1, e2 = M.make_frame(7201, 0, 10), M.make_frame(7202, 10, 0)
    return [M.make_frame(7200, 65, 3 * TILE + 5), e1, e2, bad, M.make_frame(7204, 64, 64, extents=True)]


def test_mixed_frames_in_one_call(hip):
    frames = mixed_frames()
    m = hip.LineMatcher(max_frames=5, max_observations=65, max_lines=3 * TILE + 5)
    got = m.run(frames, margin=0.05)
    m.close()
    assert [g["status"] for g in got] == ["OK", "EMPTY", "EMPTY", "INVALID_POSE", "OK"]
    for fr, g in zip(frames, got):
        ref = M.match(fr, margin=0.05)
        clear_of_boundary(ref)
        same(g, ref)
    assert got[0]["num_matched"] > 30 and got[4]["num_matched"] > 30
    assert (got[3]["best_line"] == -1).all() and np.isinf(got[3]["second_error"]).all() and (got[3]["best_observation"] == -1).all()


# ---- ties
def test_ties_go_to_the_lowest_index(hip):
    fr = M.make_frame(7300, 6, 6, rot_sigma=0.0, t_sigma=0.0)
    fr["observations"] = fr["pair"]["obs1"][:6].copy()
    twice = dict(fr, lines=np.concatenate([fr["lines"][:1], fr["lines"]]))          # line 0 again at index 1
    for ratio in (1.5, 1.0, 0.0):
        got = hip.match_lines(twice, ratio=ratio)
        same(got, M.match(twice, ratio=ratio))
        assert got["best_line"][0] == 0 and got["num_admissible"][0] >= 2
        assert got["second_error"][0].tobytes() == got["best_error"][0].tobytes() and got["best_error"][0] > 0
        assert got["match"][0] == (-1 if ratio > 1 else 0)
    two = dict(fr, observations=np.concatenate([fr["observations"][:1]] * 2), lines=fr["lines"][:1])
    got = hip.match_lines(two, ratio=1.0)
    same(got, M.match(two, ratio=1.0))
    assert got["best_observation"][0] == 0 and list(got["match"]) == [0, -1] and list(got["best_line"]) == [0, 0]


# ---- lines behind the camera, observations of zero length
def test_behind_and_zero_length(hip):
    pose = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    B = 0.12

    def project(P):
        return np.array([P[0] / P[2], P[1] / P[2]]), np.array([(P[0] - B) / P[2], P[1] / P[2]])

    def observe(P, Q):
        (pl, pr), (ql, qr) = project(P), project(Q)
        return np.concatenate([pl, ql, pr, qr])

    lines = np.array([[0.0, 0.5, -5.0, 1.0, 0.0, 0.0],          # behind the camera
                      [0.0, 0.5, 5.0, 1.0, 0.0, 0.0]])          # in front
    obs = np.stack([observe(np.array([-1.0, 0.5, -5.0]), np.array([1.0, 0.5, -5.0])),          # the line behind, as reprojection_error sees it
                    observe(np.array([-1.0, 0.5, 5.0]), np.array([1.0, 0.5, 5.0])),
                    observe(np.array([0.3, 0.5, 5.0]), np.array([0.3, 0.5, 5.0]))])            # zero length, on the line in front
    fr = dict(pose=pose, observations=obs, lines=lines)
    got = hip.match_lines(fr, ratio=1.0)
    ref = M.match(fr, ratio=1.0)
    same(got, ref)
    assert list(got["best_line"]) == [0, 1, 1]                  # without extents: what reprojection_error says
    frx = dict(fr, extents=np.array([[-10.0, 10.0], [-10.0, 10.0]]))
    gotx = hip.match_lines(frx, ratio=1.0)
    refx = M.match(frx, ratio=1.0)
    clear_of_boundary(refx)
    same(gotx, refx)
    assert M.interval(pose, obs[0, :4], lines[0])[0] == M.S.BEHIND and M.interval(pose, obs[2, :4], lines[1])[0] == M.S.DEGENERATE
    assert list(gotx["best_line"]) == [-1, 1, -1] and list(gotx["match"]) == [-1, 1, -1]
    assert list(gotx["num_admissible"]) == [0, 1, 0] and list(gotx["best_observation"]) == [-1, 1]
    # a line without a segment (t_min > t_max) and a NaN extent admit nothing
    for ext in ([[-10.0, 10.0], [np.inf, -np.inf]], [[-10.0, 10.0], [np.nan, 10.0]]):
        assert list(hip.match_lines(dict(fr, extents=np.array(ext)), ratio=1.0)["best_line"]) == [-1, -1, -1]


# ---- extents from a solved window
def test_extents_of_a_solved_window(hip):
    w = synth.make_window(31, num_lines=40, num_kf=4, num_free=2)
    x, s, _ = hip.lba_solve(w)
    seg = hip.lba_segments(w, params=x)
    C, Lw = int(w["num_cameras"]), int(w["num_lines"])
    lines = synth.orth_to_av(x[6 * C:6 * C + 4 * Lw].reshape(Lw, 4))
    ok = seg["status"] == hip.SEGMENT_OK
    ext = np.where(ok[:, None], np.stack([seg["t_min"], seg["t_max"]], axis=1), np.array([np.inf, -np.inf]))
    # a camera and a line it saw, the line's segment wholly in front of it
    cam, ln = None, None
    for i in np.nonzero(seg["obs_status"] == hip.SEGMENT_OBS_USED)[0]:
        c, l = int(w["camera_index"][i]), int(w["line_index"][i])
        R, t = synth.wt_to_rt(x[6 * c:6 * c + 6])
        z = [(R @ (lines[l, :3] + v * lines[l, 3:]) + t)[2] for v in (ext[l, 0] - 3.0, ext[l, 1] + 3.0)]
        if ok[l] and min(z) > 1.0:
            cam, ln = (R, t), l
            break
    assert cam is not None
    R, t = cam
    pose = np.concatenate([R.reshape(-1), t])
    margin, length, B = 0.25, 0.5, 0.12
    a, b = ext[ln, 0] - margin, ext[ln, 1] + margin

    def observe(s0):                                             # the exact stereo projection of [s0, s0 + length] of the line
        o = []
        for off in (0.0, B):
            for v in (s0, s0 + length):
                P = R @ (lines[ln, :3] + v * lines[ln, 3:]) + t
                o += [(P[0] - off) / P[2], P[1] / P[2]]
        return np.array(o)

    # sliding up: [s0, s0 + length] leaves [a, b] when s0 passes b; sliding down: when s0 + length passes a
    inside = [0.5 * (a + b) - 0.5 * length, b - 1e-2, b - 1e-5, a - length + 1e-5, a - length + 1e-2]
    outside = [b + 1e-5, b + 1e-2, b + 1.0, a - length - 1e-5, a - length - 1e-2, a - length - 1.0]
    obs = np.stack([observe(v) for v in inside + outside])
    fr = dict(pose=pose, observations=obs, lines=lines, extents=ext)
    ref = M.match(fr, ratio=1.0, margin=margin)
    # on the CPU reference: every slid observation cuts a USED interval whose decision is at least 1e-6 from its boundary, at an error
    # far below the threshold
    assert (ref["errors"][:, ln] < 1e-6).all()
    for k in range(len(obs)):
        st, lo, hi = M.interval(pose, obs[k, :4], lines[ln])
        assert st == M.S.USED and np.isfinite(ref["gap"][k, ln]) and ref["gap"][k, ln] >= 1e-6
    clear_of_boundary(ref)
    assert ref["admissible"][:len(inside), ln].all() and not ref["admissible"][len(inside):, ln].any()
    got = hip.match_lines(fr, ratio=1.0, margin=margin)
    same(got, ref)
    assert (got["best_line"][:len(inside)] == ln).all() and (got["best_line"][len(inside):] != ln).all()
    # without extents every position is admissible: the error alone does not see where along the line the segment lies
    assert (hip.match_lines(dict(pose=pose, observations=obs, lines=lines), ratio=1.0)["best_line"] == ln).all()


# ---- a frame's bytes do not depend on the call
def test_independent_of_the_call(hip):
    fr = M.make_frame(7400, 65, 3 * TILE + 5, extents=True)
    others = [M.make_frame(7401 + i, k, l, extents=bool(i & 1)) for i, (k, l) in enumerate([(64, 64), (1, 200), (130, 7), (63, 65), (5, 5), (65, 1), (40, 90)])]
    m = hip.LineMatcher(max_frames=8, max_observations=130, max_lines=200)
    alone = m.run([fr], margin=0.05)[0]
    among = m.run(others[:5] + [fr] + others[5:], margin=0.05)[5]
    m.close()
    same_bytes(alone, among)
    same_bytes(alone, hip.match_lines(fr, margin=0.05))
    assert alone["num_matched"] > 30


# ---- buffers persist
def test_reuse_and_growth(hip):
    a = [M.make_frame(7500 + i, 60, 64) for i in range(2)]
    m = hip.LineMatcher(max_frames=2, max_observations=64, max_lines=64)
    assert m.stats() == {"calls": 0, "allocations": 0}
    r1 = m.run(a)
    assert m.stats() == {"calls": 1, "allocations": 1}
    r2 = m.run(list(reversed(a)))
    assert m.stats() == {"calls": 2, "allocations": 1}
    r3 = m.run(a + [M.make_frame(7510 + i, 64, 64) for i in range(3)])
    assert m.stats() == {"calls": 3, "allocations": 2}
    r4 = m.run(a)
    assert m.stats() == {"calls": 4, "allocations": 2}
    m.close()
    for x, y in ((r1[0], r2[1]), (r1[1], r2[0]), (r1[0], r3[0]), (r1[1], r4[1])):
        same_bytes(x, y)
    with pytest.raises(hip.SlslamError) as ei:
        hip.LineMatcher(max_frames=2, max_observations=64, max_lines=64).run([M.make_frame(7520, 65, 64)])
    assert ei.value.status == 1


# ---- end to end: shuffled observations -> matches -> the pose of the id-paired call
def test_end_to_end_recovers_the_pairing(hip):
    fr = M.make_frame(END_TO_END_SEED, 150, 150)
    ref = M.match(fr)
    found = ref["match"] >= 0
    assert found.mean() >= 0.9                                   # (the condition on the input: tests/test_line_match_cpu.py)
    got = hip.match_lines(fr)
    same(got, ref)
    assert np.array_equal(got["match"][found], fr["perm"][found])
    tr = hip.matched_trials(fr, got, fr["obs0"], num_trials=1001)
    ids = fr["perm"][got["match"] >= 0]                          # the same pairs by landmark id
    pair = fr["pair"]
    by_id = dict(obs0=pair["obs0"][ids], obs1=pair["obs1"][ids], lines=pair["lines"][ids], samples=tr["samples"])
    est = hip.PoseEstimator(max_frames=2, max_lines=150)
    a, b = est.run([{k: tr[k] for k in ("obs0", "obs1", "lines", "samples")}, by_id])
    est.close()
    assert a["status"] == "OK" and b["status"] == "OK"
    assert np.abs(a["pose"] - b["pose"]).max() < 1e-10           # (tests/test_gpu_pose_estimator.py: _same_frame)
    assert a["num_inliers"] == b["num_inliers"] and np.array_equal(a["mask"], b["mask"])

"""The line tracker without a device: the numpy contract (tests/line_track_reference.py) at the edges of every gate term, the id rule,
the inputs of tests/test_gpu_line_track.py with their references (made once, shared, never written to), the C ABI's argument checks,
and the host half (csrc/line_track_layout.h) as a stand-alone program under ASan and UBSan against numpy, bit for bit."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_track_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NO_DEVICE = 1, 2
f32 = np.float32
W = 64                                   # kScanWidth of csrc/line_track_layout.h: frames the prefix sum takes per pass


def unit(D, *hot):
    """A descriptor [D]: 1 at the first given index, or the given (index, value) pairs."""
    d = np.zeros(D, f32)
    for h in hot:
        i, v = h if isinstance(h, tuple) else (h, 1.0)
        d[i] = v
    return d


def two(row, col, rd=None, cd=None, predict=None, **opt):
    """One row segment against one carried column segment; the row's result."""
    rd = unit(8, 0) if rd is None else rd
    cd = unit(8, 0) if cd is None else cd
    out = R.Tracker().run([(np.array([col], f32), cd[None]), (np.array([row], f32), rd[None], predict)], **opt)
    return out[1]


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


A128 = [0, 0, 128, 0]


def admitted(r):
    return r["num_admissible"][0] == 1 and r["segment_status"] == ["CONTINUED"] and r["id"][0] == 0 and r["age"][0] == 2


def refused(r):
    return r["num_admissible"][0] == 0 and r["segment_status"] == ["NEW"] and r["id"][0] == 1 and r["age"][0] == 1


# ---- every gate term at equality and one float step outside
def test_shift_at_equality_and_one_step_outside():
    assert admitted(two(A128, [40, 0, 168, 0]))                                    # midpoints 40 px apart
    assert refused(two(A128, [40, 0, up(168), 0]))
    assert admitted(two(A128, [40, 0, up(168), 0], max_shift=40.001))


def test_offset_at_equality_and_one_step_outside():
    assert admitted(two(A128, [0, 12, 128, 12]))                                   # 12 px beside the line, both ways
    assert refused(two(A128, [0, up(12), 128, up(12)]))
    assert admitted(two([0, 12, 128, 12], A128)) and refused(two([0, up(12), 128, up(12)], A128))
    # the two directions are separate tests: a short row beside the far end of a long, slightly turned column
    o = dict(max_tan2=1.0, max_shift=1000.0, min_overlap=0.0)
    assert admitted(two([100, 12, 110, 12], [0, 0, 200, 0], **o)) and refused(two([100, up(12), 110, up(12)], [0, 0, 200, 0], **o))


def test_direction_at_equality_and_one_step_outside():
    o = dict(max_tan2=0.25, max_offset=40.0)
    assert admitted(two(A128, [0, 0, 128, 64], **o))                               # tan = 0.5
    assert refused(two(A128, [0, 0, 128, up(64)], **o))
    assert admitted(two(A128, [128, 64, 0, 0], **o))                               # the end points' order does not matter
    assert refused(two(A128, [0, 0, 0, 128], max_tan2=1e300, max_offset=1000.0))   # dot = 0


def test_overlap_at_equality_and_one_step_outside():
    o = dict(max_shift=100.0)
    assert admitted(two(A128, [64, 0, 192, 0], **o))                               # half of a
    assert refused(two(A128, [up(64), 0, 192, 0], **o))
    assert admitted(two(A128, [192, 0, 64, 0], **o))
    assert refused(two(A128, [128, 0, 256, 0], max_shift=1000.0, min_overlap=0.0))  # touching: o = 0


def test_length_and_distance_thresholds():
    assert admitted(two([0, 0, 8, 0], [0, 0, 8, 0]))                               # len2 = 64 is not below 64
    r = two([0, 0, 7.999, 0], [0, 0, 8, 0])
    assert r["segment_status"] == ["SHORT"] and r["id"][0] == -1 and r["age"][0] == 0 and r["num_admissible"][0] == 0
    r = two([0, 0, 8, 0], [0, 0, 7.999, 0])                                        # a short column is nobody's partner
    assert r["num_admissible"][0] == 0 and r["segment_status"] == ["NEW"] and r["id"][0] == 0
    # r = 1 - 0.75 = 0.25 is not below max_distance; one step more alike is
    assert two(A128, A128, cd=unit(8, (0, 0.75)))["num_admissible"][0] == 0
    assert admitted(two(A128, A128, cd=unit(8, (0, up(0.75)))))


def test_predict_moves_a_pair_in_and_out_of_the_gate():
    far = [300, 200, 428, 200]
    assert refused(two(A128, far))
    assert admitted(two(A128, far, predict=[1, 0, -300, 0, 1, -200]))
    assert refused(two(A128, A128, predict=[1, 0, 41, 0, 1, 0])) and admitted(two(A128, A128, predict=[1, 0, 40, 0, 1, 0]))
    # a quarter turn: x' = -y, y' = x
    assert admitted(two(A128, [0, 0, 0, -128], predict=[0, -1, 0, 1, 0, 0]))
    # the short test is of the segment in its own frame, the gate of the warped one
    assert two(A128, [0, 0, 4, 0], predict=[32, 0, 0, 0, 1, 0], max_shift=1000)["num_admissible"][0] == 0


def test_invalid_and_short_segments_get_no_id_and_are_nobodys_partner():
    nan = float("nan")
    seg0 = np.array([A128, A128, [0, 0, 3, 0]], f32)
    d0 = np.stack([unit(8, 0), unit(8, 0), unit(8, 0)])
    d0[1, 5] = nan
    t = R.Tracker()
    a = t.run([(seg0, d0)])[0]
    assert a["segment_status"] == ["NEW", "INVALID", "SHORT"] and a["id"].tolist() == [0, -1, -1] and a["age"].tolist() == [1, 0, 0]
    seg1 = np.array([[0, 0, 3, 0], [nan, 0, 128, 0], A128], f32)
    b = t.run([(seg1, np.stack([unit(8, 0)] * 3))])[0]
    assert b["segment_status"] == ["SHORT", "INVALID", "CONTINUED"] and b["id"].tolist() == [-1, -1, 0] and b["age"].tolist() == [0, 0, 2]
    assert b["best_row"].tolist() == [2, -1, -1] and b["num_admissible"].tolist() == [0, 0, 1]
    # a carried segment that got no id stays nobody's partner when the next run would no longer call it short
    c = t.run([(np.array([[0, 0, 3, 0]], f32), unit(8, 0)[None])], min_length=1.0)[0]
    assert c["segment_status"] == ["NEW"] and c["num_admissible"].tolist() == [0] and c["id"].tolist() == [1]


def test_ties_take_the_lowest_index_and_fail_the_ratio_test():
    cols = (np.array([A128, A128], f32), np.stack([unit(8, (0, 0.9)), unit(8, (0, 0.9))]))
    r = R.Tracker().run([cols, (np.array([A128], f32), unit(8, 0)[None])])[1]
    assert r["best"].tolist() == [0] and r["best_distance"][0] == r["second_distance"][0] and r["match"].tolist() == [-1]
    assert r["best_row"].tolist() == [0, 0] and r["segment_status"] == ["NEW"]
    r = R.Tracker().run([cols, (np.array([A128], f32), unit(8, 0)[None])], ratio=1.0)[1]
    assert r["match"].tolist() == [0] and r["id"].tolist() == [0]
    # two equal rows for one column: the lowest row is its best row, the other stays NEW
    rows = (np.array([A128, A128], f32), np.stack([unit(8, 0), unit(8, 0)]))
    r = R.Tracker().run([(np.array([A128], f32), unit(8, 0)[None]), rows])[1]
    assert r["best_row"].tolist() == [0] and r["match"].tolist() == [0, -1] and r["id"].tolist() == [0, 1]


# ---- the id rule
def moving(seed, T, n, D=8, drop=0.0, empty=(), born=None):
    """T frames of up to n tracks that move about a pixel a frame, each with a descriptor of its own; a track is absent from a frame with
    probability `drop`; frames in `empty` have no segments; born: {track: first frame}.  Rows are shuffled.  Returns (frames, labels)."""
    rng = np.random.default_rng(seed)
    base = np.zeros((n, 4))
    base[:, 0], base[:, 1] = rng.uniform(40, 400, n), 60.0 * np.arange(n) + rng.uniform(0, 10, n)
    ang = rng.uniform(-0.4, 0.4, n)
    base[:, 2], base[:, 3] = base[:, 0] + 60 * np.cos(ang), base[:, 1] + 60 * np.sin(ang)
    desc = rng.normal(size=(n, D))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(f32)
    frames, labels = [], []
    for t in range(T):
        here = [k for k in range(n) if t not in empty and rng.uniform() >= drop and t >= (born or {}).get(k, 0)]
        here = list(rng.permutation(here)) if len(here) else []
        seg = np.array([base[k] + np.tile([0.9 * t, 0.4 * t], 2) for k in here], f32).reshape(-1, 4)
        frames.append((seg, desc[here].reshape(-1, D)))
        labels.append([int(k) for k in here])
    return frames, labels


def test_fresh_ids_ascend_and_ages_count_and_an_empty_frame_ends_all_tracks():
    frames, labels = moving(3, 7, 5, empty=(4,))
    out = R.Tracker(next_id=100).run(frames)
    assert out[0]["id"].tolist() == [100, 101, 102, 103, 104] and out[0]["segment_status"] == ["NEW"] * 5
    by = dict(zip(labels[0], out[0]["id"].tolist()))
    for t in (1, 2, 3):
        assert [by[k] for k in labels[t]] == out[t]["id"].tolist() and out[t]["age"].tolist() == [t + 1] * 5
    assert out[4]["status"] == "EMPTY" and out[4]["num_new"] == 0
    assert out[5]["status"] == "EMPTY" and out[5]["id"].tolist() == [105, 106, 107, 108, 109] and out[5]["age"].tolist() == [1] * 5
    assert out[6]["age"].tolist() == [2] * 5 and sorted(out[6]["id"].tolist()) == [105, 106, 107, 108, 109]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), k
            else:
                assert x[k] == y[k], k


def test_any_cut_of_a_sequence_gives_equal_outputs_and_reset_works():
    frames, _ = moving(5, 9, 12, drop=0.2)
    t = R.Tracker()
    whole = t.run(frames)
    assert sum(o["num_continued"] for o in whole) > 40 and sum(o["num_new"] for o in whole[1:]) > 5
    for cut in ([1] * 9, [4, 5], [2, 0, 6, 1]):
        u, got, at = R.Tracker(), [], 0
        for c in cut:
            got += u.run(frames[at:at + c])
            at += c
        same(got, whole)
        assert u.state() == t.state()
    t.reset(7)
    assert t.state() == {"next_id": 7, "carried_segments": 0}
    again = t.run(frames)
    assert [(o["id"][o["id"] >= 0] - 7).tolist() for o in again] == [o["id"][o["id"] >= 0].tolist() for o in whole]
    t.reset(R.INT_MAX - 3)
    assert t.run(frames[:1]) is None and t.state() == {"next_id": R.INT_MAX - 3, "carried_segments": 0}


# ---- the inputs of the GPU tests.  An input: dict(runs: lists of frames, run one after the other on one tracker; options)
def pair_frames(seed, n, m, D, noise=(0.05, 0.3), far=0):
    """A carried frame of m segments and a frame of n: most rows continue a column (moved a few pixels, the descriptor disturbed), some
    columns have a near twin (for the ratio test), the rest is unrelated.  far > 0: every column but the given ones is moved far away."""
    rng = np.random.default_rng(seed)

    def segs(k):
        c = np.stack([rng.uniform(60, 580, k), rng.uniform(60, 420, k)], axis=1)
        a, h = rng.uniform(0, np.pi, k), rng.uniform(12, 45, k)
        d = np.stack([h * np.cos(a), h * np.sin(a)], axis=1)
        return np.concatenate([c - d, c + d], axis=1)

    def descs(k):
        v = rng.normal(size=(k, D))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    cs, cd = segs(m), descs(m)
    for j in range(1, m, 7):                                     # twins
        cs[j] = cs[j - 1] + np.tile(rng.normal(0, 2.0, 2), 2)
        v = cd[j - 1] + rng.uniform(*noise) * descs(1)[0]
        cd[j] = v / np.linalg.norm(v)
    rs, rd = segs(n), descs(n)
    src = rng.permutation(m)[:min(n, m)]
    for a, j in enumerate(src):
        if rng.uniform() < 0.8:
            rs[a] = cs[j] + np.tile(rng.normal(0, 2.0, 2), 2) + rng.normal(0, 0.5, 4)
            if rng.uniform() < 0.3:
                rs[a] = rs[a][[2, 3, 0, 1]]
            v = cd[j] + rng.uniform(0.02, 0.12) * descs(1)[0]
            rd[a] = v / np.linalg.norm(v)
    p = rng.permutation(n)
    return [(cs.astype(f32), cd.astype(f32))], [(rs[p].astype(f32), rd[p].astype(f32))]


SIZES = (0, 1, 63, 64, 65, 129)
SIZE_CASES = [(n, m, 8) for n in SIZES for m in SIZES] + [(65, m, D) for m in (7, 8, 9) for D in (8, 72, 128)] + [(512, 512, 128)]
CHAIN_T = (1, 2, 3, W - 1, W, W + 1, 2 * W + 1)
SKIP_PAIRS = {5: 3, 66: 20}             # row: column of the two pairs the skip input leaves


def chain(T, empty=()):
    """A carried frame, then a run of T frames of at most 3 segments: track 0 started in the carried frame and lives through all
    frames (unless one is empty), track 1 is born in the middle, track 2 is missing from every other frame and NEW in the next."""
    frames, labels = moving(100 + T, T + 1, 3, drop=0.0, empty=tuple(e + 1 for e in empty), born={1: 1 + T // 2})
    keep = [[k for k in lab if k != 2 or t % 2 == 1 or t == 0] for t, lab in enumerate(labels)]    # (NEW in every other frame)
    frames = [(s[[i for i, k in enumerate(lab) if k in kp]], d[[i for i, k in enumerate(lab) if k in kp]])
              for (s, d), lab, kp in zip(frames, labels, keep)]
    labels = [[k for k in lab if k in kp] for lab, kp in zip(labels, keep)]
    return dict(runs=[frames[:1], frames[1:]], options={}, labels=labels)


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    inputs = {}
    for i, (n, m, D) in enumerate(SIZE_CASES):
        c, r = pair_frames(1000 + i, n, m, D)
        inputs["size_%d_%d_%d" % (n, m, D)] = dict(runs=[c, r], options={})
    # all but two groups gated out: the columns lie far from every row but for two pairs, in groups 0 and 2
    c, r = pair_frames(7, 70, 70, 72)
    cs, cd = c[0][0] + f32(2000.0), c[0][1]
    rs, rd = r[0]
    for a, j in SKIP_PAIRS.items():
        cs[j], cd[j] = rs[a] + f32(1.5), rd[a]
    inputs["skip"] = dict(runs=[[(cs, cd)], r], options={})
    inputs["gated_out"] = dict(runs=[[(c[0][0] + f32(2000.0), c[0][1])], r], options={})
    # every status: a NaN end point, a NaN descriptor value and short segments on both sides
    c, r = pair_frames(11, 40, 40, 8)
    (cs, cd), (rs, rd) = c[0], r[0]
    rs[3, 1] = np.nan; rd[9, 4] = np.inf; rs[12] = [10, 10, 13, 11]; cs[0, 2] = np.nan; cd[5, 0] = np.nan; cs[8] = [50, 50, 52, 50]
    inputs["every_status"] = dict(runs=[c, r], options={})
    # a predict that is not the identity: the carried frame lies turned by 4 degrees and moved by (70, -45) against the rows
    c, r = pair_frames(13, 65, 65, 72)
    th = np.deg2rad(4.0)
    Rm, tv = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]), np.array([70.0, -45.0])
    cs = c[0][0].astype(np.float64).reshape(-1, 2)
    cs = ((cs - tv) @ Rm).astype(f32).reshape(-1, 4)               # x = R^T (x' - t): predict maps it back
    pre = np.array([Rm[0, 0], Rm[0, 1], tv[0], Rm[1, 0], Rm[1, 1], tv[1]])
    inputs["predict"] = dict(runs=[[(cs, c[0][1])], [(r[0][0], r[0][1], pre)]], options={})
    inputs["predict_missing"] = dict(runs=[[(cs, c[0][1])], r], options={})
    for T in CHAIN_T:
        inputs["chain_%d" % T] = chain(T)
    inputs["chain_empty_%d" % (W + 1)] = chain(W + 1, empty=(W,))
    inputs["chain_empty_%d" % (2 * W + 1)] = chain(2 * W + 1, empty=(W + 6,))
    frames, _ = moving(5, 9, 12, D=72, drop=0.2)
    inputs["cut"] = dict(runs=[frames], options={})
    inputs["options"] = dict(runs=pair_frames(17, 65, 64, 8), options=dict(max_shift=6.0, max_offset=2.0, ratio=1.1, min_length=30.0))
    return inputs


BATCH = ("size_0_63_8", "size_129_65_8", "size_64_129_8")


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per run the list of per-frame results, and the state after the last run."""
    i = gpu_inputs()[name]
    t = R.Tracker()
    return [t.run(run, **i["options"]) for run in i["runs"]], t.state()


def groups_admitted(name):
    """The groups of eight columns of the input's last frame in which the gate admits anything, per wave of 64 rows."""
    i = gpu_inputs()[name]
    (cs, cd), fr = i["runs"][-2][-1], i["runs"][-1][-1]
    o = R.options(**i["options"])
    geo = R.gate(fr[0], cs, o, fr[2] if len(fr) > 2 else None)
    geo &= (R.segment_ok(fr[0], fr[1]) & ~R.is_short(fr[0], o))[:, None] & (R.segment_ok(cs, cd) & ~R.is_short(cs, o))[None, :]
    return [sorted({j // 8 for j in np.nonzero(geo[w:w + 64].any(axis=0))[0]}) for w in range(0, len(geo), 64)]


def test_the_gpu_inputs_are_what_their_tests_say():
    assert W == 64
    full = reference("size_512_512_128")[0][1][0]
    assert 63 in groups_admitted("size_512_512_128")[-1] and full["num_continued"] > 250 and full["num_new"] > 50
    assert (full["match"][full["match"] >= 0] >= 504).any()                         # a match in group 63
    assert groups_admitted("skip") == [[0], [2]]
    s = reference("skip")[0][1][0]
    assert s["num_continued"] == 2 and {a: int(s["match"][a]) for a in SKIP_PAIRS} == SKIP_PAIRS and s["num_admissible"].sum() == 2
    assert groups_admitted("gated_out") == [[], []] and reference("gated_out")[0][1][0]["num_new"] == 70
    for m in (7, 8, 9):
        g = groups_admitted("size_65_%d_72" % m)
        assert len(g) == 2 and max(max(x) for x in g if x) == (m - 1) // 8          # one group, one full group, a second of one column
    e = reference("every_status")[0][1][0]
    assert set(e["segment_status"]) == set(R.SEGMENT_STATUS) and (e["best_row"][[0, 5, 8]] == -1).all()
    p, q = reference("predict")[0][1][0], reference("predict_missing")[0][1][0]
    assert p["num_continued"] > 30 and q["num_continued"] == 0
    assert reference("options")[0][1][0]["segment_status"].count("SHORT") > 3
    for T in CHAIN_T:
        i, (runs, state) = gpu_inputs()["chain_%d" % T], reference("chain_%d" % T)
        out = runs[1]
        assert len(out) == T and max(len(f[0]) for f in i["runs"][1]) <= 3
        # track 0 started in the carried frame: its id is 0 in every frame, its age T + 1 in the last - a walk of T + 1 steps
        for t in range(T):
            a = i["labels"][t + 1].index(0)
            assert out[t]["id"][a] == runs[0][0]["id"][i["labels"][0].index(0)] and out[t]["age"][a] == t + 2
        if T >= 2:                                                                  # track 1 is born in the middle
            t0 = T // 2
            assert 1 not in i["labels"][t0] and out[t0]["segment_status"][i["labels"][t0 + 1].index(1)] == "NEW"
            born = out[t0]["id"][i["labels"][t0 + 1].index(1)]
            assert born not in runs[0][0]["id"].tolist() and out[T - 1]["id"][i["labels"][T].index(1)] == born
        if T > W:                                                                   # NEW segments on both sides of the first pass
            assert sum(o["num_new"] for o in out[:W]) > 0 and sum(o["num_new"] for o in out[W:]) > 0
    assert {T for T in CHAIN_T if T >= W - 1} == {W - 1, W, W + 1, 2 * W + 1}
    for T, e in ((W + 1, W), (2 * W + 1, W + 6)):
        out = reference("chain_empty_%d" % T)[0][1]
        assert e >= W and out[e]["status"] == "EMPTY" and len(out[e]["id"]) == 0
        assert out[e + 1 if e + 1 < T else e]["num_continued"] == 0 and (e + 1 >= T or out[e + 1]["num_new"] > 0)
    c = reference("cut")[0][0]
    assert len(c) == 9 and sum(o["num_continued"] for o in c) > 40


def test_no_decision_lies_near_its_threshold():
    """Neither a comparison of the gate nor the distance or ratio test of any GPU input lies within 1e-9 (relative) of its threshold:
    the device's bit-for-bit agreement does not hinge on a rounding."""
    def clear(v, t, reached):
        v, t = np.broadcast_arrays(np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.float64))
        look = reached & np.isfinite(v) & np.isfinite(t)
        return bool((np.abs(v - t)[look] > 1e-9 * np.maximum(np.abs(v), np.abs(t))[look]).all())
    for name, i in gpu_inputs().items():
        o = R.options(**i["options"])
        prev, (runs, _) = None, reference(name)
        frames = [f for run in i["runs"] for f in run]
        results = [r for run in runs for r in run]
        for fr, res in zip(frames, results):
            if prev is not None and len(prev[0]) and len(fr[0]):
                with np.errstate(all="ignore"):
                    for v, t, reached in R.gate(fr[0], prev[0], o, fr[2] if len(fr) > 2 else None, margins=True):
                        assert clear(v, t, reached), name
                    len2 = R.segments(R.warp(fr[0]))["len2"]
                    assert clear(len2, R.squares(o)["min_length2"], np.ones(len(len2), bool)), name
                    geo = R.gate(fr[0], prev[0], o, fr[2] if len(fr) > 2 else None)
                    r = R.DM.distances(fr[1], prev[1]).astype(np.float64)
                    assert clear(r, o["max_distance"], geo), name
                    has = np.isfinite(res["second_distance"])
                    assert clear(res["best_distance"].astype(np.float64) * o["ratio"], res["second_distance"].astype(np.float64), has), name
            prev = fr


# ---- the C ABI without a device
def _frame(n=3, m=2, D=8, **over):
    c, r = pair_frames(7, n, m, D)
    fr, res, keep, _ = capi._track_frame(r[0], m, D)
    for a in keep[3].values():
        a[...] = -7
    for k, v in over.items():
        setattr(fr, k, v)
    return fr, res, keep


def _untouched(res, keep):
    return all((a == -7).all() for a in keep[3].values()) and res.status == -1 and res.num_new == -1


def test_exports_and_defaults():
    for name in capi.EXPORTS:
        if "track" in name:
            assert hasattr(capi.lib(), name), name
    o = capi.line_track_options()
    assert {k: getattr(o, k) for k, _ in capi.LineTrackOptions._fields_} == R.DEFAULTS
    capi.lib().slslam_line_track_default_options(None)
    with pytest.raises(TypeError):
        capi.line_track_options(max_disp=3)
    assert capi.TRACK_SEGMENT_STATUS == dict(enumerate(R.SEGMENT_STATUS))


def test_arguments_and_no_device():
    L = capi.lib()
    h = C.c_void_p()
    for args in ((0, 1, 1), (4, 1, 1), (12, 1, 1), (136, 1, 1), (72, 0, 1), (72, 1, 0), (72, 1, 513), (72, -1, 8)):
        assert L.slslam_line_tracker_create(-1, *args, C.byref(h)) == INVALID_ARGUMENT, args
    assert L.slslam_line_tracker_create(-1, 72, 1, 1, None) == INVALID_ARGUMENT and not h
    assert L.slslam_line_tracker_create(-1, 8, 2, 4, C.byref(h)) == 0                            # touches no device
    good = capi.line_track_options()
    none_f = C.POINTER(C.c_float)()
    bad_predict = (C.c_double * 6)(1, 0, float("nan"), 0, 1, 0)
    for over in (dict(num_segments=-1), dict(num_segments=5), dict(segments=none_f), dict(descriptors=none_f),
                 dict(predict=C.cast(bad_predict, C.POINTER(C.c_double)))):
        fr, res, keep = _frame(**over)
        assert L.slslam_line_tracker_run(h, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        if over.get("num_segments") != 5:
            assert L.slslam_track_lines(8, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert _untouched(res, keep)
    fr, res, keep = _frame()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_tan2=-1.0), dict(max_tan2=nan), dict(max_shift=-1.0), dict(max_shift=inf), dict(max_offset=-0.5),
                dict(max_offset=nan), dict(min_overlap=1.5), dict(min_overlap=-0.5), dict(min_length=-1.0), dict(min_length=inf),
                dict(ratio=nan), dict(max_distance=nan)):
        o = capi.line_track_options(**bad)
        assert not R.options_valid(R.options(**bad))
        assert L.slslam_line_tracker_run(h, C.byref(o), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, bad
        assert L.slslam_track_lines(8, C.byref(o), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, bad
    assert R.options_valid(R.options(ratio=0.0, max_distance=inf, max_tan2=0.0, min_overlap=1.0))
    assert L.slslam_line_tracker_run(None, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_run(h, None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_run(h, C.byref(good), -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_run(h, C.byref(good), 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_run(h, C.byref(good), 1, C.byref(fr), None) == INVALID_ARGUMENT
    for D in (0, 12, 136):
        assert L.slslam_track_lines(D, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    # the state: reset, and a run whose ids would pass INT_MAX is refused before anything changes
    a, b = C.c_int(-1), C.c_int(-1)
    assert L.slslam_line_tracker_state(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert L.slslam_line_tracker_reset(h, -1) == INVALID_ARGUMENT and L.slslam_line_tracker_reset(None, 0) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_reset(h, R.INT_MAX - 2) == 0
    assert L.slslam_line_tracker_run(h, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT and _untouched(res, keep)
    assert L.slslam_line_tracker_state(h, C.byref(a), None) == 0 and a.value == R.INT_MAX - 2
    assert L.slslam_line_tracker_state(None, None, None) == INVALID_ARGUMENT
    assert L.slslam_line_tracker_reset(h, 5) == 0
    calls, allocs, ms = C.c_longlong(-1), C.c_longlong(-1), C.c_double(-1.0)
    assert L.slslam_line_tracker_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    assert L.slslam_line_tracker_timing(h, -1, C.byref(ms)) == 0 and ms.value == 0.0
    assert L.slslam_line_tracker_stats(None, None, None) == INVALID_ARGUMENT and L.slslam_line_tracker_timing(None, 0, None) == INVALID_ARGUMENT
    if capi.device_count() == 0:                                # every compute entry point says so, and leaves outputs and state alone
        assert L.slslam_line_tracker_run(h, C.byref(good), 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(res, keep)
        assert L.slslam_line_tracker_run(h, C.byref(good), 0, None, None) == NO_DEVICE
        assert L.slslam_track_lines(8, C.byref(good), 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(res, keep)
        assert L.slslam_line_tracker_state(h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (5, 0)
        c, r = pair_frames(7, 3, 2, 8)
        lt = capi.LineTracker(8, max_frames=1, max_segments=4)
        for call in (lambda: lt.run(r), lambda: capi.track_lines(c + r)):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert lt.stats() == {"calls": 0, "allocations": 0} and lt.state() == {"next_id": 0, "carried_segments": 0}
        lt.close()
    L.slslam_line_tracker_destroy(h)
    L.slslam_line_tracker_destroy(None)
    with pytest.raises(ValueError):
        capi._track_frame((np.zeros((2, 4)), np.zeros((2, 16))), 0, 8)
    with pytest.raises(TypeError):
        capi.LineTracker(8, max_disp=3)


# ---- the host half (csrc/line_track_layout.h) under the sanitizers, as a stand-alone program, against the numpy contract
def _layout(F, S, D):
    """The run's layout restated: regions one behind the other, each at a multiple of 256 bytes."""
    def carve(sizes):
        at, offs = 0, []
        for s in sizes:
            offs.append(at)
            at += (s + 255) // 256 * 256
        return offs, at
    (_, seg, ok, desc), in_bytes = carve([72 * F, 16 * S, 4 * S, 4 * S * D])
    _, match = carve([4 * F] + [4 * S] * 6)
    (_, status, ids, age, rank, new, before), out_bytes = carve([match] + [4 * S] * 4 + [4 * F, 4 * (F + 1)])
    keys = in_bytes
    out = keys + (8 * S + 255) // 256 * 256
    return dict(seg=seg, ok=ok, desc=desc, keys=keys, out=out, status=status, id=ids, age=age, rank=rank, new=new, before=before,
                out_bytes=out_bytes, host=in_bytes + out_bytes, dev=out + out_bytes, **{"in": in_bytes})


def test_host_half_under_the_sanitizers(tmp_path):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "line_track_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "line_track_layout_check.cpp"), "-o", exe])
    hx = lambda vs: " ".join(float(v).hex() for v in vs)        # noqa: E731
    lines, want = [], []

    def add(rows, cols, opt, predict=None):
        o = R.options(**opt)
        lines.append("gate " + hx([o[k] for k in ("max_tan2", "max_shift", "max_offset", "min_overlap", "min_length")]
                                  + list(R.IDENTITY if predict is None else predict)))
        geo, short = R.gate(rows, cols, o, predict), R.is_short(rows, o)
        for a in range(len(rows)):
            for b in range(len(cols)):
                if np.isfinite(rows[a]).all() and np.isfinite(cols[b]).all():
                    lines.append("pair " + hx(list(rows[a]) + list(cols[b])))
                    want.append("pair %d %d" % (geo[a, b], short[a]))
    for name in ("size_65_9_8", "skip", "every_status", "predict", "predict_missing", "options"):
        i = gpu_inputs()[name]
        fr = i["runs"][1][0]
        add(fr[0][:48], i["runs"][0][0][0][:48], i["options"], fr[2] if len(fr) > 2 else None)
    add(np.array([A128], f32), np.array([[40, 0, 168, 0], [40, 0, up(168), 0], [0, 12, 128, 12], [0, up(12), 128, up(12)], [64, 0, 192, 0],
                                         [up(64), 0, 192, 0], [128, 0, 256, 0]], f32), dict(max_shift=100.0))
    add(np.array([A128, [0, 0, 7.999, 0]], f32), np.array([[0, 0, 128, 64], [0, 0, 128, up(64)], [0, 0, 0, 128]], f32),
        dict(max_tan2=0.25, max_offset=40.0))
    # the id rule: every frame of a few inputs as one run after their first, the statuses and matches of the reference given
    ids_want = []
    for name in ("chain_3", "chain_%d" % (W + 1), "chain_empty_%d" % (2 * W + 1), "cut", "every_status"):
        runs, _ = reference(name)
        flat = [r for run in runs for r in run]
        first, rest = (flat[0], flat[1:]) if len(runs) > 1 else (None, flat)
        carried = [] if first is None else list(zip(first["id"].tolist(), first["age"].tolist()))
        next_id = 0 if first is None else first["num_new"]
        lines.append("ids %d %d %d" % (next_id, len(carried), len(rest)) + "".join(" %d %d" % c for c in carried))
        for r in rest:
            st = [R.SEGMENT_STATUS.index(s) for s in r["segment_status"]]
            lines.append("frame %d" % len(st) + "".join(" %d %d" % (s, m) for s, m in zip(st, r["match"].tolist())))
            ids_want.append("idage" + "".join(" %d %d" % (i, a) for i, a in zip(r["id"].tolist(), r["age"].tolist())))
    path = tmp_path / "pairs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "line track layout ok" in r.stdout
    got = [ln.strip() for ln in r.stdout.splitlines() if ln.startswith("pair ")]
    assert len(got) == len(want) > 5000 and got == want
    assert sum(1 for w in want if w.startswith("pair 1")) > 100
    got_ids = [ln.strip() for ln in r.stdout.splitlines() if ln.startswith("idage")]
    assert len(ids_want) > 200 and got_ids == ids_want
    layouts = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(layouts) == 4
    for t in layouts:
        F, S, D = (int(x) for x in t[1:4])
        assert dict(zip(t[4::2], (int(x) for x in t[5::2]))) == _layout(F, S, D), t

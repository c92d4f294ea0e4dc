"""The stereo line matcher without a device (include/slslam_hip.h: slslam_stereo_matcher_*, slslam_match_stereo): the gate pinned by hand
on written-down segments (every threshold at equality and one step outside, in values exactly representable in float and double), ties,
the end point swap, the normalisation against slslam_parse_frame_text, every argument check of the C ABI with untouched outputs,
SLSLAM_ERR_NO_DEVICE, the host half (csrc/stereo_match_layout.h: the functions the kernels call) against the numpy contract bit for
bit as a stand-alone program under ASan + UBSan, the accuracy the contract itself achieves on synth.make_stereo_line_pair, and the
measurements behind the GPU tests: the inputs of tests/test_gpu_stereo_match.py are made here (gpu_inputs), so that "no decision near
its threshold" and the longdouble figure are taken on exactly them."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_descriptor_reference as MSLD  # noqa: E402
import line_detect_reference as LSD  # noqa: E402
import stereo_match_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "slslam_amd", "_lib", "libslslam_host.so")
INVALID_ARGUMENT, NO_DEVICE = 1, 2
KITTI = dict(fx=406.05, fy=406.05, cx=327.783, cy=237.172)


def unit(D, *hot):
    """A descriptor of D floats with 1 / sqrt(len(hot)) at the given places: r of two equal ones is 0 up to rounding."""
    d = np.zeros(D, np.float32)
    d[list(hot)] = np.float32(1.0 / np.sqrt(len(hot)))
    return d


E0, E1, E2 = unit(8, 0), unit(8, 1), unit(8, 2)


def one(left, right, ld=None, rd=None, **opt):
    left, right = np.atleast_2d(np.array(left, np.float32)), np.atleast_2d(np.array(right, np.float32))
    ld = np.tile(E0, (len(left), 1)) if ld is None else ld
    rd = np.tile(E0, (len(right), 1)) if rd is None else rd
    return R.match(left, ld, right, rd, **opt)


# ---- the gate by hand.  Vertical left segment x = 100, rows 10 .. 50; defaults: disparity 0 .. 128, tan2 0.03, rows 3, overlap 0.5
LEFT = [100, 10, 100, 50]


def test_disparity_bounds_at_equality_and_one_step_outside():
    up, down = float(np.nextafter(np.float32(128), np.float32(0))), float(np.nextafter(np.float32(128), np.float32(999)))
    for xr, d, adm in ((100.0, 0.0, True), (100.0 - 128.0, 128.0, True), (float(np.nextafter(np.float32(100), np.float32(999))), None, False),
                       (100.0 - down, None, False), (100.0 - up, up, True), (60.0, 40.0, True)):
        m = one(LEFT, [xr, 10, xr, 50])
        assert (m["match"][0] == 0) == adm and m["num_admissible"][0] == int(adm), xr
        assert m["segment_status"] == [R.MATCHED if adm else R.UNMATCHED]
        if adm and d is not None:
            assert m["disparity"][0].tolist() == [d, d]
    # a min_disparity of its own
    assert one(LEFT, [96, 10, 96, 50], min_disparity=4.0)["match"][0] == 0
    assert one(LEFT, [96.5, 10, 96.5, 50], min_disparity=4.0)["match"][0] == -1


def test_direction_at_equality():
    # left (0, 40), right (dx, 40): cross^2 = 1600 dx^2, dot^2 = 1600^2: tan2 = dx^2 / 1600.  dx = 10: tan2 = 1 / 16, exact
    right = [90, 10, 100, 50]
    assert one(LEFT, right, max_tan2=0.0625)["match"][0] == 0
    assert one(LEFT, right, max_tan2=float(np.nextafter(0.0625, 0)))["match"][0] == -1
    # perpendicular-ish never passes: dot = 0 fails even at max_tan2 = 0 with cross = 0 impossible; a point-like right segment has dot 0
    assert one(LEFT, [90, 10, 90, 10], min_rows=0.0, max_tan2=1e30)["match"][0] == -1


def test_overlap_at_equality():
    # left rows 10 .. 50 (40), right rows 30 .. 70 (40): o = 20 = 0.5 * 40
    right = [90, 30, 90, 70]
    assert one(LEFT, right)["match"][0] == 0
    assert one(LEFT, right, min_overlap=0.5078125)["match"][0] == -1
    assert one(LEFT, [90, 30.5, 90, 70.5])["match"][0] == -1
    # touching rows: o = 0 is never enough, whatever min_overlap
    assert one(LEFT, [90, 50, 90, 90], min_overlap=0.0)["match"][0] == -1
    # the shorter extent counts: right rows 20 .. 30 lie inside the left ones
    assert one(LEFT, [90, 20, 90, 30])["match"][0] == 0


def test_flat_segments():
    m = one([[100, 10, 140, 12.5], LEFT], [[90, 10, 130, 12.5], [90, 10, 90, 50]])
    assert m["segment_status"] == [R.FLAT, R.MATCHED] and m["match"].tolist() == [-1, 1]
    assert m["num_admissible"].tolist() == [0, 1] and m["best_left"].tolist() == [-1, 1]      # the flat right one is nobody's
    assert np.isnan(m["observations"][0]).all() and np.isnan(m["disparity"][0]).all()
    # min_rows at equality: an extent of exactly 3 is enough
    assert one([100, 10, 100, 13], [90, 10, 90, 13])["segment_status"] == [R.MATCHED]
    assert one([100, 10, 100, 12.75], [90, 10, 90, 13])["segment_status"] == [R.FLAT]
    assert one([100, 10, 100, 13], [90, 10, 90, 12.75])["segment_status"] == [R.UNMATCHED]


def test_invalid_segments():
    ld = np.stack([E0, E0, E0])
    ld[1, 5] = np.nan
    m = one([[np.inf, 10, 100, 50], LEFT, LEFT], [[90, 10, 90, 50]], ld=ld)
    assert m["segment_status"] == [R.INVALID, R.INVALID, R.MATCHED] and m["match"].tolist() == [-1, -1, 0]
    rd = np.stack([E0, E0])
    rd[0, 0] = np.inf
    m = one([LEFT], [[90, 10, 90, 50], [80, 10, 80, np.nan]], rd=rd)
    assert m["segment_status"] == [R.UNMATCHED] and m["best_left"].tolist() == [-1, -1]


def test_swap_normalisation_and_slanted_disparity():
    # left from (100, 10) to (120, 50); the right line x = 80 + (y - 10) / 4 is given bottom-up, rows 2 .. 58: dot < 0 swaps its ends
    left, right = [100, 10, 120, 50], [92, 58, 78, 2]
    m = one(left, right, max_tan2=0.0625, **KITTI)
    assert m["match"][0] == 0
    # disparity at the rows of the left end points: x_right(10) = 92 + (10 - 58) / 4 = 80, x_right(50) = 90
    assert m["disparity"][0].tolist() == [20.0, 30.0]
    px = np.array(left + right[2:] + right[:2], dtype=np.float64)
    f, c = np.array([KITTI["fx"], KITTI["fy"]] * 4), np.array([KITTI["cx"], KITTI["cy"]] * 4)
    assert np.array_equal(m["observations"][0], px / f - c / f)
    # ... and without the swap when the right segment is given top-down
    m2 = one(left, right[2:] + right[:2], max_tan2=0.0625, **KITTI)
    assert np.array_equal(m2["observations"][0], m["observations"][0]) and np.array_equal(m2["disparity"][0], m["disparity"][0])
    # slslam_parse_frame_text (host/sequence_io.cpp: insert_curr_obs) makes the same eight doubles from the pixel values
    if not os.path.exists(HOST_LIB):
        import __graft_entry__
        __graft_entry__.build()
    H = C.CDLL(HOST_LIB)

    class Intr(C.Structure):
        _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]

    class Frame(C.Structure):
        _fields_ = [("num_lines", C.c_int), ("ids", C.POINTER(C.c_int)), ("observations", C.POINTER(C.c_double))]
    text = ("7 " + " ".join(repr(float(v)) for v in px) + "\n").encode()
    fr, K = Frame(), Intr(KITTI["fx"], KITTI["fy"], KITTI["cx"], KITTI["cy"])
    assert H.slslam_parse_frame_text(text, C.c_size_t(len(text)), C.byref(K), None, None, 0, C.byref(fr)) == 0 and fr.num_lines == 1
    assert [fr.observations[q] for q in range(8)] == m["observations"][0].tolist()
    H.slslam_free_frame(C.byref(fr))
    assert R.observations(m)[1].tolist() == [0] and np.array_equal(R.observations(m)[0][0], m["observations"][0])


def test_ties_take_the_lowest_index_and_fail_the_ratio_test():
    rights = [[90, 10, 90, 50], [80, 10, 80, 50]]
    half = np.stack([unit(8, 0, 1)] * 2)                           # two identical right descriptors, both admissible: r = 1 - sqrt(1 / 2)
    m = one([LEFT], rights, rd=half, max_distance=0.5)
    assert m["num_admissible"][0] == 2 and m["best"][0] == 0 and 0.29 < m["best_distance"][0] == m["second_distance"][0] < 0.3
    assert m["match"][0] == -1 and m["segment_status"] == [R.UNMATCHED]
    assert one([LEFT], rights, rd=half, max_distance=0.5, ratio=1.0)["match"][0] == 0    # ratio <= 1: no test; the lower index still wins
    # two identical left segments: the lower one is the right segment's best
    m = one([LEFT, LEFT], rights[:1])
    assert m["best_left"].tolist() == [0] and m["match"].tolist() == [0, -1]
    # max_distance is exclusive: r = 1 for orthogonal descriptors
    assert one([LEFT], rights[:1], rd=np.stack([E1]), max_distance=1.0)["match"][0] == -1
    assert one([LEFT], rights[:1], rd=np.stack([E1]), max_distance=1.0000001)["match"][0] == 0
    e = one(np.zeros((0, 4)), rights, ld=np.zeros((0, 8)))
    assert e["status"] == R.EMPTY and e["best_left"].tolist() == [-1, -1]
    assert one([LEFT], np.zeros((0, 4)), rd=np.zeros((0, 8)))["status"] == R.EMPTY


# ---- the inputs of the GPU tests
def stereo_frame(seed, n, m, D, common=None, disparity=(2.0, 100.0), noise=0.05, flip=0.3, jitter=0.0):
    """Random segments of a 752 x 480 image pair: `common` features seen by both (same rows, x_right = x_left - d per end point, some
    right ones with their end points in the other order), the rest unrelated; unit descriptors, the right one of a common feature the
    left one plus noise; both lists shuffled.  jitter: the common right segments' end points are moved along their
    line by up to that many pixels, as the end points of a detection are, so that the two segments' rows differ."""
    rng = np.random.default_rng(np.random.SeedSequence([19, int(seed)]))
    k = min(n, m) if common is None else common

    def segs(cnt):
        c = np.stack([rng.uniform(150, 700, cnt), rng.uniform(50, 430, cnt)], axis=1)
        th, half = rng.uniform(0, 2 * np.pi, cnt), 0.5 * rng.uniform(12, 90, cnt)
        h = half[:, None] * np.stack([np.cos(th), np.sin(th)], axis=1)
        return np.concatenate([c - h, c + h], axis=1)

    def descs(cnt):
        d = rng.standard_normal((cnt, D))
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    left, ld = segs(n), descs(n)
    right, rd = segs(m), descs(m)
    base = rng.uniform(disparity[0] + 2, disparity[1] - 2, k)
    tilt = rng.uniform(-1.5, 1.5, k)
    right[:k] = left[:k] - np.stack([base - tilt, np.zeros(k), base + tilt, np.zeros(k)], axis=1)
    if jitter > 0:
        u = right[:k, 2:] - right[:k, :2]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        right[:k, :2] += rng.uniform(-jitter, jitter, (k, 1)) * u
        right[:k, 2:] += rng.uniform(-jitter, jitter, (k, 1)) * u
    swap = rng.uniform(size=k) < flip
    right[:k][swap] = right[:k][swap][:, [2, 3, 0, 1]]
    d = ld[:k] + noise * rng.standard_normal((k, D))
    rd[:k] = d / np.linalg.norm(d, axis=1, keepdims=True)
    pl, pr = rng.permutation(n), rng.permutation(m)
    return (left[pl].astype(np.float32), ld[pl].astype(np.float32), right[pr].astype(np.float32), rd[pr].astype(np.float32))


SIZES = (0, 1, 63, 64, 65, 129)
SIZE_CASES = [(n, m, 8) for n in SIZES for m in SIZES] + [(65, m, D) for m in (7, 8, 9) for D in (8, 72, 128)] + \
             [(129, 129, 72), (129, 65, 128), (512, 512, 72)]


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """name -> (left segments, left descriptors, right segments, right descriptors, options)"""
    inp = {}
    for i, (n, m, D) in enumerate(SIZE_CASES):
        inp["size_%d_%d_%d" % (n, m, D)] = stereo_frame(i, n, m, D) + ({},)
    f = stereo_frame(100, 70, 40, 72)
    inp["gated_out"] = f + (dict(min_disparity=-90.0, max_disparity=-1.0),)
    loose = dict(max_distance=2.0, max_tan2=1e6, min_overlap=0.0, min_disparity=-700.0, max_disparity=700.0)   # many admissible pairs
    inp["ratio_off"] = stereo_frame(101, 70, 70, 8, noise=0.4) + (dict(loose, ratio=0.5),)
    inp["ratio_on"] = inp["ratio_off"][:4] + (dict(loose, ratio=1.2),)
    inp["max_distance"] = stereo_frame(102, 70, 70, 8, noise=0.3) + (dict(max_distance=0.0625),)
    inp["intrinsics"] = stereo_frame(103, 70, 70, 72, jitter=4.0) + (dict(KITTI),)
    # the skip path: 70 left segments in rows 300 .. 340, 24 right segments (three groups) in rows 10 .. 50 - nobody admits any - but
    # right segment 3 (group 0), which answers left segment 5 alone; group 1 is admitted by nobody, group 2 by left segment 66 (the
    # second wave) through right segment 20, so the first wave skips groups 1 and 2 and the second groups 0 and 1
    ls, ld, rs, rd = stereo_frame(104, 70, 24, 72, common=0)
    ls[:] = np.array([[300 + 5 * i, 300, 302 + 5 * i, 340] for i in range(70)], np.float32)
    rs[:] = np.array([[100 + 5 * i, 10, 101 + 5 * i, 50] for i in range(24)], np.float32)
    rs[3], rd[3] = ls[5] - np.float32([20, 0, 20, 0]), ld[5]
    rs[20], rd[20] = ls[66] - np.float32([7, 0, 7, 0]), ld[66]
    inp["skip"] = (ls, ld, rs, rd, {})
    # non-finite values on both sides, flat segments on both sides
    ls, ld, rs, rd = stereo_frame(105, 70, 70, 8)
    ls[3, 2], ld[10, 7], ld[64, 0], rs[5, 1], rd[6, 3], rd[69, 7] = np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan
    ls[20] = [200, 100, 260, 101.5]
    ls[65] = [200, 100, 260, 100]
    rs[8] = [180, 100, 240, 101.5]
    rs[9] = [180, 300, 240, 300]
    inp["invalid_and_flat"] = (ls, ld, rs, rd, {})
    # ties: identical right descriptors with both right segments admissible, identical left segments, in both waves
    ls, ld, rs, rd = stereo_frame(106, 70, 70, 8)
    ls[:] = np.array([[300 + 3.5 * i, 100, 305 + 3.5 * i, 160] for i in range(70)], np.float32)
    rs[:] = np.array([[250 + 3.5 * i, 100, 255 + 3.5 * i, 160] for i in range(70)], np.float32)
    rd[:] = stereo_frame(107, 70, 70, 8, noise=0.0)[1]
    rd[:] = (ld + 0.1 * rd) / np.linalg.norm(ld + 0.1 * rd, axis=1, keepdims=True)      # right i shows left i, r > 0
    rd[11], rd[40], rd[69] = rd[2], rd[2], rd[68]
    ls[30], ld[30], ls[67], ld[67] = ls[4], ld[4], ls[1], ld[1]
    inp["ties"] = (ls, ld, rs, rd, dict(ratio=1.0))
    inp["ties_ratio"] = (ls, ld, rs, rd, {})
    for v in inp.values():
        for a in v[:4]:
            a.setflags(write=False)
    return inp


BATCH = ("size_0_63_8", "size_129_65_8", "size_64_129_8")          # one empty, one with n > m, one with m > n


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of one GPU input: computed once, shared by the tests, never written to."""
    ls, ld, rs, rd, opt = gpu_inputs()[name]
    out = R.match(ls, ld, rs, rd, **opt)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_the_gpu_inputs_are_what_their_tests_say():
    assert reference("gated_out")["num_admissible"].max() == 0 and reference("gated_out")["num_matched"] == 0
    r = reference("skip")
    assert r["match"][5] == 3 and r["match"][66] == 20 and r["num_matched"] == 2 and r["admissible"].sum() == 2
    r = reference("invalid_and_flat")
    assert [r["segment_status"][i] for i in (3, 10, 64, 20, 65)] == [R.INVALID] * 3 + [R.FLAT] * 2
    assert r["best_left"][[5, 6, 69, 8, 9]].tolist() == [-1] * 5 and r["num_matched"] > 20
    r, rr = reference("ties"), reference("ties_ratio")
    assert r["match"][2] == 2 and r["best"][2] == 2 and r["num_admissible"][2] >= 2 and r["best_left"][4] == 4 and r["match"][30] == -1 and r["best_left"][1] == 1 and r["match"][67] == -1
    assert 0 < r["best_distance"][2] == r["second_distance"][2] and rr["match"][2] == -1 and rr["match"][68] == -1 and r["match"][68] == 68
    assert reference("ratio_off")["num_matched"] > reference("ratio_on")["num_matched"] > 0
    r = reference("max_distance")
    assert 0 < r["num_matched"] < 70 and (r["best_distance"][r["best"] >= 0] < 0.0625).all()
    assert reference("size_512_512_72")["num_matched"] > 400
    assert [reference(n)["status"] for n in BATCH] == [R.EMPTY, R.OK, R.OK]
    for (n, m, D) in SIZE_CASES:
        r = reference("size_%d_%d_%d" % (n, m, D))
        assert r["num_matched"] >= 0.8 * min(n, m) - 3, (n, m, D)
        swapped = sum(1 for a in np.nonzero(r["match"] >= 0)[0] if r["observations"][a][5] != gpu_inputs()["size_%d_%d_%d" % (n, m, D)][2][
            r["match"][a]][1])
        assert min(n, m) < 60 or swapped > 5                       # the end point swap is exercised


def test_no_decision_lies_near_its_threshold():
    worst = np.inf
    for name, (ls, ld, rs, rd, opt) in gpu_inputs().items():
        if len(ls) == 0 or len(rs) == 0:
            continue
        o = R.options(**opt)
        ok = R.segment_ok(ls, ld)[:, None] & R.segment_ok(rs, rd)[None, :]
        checks = R.gate(ls, rs, o, margins=True)
        geo, _ = R.gate(ls, rs, o)
        r = R.DM.distances(ld, rd).astype(np.float64)
        checks.append((r, o["max_distance"], geo & np.isfinite(r)))
        for value, thr, reached in checks:
            thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), value.shape)
            sel = reached & ok & np.isfinite(value) & np.isfinite(thr)
            if name == "invalid_and_flat":                         # its flat segments sit on rows of their own choosing, not on a threshold
                sel = sel & (value != 0)
            with np.errstate(all="ignore"):
                rel = np.abs(value - thr)[sel] / np.maximum(np.maximum(np.abs(value), np.abs(thr))[sel], 1e-300)
            rel = rel[(value[sel] != 0) | (thr[sel] != 0)]          # 0 against 0 (touching rows, dot 0) decides exactly
            if rel.size:
                worst = min(worst, float(rel.min()))
                assert rel.min() > 1e-6, (name, float(rel.min()))
    print("the nearest decision lies a relative %.3g from its threshold" % worst)


@functools.lru_cache(maxsize=None)
def float64_figure():
    """The largest difference of an observation value and of a disparity between the contract in float64 and in np.longdouble over the
    matched rows of every GPU input: the reference's own fp64 rounding."""
    obs = disp = 0.0
    for name, (ls, ld, rs, rd, opt) in gpu_inputs().items():
        r = reference(name)
        o = R.options(**opt)
        for a in np.nonzero(r["match"] >= 0)[0]:
            eo, ed = R.emit(ls[a], rs[r["match"][a]], o, real=np.longdouble)
            obs = max(obs, float(np.abs(eo - r["observations"][a].astype(np.longdouble)).max()))
            disp = max(disp, float(np.abs(ed - r["disparity"][a].astype(np.longdouble)).max()))
    return obs, disp


def test_float64_figure():
    obs, disp = float64_figure()
    print("float64 against longdouble: observations %.3g, disparity %.3g px" % (obs, disp))
    # recorded in DESIGN.md 6.9; the values are pixels up to 752 (or pixels / 406): a few ulp of that
    assert 0 < obs <= 2.0 ** -40 and 0 < disp <= 2.0 ** -40


# ---- the accuracy of the contract itself, reference alone
PAIR_SEED, PAIR_DISPARITY, PAIR_OPTIONS = 6, (2.0, 10.0), dict(max_disparity=16.0)
CHAIN_TRUE_MATCHES = 6           # matches of the reference chain that join detections of the same drawn edge: recorded, not chosen
CHAIN_EDGES = 5                  # drawn edges among them


@functools.lru_cache(maxsize=None)
def pair():
    return synth.make_stereo_line_pair(PAIR_SEED, 160, 224, 20, disparity=PAIR_DISPARITY, max_length=60)


def line_distance(seg, p):
    d = (seg[2:] - seg[:2]) / np.hypot(*(seg[2:] - seg[:2]))
    return abs((p[0] - seg[0]) * d[1] - (p[1] - seg[1]) * d[0])


def owner(drawn, seg, reach=2.0, beyond=6.0):
    """The drawn segment that the detection `seg` lies on (tests/test_line_detect_cpu.py words it the same way); -1: none."""
    for i, s in enumerate(np.asarray(drawn, dtype=np.float64)):
        length = np.hypot(*(s[2:] - s[:2]))
        d = (s[2:] - s[:2]) / length
        along = [(p[0] - s[0]) * d[0] + (p[1] - s[1]) * d[1] for p in (seg[:2], seg[2:])]
        if all(line_distance(s, p) <= reach for p in (seg[:2], seg[2:])) and all(-beyond <= a <= length + beyond for a in along):
            return i
    return -1


@functools.lru_cache(maxsize=None)
def chain_reference():
    p = pair()
    a, b = LSD.detect(p["left"]), LSD.detect(p["right"])
    da = MSLD.describe(p["left"], a["segments"].astype(np.float32))
    db = MSLD.describe(p["right"], b["segments"].astype(np.float32))
    ka, kb = (np.nonzero(np.array([s == MSLD.OK for s in d["status"]]))[0] for d in (da, db))
    m = R.match(a["segments"][ka], da["descriptors"][ka].astype(np.float32), b["segments"][kb], db["descriptors"][kb].astype(np.float32),
                **PAIR_OPTIONS)
    return a, b, ka, kb, m


def test_make_stereo_line_pair():
    p, q = pair(), synth.make_stereo_line_pair(PAIR_SEED, 160, 224, 20, disparity=PAIR_DISPARITY, max_length=60)
    assert all(np.array_equal(p[k], q[k]) for k in p) and p["left"].dtype == np.uint8 and p["left"].shape == p["right"].shape == (160, 224)
    assert sorted(p["truth"].tolist()) == list(range(20)) and p["truth"].tolist() != list(range(20))
    ls, rs = p["left_segments"].astype(np.float64), p["right_segments"][p["truth"]].astype(np.float64)
    assert np.array_equal(ls[:, [1, 3]], rs[:, [1, 3]])                                       # the same rows
    assert np.abs(ls[:, [0, 2]] - rs[:, [0, 2]] - p["disparity"]).max() < 1e-4
    assert p["disparity"].min() >= 2.0 and p["disparity"].max() <= 10.0 and np.ptp(p["disparity"]) > 4
    assert rs[:, [0, 2]].min() >= 26.0 and not np.array_equal(p["left"], p["right"])
    # existing generators keep their bytes: the scene of make_line_image is the left view's
    assert np.array_equal(synth.make_line_image(PAIR_SEED, 160, 224, 20, max_length=60, margin=36.0)["image"], p["left"])


def test_accuracy_on_the_generators_segments():
    """The drawn segments with reference MSLD descriptors: every match is the true one."""
    p = pair()
    dl, dr = MSLD.describe(p["left"], p["left_segments"]), MSLD.describe(p["right"], p["right_segments"])
    assert set(dl["status"]) | set(dr["status"]) == {MSLD.OK}
    m = R.match(p["left_segments"], dl["descriptors"].astype(np.float32), p["right_segments"], dr["descriptors"].astype(np.float32),
                **PAIR_OPTIONS)
    good = sum(1 for a, b in enumerate(m["match"]) if b >= 0 and b == p["truth"][a])
    flat = m["segment_status"].count(R.FLAT)
    print("generator segments: %d matched of %d (%d flat), %d wrong; the gate admits %.1f%% of the pairs"
          % (m["num_matched"], len(m["match"]), flat, m["num_matched"] - good, 100.0 * R.gate(p["left_segments"], p["right_segments"],
                                                                                                R.options(**PAIR_OPTIONS))[0].mean()))
    assert m["num_matched"] == good and good >= 10 and good + flat >= 14
    d = m["disparity"][m["match"] >= 0]
    assert np.abs(d - p["disparity"][m["match"] >= 0]).max() < 1e-3                           # float end points


def test_accuracy_of_the_reference_chain():
    """detector -> MSLD -> pairing, reference implementations: how many matches join detections of the same drawn edge."""
    p = pair()
    a, b, ka, kb, m = chain_reference()
    own_a = [owner(p["left_segments"], s) for s in a["segments"][ka].astype(np.float64)]
    own_b = [owner(p["right_segments"], s) for s in b["segments"][kb].astype(np.float64)]
    true = [(x, y) for x, y in enumerate(m["match"]) if y >= 0 and own_a[x] >= 0 and own_b[y] >= 0 and p["truth"][own_a[x]] == own_b[y]]
    wrong = [(x, y) for x, y in enumerate(m["match"]) if y >= 0 and own_a[x] >= 0 and own_b[y] >= 0 and p["truth"][own_a[x]] != own_b[y]]
    edges = {own_a[x] for x, _ in true}
    print("detections %d and %d, matches %d, of the same drawn edge %d (%d edges), of two different drawn edges %d"
          % (len(ka), len(kb), m["num_matched"], len(true), len(edges), len(wrong)))
    assert len(true) == CHAIN_TRUE_MATCHES and len(edges) == CHAIN_EDGES and len(wrong) == 0
    # the disparity of a true match is the drawn one, within the detector's end point accuracy
    for x, y in true:
        assert np.abs(m["disparity"][x] - p["disparity"][own_a[x]].mean()).max() < 2.5


# ---- the C ABI without a device
def _frame(n=3, m=2, D=8, **over):
    ls, ld, rs, rd = stereo_frame(7, n, m, D)
    fr, res, keep, _ = capi._stereo_frame((ls, ld), (rs, rd), D)
    b = keep[4]
    for k, a in b.items():
        a[...] = -7
    for k, v in over.items():
        setattr(fr, k, v)
    return fr, res, keep


def _untouched(res, keep):
    return all((a == -7).all() for a in keep[4].values()) and res.status == -1


def test_exports_and_defaults():
    for name in capi.EXPORTS:
        if "stereo" in name:
            assert hasattr(capi.lib(), name), name
    o = capi.stereo_match_options()
    assert {k: getattr(o, k) for k, _ in capi.StereoMatchOptions._fields_} == R.DEFAULTS
    capi.lib().slslam_stereo_match_default_options(None)
    with pytest.raises(TypeError):
        capi.stereo_match_options(max_disp=3)
    assert capi.STEREO_SEGMENT_STATUS == dict(enumerate(R.SEGMENT_STATUS))


def test_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    for args in ((0, 1, 1), (4, 1, 1), (12, 1, 1), (136, 1, 1), (72, 0, 1), (72, 1, 0), (72, 1, 513), (72, -1, 8)):
        assert L.slslam_stereo_matcher_create(-1, *args, C.byref(h)) == INVALID_ARGUMENT, args
    assert L.slslam_stereo_matcher_create(-1, 72, 1, 1, None) == INVALID_ARGUMENT and not h
    assert L.slslam_stereo_matcher_create(-1, 128, 4096, 512, C.byref(h)) == 0                  # the limits; touches no device
    calls, allocs, ms = C.c_longlong(-1), C.c_longlong(-1), C.c_double(-1.0)
    assert L.slslam_stereo_matcher_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    assert L.slslam_stereo_matcher_timing(h, -1, C.byref(ms)) == 0 and ms.value == 0.0
    assert L.slslam_stereo_matcher_stats(None, None, None) == INVALID_ARGUMENT
    assert L.slslam_stereo_matcher_timing(None, 0, None) == INVALID_ARGUMENT
    L.slslam_stereo_matcher_destroy(h)
    L.slslam_stereo_matcher_destroy(None)


def test_run_arguments_and_no_device():
    L = capi.lib()
    h = C.c_void_p()
    assert L.slslam_stereo_matcher_create(-1, 8, 2, 4, C.byref(h)) == 0
    good = capi.stereo_match_options()
    none_f = C.POINTER(C.c_float)()
    for over in (dict(num_left=-1), dict(num_right=-1), dict(num_left=5), dict(num_right=5), dict(left_segments=none_f),
                 dict(left_descriptors=none_f), dict(right_segments=none_f), dict(right_descriptors=none_f)):
        fr, res, keep = _frame(**over)
        assert L.slslam_stereo_matcher_run(h, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        if "num_left" not in over and "num_right" not in over or min(over.values()) < 0:
            assert L.slslam_match_stereo(8, C.byref(good), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert _untouched(res, keep)
    fr, res, keep = _frame()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(min_disparity=200.0), dict(min_disparity=-inf), dict(max_disparity=inf), dict(max_tan2=-1.0), dict(max_tan2=nan),
                dict(min_rows=-1.0), dict(min_rows=inf), dict(min_overlap=1.5), dict(min_overlap=-0.5), dict(ratio=nan),
                dict(max_distance=nan), dict(fx=0.0), dict(fy=0.0), dict(fx=inf), dict(cx=nan), dict(cy=inf)):
        o = capi.stereo_match_options(**bad)
        assert not R.options_valid(R.options(**bad))
        assert L.slslam_stereo_matcher_run(h, C.byref(o), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, bad
        assert L.slslam_match_stereo(8, C.byref(o), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, bad
    assert L.slslam_stereo_matcher_run(None, C.byref(good), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_stereo_matcher_run(h, None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_stereo_matcher_run(h, C.byref(good), -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_stereo_matcher_run(h, C.byref(good), 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_stereo_matcher_run(h, C.byref(good), 1, C.byref(fr), None) == INVALID_ARGUMENT
    for D in (0, 12, 136):
        assert L.slslam_match_stereo(D, C.byref(good), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_match_stereo(8, None, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_match_stereo(8, C.byref(good), None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_match_stereo(8, C.byref(good), C.byref(fr), None) == INVALID_ARGUMENT
    big = _frame(513, 1)
    assert L.slslam_match_stereo(8, C.byref(good), C.byref(big[0]), C.byref(big[1])) == INVALID_ARGUMENT and _untouched(big[1], big[2])
    assert _untouched(res, keep)
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_stereo_matcher_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)

    if capi.device_count() == 0:                                # every compute entry point says so, and leaves its outputs alone
        assert L.slslam_stereo_matcher_run(h, C.byref(good), 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(res, keep)
        assert L.slslam_stereo_matcher_run(h, C.byref(good), 0, None, None) == NO_DEVICE
        assert L.slslam_match_stereo(8, C.byref(good), C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(res, keep)
        ls, ld, rs, rd = stereo_frame(7, 3, 2, 8)
        sm = capi.StereoMatcher(8, max_frames=1, max_segments=4)
        for call in (lambda: sm.run([((ls, ld), (rs, rd))]), lambda: capi.match_stereo((ls, ld), (rs, rd))):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert sm.stats() == {"calls": 0, "allocations": 0}
        sm.close()
    L.slslam_stereo_matcher_destroy(h)
    with pytest.raises(ValueError):
        capi._stereo_frame((np.zeros((2, 4)), np.zeros((2, 8))), (np.zeros((2, 4)), np.zeros((2, 16))))
    with pytest.raises(TypeError):
        capi.StereoMatcher(8, max_disp=3)


# ---- the host half (csrc/stereo_match_layout.h) under the sanitizers, as a stand-alone program, against the numpy contract
def _layout(F, A, J, D):
    """The call's layout restated: regions one behind the other, each at a multiple of 256 bytes."""
    def carve(sizes):
        at, offs = 0, []
        for s in sizes:
            offs.append(at)
            at += (s + 255) // 256 * 256
        return offs, at
    (_, lseg, rseg, lok, rok, ldesc, rdesc), in_bytes = carve([24 * F, 16 * A, 16 * J, 4 * A, 4 * J, 4 * A * D, 4 * J * D])
    _, match = carve([4 * F] + [4 * A] * 5 + [4 * J])
    (_, status, obs, disp), out_bytes = carve([match, 4 * A, 64 * A, 16 * A])
    keys = in_bytes
    out = keys + (8 * J + 255) // 256 * 256
    return dict(lseg=lseg, rseg=rseg, lok=lok, rok=rok, ldesc=ldesc, rdesc=rdesc, keys=keys, out=out, status=status, obs=obs, disp=disp,
                out_bytes=out_bytes, host=in_bytes + out_bytes, dev=out + out_bytes, **{"in": in_bytes})


def test_host_half_under_the_sanitizers(tmp_path):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "stereo_match_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "stereo_match_layout_check.cpp"), "-o", exe])
    # every pair of a few GPU inputs under their options, and the hand-made equality cases
    lines, want = [], []

    def add(ls, rs, opt):
        o = R.options(**opt)
        lines.append("gate " + " ".join(float(o[k]).hex() for k in ("min_disparity", "max_disparity", "max_tan2", "min_rows", "min_overlap",
                                                                     "fx", "fy", "cx", "cy")))
        geo, _ = R.gate(ls, rs, o)
        flat = ~(R.segments(ls)["ext"] >= o["min_rows"])
        for a in range(len(ls)):
            for b in range(len(rs)):
                if not (np.isfinite(ls[a]).all() and np.isfinite(rs[b]).all()):
                    continue
                lines.append("pair " + " ".join(float(v).hex() for v in list(ls[a]) + list(rs[b])))
                obs, disp = R.emit(ls[a], rs[b], o) if geo[a, b] else (np.zeros(8), np.zeros(2))
                st = 2 if flat[a] else 0 if geo[a, b] else 1
                want.append("pair %d %d " % (geo[a, b], st) + " ".join(float(v).hex() for v in list(obs) + list(disp)))
    for name in ("size_65_9_8", "skip", "invalid_and_flat", "ties", "intrinsics"):
        ls, _, rs, _, opt = gpu_inputs()[name]
        add(ls[:40], rs[:40], opt)
    f32 = np.float32
    add(np.array([LEFT, [100, 10, 120, 50]], f32), np.array([[100, 10, 100, 50], [-28, 10, -28, 50], [90, 10, 100, 50], [90, 30, 90, 70],
                                                             [90, 50, 90, 90], [92, 58, 78, 2]], f32), dict(max_tan2=0.0625, **KITTI))
    path = tmp_path / "pairs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stereo match layout ok" in r.stdout
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("pair ")]
    assert len(got) == len(want) > 5000

    def canon(ln):
        t = ln.split()
        return t[:3] + [float.fromhex(x) for x in t[3:]]
    for g, w in zip(got, want):
        assert canon(g) == canon(w), (g, w)
    assert sum(1 for w in want if w.startswith("pair 1")) > 60
    layouts = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(layouts) == 4
    for t in layouts:
        F, A, J, D = (int(x) for x in t[1:5])
        assert dict(zip(t[5::2], (int(x) for x in t[6::2]))) == _layout(F, A, J, D), t

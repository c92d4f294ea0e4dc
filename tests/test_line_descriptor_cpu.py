"""The MSLD line descriptor without a device (include/slslam_hip.h: slslam_line_descriptor_*, slslam_describe_lines): hand-computed cases
that pin the numpy reference (tests/line_descriptor_reference.py), every status, the swap invariance the centred samples and the
all-rows polarity give, the property of the synthetic pair that the GPU end-to-end test rests on, every argument check of the C ABI (made
before a device is asked for), SLSLAM_ERR_NO_DEVICE on a machine without one, the host layout under the sanitizers as a stand-alone
program, and the measurement behind the GPU tests' tolerance.  The inputs of tests/test_gpu_line_descriptor.py are made here
(gpu_inputs), so that the tolerance is measured on exactly them."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as DM  # noqa: E402
import line_descriptor_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NO_DEVICE = 1, 2
RS2 = 1.0 / np.sqrt(2.0)
F0 = float(np.float32(np.exp(-0.5)))                    # the weight of the outer rows at M w = 3, as the table holds it
PAIR_SEED, PAIR_RATIO, PAIR_MAX_DISTANCE = 3, 1.5, 0.25
SWAP_OPTIONS = [(9, 5), (3, 3), (1, 1), (16, 1), (2, 2)]
DEVICE_OPTIONS = [(9, 5), (3, 3), (1, 1), (16, 1), (16, 9)]


# ---- hand-computed cases, also run on the device
def step_image(negated=False):
    """12 x 16 (H x W): 0 left of column 8, 100 from it on; negated: 255 - that.  gx = 50 (-50) at columns 7 and 8, else 0; gy = 0."""
    img = np.zeros((12, 16), np.uint8)
    img[:, 8:] = 100
    return 255 - img if negated else img


def ramp_image():
    """12 x 16: I = 10 y.  gy = 5 in rows 0 and 11 (the replicated border), 10 between; gx = 0."""
    return np.repeat((10 * np.arange(12, dtype=np.uint8))[:, None], 16, axis=1)


ON_EDGE = [8, 2, 8, 9]          # on the step, downwards: L = N = 7, d_L = (0, 1), d_perp = (-1, 0), g_perp = -gx, samples at y = 2.5 .. 8.5
ROW_0 = [2, 0, 9, 0]            # along row 0: L = N = 7, d_L = (1, 0), d_perp = (0, 1), g_perp = gy
NORM3 = np.sqrt(1.0 + F0 * F0)
NORM_ROW0 = np.sqrt((5 * F0) ** 2 + 25.0 + (10 * F0) ** 2)
# name: (image, segment, options, status, N, polarity, the non-zero components of the descriptor)
HAND = {
    # one row at rho = 0 of weight 1: every sample sees g_perp = -50; polarity -350 flips, the positive-perpendicular component carries
    # everything, the standard deviations are 0
    "step_1_1": (step_image(), ON_EDGE, dict(bands=1, band_width=1), R.OK, 7, 350.0, {0: RS2}),
    # ... and without the flip it is the negative-perpendicular component
    "step_1_1_unoriented": (step_image(), ON_EDGE, dict(bands=1, band_width=1, orient=False), R.OK, 7, -350.0, {1: RS2}),
    # the negated image has g_perp = +50: the same descriptor under orient = 1, a positive polarity without a flip ...
    "negated_1_1": (step_image(True), ON_EDGE, dict(bands=1, band_width=1), R.OK, 7, 350.0, {0: RS2}),
    # ... and with orient = 0 the two components have traded places
    "negated_1_1_unoriented": (step_image(True), ON_EDGE, dict(bands=1, band_width=1, orient=False), R.OK, 7, 350.0, {0: RS2}),
    # three rows at rho = -1, 0, 1 (x = 9, 8, 7: gx = 0, 50, 50) of weights F0, 1, F0, row r = band r: unflipped the bands hold
    # (0, 50, 50 F0) in component 1; polarity = -7 (50 + 50 F0) flips: rows reversed, component 0: (50 F0, 50, 0)
    "step_3_1": (step_image(), ON_EDGE, dict(bands=3, band_width=1), R.OK, 7, 350.0 * (1 + F0), {0: RS2 * F0 / NORM3, 4: RS2 / NORM3}),
    "step_3_1_unoriented": (step_image(), ON_EDGE, dict(bands=3, band_width=1, orient=False), R.OK, 7, -350.0 * (1 + F0),
                            {5: RS2 / NORM3, 9: RS2 * F0 / NORM3}),
    # the negated image at three rows: g_perp = +50, no flip, rows as they lie - the step is not symmetric about the segment (columns 7
    # and 8 carry it, the segment lies on 8), so this is the mirror image of step_3_1 across the line, not its equal
    "negated_3_1": (step_image(True), ON_EDGE, dict(bands=3, band_width=1), R.OK, 7, 350.0 * (1 + F0),
                    {4: RS2 / NORM3, 8: RS2 * F0 / NORM3}),
    # the replicated border: the row at rho = -1 lies at y = -1 and reads the gradient of row 0 (5), rho = 0 reads 5, rho = 1 reads 10
    "row0_1_1": (ramp_image(), ROW_0, dict(bands=1, band_width=1), R.OK, 7, 35.0, {0: RS2}),
    "row0_3_1": (ramp_image(), ROW_0, dict(bands=3, band_width=1), R.OK, 7, 7 * (5 * F0 + 5 + 10 * F0),
                 {0: RS2 * 5 * F0 / NORM_ROW0, 4: RS2 * 5 / NORM_ROW0, 8: RS2 * 10 * F0 / NORM_ROW0}),
    "constant": (np.full((12, 16), 77, np.uint8), ON_EDGE, dict(), R.FLAT, 7, 0.0, {}),
}


def check_hand(got, name, tol):
    _, _, opt, status, n, polarity, nonzero = HAND[name]
    want = np.zeros(8 * opt.get("bands", 9))
    for i, v in nonzero.items():
        want[i] = v
    assert list(got["status"]) == [status] and got["num_samples"].tolist() == [n]
    assert abs(float(got["polarity"][0]) - polarity) <= 1e-3 * max(1.0, abs(polarity))
    assert np.abs(np.asarray(got["descriptors"][0], dtype=np.float64) - want).max() <= tol
    zero = [i for i in range(len(want)) if i not in nonzero]
    assert (np.asarray(got["descriptors"][0])[zero] == 0).all()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed(name):
    image, seg, opt = HAND[name][:3]
    check_hand(R.describe(image, [seg], **opt), name, 1e-12)


def test_weight_table_by_hand():
    wa, wb, f, band = R.weight_table(2, 2)                 # rho = -1.5 .. 1.5, sigma = 1.5; t = -0.25, 0.25, 0.75, 1.25
    e = np.exp(-np.array([1.5, 0.5, 0.5, 1.5]) ** 2 / 4.5)
    assert band.tolist() == [-1, 0, 0, 1]
    assert np.allclose(wa, e * [0.25, 0.75, 0.25, 0.75], rtol=1e-7) and np.allclose(wb, e * [0.75, 0.25, 0.75, 0.25], rtol=1e-7)
    assert np.allclose(f, e, rtol=1e-7) and wa.dtype == wb.dtype == f.dtype == np.float32
    wa, wb, f, band = R.weight_table(1, 1)
    assert (wa.tolist(), wb.tolist(), f.tolist(), band.tolist()) == ([1.0], [0.0], [1.0], [0])


# ---- every status, N = floor(L), the order of the refusals
STATUS_SEGMENTS = [
    ([2, 3, 12, 3], R.OK, 10),
    ([2, 3, float(np.nextafter(np.float32(12), np.float32(0))), 3], R.OK, 9),          # L just below 10
    ([2, 3, float(np.nextafter(np.float32(12), np.float32(99))), 3], R.OK, 10),        # ... and just above
    ([2, 3, 4, 3], R.OK, 2),                                                           # L = 2 runs
    ([2, 3, float(np.nextafter(np.float32(4), np.float32(0))), 3], R.TOO_SHORT, 0),
    ([5, 5, 5, 5], R.TOO_SHORT, 0),                                                    # L = 0
    ([0, 0, 15, 11], R.OK, 18),                                                        # corner to corner: the end points may lie on the border
    ([-0.01, 3, 9, 3], R.OUTSIDE, 0),
    ([2, 3, 15.01, 3], R.OUTSIDE, 0),
    ([2, 3, 9, 11.5], R.OUTSIDE, 0),
    ([2, -1, 2, -1], R.OUTSIDE, 0),                                                    # outside before too short
    ([2, 3, float("nan"), 3], R.INVALID, 0),
    ([float("inf"), 3, 9, 3], R.INVALID, 0),
    ([-5, float("nan"), 9, 3], R.INVALID, 0),                                          # invalid before outside
]


def status_frame():
    """The step image with a texture over it (no segment is flat), and STATUS_SEGMENTS."""
    img = (step_image().astype(np.int32) + 7 * (np.arange(16)[None, :] % 3) + 5 * (np.arange(12)[:, None] % 4)).astype(np.uint8)
    return img, np.array([s for s, _, _ in STATUS_SEGMENTS], np.float32)


def test_statuses_and_num_samples():
    img, seg = status_frame()
    got = R.describe(img, seg)
    assert got["status"] == [st for _, st, _ in STATUS_SEGMENTS]
    assert got["num_samples"].tolist() == [n for _, _, n in STATUS_SEGMENTS]
    for i, st in enumerate(got["status"]):
        d = got["descriptors"][i]
        if st == R.OK:
            assert abs(np.linalg.norm(d) - 1) < 1e-12 and abs(np.linalg.norm(d[:36]) - RS2) < 1e-12
        else:
            assert (d == 0).all() and got["polarity"][i] == 0


# ---- the inputs of the GPU tests: name -> (image, segments, options)
def along_frame():
    """One 96 x 160 (H x W) image and segments of 2, 3, 63, 64, 65, 128, 129 and 150 samples, at mixed angles."""
    img = synth.make_line_image(21, 96, 160, 12, max_length=60, margin=8)["image"]
    seg = []
    for k, n in enumerate((2, 3, 63, 64, 65, 128, 129, 150)):
        length, th = n + 0.37, (-0.25, 0.1, 0.4)[k % 3]
        c, h = np.array([79.5 + 0.3 * k, 47.3 + 0.2 * k]), 0.5 * length * np.array([np.cos(th), np.sin(th)])
        seg.append(np.concatenate([c - h, c + h]))
    return img, np.array(seg, np.float32)


def border_frame():
    """A textured 40 x 56 image: a segment along each border, one corner to corner, and an OUTSIDE, an INVALID and a TOO_SHORT segment
    between segments that run."""
    s = synth.make_line_image(22, 40, 56, 4, max_length=20, margin=6)
    w, h = 55, 39
    extra = [[0, 0, w, 0], [0, h, w, h], [0, 0, 0, h], [w, h, w, 0], [0, 0, w, h], [w, 0, 0, h]]
    seg = [s["segments"][0], [3, 3, 80, 3], s["segments"][1], [3, float("nan"), 9, 9], s["segments"][2], [7, 7, 8, 7.5], s["segments"][3]]
    return s["image"], np.array(extra + [list(map(float, x)) for x in seg], np.float32)


BORDER_STATUS = [R.OK] * 7 + [R.OUTSIDE, R.OK, R.INVALID, R.OK, R.TOO_SHORT, R.OK]
COUNTS = (1, 63, 64, 65, 130)
FRAME_SIZES = ((64, 48), (320, 240), (97, 33))              # width x height


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    inputs = {"hand_" + k: v[:3] for k, v in HAND.items()}
    img, seg = along_frame()
    inputs["along"] = (img, seg, {})
    for n in COUNTS:
        s = synth.make_line_image(30 + n, 72, 96, n, max_length=30, margin=6)
        inputs["count_%d" % n] = (s["image"], s["segments"], {})
    s = synth.make_line_image(23, 80, 112, 20, max_length=50, margin=10)
    for m, w in DEVICE_OPTIONS:
        for orient in (False, True):
            inputs["options_%d_%d_%d" % (m, w, orient)] = (s["image"], s["segments"], dict(bands=m, band_width=w, orient=orient))
    for i, (w, h) in enumerate(FRAME_SIZES):
        s = synth.make_line_image(40 + i, h, w, (9, 0, 7)[i], min_length=8, max_length=24, margin=3)
        inputs["frames_%d" % i] = (s["image"], s["segments"], {})
    img, seg = border_frame()
    inputs["border"] = (img, seg, {})
    img, seg = status_frame()
    inputs["statuses"] = (img, seg, {})
    p = pair()
    inputs["pair_a"] = (p["image"], p["segments"], {})
    inputs["pair_b"] = (p["image2"], p["segments2"], {})
    return inputs


@functools.lru_cache(maxsize=None)
def pair():
    return synth.make_line_image_pair(PAIR_SEED, 240, 320, 60)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 reference of one GPU input: computed once, shared by the tests, never written to."""
    image, seg, opt = gpu_inputs()[name]
    out = R.describe(image, seg, **opt)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_the_gpu_inputs_are_what_their_tests_say():
    assert reference("along")["num_samples"].tolist() == [2, 3, 63, 64, 65, 128, 129, 150] and reference("along")["status"] == [R.OK] * 8
    for n in COUNTS:
        assert reference("count_%d" % n)["status"] == [R.OK] * n
    assert reference("border")["status"] == BORDER_STATUS
    assert [len(reference("frames_%d" % i)["status"]) for i in range(3)] == [9, 0, 7]
    assert all(reference("options_%d_%d_%d" % (m, w, o))["status"] == [R.OK] * 20 for m, w in DEVICE_OPTIONS for o in (0, 1))


def test_make_line_image():
    s = synth.make_line_image(5, 120, 160, 25, margin=20)
    img, seg = s["image"], s["segments"]
    assert img.dtype == np.uint8 and img.shape == (120, 160) and seg.dtype == np.float32 and seg.shape == (25, 4)
    assert seg[:, [0, 2]].min() >= 20 and seg[:, [0, 2]].max() <= 139 and seg[:, [1, 3]].min() >= 20 and seg[:, [1, 3]].max() <= 99
    length = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1])
    assert length.min() >= 12 - 1e-3 and length.max() <= 80 + 1e-3
    assert np.array_equal(synth.make_line_image(5, 120, 160, 25, margin=20)["image"], img)          # seeded
    # every segment follows an edge: over the three rows about the line the gradient across it, in the oriented direction, is the
    # strongest of the four mean components, and the texture's share stays well below it
    r = R.describe(img, seg, bands=1, band_width=3)
    assert r["status"] == [R.OK] * 25
    d = r["descriptors"][:, :4]
    assert (d[:, 0] > 1.5 * np.abs(d[:, 1:]).max(axis=1)).all()
    p = pair()
    assert np.array_equal(np.sort(p["truth"]), np.arange(60)) and not np.array_equal(p["truth"], np.arange(60))
    assert np.allclose(p["segments2"][p["truth"]] - p["segments"], [2.3, -1.6, 2.3, -1.6], atol=1e-4)


# ---- the flip rule, shared with the GPU test: a segment counts when |polarity| >= 1 grey level, and at most 10 % may not count
def counted(polarity):
    ok = np.abs(np.asarray(polarity, dtype=np.float64)) >= 1.0
    assert (~ok).sum() <= 0.1 * len(ok)
    return ok


@pytest.mark.parametrize("bands,band_width", SWAP_OPTIONS)
def test_swapping_the_end_points_changes_nothing(bands, band_width):
    image, seg, _ = gpu_inputs()["pair_a"]
    a = R.describe(image, seg, bands, band_width)
    b = R.describe(image, seg[:, [2, 3, 0, 1]], bands, band_width)
    ok = counted(a["polarity"])
    assert a["status"] == b["status"] == [R.OK] * len(seg)
    assert np.abs(a["descriptors"] - b["descriptors"])[ok].max() <= 1e-12
    assert np.abs(a["polarity"] - b["polarity"])[ok].max() <= 1e-9 and (a["polarity"][ok] > 0).all()
    # ... and without the orientation the swapped segment's polarity is the negative
    c = R.describe(image, seg[:, [2, 3, 0, 1]], bands, band_width, orient=False)
    d = R.describe(image, seg, bands, band_width, orient=False)
    assert np.abs(c["polarity"] + d["polarity"]).max() <= 1e-9 and (d["polarity"] < 0).any() and (d["polarity"] > 0).any()


def test_the_pair_matches_on_the_reference():
    """What the GPU end-to-end test rests on: with the reference descriptors of both views every segment finds its true partner."""
    p = pair()
    a, b = reference("pair_a"), reference("pair_b")
    m = DM.match(a["descriptors"].astype(np.float32), b["descriptors"].astype(np.float32), PAIR_RATIO, PAIR_MAX_DISTANCE)
    assert m["status"] == "OK" and np.array_equal(m["match"], p["truth"]) and m["num_matched"] == 60
    assert np.allclose(np.linalg.norm(a["descriptors"], axis=1), 1, atol=1e-12)


def test_float32_figure():
    """The tolerance of the GPU tests is measured, not guessed: the same reference evaluated in float32 stays within R.F32_FIGURE of the
    fp64 result on every input of the GPU tests, statuses and sample counts equal."""
    worst = {}
    for name, (image, seg, opt) in gpu_inputs().items():
        ref = reference(name)
        f32 = R.describe(image, seg, dtype=np.float32, **opt)
        assert f32["descriptors"].dtype == np.float32
        assert f32["status"] == ref["status"] and np.array_equal(f32["num_samples"], ref["num_samples"]), name
        worst[name] = float(np.abs(f32["descriptors"].astype(np.float64) - ref["descriptors"]).max()) if len(seg) else 0.0
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("float32 against float64, the five largest:", top)
    assert top[0][1] <= R.F32_FIGURE, top
    assert R.F32_FIGURE <= 4 * top[0][1]                    # (the figure is the measurement, not a generous bound)
    assert R.DEVICE_TOLERANCE == 8 * R.F32_FIGURE


# ---- the C ABI: the exports, the argument checks (before a device is asked for), no device
NAMES = ["slslam_msld_default_options", "slslam_line_descriptor_create", "slslam_line_descriptor_destroy", "slslam_line_descriptor_run",
         "slslam_line_descriptor_stats", "slslam_line_descriptor_timing", "slslam_describe_lines"]


def test_exports_and_defaults():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(L, name)
    o = capi.MsldOptions(-1, -1, -1)
    L.slslam_msld_default_options(C.byref(o))
    assert (o.bands, o.band_width, o.orient) == (9, 5, 1)
    L.slslam_msld_default_options(None)
    assert capi.MSLD_STATUS == {0: R.OK, 1: R.FLAT, 2: R.TOO_SHORT, 3: R.OUTSIDE, 4: R.INVALID}


def _frame(img, seg, **over):
    fr, res, keep = capi._msld_frame(img, seg, 72)
    keep[2]["descriptors"][:] = -7
    keep[2]["status"][:] = -7
    for k, v in over.items():
        setattr(fr, k, v)
    return fr, res, keep


def _untouched(keep):
    return (keep[2]["descriptors"] == -7).all() and (keep[2]["status"] == -7).all()


def test_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    good = capi.msld_options()
    for bad in (capi.MsldOptions(0, 5, 1), capi.MsldOptions(17, 5, 1), capi.MsldOptions(9, 0, 1), capi.MsldOptions(9, 10, 1),
                capi.MsldOptions(9, 5, 2), capi.MsldOptions(9, 5, -1)):
        assert L.slslam_line_descriptor_create(-1, C.byref(bad), 1, 100, 10, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_create(-1, None, 1, 100, 10, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_create(-1, C.byref(good), 1, 100, 10, None) == INVALID_ARGUMENT
    for args in ((0, 100, 10), (1, 0, 10), (1, 100, 0), (-1, 100, 10)):
        assert L.slslam_line_descriptor_create(-1, C.byref(good), *args, C.byref(h)) == INVALID_ARGUMENT
    # a capacity the first run could not allocate: a frame beyond 8192^2 pixels, more than 2^24 segments, more than 2^32 pixels
    for args in ((1, 8192 * 8192 + 1, 10), (2, 100, 2 ** 23 + 1), (65, 8192 * 8192, 10)):
        assert L.slslam_line_descriptor_create(-1, C.byref(good), *args, C.byref(h)) == INVALID_ARGUMENT, args
    assert not h
    assert L.slslam_line_descriptor_create(-1, C.byref(good), 64, 8192 * 8192, 2 ** 18, C.byref(h)) == 0           # the capacity's limits
    ms = C.c_double(-1.0)
    assert L.slslam_line_descriptor_timing(h, -1, C.byref(ms)) == 0 and ms.value == 0.0
    L.slslam_line_descriptor_destroy(h)
    h = C.c_void_p()
    assert L.slslam_line_descriptor_create(-1, C.byref(capi.MsldOptions(16, 9, 0)), 1, 1, 1, C.byref(h)) == 0      # the limits; no device
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_line_descriptor_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    assert L.slslam_line_descriptor_stats(None, None, None) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_timing(None, 0, None) == INVALID_ARGUMENT
    L.slslam_line_descriptor_destroy(h)
    L.slslam_line_descriptor_destroy(None)


def test_run_arguments_and_no_device():
    L = capi.lib()
    h = C.c_void_p()
    opt = capi.msld_options()
    assert L.slslam_line_descriptor_create(-1, C.byref(opt), 2, 12 * 16, 4, C.byref(h)) == 0
    img, seg = status_frame()
    big = np.zeros((2, 8193), np.uint8)
    cases = [dict(width=0), dict(height=0), dict(width=-3), dict(stride=15), dict(num_segments=-1),
             dict(image=C.POINTER(C.c_ubyte)()), dict(segments=C.POINTER(C.c_float)())]
    for over in cases:
        fr, res, keep = _frame(img, seg, **over)
        assert L.slslam_line_descriptor_run(h, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert L.slslam_describe_lines(C.byref(opt), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert _untouched(keep)
    for image in (big, big.T):                                                  # a side beyond 8192
        fr, res, keep = _frame(np.ascontiguousarray(image), seg)
        assert L.slslam_line_descriptor_run(h, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    fr, res, keep = _frame(img, seg)
    assert L.slslam_line_descriptor_run(None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_run(h, -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_run(h, 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_descriptor_run(h, 1, C.byref(fr), None) == INVALID_ARGUMENT
    assert L.slslam_describe_lines(None, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_describe_lines(C.byref(capi.MsldOptions(9, 5, 3)), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_describe_lines(C.byref(opt), None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_describe_lines(C.byref(opt), C.byref(fr), None) == INVALID_ARGUMENT
    assert _untouched(keep)
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_line_descriptor_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)

    if capi.device_count() == 0:                                # every compute entry point says so, and leaves its outputs alone
        assert L.slslam_line_descriptor_run(h, 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        assert L.slslam_line_descriptor_run(h, 0, None, None) == NO_DEVICE
        assert L.slslam_describe_lines(C.byref(opt), C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        d = capi.LineDescriptor(max_frames=1, max_pixels=12 * 16, max_segments=4)
        for call in (lambda: d.run([(img, seg)]), lambda: capi.describe_lines(img, seg)):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert d.stats() == {"calls": 0, "allocations": 0}
        d.close()
    L.slslam_line_descriptor_destroy(h)


def test_a_strided_image_passes_its_stride():
    base = np.zeros((12, 40), np.uint8)
    view = base[:, 3:19]
    fr, _, keep = capi._msld_frame(view, np.zeros((0, 4)), 72)
    assert (fr.width, fr.height, fr.stride) == (16, 12, 40) and keep[0] is view
    assert C.addressof(fr.image.contents) == view.ctypes.data
    fr, _, keep = capi._msld_frame(base[:, ::2], np.zeros((0, 4)), 72)           # columns apart: copied
    assert (fr.width, fr.stride) == (20, 20) and keep[0].flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        capi._msld_frame(base.astype(np.float32), np.zeros((0, 4)), 72)


# ---- the host layout (csrc/line_descriptor_layout.h) under the sanitizers, as a stand-alone program
def test_host_layout_under_the_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "line_descriptor_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "line_descriptor_layout_check.cpp"), "-o", exe])
    # the table of every (M, w) the tests use and the status table above, as the program's input: it prints what it computes
    img, seg = status_frame()
    lines = ["%d %d" % mw for mw in sorted(set(SWAP_OPTIONS + DEVICE_OPTIONS))]
    r = subprocess.run([exe] + lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "line descriptor layout ok" in r.stdout
    tables = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "row":
            tables.setdefault((int(t[1]), int(t[2])), []).append((float(t[4]), float(t[5]), float(t[6]), int(t[7])))
    for (m, w), rows in tables.items():
        wa, wb, f, band = R.weight_table(m, w)
        got = np.array(rows)
        assert len(rows) == m * w and got[:, 3].tolist() == band.tolist(), (m, w)
        # exp may differ in its last bit between the two libraries: one ulp of the float it is rounded to
        for col, want in ((0, wa), (1, wb), (2, f)):
            assert np.abs(got[:, col] - want.astype(np.float64)).max() <= 2.0 ** -23, (m, w, col)
    status = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("segment ")]
    names = [R.OK, R.FLAT, R.TOO_SHORT, R.OUTSIDE, R.INVALID]
    assert [(names[int(s)], int(n)) for s, n in status] == [(st, n) for _, st, n in STATUS_SEGMENTS]

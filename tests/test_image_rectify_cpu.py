"""The image rectifier without a device: the numpy contract (tests/image_rectify_reference.py) by hand, the smoothing taps and
slslam_stereo_rectify of the library against their restatements, the C ABI's argument checks, the host half (csrc/image_rectify_layout.h)
as a stand-alone program under the sanitizers, the inputs of tests/test_gpu_image_rectify.py with the condition their bit-for-bit
comparison rests on, and the accuracy of the contract on synth.make_raw_stereo_pair through the reference detector, MSLD and stereo
matcher."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_rectify_reference as R  # noqa: E402
import line_descriptor_reference as MSLD  # noqa: E402
import line_detect_reference as LSD  # noqa: E402
import line_track_reference as TR  # noqa: E402
import stereo_match_reference as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NO_DEVICE = 1, 2
TILE_W, TILE_H, BLOCK = 64, 16, 256          # csrc/image_rectify_layout.h: kTileW, kTileH, kBlock
SIGMA_OF_RADIUS = {1: 0.28, 2: 0.6, 3: 0.95, 4: 1.28, 5: 1.6, 6: 1.95, 7: 2.4}


def image_of(seed, h, w):
    """A seeded uint8 image with structure at every scale: noise over a ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((rng.integers(0, 256, (h, w)) + 3 * xx + 5 * yy) % 256).astype(np.uint8)


# ---- the reference by hand
def test_identity_returns_the_input():
    img = image_of(1, 9, 13)
    cam = R.camera(13, 9)
    m = R.make_map(cam)
    assert (m["qx"] & 255 == 0).all() and (m["qy"] & 255 == 0).all() and m["valid"].all()
    assert np.array_equal(m["qx"] >> 8, np.tile(np.arange(13), (9, 1))) and np.array_equal(m["sy"], np.tile(np.arange(9.0)[:, None], (1, 13)))
    out = R.rectify(img, cam)
    assert np.array_equal(out["image"], img) and out["num_valid"] == 9 * 13
    # ... with intrinsics that are not 1 and 0, rectified like raw
    cam = R.camera(13, 9, fx=200.0, fy=180.0, cx=6.0, cy=4.0)
    assert np.array_equal(R.rectify(img, cam)["image"], img)


def test_integer_shift_of_the_principal_point_shifts_the_image():
    img = image_of(2, 12, 16)
    cam = R.camera(16, 12, fx=1.0, fy=1.0, cx=3.0, cy=-2.0, cx2=0.0, cy2=0.0)          # sx = u + 3, sy = v - 2
    for mode in (R.CONSTANT, R.REPLICATE):
        out = R.rectify(img, cam, mode, 77)
        assert np.array_equal(out["image"][2:, :13], img[:10, 3:])
        assert out["num_valid"] == 10 * 13 and not out["valid"][:2].any() and not out["valid"][:, 13:].any()
        if mode == R.CONSTANT:
            assert (out["image"][:2] == 77).all() and (out["image"][:, 13:] == 77).all()
        else:                                                   # the value at the clamped coordinates
            assert np.array_equal(out["image"][0, :13], img[0, 3:]) and np.array_equal(out["image"][2:, 15], img[:10, 15])
            assert out["image"][0, 15] == img[0, 15]


def test_half_pixel_shift_is_the_rounded_mean_of_two_neighbours():
    img = image_of(3, 6, 10)
    cam = R.camera(10, 6, cx=0.5, cx2=0.0)                                            # sx = u + 0.5
    m = R.make_map(cam)
    assert (m["qx"] & 255 == 128).all() and (m["qy"] & 255 == 0).all()
    out = R.rectify(img, cam)["image"]
    a, b = img[:, :-1].astype(np.int64), img[:, 1:].astype(np.int64)
    assert np.array_equal(out[:, :-1], (128 * 256 * a + 128 * 256 * b + 32768) >> 16)
    assert np.array_equal(out[:, :-1], (a + b + 1) >> 1)                               # which is the mean, halves up
    assert not m["valid"][:, -1].any() and m["valid"][:, :-1].all()                    # sx = 9.5 is the bound itself: outside


def test_distortion_bends_the_map_the_right_way():
    base = dict(fx=40.0, fy=40.0, cx=32.0, cy=24.0)
    none = R.make_map(R.camera(65, 49, **base))
    barrel = R.make_map(R.camera(65, 49, k1=-0.3, **base))
    pin = R.make_map(R.camera(65, 49, k1=0.3, **base))
    # k1 < 0: a rectified pixel away from the centre reads the raw image nearer the centre; k1 > 0: farther out
    r0 = np.hypot(none["sx"] - 32.0, none["sy"] - 24.0)
    off = r0 > 1.0
    assert (np.hypot(barrel["sx"] - 32.0, barrel["sy"] - 24.0)[off] < r0[off]).all()
    assert (np.hypot(pin["sx"] - 32.0, pin["sy"] - 24.0)[off] > r0[off]).all()
    assert barrel["valid"].all() and not pin["valid"].all()
    assert barrel["sx"][24, 32] == 32.0 and barrel["sy"][24, 32] == 24.0              # the centre stays
    # tangential terms alone: p2 moves the centre row along x by p2 3 x^2, p1 the centre column along y
    tang = R.make_map(R.camera(65, 49, p1=0.01, p2=0.02, **base))
    x = (np.arange(65) - 32.0) / 40.0
    assert np.abs(tang["sx"][24] - (40.0 * (x + 0.02 * 3.0 * x * x) + 32.0)).max() < 1e-12


def test_behind_the_camera_is_invalid_without_coordinates():
    rot = synth.rodrigues([0.0, np.deg2rad(100.0), 0.0])
    cam = R.camera(16, 12, fx=20.0, fy=20.0, cx=8.0, cy=6.0, R=rot)
    m = R.make_map(cam)
    assert not m["coords"].all() and (m["qx"][~m["coords"]] == R.NO_COORD).all() and (m["qy"][~m["coords"]] == R.NO_COORD).all()
    assert np.isnan(m["sx"][~m["coords"]]).all() and not m["valid"][~m["coords"]].any()
    img = image_of(4, 12, 16)
    for mode in (R.CONSTANT, R.REPLICATE):                       # no coordinates: the border value under both modes
        assert (R.rectify(img, cam, mode, 91)["image"][~m["coords"]] == 91).all()
    turned = R.make_map(R.camera(16, 12, fx=20.0, fy=20.0, cx=8.0, cy=6.0, R=synth.rodrigues([0.0, 3.0, 0.0])))
    assert not turned["coords"].any() and turned["valid"].sum() == 0


def test_both_border_modes():
    img = image_of(5, 8, 8)
    cam = R.camera(8, 8, 12, 12, cx=0.0, cy=0.0, cx2=2.25, cy2=2.0)                   # sx = u - 2.25: two columns and rows outside each way
    m = R.make_map(cam)
    const, repl = R.rectify(img, cam, R.CONSTANT, 200), R.rectify(img, cam, R.REPLICATE, 200)
    inside = m["valid"] != 0
    assert 0 < inside.sum() < inside.size and np.array_equal(const["image"][inside], repl["image"][inside])
    assert (const["image"][~inside] == 200).all()
    assert repl["image"][0, 0] == img[0, 0] and repl["image"][11, 11] == img[7, 7] and repl["image"][0, 11] == img[0, 7]
    assert np.array_equal(repl["image"][0, 3:10], repl["image"][2, 3:10])              # a row above the source repeats row 0's remap


# ---- smoothing
def test_taps_of_the_library():
    for sigma, radius in [(0.3, 1), (0.6, 2), (1.0, 3), (2.0, 6), (2.4, 7)] + [(s, r) for r, s in SIGMA_OF_RADIUS.items()]:
        r, t = capi.smooth_taps(sigma)
        assert r == radius == R.taps_restated(sigma)[0], sigma
        assert t[0] + 2 * t[1:].sum() == 16384 and (t[r + 1:] == 0).all() and (t[:r + 1] >= 0).all()
        assert (np.diff(t[:r + 1]) <= 0).all(), (sigma, t)                                 # symmetric by construction, non-increasing
        want = R.taps_restated(sigma)[1]
        assert np.abs(t - want).max() <= 1, (sigma, t, want)
    assert capi.smooth_taps(0.0)[0] == 0 and capi.smooth_taps(0.0)[1].tolist() == [16384] + [0] * 7
    assert capi.smooth_taps(16.0)[0] == 7
    L = capi.lib()
    r, t = C.c_int(-5), np.full(8, -5, dtype=np.int32)
    for bad in (-0.1, float("nan"), float("inf"), 16.5):
        assert L.slslam_rectify_smooth_taps(bad, C.byref(r), capi._ip(t)) == INVALID_ARGUMENT
    assert L.slslam_rectify_smooth_taps(1.0, None, capi._ip(t)) == INVALID_ARGUMENT
    assert L.slslam_rectify_smooth_taps(1.0, C.byref(r), None) == INVALID_ARGUMENT
    assert r.value == -5 and (t == -5).all()


def test_smoothing_a_constant_and_an_impulse():
    for sigma in (0.3, 0.6, 1.0, 2.0, 2.4):
        r, t = capi.smooth_taps(sigma)
        for value in (0, 1, 127, 255):
            flat = np.full((9, 11), value, np.uint8)
            assert np.array_equal(R.smooth(flat, r, t), flat), (sigma, value)
        imp = np.zeros((2 * r + 5, 2 * r + 7), np.uint8)
        imp[r + 2, r + 3] = 255
        full = np.concatenate([t[r:0:-1], t[:r + 1]]).astype(np.int64)            # t_r .. t_1 t_0 t_1 .. t_r
        hor = (full * 255 + 32) >> 6
        want = (np.outer(full, hor) + (1 << 21)) >> 22
        got = R.smooth(imp, r, t)
        assert np.array_equal(got[2:2 + 2 * r + 1, 3:3 + 2 * r + 1], want), sigma
        mask = np.ones_like(imp, dtype=bool)
        mask[2:2 + 2 * r + 1, 3:3 + 2 * r + 1] = False
        assert (got[mask] == 0).all()


# ---- slslam_stereo_rectify
RIG_L = dict(fx=410.0, fy=408.0, cx=320.5, cy=241.0, k1=-0.2, k2=0.05, p1=0.001, p2=-0.002, k3=0.01, width=640, height=480)
RIG_R = dict(fx=405.0, fy=407.0, cx=318.0, cy=239.5, k1=-0.22, k2=0.06, p1=-0.001, p2=0.001, k3=0.0, width=656, height=488)


def cam_array(c):
    d = c.as_dict()
    return np.concatenate([[d[k] for k in R.CAMERA_KEYS[:9]], d["R"].reshape(-1), [d[k] for k in R.CAMERA_KEYS[9:]],
                           [d["src_width"], d["src_height"], d["dst_width"], d["dst_height"]]])


def ref_array(d):
    return np.concatenate([[d[k] for k in R.CAMERA_KEYS[:9]], d["R"].reshape(-1), [d[k] for k in R.CAMERA_KEYS[9:]],
                           [d["src_width"], d["src_height"], d["dst_width"], d["dst_height"]]])


def test_stereo_rectify():
    rot = synth.rodrigues([0.02, -0.03, 0.015])
    centre = np.array([0.12, 0.005, -0.004])
    t = -(rot @ centre)
    for kw in (dict(), dict(dst_size=(600, 440), principal=(300.25, 219.5))):
        got, want = capi.stereo_rectify(RIG_L, RIG_R, rot, t, **kw), R.stereo_rectify(RIG_L, RIG_R, rot, t, **kw)
        for side in ("left", "right"):
            assert np.abs(cam_array(got[side]) - ref_array(want[side])).max() <= 1e-12, side
            Rs = got[side].as_dict()["R"]
            assert np.abs(Rs @ Rs.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Rs) - 1.0) <= 1e-14
        for k in ("baseline", "fx", "fy", "cx", "cy"):
            assert abs(got[k] - want[k]) <= 1e-12, k
        Rl, Rr = got["left"].as_dict()["R"], got["right"].as_dict()["R"]
        # the right centre in the rectified frame: along +x, at the baseline
        assert np.abs(Rl @ centre - [got["baseline"], 0.0, 0.0]).max() <= 1e-14 and abs(got["baseline"] - np.linalg.norm(centre)) <= 1e-15
        assert np.abs(Rr - Rl @ rot.T).max() <= 1e-15                                   # both views look the same way
        assert got["fx"] == got["fy"] == (410.0 + 408.0 + 405.0 + 407.0) / 4.0
        assert (got["cx"], got["cy"]) == (kw.get("principal") or (320.5, 241.0))
        assert (got["right"].src_width, got["right"].src_height, got["right"].dst_width) == (656, 488, kw.get("dst_size", (640, 480))[0])
    # a rig that is rectified already
    got = capi.stereo_rectify(RIG_L, RIG_R, np.eye(3), [-0.12, 0.0, 0.0])
    assert np.array_equal(got["left"].as_dict()["R"], np.eye(3)) and np.array_equal(got["right"].as_dict()["R"], np.eye(3))
    assert got["baseline"] == 0.12
    # arguments
    L = capi.lib()
    g = capi.StereoRig()
    a, b, base, k = capi.RectifyCamera(), capi.RectifyCamera(), C.c_double(-3.0), np.full(4, -3.0)
    a.fx = b.fx = -3.0
    assert L.slslam_stereo_rectify(None, C.byref(a), C.byref(b), C.byref(base), capi._dp(k)) == INVALID_ARGUMENT
    for make in (lambda: capi.stereo_rectify(RIG_L, RIG_R, np.eye(3), [0.0, 0.0, 0.0]),              # no baseline
                 lambda: capi.stereo_rectify(RIG_L, RIG_R, np.eye(3), [0.0, 0.0, -0.1]),             # ... along the optical axis
                 lambda: capi.stereo_rectify(dict(RIG_L, fx=0.0), RIG_R, np.eye(3), [-0.1, 0.0, 0.0]),
                 lambda: capi.stereo_rectify(dict(RIG_L, k1=float("nan")), RIG_R, np.eye(3), [-0.1, 0.0, 0.0]),
                 lambda: capi.stereo_rectify(dict(RIG_L, width=8193), RIG_R, np.eye(3), [-0.1, 0.0, 0.0]),
                 lambda: capi.stereo_rectify(RIG_L, RIG_R, np.eye(3), [-0.1, 0.0, 0.0], dst_size=(0, 5))):
        with pytest.raises(capi.SlslamError) as ei:
            make()
        assert ei.value.status == INVALID_ARGUMENT
    assert L.slslam_stereo_rectify(C.byref(g), C.byref(a), C.byref(b), C.byref(base), capi._dp(k)) == INVALID_ARGUMENT      # all zero
    assert a.fx == b.fx == -3.0 and base.value == -3.0 and (k == -3.0).all()


# ---- the inputs of the GPU tests
def _cam(kind, sw, sh, dw, dh):
    f = 0.8 * max(dw, dh) + 0.37
    mid = dict(fx=f * 1.01, fy=f * 0.99, cx=0.5 * (sw - 1) + 0.31, cy=0.5 * (sh - 1) - 0.23, fx2=f, fy2=f, cx2=0.5 * (dw - 1) + 0.11,
               cy2=0.5 * (dh - 1) + 0.07)
    if kind == "identity":
        return R.camera(sw, sh, dw, dh)
    if kind == "shift_int":
        return R.camera(sw, sh, dw, dh, cx=3.0, cy=-2.0, cx2=0.0, cy2=0.0)
    if kind == "shift_half":                                  # (sx = u + 1.5, sy = v + 2.5: no pixel on a validity bound when the source is larger)
        return R.camera(sw, sh, dw, dh, cx=1.5, cy=2.5, cx2=0.0, cy2=0.0)
    if kind == "barrel":
        return R.camera(sw, sh, dw, dh, k1=-0.35, k2=0.11, k3=-0.013, **mid)
    if kind == "pincushion":
        return R.camera(sw, sh, dw, dh, k1=0.31, k2=0.052, **mid)
    if kind == "tangential":
        return R.camera(sw, sh, dw, dh, p1=0.021, p2=-0.017, **mid)
    if kind == "rot_partial":                                 # a wide view turned by 52 degrees: Z <= 0 in a part of the output
        wide = dict(mid, fx2=0.3 * max(dw, dh) + 0.013, fy2=0.3 * max(dw, dh) + 0.013)
        return R.camera(sw, sh, dw, dh, R=synth.rodrigues([0.013, 0.9, 0.11]), **wide)
    if kind == "rot_all":                                     # turned past 90 degrees: no pixel has coordinates
        return R.camera(sw, sh, dw, dh, R=synth.rodrigues([0.0, 3.0, 0.0]), **mid)
    if kind == "tiny":                                        # a source of one or two pixels a side under an 8 x 8 output
        return R.camera(sw, sh, dw, dh, fx=0.31 * sw, fy=0.29 * sh, cx=0.5 * (sw - 1) + 0.013, cy=0.5 * (sh - 1) - 0.017, k1=-0.004,
                        fx2=1.0, fy2=1.0, cx2=3.4, cy2=3.6)
    if kind == "zoom":                                        # an output three times its source, or a third of it
        s = dw / sw
        return R.camera(sw, sh, dw, dh, fx=f / s, fy=f / s, cx=0.5 * (sw - 1) + 0.21, cy=0.5 * (sh - 1) - 0.13, k1=-0.2, k2=0.04, p1=0.003,
                        fx2=f, fy2=f, cx2=0.5 * (dw - 1), cy2=0.5 * (dh - 1))
    raise ValueError(kind)


SIZES = [(1, 1), (70, 1), (1, 70), (8, 8), (31, 31), (32, 32), (33, 33), (65, 63), (63, 65)]           # (dst_width, dst_height)
KINDS = ("identity", "shift_int", "shift_half", "barrel", "pincushion", "tangential", "rot_partial", "rot_all")


@functools.lru_cache(maxsize=None)
def gpu_cameras():
    """name -> camera dict: every camera the GPU tests use."""
    out = {}
    for dw, dh in SIZES:
        out["identity_%dx%d" % (dw, dh)] = _cam("identity", dw, dh, dw, dh)
        out["barrel_%dx%d" % (dw, dh)] = _cam("barrel", dw + 6, dh + 4, dw, dh)
        out["rot_partial_%dx%d" % (dw, dh)] = _cam("rot_partial", dw + 2, dh + 5, dw, dh)
    for kind in KINDS:
        out["%s_65x63" % kind] = _cam(kind, 71, 67, 65, 63)
        out["%s_33x33" % kind] = _cam(kind, 39, 37, 33, 33)
    out["identity_65x63"] = _cam("identity", 65, 63, 65, 63)
    out["identity_33x33"] = _cam("identity", 33, 33, 33, 33)
    out["tiny_1x1"] = _cam("tiny", 1, 1, 8, 8)
    out["tiny_2x2"] = _cam("tiny", 2, 2, 8, 8)
    out["zoom_in"] = _cam("zoom", 22, 21, 66, 63)
    out["zoom_out"] = _cam("zoom", 130, 126, 65, 63)
    out["barrel_200x130"] = _cam("barrel", 210, 140, 200, 130)          # four tiles by nine of the smoothing kernel
    p = raw_pair()
    out["pair_left"], out["pair_right"] = pair_cameras()["left"], pair_cameras()["right"]
    assert p["left"].shape == (out["pair_left"]["src_height"], out["pair_left"]["src_width"])
    return out


@functools.lru_cache(maxsize=None)
def gpu_map(name):
    return R.make_map(gpu_cameras()[name])


@functools.lru_cache(maxsize=None)
def gpu_image(name):
    c = gpu_cameras()[name]
    return image_of(sum(name.encode()), c["src_height"], c["src_width"])


def test_the_gpu_cameras_are_what_their_tests_say():
    cams = gpu_cameras()
    for name, c in cams.items():
        m = gpu_map(name)
        n = m["valid"].size
        if name.startswith("rot_all"):
            assert not m["coords"].any(), name
        elif name.startswith("rot_partial") and n > 100:
            assert 0 < (~m["coords"]).sum() < n and 0 < m["valid"].sum() < n, name
        elif name.startswith(("identity", "barrel", "shift_half")):
            assert m["valid"].all(), name
        elif name.startswith(("shift_int", "pincushion", "tiny")):
            assert 0 < m["valid"].sum() < n, name
    assert (gpu_map("shift_half_65x63")["qx"] & 255 == 128).all() and (gpu_map("shift_int_65x63")["qx"] & 255 == 0).all()
    # sources of 1 x 1 and 2 x 2: every read clamps (both neighbours of a pair are the same pixel, or the pair is the whole source)
    for name in ("tiny_1x1", "tiny_2x2"):
        c, m = cams[name], gpu_map(name)
        ix = m["qx"][m["coords"]] >> 8
        assert c["src_width"] == c["src_height"] <= 2 and (ix < 0).any() and (ix + 1 > c["src_width"] - 1).any()
    assert cams["zoom_in"]["dst_width"] == 3 * cams["zoom_in"]["src_width"] and 2 * cams["zoom_out"]["dst_width"] == cams["zoom_out"]["src_width"]
    assert gpu_map("zoom_in")["valid"].sum() > 0.5 * gpu_map("zoom_in")["valid"].size
    # barrel at 65 x 63 reads between pixels everywhere: every subpixel phase occurs
    assert len(np.unique(gpu_map("barrel_65x63")["qx"] & 255)) > 200


def test_no_pixel_sits_on_a_rounding_or_validity_boundary():
    """What the equality of qx, qy and the valid bytes on the device rests on: over every camera of the GPU tests no sx 256 + 0.5 lies
    within 1e-8 of an integer and no sx, sy within 1e-8 of a validity bound.  A distance of exactly one half is the identity's and the
    shifts'.  No pixel is left out."""
    for name, c in gpu_cameras().items():
        m = gpu_map(name)
        for s, side in ((m["sx"], c["src_width"]), (m["sy"], c["src_height"])):
            s = s[m["coords"]]
            q = s * 256.0 + 0.5
            assert (np.abs(q - np.rint(q)) > 1e-8).all(), name
            assert (np.abs(s + 0.5) > 1e-8).all() and (np.abs(s - (side - 0.5)) > 1e-8).all(), name


def test_float64_figure():
    """The tolerance of the device's sx, sy is measured: the largest difference between the float64 and the np.longdouble evaluation
    of the map over the cameras of the GPU tests."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    worst, relative = {}, {}
    for name, c in gpu_cameras().items():
        m = gpu_map(name)
        lx, ly, lc = R.source_coordinates(c, dtype=np.longdouble)
        assert np.array_equal(lc, m["coords"]), name
        d = [(np.abs(lx[lc] - m["sx"][lc]), m["sx"][lc]), (np.abs(ly[lc] - m["sy"][lc]), m["sy"][lc])]
        worst[name] = float(max(x.max(initial=0.0) for x, _ in d))
        relative[name] = float(max((x / np.maximum(1.0, np.abs(s))).max(initial=0.0) for x, s in d))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:3]
    rel = sorted(relative.items(), key=lambda kv: -kv[1])[:3]
    print("longdouble against float64, the three largest:", top)
    print("... divided by max(1, |s|), the three largest:", rel)
    # the figure is the turned cameras': a pixel next to Z = 0 lies 1e5 source pixels out, and a double there is spaced 1e-11 apart
    assert top[0][1] <= R.F64_FIGURE <= 4 * top[0][1], top
    assert rel[0][1] <= R.F64_RELATIVE <= 4 * rel[0][1], rel
    assert R.DEVICE_TOLERANCE == 8 * R.F64_FIGURE and R.DEVICE_RELATIVE == 8 * R.F64_RELATIVE


def test_the_loops_take_more_than_one_pass():
    """k_rect_smooth's three block-strided loops and its tap loop (tests/test_gpu_image_rectify.py: test_loops_past_one_pass)."""
    for r in range(1, 8):
        assert (TILE_W + 2 * r) * (TILE_H + 2 * r) > BLOCK and TILE_W * (TILE_H + 2 * r) > BLOCK and TILE_W * TILE_H > BLOCK
        assert capi.smooth_taps(SIGMA_OF_RADIUS[r])[0] == r
    c = gpu_cameras()["barrel_200x130"]
    assert -(-c["dst_width"] // TILE_W) == 4 and -(-c["dst_height"] // TILE_H) == 9 and c["dst_width"] * c["dst_height"] > 100 * BLOCK
    assert (capi.RECTIFY_TILE, capi.RECTIFY_SUBPIXEL_BITS, capi.RECTIFY_NO_COORD) == ((TILE_W, TILE_H), R.SUBPIXEL_BITS, R.NO_COORD)


# ---- the C ABI: exports, argument checks before a device is asked for, no device
NAMES = ["slslam_rectify_default_options", "slslam_rectify_smooth_taps", "slslam_stereo_rectify", "slslam_image_rectifier_create",
         "slslam_image_rectifier_destroy", "slslam_image_rectifier_run", "slslam_image_rectifier_get_map", "slslam_image_rectifier_stats",
         "slslam_image_rectifier_timing", "slslam_rectify_images"]


def test_exports_and_defaults():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(L, name)
    o = capi.RectifyOptions(-1, -1, -1.0)
    L.slslam_rectify_default_options(C.byref(o))
    assert (o.border_mode, o.border_value, o.smooth_sigma) == (0, 0, 0.0)
    L.slslam_rectify_default_options(None)
    d = capi.rectify_options()
    assert (d.border_mode, d.border_value, d.smooth_sigma) == (0, 0, 0.0)
    assert capi.rectify_options("replicate", 5, 1.5).border_mode == 1 == R.REPLICATE
    assert C.sizeof(capi.RectifyCamera) == 192 and C.sizeof(capi.StereoRig) == 288


def bad_cameras():
    good = dict(src_width=16, src_height=12)
    nan = float("nan")
    over = [dict(fx=0.0), dict(fy=-1.0), dict(fx2=0.0), dict(fy2=nan), dict(cx=nan), dict(k1=float("inf")), dict(p2=nan),
            dict(R=np.full((3, 3), nan)), dict(src_width=0), dict(src_height=8193), dict(dst_width=0), dict(dst_height=8193)]
    return [capi.RectifyCamera.make(**dict(good, **o)) for o in over]


def test_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    good, cam = capi.rectify_options(), capi.RectifyCamera.make(16, 12)
    for bad in (capi.rectify_options(2), capi.rectify_options(-1), capi.rectify_options(0, 256), capi.rectify_options(0, -1),
                capi.rectify_options(0, 0, -0.5), capi.rectify_options(0, 0, float("nan")), capi.rectify_options(0, 0, 16.5)):
        assert L.slslam_image_rectifier_create(-1, C.byref(bad), 1, C.byref(cam), 1, 100, C.byref(h)) == INVALID_ARGUMENT
    for bad in bad_cameras():
        assert L.slslam_image_rectifier_create(-1, C.byref(good), 1, C.byref(bad), 1, 100, C.byref(h)) == INVALID_ARGUMENT
        both = capi._camera_array([cam, bad])
        assert L.slslam_image_rectifier_create(-1, C.byref(good), 2, both, 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_create(-1, None, 1, C.byref(cam), 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_create(-1, C.byref(good), 1, None, 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_create(-1, C.byref(good), 1, C.byref(cam), 1, 100, None) == INVALID_ARGUMENT
    for n in (0, -1, 65):
        assert L.slslam_image_rectifier_create(-1, C.byref(good), n, capi._camera_array([cam] * 65), 1, 100, C.byref(h)) == INVALID_ARGUMENT
    for args in ((0, 100), (1, 0), (-1, 100), (1, 8192 * 8192 + 1), (17, 8192 * 8192)):
        assert L.slslam_image_rectifier_create(-1, C.byref(good), 1, C.byref(cam), *args, C.byref(h)) == INVALID_ARGUMENT, args
    big = capi.RectifyCamera.make(16, 12, 8192, 8192)                                  # five outputs of 2^26 pixels: more than 2^28 of maps
    assert L.slslam_image_rectifier_create(-1, C.byref(good), 5, capi._camera_array([big] * 5), 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert not h
    assert L.slslam_image_rectifier_create(-1, C.byref(good), 4, capi._camera_array([big] * 4), 16, 8192 * 8192, C.byref(h)) == 0   # the limits; no device
    ms = C.c_double(-1.0)
    assert L.slslam_image_rectifier_timing(h, -1, C.byref(ms)) == 0 and ms.value == 0.0
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_image_rectifier_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    assert L.slslam_image_rectifier_stats(None, None, None) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_timing(None, 0, None) == INVALID_ARGUMENT
    L.slslam_image_rectifier_destroy(h)
    L.slslam_image_rectifier_destroy(None)


def _frame(cams, k, img, **over):
    fr, res, keep = capi._rectify_frame(cams, k, img, True)
    keep[1]["image"][...] = 7
    keep[1]["valid"][...] = 7
    keep[1]["num_valid"][...] = -7
    for name, v in over.items():
        setattr(res if name.startswith("res_") else fr, name.replace("res_", ""), v)
    return fr, res, keep


def _untouched(keep):
    return (keep[1]["image"] == 7).all() and (keep[1]["valid"] == 7).all() and keep[1]["num_valid"][0] == -7


def test_run_arguments_and_no_device():
    L = capi.lib()
    cams = [capi.RectifyCamera.make(16, 12), capi.RectifyCamera.make(20, 10, 8, 6)]
    arr, opt = capi._camera_array(cams), capi.rectify_options()
    h = C.c_void_p()
    assert L.slslam_image_rectifier_create(-1, C.byref(opt), 2, arr, 2, 16 * 12, C.byref(h)) == 0
    img = image_of(6, 12, 16)
    null = C.POINTER(C.c_ubyte)()
    for over in (dict(camera=-1), dict(camera=2), dict(stride=15), dict(stride=2 ** 31), dict(image=null), dict(res_image=null),
                 dict(res_stride=15), dict(camera=1)):                                 # (camera 1 reads 20 bytes a row: the stride of 16 is too small)
        fr, res, keep = _frame(cams, 0, img, **over)
        assert L.slslam_image_rectifier_run(h, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert L.slslam_rectify_images(C.byref(opt), 2, arr, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert _untouched(keep)
    fr, res, keep = _frame(cams, 0, img)
    assert L.slslam_image_rectifier_run(None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_run(h, -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_run(h, 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_run(h, 1, C.byref(fr), None) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(None, 2, arr, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(capi.rectify_options(3)), 2, arr, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 0, arr, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 2, None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 1, C.byref(bad_cameras()[0]), 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 2, arr, -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 2, arr, 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_rectify_images(C.byref(opt), 2, arr, 1, C.byref(fr), None) == INVALID_ARGUMENT
    q = np.full((12, 16), -7, dtype=np.int32)
    assert L.slslam_image_rectifier_get_map(None, 0, capi._ip(q), None, None, None, None) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_get_map(h, 2, capi._ip(q), None, None, None, None) == INVALID_ARGUMENT
    assert L.slslam_image_rectifier_get_map(h, -1, capi._ip(q), None, None, None, None) == INVALID_ARGUMENT
    assert _untouched(keep) and (q == -7).all()
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_image_rectifier_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    with pytest.raises(ValueError):
        capi.rectify_images(cams, [(1, img)])                    # the wrapper: a frame has its camera's source size

    if capi.device_count() == 0:                                # every compute entry point says so, and leaves its outputs alone
        assert L.slslam_image_rectifier_run(h, 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        assert L.slslam_image_rectifier_run(h, 0, None, None) == NO_DEVICE
        assert L.slslam_image_rectifier_get_map(h, 0, capi._ip(q), None, None, None, None) == NO_DEVICE and (q == -7).all()
        assert L.slslam_rectify_images(C.byref(opt), 2, arr, 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        r = capi.ImageRectifier(cams, max_frames=1, max_pixels=16 * 12)
        for call in (lambda: r.run([(0, img)]), lambda: r.get_map(0), lambda: capi.rectify_images(cams, [(0, img)]),
                     lambda: capi.rectify_detect_describe_pair_and_track(r, None, None, None, None, [(img, img)], cameras=(0, 0))):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert r.stats() == {"calls": 0, "allocations": 0}
        r.close()
    L.slslam_image_rectifier_destroy(h)


# ---- the host half (csrc/image_rectify_layout.h) under the sanitizers, as a stand-alone program
def test_host_half_under_the_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "image_rectify_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "image_rectify_layout_check.cpp"), "-o", exe])
    # the program's input: a camera (22 doubles and 4 sizes), then "camera index" per frame of a call over that camera twice
    c = gpu_cameras()["rot_partial_33x33"]
    args = ["%.17g" % v for v in ref_array(c)[:22]] + [str(c[k]) for k in ("src_width", "src_height", "dst_width", "dst_height")]
    frames = [0, 1, 1, 0, 0]
    r = subprocess.run([exe] + args + [str(f) for f in frames], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "image rectify layout ok" in r.stdout
    lines = r.stdout.splitlines()
    # the layout against numpy's: frames at multiples of 256 bytes
    al = lambda n: -(-n // 256) * 256  # noqa: E731
    ns, nd = al(c["src_width"] * c["src_height"]), al(c["dst_width"] * c["dst_height"])
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("frame ")]
    assert got == [(i * ns, i * nd, f) for i, f in enumerate(frames)]
    sizes = dict(ln.split()[1:] for ln in lines if ln.startswith("size "))
    F = len(frames)
    assert int(sizes["off_src"]) == al(24 * F) and int(sizes["in_bytes"]) == al(24 * F) + F * ns == int(sizes["off_out"])
    assert int(sizes["out_bytes"]) == F * nd and int(sizes["dev"]) == int(sizes["host"]) == al(24 * F) + F * ns + F * nd
    # the map as the host compiles it against numpy's, bit for bit (the device compiles the same function)
    m = gpu_map("rot_partial_33x33")
    rows = np.array([[float.fromhex(v) if "x" in v or "nan" in v else int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("map ")])
    assert rows.shape == (33 * 33, 5)
    assert np.array_equal(rows[:, 0].astype(np.int64), m["qx"].reshape(-1)) and np.array_equal(rows[:, 1].astype(np.int64), m["qy"].reshape(-1))
    assert np.array_equal(rows[:, 2].astype(np.uint8), m["valid"].reshape(-1))
    assert np.array_equal(rows[:, 3], m["sx"].reshape(-1), equal_nan=True) and np.array_equal(rows[:, 4], m["sy"].reshape(-1), equal_nan=True)
    # the taps and the rig as the program prints them against the library's
    for ln in lines:
        if ln.startswith("taps "):
            v = ln.split()
            r_, t_ = capi.smooth_taps(float(v[1]))
            assert [int(x) for x in v[2:]] == [r_] + t_.tolist()
    assert sum(ln.startswith("taps ") for ln in lines) == 7


# ---- the accuracy of the contract: raw images of a rig through rectifier, detector, MSLD and stereo matcher, all numpy
PAIR_SEED = 3
PAIR_SIGMA = 0.6
PAIR_STEREO = dict(max_disparity=16.0)
PAIR_RAW_RIGHT_ON_RECTIFIED_LINES = 0    # drawn edges a detection of the RAW right image follows on its rectified line: measured
PAIR_RAW_RIGHT_STRAIGHT = 6      # ... on the chord of the edge as it lies in the raw image, within the bound: measured
PAIR_EDGES_FOUND = (8, 8)        # drawn edges found in the rectified left and right image: measured
PAIR_MATCHED = 7                 # stereo pairs of the same drawn edge: measured
PAIR_WORST = 0.19                # px, the largest distance of an end point of such a detection from its drawn line: measured
PAIR_BOUND = 2 * PAIR_WORST


# the drawn edges in rectified left coordinates: those of the detector's accuracy test, none crossing another
PAIR_EDGES = np.array([[20.3, 18.7, 70.9, 30.2], [120.6, 15.1, 95.2, 70.8], [30.4, 60.3, 30.9, 120.7], [60.2, 130.6, 150.8, 110.3],
                       [180.5, 40.2, 200.1, 90.6], [90.7, 95.4, 140.3, 60.9], [170.3, 130.2, 205.7, 145.8], [140.5, 10.5, 165.5, 35.5]])


@functools.lru_cache(maxsize=None)
def raw_pair():
    return synth.make_raw_stereo_pair(PAIR_SEED, segments=PAIR_EDGES)


@functools.lru_cache(maxsize=None)
def pair_cameras():
    p = raw_pair()
    return R.stereo_rectify(p["rig"]["left"], p["rig"]["right"], p["rig"]["R"], p["rig"]["t"])


def on_line(seg, line, beyond=6.0):
    """The larger distance of the detection's two end points from the drawn line when both lie along the drawn segment; else inf."""
    length = np.hypot(line[2] - line[0], line[3] - line[1])
    ex, ey = (line[2] - line[0]) / length, (line[3] - line[1]) / length
    worst = 0.0
    for p in (seg[:2], seg[2:]):
        along = (p[0] - line[0]) * ex + (p[1] - line[1]) * ey
        if not -beyond <= along <= length + beyond:
            return np.inf
        worst = max(worst, abs((p[0] - line[0]) * ey - (p[1] - line[1]) * ex))
    return worst


def owners(segments, lines, bound):
    """Per detection the drawn line it follows within `bound` (-1: none) and its distance."""
    own, dist = [], []
    for s in np.asarray(segments, dtype=np.float64):
        d = [on_line(s, ln) for ln in lines]
        k = int(np.argmin(d)) if len(d) else -1
        own.append(k if k >= 0 and d[k] <= bound else -1)
        dist.append(d[k] if k >= 0 else np.inf)
    return np.array(own, dtype=np.int64), np.array(dist)


@functools.lru_cache(maxsize=None)
def pair_chain():
    """The reference chain on the raw pair: rectify with smoothing, detect, describe, pair, track one frame."""
    p, cams = raw_pair(), pair_cameras()
    r, t = capi.smooth_taps(PAIR_SIGMA)
    rect = [R.rectify(p[side], cams[side], R.REPLICATE, 0, r, t)["image"] for side in ("left", "right")]
    found = [LSD.detect(im) for im in rect]
    desc = [MSLD.describe(im, f["segments"].astype(np.float32)) for im, f in zip(rect, found)]
    rows = [np.nonzero(np.array([x == MSLD.OK for x in d["status"]], dtype=bool))[0] for d in desc]
    sides = [(f["segments"][k].astype(np.float32), d["descriptors"][k].astype(np.float32).reshape(len(k), -1))
             for f, d, k in zip(found, desc, rows)]
    k = {n: cams[n] for n in ("fx", "fy", "cx", "cy")}
    stereo = SR.match(sides[0][0], sides[0][1], sides[1][0], sides[1][1], **dict(PAIR_STEREO, **k))
    track = TR.track([sides[0]])[0]
    obs, idx = SR.observations(stereo)
    return dict(rectified=rect, found=found, rows=rows, sides=sides, stereo=stereo, track=track, observations=obs, index=idx,
                ids=track["id"][idx])


def test_make_raw_stereo_pair():
    p, q = raw_pair(), synth.make_raw_stereo_pair(PAIR_SEED, segments=PAIR_EDGES)
    assert np.array_equal(p["left"], q["left"]) and np.array_equal(p["right"], q["right"]) and p["left"].dtype == np.uint8
    cams = pair_cameras()
    assert np.abs(cams["left"]["R"] - p["Rl"]).max() < 1e-15 and np.abs(cams["right"]["R"] - p["Rr"]).max() < 1e-15
    assert abs(cams["baseline"] - p["baseline"]) < 1e-15 and cams["fx"] == p["focal"] and (cams["cx"], cams["cy"]) == (p["cx"], p["cy"])
    assert np.abs(p["Rr"] - np.eye(3)).max() > 0.01 and abs(p["rig"]["right"]["k1"]) > 0.1       # rotated and distorted
    assert np.array_equal(p["left_segments"][:, 1::2], p["right_segments"][:, 1::2])              # common rows after rectification
    d = p["left_segments"][:, 0] - p["right_segments"][:, 0]
    assert np.abs(d - p["disparity"]).max() < 1e-12 and (d >= 4.0).all() and (d <= 14.0).all()
    # every pixel of the rectified views has a source: the lenses are barrel lenses
    assert R.make_map(cams["left"])["valid"].all() and R.make_map(cams["right"])["valid"].all()


def to_raw(cam, pts):
    """Rectified pixel positions [n, 2] in the raw image of `cam`: the map of the header at positions that are not integers."""
    x, y = (pts[:, 0] - cam["cx2"]) / cam["fx2"], (pts[:, 1] - cam["cy2"]) / cam["fy2"]
    X = np.stack([x, y, np.ones_like(x)], axis=1) @ cam["R"]                           # R^T (x, y, 1)
    x, y = X[:, 0] / X[:, 2], X[:, 1] / X[:, 2]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (cam["k1"] + r2 * (cam["k2"] + r2 * cam["k3"]))
    xd = x * rad + 2.0 * cam["p1"] * x * y + cam["p2"] * (r2 + 2.0 * x * x)
    yd = y * rad + cam["p1"] * (r2 + 2.0 * y * y) + 2.0 * cam["p2"] * x * y
    return np.stack([cam["fx"] * xd + cam["cx"], cam["fy"] * yd + cam["cy"]], axis=1)


def paired_rows(c, same):
    """Per matched pair of `same` the differences of the rows of the two detections' end points, first against first (the right
    segment turned to the left one's direction)."""
    ls, rs = c["sides"][0][0].astype(np.float64), c["sides"][1][0].astype(np.float64)
    out = []
    for a in same:
        A, B = ls[a], rs[c["stereo"]["match"][a]]
        if (A[2] - A[0]) * (B[2] - B[0]) + (A[3] - A[1]) * (B[3] - B[1]) < 0:
            B = B[[2, 3, 0, 1]]
        out.append([A[1] - B[1], A[3] - B[3]])
    return np.array(out)


def test_accuracy_of_the_contract_on_a_raw_pair():
    p, c, cams = raw_pair(), pair_chain(), pair_cameras()
    # the raw right image.  Where the drawn edges lie in it: their end points through the map, the chord between them, and how far the
    # curve an edge has become leaves that chord
    n = len(p["right_segments"])
    ends = to_raw(cams["right"], p["right_segments"].reshape(-1, 2)).reshape(n, 4)
    sag = []
    for seg, chord in zip(p["right_segments"], ends):
        t = np.linspace(0.0, 1.0, 65)[:, None]
        curve = to_raw(cams["right"], seg[:2] + t * (seg[2:] - seg[:2]))
        d = (chord[2:] - chord[:2]) / np.hypot(*(chord[2:] - chord[:2]))
        sag.append(np.abs((curve[:, 0] - chord[0]) * d[1] - (curve[:, 1] - chord[1]) * d[0]).max())
    raw = LSD.detect(p["right"])
    on_rect, _ = owners(raw["segments"], p["right_segments"], PAIR_BOUND)
    on_chord, dist = owners(raw["segments"], ends, PAIR_BOUND)
    followed = set(on_chord[on_chord >= 0].tolist())
    print("raw right image: %d OK segments; %d of %d drawn edges on their rectified lines within %.2f px; %d on the chord of the edge as "
          "it lies in the raw image; the edges leave their chords by %.2f to %.2f px" % (raw["num_ok"], len(set(on_rect[on_rect >= 0].tolist())),
                                                                                        n, PAIR_BOUND, len(followed), min(sag), max(sag)))
    assert len(set(on_rect[on_rect >= 0].tolist())) == PAIR_RAW_RIGHT_ON_RECTIFIED_LINES
    assert len(followed) == PAIR_RAW_RIGHT_STRAIGHT, (followed, sag)
    worst, count = 0.0, []
    labels = []
    for f, lines in zip(c["found"], (p["left_segments"], p["right_segments"])):
        own, dist = owners(f["segments"], lines, PAIR_BOUND)
        labels.append(own)
        count.append(len(set(own[own >= 0].tolist())))
        worst = max(worst, float(dist[own >= 0].max()))
    print("rectified pair: drawn edges found %s of %d, largest end point distance %.3f px (bound %.2f)" % (count, n, worst, PAIR_BOUND))
    assert tuple(count) == PAIR_EDGES_FOUND and worst <= PAIR_BOUND and PAIR_WORST <= 2 * worst
    # matched pairs: the same drawn edge on both sides
    m = c["stereo"]["match"]
    la, lb = labels[0][c["rows"][0]], labels[1][c["rows"][1]]
    same = [a for a in np.nonzero(m >= 0)[0] if la[a] >= 0 and la[a] == lb[m[a]]]
    wrong = [a for a in np.nonzero(m >= 0)[0] if la[a] >= 0 and lb[m[a]] >= 0 and la[a] != lb[m[a]]]
    print("stereo pairs %d, of the same drawn edge %d, of two different ones %d" % ((m >= 0).sum(), len(same), len(wrong)))
    assert len(same) == PAIR_MATCHED and not wrong
    # ... and the rows of their end points are equal within the same bound
    rows = paired_rows(c, same)
    print("end point rows of the matched pairs, left - right:", np.round(rows, 3).tolist())
    assert np.abs(rows).max() <= PAIR_BOUND, rows
    # ... and at the rows of the left end points the two differ along x by the drawn disparity: two bounds, taken along x, every pair
    for a in same:
        line = p["left_segments"][la[a]]
        ey = abs(line[3] - line[1]) / np.hypot(line[2] - line[0], line[3] - line[1])
        assert ey > 0.2 and np.abs(c["stereo"]["disparity"][a] - p["disparity"][la[a]]).max() <= 2 * PAIR_BOUND / ey, a
    assert c["observations"].shape == ((m >= 0).sum(), 8) and len(c["ids"]) == (m >= 0).sum()

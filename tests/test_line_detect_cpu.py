"""The line segment detector without a device (include/slslam_hip.h: slslam_line_detector_*, slslam_detect_lines): hand-computed cases that
pin the numpy reference (tests/line_detect_reference.py), its accuracy on edges at known sub-pixel positions, the chain detector ->
MSLD -> matcher on the synthetic pair, every argument check of the C ABI (made before a device is asked for), SLSLAM_ERR_NO_DEVICE on a
machine without one, the host layout under the sanitizers as a stand-alone program, and the measurement behind the GPU tests' tolerance.
The inputs of tests/test_gpu_line_detect.py are made here (gpu_inputs), so that the tolerance is measured on exactly them."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as DM  # noqa: E402
import line_descriptor_reference as MSLD  # noqa: E402
import line_detect_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARGUMENT, NO_DEVICE = 1, 2
T = capi.LSD_TILE
# kChunk and kBlock of csrc/line_detect_layout.h (test_the_gpu_inputs_are_what_their_tests_say reads them there): a block of the per-pixel
# kernels takes CHUNK pixels; k_scan, k_emit and k_fit take BLOCK chunks or slots a pass or a block
CHUNK, BLOCK = 1024, 256
MAX_SEGMENTS = capi.line_detect_options().max_segments    # the default, 512: what a run without the option truncates at
SUMS =("n", "sw", "swu", "swv", "swuu", "swuv", "swvv", "sgx", "sgy")


# ---- hand-computed cases
def step_image(height=100, negated=False, size=16):
    """size x size: 0 left of column 8, `height` from it on; negated: 255 - that.  gx = height (-height) at columns 7 and 8, gy = 0."""
    img = np.zeros((size, size), np.uint8)
    img[:, 8:] = height
    return 255 - img if negated else img


def test_vertical_step_by_hand():
    """32 strong pixels of gradient (100, 0), columns 7 and 8 of every row: one component of label 7.  About (7, 0): u in {0, 1}, v in
    0 .. 15, w = 100.  c = (0.5, 7.5), sxx = 0.25, syy = 21.25, sxy = 0: h = -10.5, the axis (0, 1), lmin = 0.25, thickness 0.5; t = v - 7.5,
    length 15, the end points (7.5, 0) and (7.5, 15); ex Sgy - ey Sgx = -3200 < 0 swaps them."""
    r = R.detect(step_image())
    assert r["num_components"] == 1 and r["num_ok"] == 1 and r["num_written"] == 1 and r["status_counts"] == [1, 0, 0, 0, 0]
    assert r["all"][0]["label"] == 7 and r["label"].tolist() == [7] and r["pixels"].tolist() == [32]
    assert r["all"][0]["sums"] == dict(n=32, sw=3200, swu=1600, swv=24000, swuu=1600, swuv=12000, swvv=248000, sgx=3200, sgy=0)
    assert r["segments"].tolist() == [[7.5, 15.0, 7.5, 0.0]]
    assert (r["length"].tolist(), r["thickness"].tolist(), r["strength"].tolist()) == ([15.0], [0.5], [100.0])
    want = np.full((16, 16), -1, np.int32)
    want[:, 7:9] = 7
    assert np.array_equal(r["labels"], want) and r["labels"].dtype == np.int32
    # the negated image: the same segment with its end points swapped
    n = R.detect(step_image(negated=True))
    assert n["segments"].tolist() == [[7.5, 0.0, 7.5, 15.0]] and n["all"][0]["sums"]["sgx"] == -3200
    assert np.array_equal(n["labels"], want) and n["length"].tolist() == [15.0]
    # cross(p1 - p0, G) >= 0 in both
    for d in (r, n):
        x0, y0, x1, y1 = d["segments"][0]
        g = d["all"][0]["sums"]
        assert (x1 - x0) * g["sgy"] - (y1 - y0) * g["sgx"] >= 0


def test_threshold_is_on_the_scale_that_is_not_halved():
    """A step of height T has the difference T - the halved central difference T / 2 of the MSLD gradient - and is strong; one grey level
    below it nothing is."""
    at = R.detect(step_image(height=24))
    assert at["num_components"] == 1 and (at["labels"] >= 0).sum() == 32 and at["strength"].tolist() == [24.0]
    below = R.detect(step_image(height=23))
    assert below["num_components"] == 0 and (below["labels"] == -1).all()
    assert R.detect(step_image(height=23), grad_threshold=23)["num_components"] == 1


def test_tolerance_by_hand():
    """ga = (8, 0) against gb = (8, k): dot = 64, cross = 8 k, 64 (8 k)^2 <= 11 64^2 iff k^2 <= 11: k = 3 is inside, k = 4 outside."""
    assert R.linked(8, 0, 8, 3, 11, 64) and R.linked(8, 0, 8, -3, 11, 64)
    assert not R.linked(8, 0, 8, 4, 11, 64) and not R.linked(8, 0, 8, -4, 11, 64)
    assert R.linked(2, 0, 2, 1, 1, 4) and not R.linked(2, 0, 2, 1, 1, 5)             # equality links: 4 2^2 = 1 4^2
    assert not R.linked(8, 0, -8, 0, 11, 64) and not R.linked(8, 0, 0, 8, 11, 64)    # opposite, orthogonal (dot = 0)
    assert R.linked(255, 255, 255, 255, 2 ** 20, 2 ** 20)                             # the largest terms stay inside int64
    # in an image: I = 4 x + k y with row 0 a copy of row 1 has the gradient (8, 0) in row 0 and (8, k) in row 1; the link S joins them
    for k, joined in ((3, True), (4, False)):
        yy, xx = np.mgrid[0:6, 0:12]
        img = (4 * xx + k * yy).astype(np.uint8)
        img[0] = img[1]
        gx, gy, strong, links = R.link_planes(img, grad_threshold=8)
        assert (gx[0, 3], gy[0, 3], gx[1, 3], gy[1, 3]) == (8, 0, 8, k) and strong[0, 3] and strong[1, 3]
        assert links[2][0, 3] == joined


def test_corner_border_and_constant():
    # a 90 degree corner: the two edges are a component each; the corner pixel (8, 8) has the gradient (100, 100) and joins neither
    img = np.zeros((24, 24), np.uint8)
    img[8:, 8:] = 100
    r = R.detect(img)
    assert r["num_ok"] == 2 and r["status_counts"][0] == 2 and r["num_components"] == 3 and r["status_counts"][1] == 1
    ax = np.abs(r["segments"][:, 2:] - r["segments"][:, :2])
    # (column 7 carries its edge from row 8 and column 8 from row 9, so the axes lean a little: one nearly vertical, one nearly horizontal)
    assert sorted((ax[:, 0] < 0.5).tolist()) == [False, True] and sorted((ax[:, 1] < 0.5).tolist()) == [False, True]
    assert (r["length"] > 14).all()
    assert r["labels"][8, 8] == 8 * 24 + 8 and (r["labels"] == 8 * 24 + 8).sum() == 1
    # the replicated border: an edge between rows 0 and 1 - gy = I(1) - I(0) in row 0, I(2) - I(0) in row 1
    img = np.full((12, 20), 100, np.uint8)
    img[0] = 0
    r = R.detect(img)
    assert r["num_components"] == 1 and r["label"].tolist() == [0] and r["pixels"].tolist() == [40]
    assert r["segments"].tolist() == [[0.0, 0.5, 19.0, 0.5]] and r["thickness"].tolist() == [0.5]
    # a constant image
    r = R.detect(np.full((9, 13), 77, np.uint8))
    assert r["num_components"] == 0 and r["num_ok"] == 0 and r["status_counts"] == [0] * 5 and (r["labels"] == -1).all()
    assert r["segments"].shape == (0, 4) and r["length"].shape == (0,)


def test_status_order():
    """SMALL before ISOTROPIC before SHORT before THICK before OK, on the step (n = 32, length 15, thickness 0.5)."""
    img = step_image()
    status = lambda **o: R.detect(img, **o)["all"][0]["status"]  # noqa: E731
    assert status() == R.OK
    assert status(max_thickness=0.4) == R.THICK and status(max_thickness=0.5) == R.OK
    assert status(min_length=15.5) == R.SHORT and status(min_length=15.0) == R.OK
    assert status(min_length=15.5, max_thickness=0.4) == R.SHORT
    assert status(min_pixels=33, min_length=15.5, max_thickness=0.4) == R.SMALL and status(min_pixels=32) == R.OK
    # two rows of the step: a 2 x 2 block of equal weights, sxx = syy, sxy = 0, no axis - isotropic before it is short
    two = step_image()[:2]
    r = R.detect(two, min_pixels=4)
    assert r["all"][0]["status"] == R.ISOTROPIC and r["status_counts"] == [0, 0, 1, 0, 0] and r["num_ok"] == 0
    assert R.detect(two, min_pixels=5)["all"][0]["status"] == R.SMALL
    assert R.STATUS == [R.OK, R.SMALL, R.ISOTROPIC, R.SHORT, R.THICK] and capi.LSD_STATUS == dict(enumerate(R.STATUS))


def test_isqrt():
    k = np.arange(1, 362, dtype=np.int64)
    assert np.array_equal(R.isqrt(k * k - 1), k - 1) and np.array_equal(R.isqrt(k * k), k) and np.array_equal(R.isqrt(k * k + 1), k)
    assert R.isqrt(0) == 0 and R.isqrt(2 * 255 * 255) == 360


def test_truncation_keeps_the_first():
    img = gpu_inputs()["field_63x65"][0]
    full = R.detect(img)
    cut = R.detect(img, max_segments=2)
    assert full["num_ok"] > 2 and cut["num_ok"] == full["num_ok"] and cut["num_written"] == 2
    assert np.array_equal(cut["segments"], full["segments"][:2]) and np.array_equal(cut["label"], full["label"][:2])
    assert (np.diff(full["label"]) > 0).all()


# ---- accuracy on edges at known sub-pixel positions
EDGES = np.array([[20.3, 18.7, 70.9, 30.2], [120.6, 15.1, 95.2, 70.8], [30.4, 60.3, 30.9, 120.7], [60.2, 130.6, 150.8, 110.3],
                  [180.5, 40.2, 200.1, 90.6], [90.7, 95.4, 140.3, 60.9], [170.3, 130.2, 205.7, 145.8], [140.5, 10.5, 165.5, 35.5]])
# the largest distance of a detected end point from the line it was drawn on, over EDGES: measured 0.513 px on the
# near-vertical edge, 0.05 to 0.35 px on the others
EDGE_DISTANCE_OBSERVED = 0.52
EDGE_DISTANCE_BOUND = 2 * EDGE_DISTANCE_OBSERVED


def edge_image():
    return synth.make_edge_image(160, 224, EDGES, amplitude=[60, -60, 70, -50, 60, -70, 55, 65], softness=1.5)


def line_distance(seg, p):
    d = (seg[2:] - seg[:2]) / np.hypot(*(seg[2:] - seg[:2]))
    return abs((p[0] - seg[0]) * d[1] - (p[1] - seg[1]) * d[0])


def owner(drawn, seg, reach=2.0, beyond=6.0):
    """The drawn segment that the detection `seg` lies on: both end points within `reach` of its line and no more than `beyond` past
    its ends (a drawn edge fades out over a few pixels); -1: none."""
    for i, s in enumerate(np.asarray(drawn, dtype=np.float64)):
        length = np.hypot(*(s[2:] - s[:2]))
        d = (s[2:] - s[:2]) / length
        along = [(p[0] - s[0]) * d[0] + (p[1] - s[1]) * d[1] for p in (seg[:2], seg[2:])]
        if all(line_distance(s, p) <= reach for p in (seg[:2], seg[2:])) and all(-beyond <= a <= length + beyond for a in along):
            return i
    return -1


def test_make_edge_image_and_accuracy():
    img = edge_image()
    assert img.dtype == np.uint8 and img.shape == (160, 224) and img[0, 0] == 118 and np.array_equal(img, edge_image())
    gx, gy = R.gradients(img)
    r = R.detect(img)
    worst, found = 0.0, set()
    for seg in r["segments"]:
        i = owner(EDGES, seg)
        assert i >= 0
        found.add(i)
        worst = max(worst, line_distance(EDGES[i], seg[:2]), line_distance(EDGES[i], seg[2:]))
        # the peak gradient along the drawn edge is at least 2 T
        assert np.hypot(gx, gy)[int(round((EDGES[i][1] + EDGES[i][3]) / 2)), int(round((EDGES[i][0] + EDGES[i][2]) / 2))] >= 48
    print("edges found %d of %d, detections %d, largest end-point distance %.4f px" % (len(found), len(EDGES), r["num_ok"], worst))
    assert found == set(range(len(EDGES)))                   # every edge is found
    assert worst <= EDGE_DISTANCE_BOUND and EDGE_DISTANCE_BOUND <= 4 * worst
    # each detection covers most of its edge
    for seg, length in zip(r["segments"], r["length"]):
        e = EDGES[owner(EDGES, seg)]
        assert length >= 0.8 * np.hypot(*(e[2:] - e[:2])) - 2


# ---- the chain on the synthetic pair: detect, describe, match
PAIR_SEED, PAIR_RATIO, PAIR_MAX_DISTANCE = 3, 1.5, 0.25
CHAIN_TRUE_MATCHES = 9           # mutual matches that join detections of the same drawn edge, on the reference: recorded, not chosen


@functools.lru_cache(maxsize=None)
def pair():
    return synth.make_line_image_pair(PAIR_SEED, 160, 224, 20, max_length=60)


def true_matches(p, seg_a, seg_b, match):
    """Of the matches a -> match[a], those that join detections of the same drawn edge."""
    own_a = [owner(p["segments"], s) for s in np.asarray(seg_a, dtype=np.float64)]
    own_b = [int(p["truth"][owner(p["segments2"][p["truth"]], s)]) if owner(p["segments2"][p["truth"]], s) >= 0 else -1
             for s in np.asarray(seg_b, dtype=np.float64)]
    second = {int(p["truth"][i]): i for i in range(len(p["truth"]))}             # row of the second view -> drawn edge
    return sum(1 for a, b in enumerate(match) if b >= 0 and own_a[a] >= 0 and own_b[b] >= 0 and second[own_b[b]] == own_a[a])


@functools.lru_cache(maxsize=None)
def chain_reference():
    p = pair()
    a, b = R.detect(p["image"]), R.detect(p["image2"])
    da = MSLD.describe(p["image"], a["segments"].astype(np.float32))
    db = MSLD.describe(p["image2"], b["segments"].astype(np.float32))
    m = DM.match(da["descriptors"].astype(np.float32), db["descriptors"].astype(np.float32), PAIR_RATIO, PAIR_MAX_DISTANCE)
    return a, b, da, db, m


def test_chain_on_the_pair():
    p = pair()
    a, b, da, db, m = chain_reference()
    assert set(da["status"]) <= {MSLD.OK, MSLD.FLAT} and set(db["status"]) <= {MSLD.OK, MSLD.FLAT}
    n = true_matches(p, a["segments"], b["segments"], m["match"])
    print("detections %d and %d, mutual matches %d, of the same drawn edge %d" % (a["num_ok"], b["num_ok"], m["num_matched"], n))
    assert n == CHAIN_TRUE_MATCHES and n >= 1
    # orientation: over the three rows about a detected segment the MSLD polarity is positive, so orient = 1 leaves the segment as it is
    # (over the default 45 rows the polarity also sums the texture and the far flanks of these synthetic edges, and may have either sign)
    pol = MSLD.describe(p["image"], a["segments"].astype(np.float32), bands=1, band_width=3, orient=False)["polarity"]
    assert (pol > 1.0).all(), pol


# ---- the inputs of the GPU tests: name -> (image, options)
def field(seed, height, width, sigma=2.0, contrast=900.0):
    """Smoothed noise: strong gradients whose direction changes slowly, components of every shape."""
    rng = np.random.default_rng(np.random.SeedSequence([18, int(seed)]))
    val = 118.0 + contrast * gaussian_filter(rng.standard_normal((height, width)), sigma, mode="reflect")
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def diagonal_image(size=200):
    """A step across the main diagonal: the strong pixels are x in {y, y + 1}, every gradient (180, -180) away from the corners."""
    yy, xx = np.mgrid[0:size, 0:size]
    return np.where(xx > yy, 200, 20).astype(np.uint8)


def serpentine_image():
    """64 x 64: a band of half-width 3.5 about a centre line that runs right along y = 10, turns through a half circle of radius 8, runs
    left along y = 26, turns, runs right along y = 42; smoothed.  Its outline is one closed edge far longer than the image's side."""
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    pts = [(x, 10.0) for x in np.arange(14, 50.01, 0.25)]
    pts += [(50 + 8 * np.sin(a), 18 - 8 * np.cos(a)) for a in np.linspace(0, np.pi, 120)]
    pts += [(x, 26.0) for x in np.arange(50, 13.99, -0.25)]
    pts += [(14 - 8 * np.sin(a), 34 - 8 * np.cos(a)) for a in np.linspace(0, np.pi, 120)]
    pts += [(x, 42.0) for x in np.arange(14, 50.01, 0.25)]
    pts = np.array(pts)
    dist = np.sqrt(((xx[..., None] - pts[:, 0]) ** 2 + (yy[..., None] - pts[:, 1]) ** 2).min(axis=2))
    return np.clip(np.rint(gaussian_filter(30.0 + 170.0 * (dist < 3.5), 1.2)), 0, 255).astype(np.uint8)


def spiral_image(size=160, r0=10.0, pitch=16.0, turns=3.75):
    """size x size: a band of half-width 3.5 about the spiral r = r0 + pitch phi / (2 pi) around the centre, phi from 0 over `turns`
    turns (the radius 10 -> 70), with round ends; smoothed as the serpentine is.  Its outline is one closed edge that runs out along one
    flank and back along the other: about 1900 pixels long, through nearly every tile of the frame, several times through most."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    dx, dy = xx - (size - 1) / 2.0, yy - (size - 1) / 2.0
    r, theta = np.hypot(dx, dy), np.mod(np.arctan2(dy, dx), 2 * np.pi)
    phi = theta + 2 * np.pi * np.rint((r - r0 - pitch * theta / (2 * np.pi)) / pitch)       # the turn nearest to the pixel, along its ray
    dist = np.where((phi >= 0) & (phi <= 2 * np.pi * turns), np.abs(r - r0 - pitch * phi / (2 * np.pi)), np.inf)
    for end in (0.0, 2 * np.pi * turns):
        rho = r0 + pitch * end / (2 * np.pi)
        dist = np.minimum(dist, np.hypot(dx - rho * np.cos(end), dy - rho * np.sin(end)))
    return np.clip(np.rint(gaussian_filter(30.0 + 170.0 * (dist < 3.5), 1.2)), 0, 255).astype(np.uint8)


def stripes_image(width=1030, height=40):
    """Vertical stripes three pixels wide, 0 and 200: every edge is a component of two columns whose root lies in row 0, three pixels
    from the next one's."""
    yy, xx = np.mgrid[0:height, 0:width]
    return (((xx // 3) % 2) * 200).astype(np.uint8)


def ridge_image(broken):
    """96 x 96: a bright ridge one pixel wide on x = y + 1.  Its two flanks x = y and x = y + 2 are chains whose pixels touch only
    diagonally; the chain x = y passes the tile corners (31, 31) -> (32, 32) and (63, 63) -> (64, 64).  broken: from row 64 on the
    ridge is dark on bright, so the gradients on both sides of the second corner are opposed and the chain ends there."""
    yy, xx = np.mgrid[0:96, 0:96]
    img = np.where(xx == yy + 1, 200, 0)
    if broken:
        img = np.where(yy >= 64, 200 - img, img)
    return img.astype(np.uint8)


FRAME_SIZES = ((70, 44), (33, 90), (97, 33))                 # width x height, of the batch test


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    inputs = {}
    sizes = [(1, 1), (1, 70), (70, 1), (8, 8), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, T - 1), (63, 65), (65, 63)]
    for i, (w, h) in enumerate(sizes):
        inputs["field_%dx%d" % (w, h)] = (field(i, h, w), {})
    inputs["field_1x70_sparse"] = (field(40, 70, 1, sigma=1.0, contrast=400.0), dict(min_pixels=2, min_length=0.5))
    inputs["diagonal"] = (diagonal_image(), {})
    inputs["serpentine"] = (serpentine_image(), {})
    inputs["corner_linked"] = (ridge_image(False), {})
    inputs["corner_broken"] = (ridge_image(True), {})
    yy, xx = np.mgrid[0:256, 0:256]
    inputs["ramp"] = (xx.astype(np.uint8), dict(grad_threshold=1))
    inputs["constant"] = (np.full((40, 56), 200, np.uint8), {})
    inputs["truncated"] = (inputs["field_63x65"][0], dict(max_segments=2))
    inputs["loose"] = (field(21, 80, 112), dict(grad_threshold=12, tol_num=1, tol_den=1, min_pixels=5, min_length=4.0, max_thickness=2.0))
    inputs["step"] = (step_image(), {})
    inputs["isotropic"] = (step_image()[:2], dict(min_pixels=4))
    inputs["edges"] = (edge_image(), {})
    for i, (w, h) in enumerate(FRAME_SIZES):
        inputs["frames_%d" % i] = (np.full((h, w), 9, np.uint8) if i == 1 else field(50 + i, h, w), {})
    p = pair()
    inputs["pair_a"] = (p["image"], {})
    inputs["pair_b"] = (p["image2"], {})
    # Beyond one pass of the in-kernel loops.  k_scan takes BLOCK chunks a pass: 512 x 512 is the last frame of one pass, 513 x 512 the
    # first of two (its last chunk half full), 520 x 512 has full chunks in the second.  k_emit takes BLOCK fitted slots a pass and k_fit
    # a block: `many` is a small frame with more than BLOCK of them, `dense` has four passes.  Where more components are OK than the
    # default max_segments, the option is written out: the reference truncates only when it is given.
    cut = dict(max_segments=MAX_SEGMENTS)
    inputs["field_512x512"] = (field(75, 512, 512), cut)
    inputs["field_513x512"] = (field(76, 512, 513), cut)
    inputs["field_520x512"] = (field(70, 512, 520), cut)
    inputs["many"] = (field(71, 200, 240), {})
    # (the lengths below are not integers: an axis-parallel run of 3 or 4 pixels would sit on the threshold otherwise)
    dense, dense_opt = field(73, 128, 128, sigma=1.2, contrast=500.0), dict(min_pixels=4, min_length=3.5)
    inputs["dense"] = (dense, dict(dense_opt, **cut))
    for s in (BLOCK - 1, BLOCK, BLOCK + 1):                     # truncation on both sides of k_emit's first pass boundary
        inputs["dense_%d" % s] = (dense, dict(dense_opt, max_segments=s))
    inputs["dense_all"] = (dense, dict(dense_opt, max_segments=4 * BLOCK))
    inputs["wide_2049x3"] = (field(72, 3, 2049), dict(min_pixels=3, min_length=2.5))       # a row longer than two chunks
    inputs["tall_3x2049"] = (field(74, 2049, 3), dict(min_pixels=3, min_length=2.5))
    inputs["stripes"] = (stripes_image(), {})
    inputs["spiral"] = (spiral_image(), {})
    return inputs


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of one GPU input: computed once, shared by the tests, never written to."""
    image, opt = gpu_inputs()[name]
    out = R.detect(image, **opt)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_the_gpu_inputs_are_what_their_tests_say():
    d = reference("diagonal")
    # one component over 7 x 7 tiles; the pixels (0, 0) and (199, 199) see half the step and stay alone
    assert d["num_components"] == 3 and d["pixels"].tolist() == [397] and d["label"].tolist() == [1] and d["status_counts"] == [1, 2, 0, 0, 0]
    s = reference("serpentine")
    big = max(c["sums"]["n"] for c in s["all"])
    assert big >= 8 * 64, big                                # one component whose geodesic is many times the side
    assert s["status_counts"][R.STATUS.index(R.THICK)] >= 1
    for name, joined in (("corner_linked", True), ("corner_broken", False)):
        img = gpu_inputs()[name][0]
        _, _, strong, links = R.link_planes(img)
        lab = reference(name)["labels"]
        assert strong[31, 31] and strong[32, 32] and strong[63, 63] and strong[64, 64]
        assert links[3][31, 31] and links[3][63, 63] == joined
        assert not links[0][31, 31] and not links[2][31, 31] and not links[1][31, 32]        # the chain touches only diagonally
        assert lab[31, 31] == lab[32, 32] == 97 and (lab[64, 64] == lab[63, 63]) == joined     # (the chain starts at (1, 1))
    r = reference("ramp")
    assert r["num_components"] == 1 and r["status_counts"] == [0, 0, 0, 0, 1] and (r["labels"] == 0).all()
    assert r["all"][0]["sums"]["n"] == 65536
    assert reference("constant")["num_components"] == 0
    t = reference("truncated")
    assert t["num_ok"] > t["num_written"] == 2
    assert reference("frames_1")["num_components"] == 0 and reference("frames_0")["num_ok"] >= 1 and reference("frames_2")["num_ok"] >= 1
    # every status occurs somewhere, and the small fields have components at all
    total = np.sum([reference(n)["status_counts"] for n in gpu_inputs()], axis=0)
    assert (total > 0).all(), total
    for name in ("field_8x8", "field_1x70", "field_70x1", "field_%dx%d" % (T, T)):
        assert reference(name)["num_components"] >= 1, name

    # ---- beyond one pass of k_scan, k_emit and k_fit
    layout = open(os.path.join(ROOT, "slslam_amd", "csrc", "line_detect_layout.h")).read()
    assert "constexpr int kBlock = %d, kChunk = %d;" % (BLOCK, CHUNK) in layout and CHUNK == 4 * BLOCK and MAX_SEGMENTS == 2 * BLOCK
    chunks = lambda name: -(-gpu_inputs()[name][0].size // CHUNK)  # noqa: E731
    roots = lambda name: np.array([c["label"] for c in reference(name)["all"]])  # noqa: E731
    fitted = lambda name: [c for c in reference(name)["all"] if c["status"] != R.SMALL]  # noqa: E731
    second = BLOCK * CHUNK                                    # the first pixel of k_scan's second pass
    assert chunks("field_512x512") == BLOCK                   # the last frame of one pass
    assert chunks("field_513x512") == BLOCK + 1 and gpu_inputs()["field_513x512"][0].size % CHUNK == CHUNK // 2
    assert (roots("field_513x512") >= second).any()           # num_components goes through the second pass
    assert chunks("field_520x512") >= BLOCK + 4
    assert max(c["label"] for c in fitted("field_520x512")) >= second          # a slot that depends on the carried base_f
    for name in ("field_512x512", "field_513x512", "field_520x512"):
        assert gpu_inputs()[name][1] == dict(max_segments=MAX_SEGMENTS) and len(fitted(name)) > BLOCK
    assert len(fitted("many")) > BLOCK and gpu_inputs()["many"][0].size < second // 4 and gpu_inputs()["many"][1] == {}
    assert reference("many")["num_ok"] < MAX_SEGMENTS
    assert len(fitted("dense")) > 3 * BLOCK
    # truncation by the default max_segments lies behind k_emit's second pass: the first two hold at most 2 BLOCK = 512 OK components
    for name in ("dense", "field_513x512"):
        assert reference(name)["num_ok"] > MAX_SEGMENTS == reference(name)["num_written"], name
    passes = {i // BLOCK for i, c in enumerate(fitted("dense")) if c["status"] == R.OK}
    assert passes == {0, 1, 2, 3}, passes                     # OK components among the fitted of each of four passes
    full = reference("dense_all")
    assert full["num_written"] == full["num_ok"] == reference("dense")["num_ok"] > BLOCK + 1
    for s in (BLOCK - 1, BLOCK, BLOCK + 1):
        r = reference("dense_%d" % s)
        assert gpu_inputs()["dense_%d" % s][1]["max_segments"] == s == r["num_written"] and r["num_ok"] == full["num_ok"]
        assert np.array_equal(r["label"], full["label"][:s]) and np.array_equal(r["segments"], full["segments"][:s])
    for name, (w, h) in (("wide_2049x3", (2 * CHUNK + 1, 3)), ("tall_3x2049", (3, 2 * CHUNK + 1))):
        image = gpu_inputs()[name][0]
        assert image.shape == (h, w) and len(fitted(name)) > BLOCK and reference(name)["num_ok"] >= 1, name
    # stripes: every root in row 0, more of them in chunk 0 than its block has threads, two among one thread's four pixels
    s, lab = reference("stripes"), roots("stripes")
    width = gpu_inputs()["stripes"][0].shape[1]
    assert width > CHUNK and (lab < width).all() and (lab >= CHUNK).any()
    assert (lab < CHUNK).sum() > BLOCK
    assert (np.bincount(lab // 4) >= 2).any()
    assert s["num_ok"] == s["num_components"] == len(lab) and s["status_counts"] == [len(lab), 0, 0, 0, 0]
    # the spiral: one component through many tiles, many times longer than the side
    sp = reference("spiral")
    big = max(sp["all"], key=lambda c: c["sums"]["n"])
    ys, xs = np.nonzero(sp["labels"] == big["label"])
    assert len(set(zip((ys // T).tolist(), (xs // T).tolist()))) >= 16
    assert big["sums"]["n"] >= 3000 and big["status"] == R.THICK and sp["labels"].shape == (160, 160)


def test_no_component_sits_on_a_threshold():
    """What the accept / reject comparison of the GPU tests rests on: in the reference no fitted component's length or thickness lies
    within 1e-6 of its threshold."""
    for name, (_, opt) in gpu_inputs().items():
        o = dict(R.DEFAULTS)
        o.update(opt)
        for c in reference(name)["all"]:
            if "length" in c:
                assert abs(c["length"] - o["min_length"]) > 1e-6 and abs(c["thickness"] - o["max_thickness"]) > 1e-6, (name, c)


def fp_arrays(r):
    return np.concatenate([np.asarray(r["segments"], dtype=np.longdouble).reshape(-1)] +
                          [np.asarray(r[k], dtype=np.longdouble) for k in ("length", "thickness", "strength")])


def test_float64_figure():
    """The tolerance of the GPU tests is measured, not guessed: the reference's fit evaluated in np.longdouble stays within R.F64_FIGURE
    of its fp64 evaluation on every input of the GPU tests, the integer stages and the accept sets being equal."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    worst = {}
    for name, (image, opt) in gpu_inputs().items():
        ref = reference(name)
        wide = R.detect(image, dtype=np.longdouble, **opt)
        assert wide["status_counts"] == ref["status_counts"] and np.array_equal(wide["label"], ref["label"]), name
        d = np.abs(fp_arrays(wide) - fp_arrays(ref))
        worst[name] = float(d.max()) if d.size else 0.0
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print("longdouble against float64, the five largest:", top)
    assert top[0][1] <= R.F64_FIGURE, top
    assert R.F64_FIGURE <= 4 * top[0][1]                    # (the figure is the measurement, not a generous bound)
    assert R.DEVICE_TOLERANCE == 8 * R.F64_FIGURE


# ---- the C ABI: the exports, the argument checks (before a device is asked for), no device
NAMES = ["slslam_line_detect_default_options", "slslam_line_detector_create", "slslam_line_detector_destroy", "slslam_line_detector_run",
         "slslam_line_detector_stats", "slslam_line_detector_timing", "slslam_detect_lines"]


def test_exports_and_defaults():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(L, name)
    o = capi.LineDetectOptions(-1, -1, -1, -1, -1.0, -1.0, -1)
    L.slslam_line_detect_default_options(C.byref(o))
    assert (o.grad_threshold, o.tol_num, o.tol_den, o.min_pixels, o.min_length, o.max_thickness, o.max_segments) == (24, 11, 64, 12, 10.0, 3.0, 512)
    L.slslam_line_detect_default_options(None)
    d = capi.line_detect_options()
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert callable(capi.detect_lines) and callable(capi.detect_and_describe) and capi.LineDetector is not None


def bad_options():
    nan, inf = float("nan"), float("inf")
    over = [dict(grad_threshold=0), dict(grad_threshold=1025), dict(tol_num=-1), dict(tol_num=2 ** 20 + 1), dict(tol_den=0),
            dict(tol_den=2 ** 20 + 1), dict(min_pixels=0), dict(min_length=-1.0), dict(min_length=nan), dict(min_length=inf),
            dict(max_thickness=-0.5), dict(max_thickness=nan), dict(max_thickness=inf), dict(max_segments=0), dict(max_segments=2 ** 20 + 1)]
    return [capi.line_detect_options(**o) for o in over]


def test_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    good = capi.line_detect_options()
    for bad in bad_options():
        assert L.slslam_line_detector_create(-1, C.byref(bad), 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_line_detector_create(-1, None, 1, 100, C.byref(h)) == INVALID_ARGUMENT
    assert L.slslam_line_detector_create(-1, C.byref(good), 1, 100, None) == INVALID_ARGUMENT
    # counts, and a capacity the first run could not allocate: a frame beyond 8192^2 pixels, more than 2^30 pixels, more than 2^24 segments
    for args in ((0, 100), (1, 0), (-1, 100), (1, 8192 * 8192 + 1), (17, 8192 * 8192), (2 ** 15 + 1, 100)):
        assert L.slslam_line_detector_create(-1, C.byref(good), *args, C.byref(h)) == INVALID_ARGUMENT, args
    assert not h
    assert L.slslam_line_detector_create(-1, C.byref(good), 16, 8192 * 8192, C.byref(h)) == 0           # the capacity's limits; no device
    ms = C.c_double(-1.0)
    assert L.slslam_line_detector_timing(h, -1, C.byref(ms)) == 0 and ms.value == 0.0
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_line_detector_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)
    assert L.slslam_line_detector_stats(None, None, None) == INVALID_ARGUMENT
    assert L.slslam_line_detector_timing(None, 0, None) == INVALID_ARGUMENT
    L.slslam_line_detector_destroy(h)
    L.slslam_line_detector_destroy(None)
    limits = capi.line_detect_options(1024, 2 ** 20, 2 ** 20, 1, 0.0, 0.0, 2 ** 20)
    h = C.c_void_p()
    assert L.slslam_line_detector_create(-1, C.byref(limits), 16, 1, C.byref(h)) == 0
    L.slslam_line_detector_destroy(h)


def _frame(img, **over):
    fr, res, keep = capi._detect_frame(img, 512, True)
    for k in ("segments", "length", "pixels", "counts", "status_counts", "labels"):
        keep[1][k][...] = -7
    for k, v in over.items():
        setattr(fr, k, v)
    return fr, res, keep


def _untouched(keep):
    return all((keep[1][k] == -7).all() for k in ("segments", "length", "pixels", "counts", "status_counts", "labels"))


def test_run_arguments_and_no_device():
    L = capi.lib()
    h = C.c_void_p()
    opt = capi.line_detect_options()
    assert L.slslam_line_detector_create(-1, C.byref(opt), 2, 16 * 16, C.byref(h)) == 0
    img = step_image()
    for over in (dict(width=0), dict(height=0), dict(width=-3), dict(height=8193), dict(width=8193, stride=8193), dict(stride=15),
                 dict(image=C.POINTER(C.c_ubyte)())):
        fr, res, keep = _frame(img, **over)
        assert L.slslam_line_detector_run(h, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert L.slslam_detect_lines(C.byref(opt), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT, over
        assert _untouched(keep)
    fr, res, keep = _frame(img)
    assert L.slslam_line_detector_run(None, 1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_detector_run(h, -1, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_detector_run(h, 1, None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_line_detector_run(h, 1, C.byref(fr), None) == INVALID_ARGUMENT
    assert L.slslam_detect_lines(None, C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    for bad in bad_options():
        assert L.slslam_detect_lines(C.byref(bad), C.byref(fr), C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_detect_lines(C.byref(opt), None, C.byref(res)) == INVALID_ARGUMENT
    assert L.slslam_detect_lines(C.byref(opt), C.byref(fr), None) == INVALID_ARGUMENT
    assert _untouched(keep)
    calls, allocs = C.c_longlong(-1), C.c_longlong(-1)
    assert L.slslam_line_detector_stats(h, C.byref(calls), C.byref(allocs)) == 0 and (calls.value, allocs.value) == (0, 0)

    if capi.device_count() == 0:                                # every compute entry point says so, and leaves its outputs alone
        assert L.slslam_line_detector_run(h, 1, C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        assert L.slslam_line_detector_run(h, 0, None, None) == NO_DEVICE
        assert L.slslam_detect_lines(C.byref(opt), C.byref(fr), C.byref(res)) == NO_DEVICE and _untouched(keep)
        d = capi.LineDetector(max_frames=1, max_pixels=16 * 16)
        msld = capi.LineDescriptor(max_frames=1, max_pixels=16 * 16, max_segments=4)
        for call in (lambda: d.run([img]), lambda: capi.detect_lines(img), lambda: capi.detect_and_describe(d, msld, [img])):
            with pytest.raises(capi.SlslamError) as ei:
                call()
            assert ei.value.status == NO_DEVICE
        assert d.stats() == {"calls": 0, "allocations": 0}
        d.close()
        msld.close()
    L.slslam_line_detector_destroy(h)


def test_a_strided_image_passes_its_stride():
    base = np.zeros((12, 40), np.uint8)
    view = base[:, 3:19]
    fr, res, keep = capi._detect_frame(view, 8, False)
    assert (fr.width, fr.height, fr.stride) == (16, 12, 40) and keep[0] is view
    assert C.addressof(fr.image.contents) == view.ctypes.data and not res.labels
    fr, res, keep = capi._detect_frame(base[:, ::2], 8, True)                       # columns apart: copied
    assert (fr.width, fr.stride) == (20, 20) and keep[0].flags["C_CONTIGUOUS"] and keep[1]["labels"].shape == (12, 20) and res.labels
    with pytest.raises(ValueError):
        capi._detect_frame(base.astype(np.float32), 8, False)


# ---- the host layout (csrc/line_detect_layout.h) under the sanitizers, as a stand-alone program
def test_host_layout_under_the_sanitizers():
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "line_detect_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "line_detect_layout_check.cpp"), "-o", exe])
    # the frames of the batch test and two more as the program's input: it prints the layout it computes
    frames = list(FRAME_SIZES) + [(1, 1), (752, 480)]
    r = subprocess.run([exe, "12", "512"] + ["%d %d" % wh for wh in frames], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "line detect layout ok" in r.stdout
    got = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    first = comp0 = 0
    want = []
    for w, h in frames:                                         # the numpy layout: planes in chunks of 1024, slots floor(n / 12) + 1
        want.append((first, comp0, w, h, w * h // 12 + 1, first // 1024))
        first += -(-w * h // 1024) * 1024
        comp0 += w * h // 12 + 1
    assert got == want
    sizes = dict(ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("size "))
    al = lambda n: -(-n // 256) * 256  # noqa: E731
    F, S = len(frames), 512
    out = al(48 * F) + al(16 * F * S) + 3 * al(8 * F * S) + 2 * al(4 * F * S)
    assert int(sizes["in_bytes"]) == al(32 * F) + al(first) and int(sizes["out_bytes"]) == out
    assert int(sizes["out_bytes_labels"]) == out + al(4 * first)
    assert int(sizes["dev"]) == al(32 * F) + 2 * al(first) + al(4 * first) + al(8 * (first // 1024)) + al(128 * comp0) + out + al(4 * first)
    assert int(sizes["host"]) == int(sizes["in_bytes"]) + out and int(sizes["host_labels"]) == int(sizes["in_bytes"]) + out + al(4 * first)

"""The line segment detector on the device (include/slslam_hip.h: slslam_line_detector_*, slslam_detect_lines; csrc/line_detect.h) against
the numpy reference (tests/line_detect_reference.py).  The inputs and the reference results are made once by
tests/test_line_detect_cpu.py (gpu_inputs, reference).  The integer stages - label plane, counts, pixels, labels - are compared bit for
bit; the fp64 stages within the tolerance measured there: 8 x the largest difference between the np.longdouble and the float64
evaluation of the reference on these very inputs; the accept / reject sets must be equal (no component of the reference sits on a
threshold: asserted there)."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_detect_reference as R  # noqa: E402
import test_line_detect_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = R.DEVICE_TOLERANCE


def check(got, name):
    """One frame's device results against the reference of the input `name`; nothing is left out."""
    ref = T.reference(name)
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"]), name
    assert (got["num_components"], got["num_ok"], got["num_written"]) == (ref["num_components"], ref["num_ok"], ref["num_written"]), name
    assert [got["status_counts"][s] for s in R.STATUS] == ref["status_counts"], name
    assert np.array_equal(got["pixels"], ref["pixels"]) and np.array_equal(got["label"], ref["label"]), name
    worst = 0.0
    for key in ("length", "thickness", "strength"):
        assert got[key].dtype == np.float64 and got[key].shape == ref[key].shape
        if ref[key].size:
            worst = max(worst, float(np.abs(got[key] - ref[key]).max()))
    # the float segments after the same rounding: within the tolerance of the reference, and half a float's spacing there
    assert got["segments"].dtype == np.float32 and got["segments"].shape == ref["segments"].shape
    if ref["segments"].size:
        d = np.abs(got["segments"].astype(np.float64) - ref["segments"])
        assert (d <= TOL + 0.5 * np.spacing(np.abs(ref["segments"]).astype(np.float32)).astype(np.float64)).all(), name
    print("%s: %d components, %d segments, largest fp64 difference %.3g (tolerance %.3g)" % (name, ref["num_components"], ref["num_written"], worst, TOL))
    assert worst <= TOL, name


def run(name):
    image, opt = T.gpu_inputs()[name]
    return capi.detect_lines(image, labels=True, **opt)


SIZES = ["field_1x1", "field_1x70", "field_70x1", "field_8x8"] + ["field_%dx%d" % (s, s) for s in (T.T - 1, T.T, T.T + 1)] + \
        ["field_%dx%d" % (2 * T.T + 1, T.T - 1), "field_63x65", "field_65x63", "field_1x70_sparse"]


@pytest.mark.parametrize("name", SIZES)
def test_sizes_about_the_tile(name):
    check(run(name), name)


@pytest.mark.parametrize("name", ["step", "isotropic", "diagonal", "serpentine", "corner_linked", "corner_broken", "ramp", "constant",
                                  "loose", "edges"])
def test_shapes(name):
    check(run(name), name)


def test_truncation_keeps_the_first():
    got = run("truncated")
    check(got, "truncated")
    full = run("field_63x65")
    assert got["num_written"] == 2 < got["num_ok"] == full["num_ok"]
    for key in ("segments", "length", "thickness", "strength", "pixels", "label"):
        assert got[key].tobytes() == full[key][:2].tobytes(), key


ARRAYS = ("segments", "length", "thickness", "strength", "pixels", "label")


@pytest.mark.parametrize("name", ["field_512x512", "field_513x512", "field_520x512", "many", "dense", "wide_2049x3", "tall_3x2049",
                                  "stripes", "spiral"])
def test_past_one_pass(name):
    """Where k_scan (more than 256 chunks) and k_emit (more than 256 fitted slots) take a second pass and k_fit a second block; a chunk
    with more fitted roots than threads and two roots among a thread's four pixels (stripes); neighbours one and two chunks away (wide,
    tall); one component wound through 23 tiles (spiral).  What each input is, test_line_detect_cpu.py asserts."""
    check(run(name), name)


def test_truncation_about_the_pass_boundary():
    """max_segments one below, at and one above k_emit's pass of 256, at the default (in the third pass) and beyond num_ok: each is the
    beginning of the untruncated result, byte for byte, and counts the same OK components."""
    full = run("dense_all")
    check(full, "dense_all")
    assert full["num_written"] == full["num_ok"] > 2 * T.BLOCK
    for name in ("dense_%d" % (T.BLOCK - 1), "dense_%d" % T.BLOCK, "dense_%d" % (T.BLOCK + 1), "dense"):
        got = run(name)
        check(got, name)
        n = got["num_written"]
        assert n == T.gpu_inputs()[name][1]["max_segments"] < got["num_ok"] == full["num_ok"], name
        for key in ARRAYS:
            assert got[key].shape[0] == n and got[key].tobytes() == full[key][:n].tobytes(), (name, key)
        assert got["labels"].tobytes() == full["labels"].tobytes() and got["status_counts"] == full["status_counts"], name


def test_a_large_frame_behind_a_small_one():
    """A frame of two k_scan passes as frame 1 of a call: its first pixel, chunk and slot are not 0, and the frame behind it has more
    than 256 fitted slots of its own."""
    names = ["frames_0", "field_513x512", "many"]
    frames = [T.gpu_inputs()[n][0] for n in names]
    assert all(T.gpu_inputs()[n][1].get("max_segments", T.MAX_SEGMENTS) == T.MAX_SEGMENTS for n in names)       # the handle's default
    d = capi.LineDetector(max_frames=3, max_pixels=frames[1].size)
    together = d.run(frames, labels=True)
    for i, name in enumerate(names):
        check(together[i], name)
        alone = d.run([frames[i]], labels=True)[0]
        for key in ARRAYS + ("labels",):
            assert together[i][key].tobytes() == alone[key].tobytes(), (name, key)
        assert together[i]["status_counts"] == alone["status_counts"], name
        assert [together[i][k] for k in ("num_components", "num_ok", "num_written")] == [alone[k] for k in ("num_components", "num_ok", "num_written")]
    again = d.run(frames, labels=True)                          # integer atomics: the order of the waves changes nothing
    for i, name in enumerate(names):
        for key in ARRAYS + ("labels",):
            assert again[i][key].tobytes() == together[i][key].tobytes(), (name, key)
        assert again[i]["status_counts"] == together[i]["status_counts"] and again[i]["num_ok"] == together[i]["num_ok"], name
    d.close()


def test_without_the_label_plane_and_with_null_outputs():
    image, opt = T.gpu_inputs()["field_63x65"]
    with_plane, without = capi.detect_lines(image, labels=True), capi.detect_lines(image)
    assert "labels" not in without
    for key in ("segments", "length", "thickness", "strength", "pixels", "label"):
        assert with_plane[key].tobytes() == without[key].tobytes(), key
    o = capi.line_detect_options()
    fr, _, keep = capi._detect_frame(image, o.max_segments, False)
    assert capi.lib().slslam_detect_lines(o, fr, capi.LineDetectResult()) == 0          # every output NULL


def test_frames_of_different_sizes_in_one_call():
    inputs = [T.gpu_inputs()["frames_%d" % i][0] for i in range(3)]
    assert [(im.shape[1], im.shape[0]) for im in inputs] == list(T.FRAME_SIZES)
    wide = np.zeros((33, 160), np.uint8)
    wide[:, 11:108] = inputs[2]
    strided = wide[:, 11:108]                                   # the third frame as a view: rows 160 bytes apart
    assert not strided.flags["C_CONTIGUOUS"]
    d = capi.LineDetector(max_frames=3, max_pixels=97 * 33)
    assert d.stats() == {"calls": 0, "allocations": 0}
    frames = [inputs[0], inputs[1], strided]
    together = d.run(frames, labels=True)
    assert d.stats() == {"calls": 1, "allocations": 1}
    assert together[1]["num_components"] == 0 and together[1]["segments"].shape == (0, 4) and (together[1]["labels"] == -1).all()
    for i in range(3):
        check(together[i], "frames_%d" % i)
        alone = d.run([frames[i]], labels=True)[0]
        for key in ("segments", "length", "thickness", "strength", "pixels", "label", "labels"):
            assert together[i][key].tobytes() == alone[key].tobytes(), (i, key)
        assert together[i]["status_counts"] == alone["status_counts"] and together[i]["num_ok"] == alone["num_ok"]
    assert d.stats() == {"calls": 4, "allocations": 1}          # the handle is reused: a call that fits allocates nothing
    check(d.run([T.gpu_inputs()["diagonal"][0]], labels=True)[0], "diagonal")      # a frame larger than the blocks were made for
    assert d.stats() == {"calls": 5, "allocations": 2}          # ... grows them once
    check(d.run([T.gpu_inputs()["diagonal"][0], inputs[0]], labels=True)[1], "frames_0")
    assert d.stats()["calls"] == 6
    assert d.run([]) == []
    d.close()


def test_chain_detect_describe_match():
    p = T.pair()
    det = capi.LineDetector(max_frames=2, max_pixels=160 * 224)
    msld = capi.LineDescriptor(max_frames=2, max_pixels=160 * 224, max_segments=512)
    a, b = capi.detect_and_describe(det, msld, [p["image"], p["image2"]])
    det.close()
    msld.close()
    ra, rb = T.reference("pair_a"), T.reference("pair_b")
    assert np.array_equal(a["label"], ra["label"]) and np.array_equal(b["label"], rb["label"])
    assert set(a["descriptor_status"]) <= {"OK", "FLAT"} and set(b["descriptor_status"]) <= {"OK", "FLAT"}
    assert a["descriptors"].shape == (a["num_written"], 72)
    m = capi.match_descriptors(a["descriptors"], b["descriptors"], ratio=T.PAIR_RATIO, max_distance=T.PAIR_MAX_DISTANCE)
    n = T.true_matches(p, a["segments"], b["segments"], m["match"])
    print("device chain: detections %d and %d, mutual matches %d, of the same drawn edge %d" % (a["num_ok"], b["num_ok"], m["num_matched"], n))
    assert m["status"] == "OK" and n == T.CHAIN_TRUE_MATCHES

"""The image rectifier on the device (include/slslam_hip.h: slslam_image_rectifier_*, slslam_rectify_images; csrc/image_rectify.h) against
the numpy contract (tests/image_rectify_reference.py).  The cameras, their reference maps and the images are made once by
tests/test_image_rectify_cpu.py (gpu_cameras, gpu_map, gpu_image), which also asserts the condition the equality rests on.  qx, qy, the
valid bytes, num_valid and the output bytes are compared for equality; sx, sy within 8 x the measured longdouble figure."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_rectify_reference as R  # noqa: E402
import test_image_rectify_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = (("constant", R.CONSTANT, 93), ("replicate", R.REPLICATE, 201))


def check_map(rect, index, name):
    got, ref = rect.get_map(index, fp64=True), T.gpu_map(name)
    assert got["qx"].dtype == np.int32 and np.array_equal(got["qx"], ref["qx"]) and np.array_equal(got["qy"], ref["qy"]), name
    assert np.array_equal(got["valid"], ref["valid"]), name
    c = ref["coords"]
    assert np.isnan(got["sx"][~c]).all() and np.isnan(got["sy"][~c]).all(), name
    worst = 0.0
    for k in ("sx", "sy"):
        d = np.abs(got[k][c] - ref[k][c])
        worst = max(worst, float(d.max(initial=0.0)))
        assert (d <= R.DEVICE_TOLERANCE).all() and (d <= R.DEVICE_RELATIVE * np.maximum(1.0, np.abs(ref[k][c]))).all(), (name, k)
    print("%s: largest fp64 difference of sx, sy %.3g (tolerance %.3g)" % (name, worst, R.DEVICE_TOLERANCE))


def check(name, sigma=0.0, with_map=True):
    """One camera and its image through a handle of its own under both border modes: everything against the reference."""
    cam, image, m = T.gpu_cameras()[name], T.gpu_image(name), T.gpu_map(name)
    radius, taps = capi.smooth_taps(sigma)
    for border, mode, value in MODES:
        rect = capi.ImageRectifier([R.to_capi(cam)], max_frames=1, max_pixels=max(image.size, m["valid"].size), border=border,
                                   border_value=value, smooth_sigma=sigma)
        got = rect.run([(0, image)], valid=True)[0]
        ref = R.rectify(image, cam, mode, value, radius, taps, m=m)
        assert got["image"].dtype == np.uint8 and np.array_equal(got["image"], ref["image"]), (name, border, sigma)
        assert np.array_equal(got["valid"], ref["valid"]) and got["num_valid"] == ref["num_valid"], (name, border)
        if with_map and mode == R.CONSTANT:
            check_map(rect, 0, name)
        rect.close()


@pytest.mark.parametrize("name", ["%s_%dx%d" % (k, w, h) for (w, h) in T.SIZES for k in ("identity", "barrel", "rot_partial")])
def test_sizes(name):
    check(name)


@pytest.mark.parametrize("name", ["tiny_1x1", "tiny_2x2", "zoom_in", "zoom_out"])
def test_sources_that_clamp_and_outputs_of_another_size(name):
    check(name)


@pytest.mark.parametrize("name", ["%s_%s" % (k, s) for s in ("65x63", "33x33") for k in T.KINDS])
def test_cameras(name):
    check(name)


@pytest.mark.parametrize("radius", range(1, 8))
@pytest.mark.parametrize("name", ["barrel_8x8", "rot_partial_8x8", "barrel_65x63", "pincushion_65x63", "rot_partial_63x65"])
def test_smoothing(name, radius):
    """One fused launch: the bytes are those of the reference's remap followed by the reference's smoothing.  At 8 x 8 the halo is wider
    than the image, at 65 x 63 and 63 x 65 it crosses tile borders both ways."""
    check(name, sigma=T.SIGMA_OF_RADIUS[radius], with_map=False)


@pytest.mark.parametrize("radius", (1, 2, 7))
def test_loops_past_one_pass(radius):
    """k_rect_smooth's loops, each sized by a bound: the remap loop over (kTileW + 2 radius) (kTileH + 2 radius) pixels, the horizontal
    loop over kTileW (kTileH + 2 radius) and the vertical loop over kTileW kTileH, each kBlock = 256 a pass - more than one pass at
    every radius -, and the tap loops of `radius` passes; on an output of four tiles by nine, the last column and row of tiles
    partial.  tests/test_image_rectify_cpu.py asserts that the input is that (test_the_loops_take_more_than_one_pass).  k_rect_map and
    k_rect_remap have no loop."""
    check("barrel_200x130", sigma=T.SIGMA_OF_RADIUS[radius], with_map=False)
    if radius == 1:
        check("barrel_200x130")


def test_two_cameras_and_five_frames_in_one_call():
    names = ["barrel_65x63", "rot_partial_33x33"]
    cams = [T.gpu_cameras()[n] for n in names]
    order = [0, 1, 1, 0, 1]
    images = [T.image_of(100 + i, cams[k]["src_height"], cams[k]["src_width"]) for i, k in enumerate(order)]
    wide = np.zeros((cams[1]["src_height"], 160), np.uint8)
    wide[:, 7:7 + cams[1]["src_width"]] = images[2]
    images[2] = wide[:, 7:7 + cams[1]["src_width"]]             # the third frame as a view: rows 160 bytes apart
    assert not images[2].flags["C_CONTIGUOUS"] and cams[0]["dst_width"] != cams[1]["dst_width"]
    for sigma in (0.0, 0.6):
        radius, taps = capi.smooth_taps(sigma)
        rect = capi.ImageRectifier([R.to_capi(c) for c in cams], max_frames=5, max_pixels=71 * 67, border="replicate", border_value=9,
                                   smooth_sigma=sigma)
        assert rect.stats() == {"calls": 0, "allocations": 0}
        frames = list(zip(order, images))
        together = rect.run(frames, valid=True)
        assert rect.stats() == {"calls": 1, "allocations": 1}
        again = rect.run(frames, valid=True)
        for i, k in enumerate(order):
            ref = R.rectify(images[i], cams[k], R.REPLICATE, 9, radius, taps, m=T.gpu_map(names[k]))
            assert np.array_equal(together[i]["image"], ref["image"]) and together[i]["num_valid"] == ref["num_valid"], (sigma, i)
            assert np.array_equal(together[i]["valid"], ref["valid"])
            alone = rect.run([frames[i]], valid=True)[0]
            for key in ("image", "valid"):
                assert together[i][key].tobytes() == alone[key].tobytes() == again[i][key].tobytes(), (sigma, i, key)
            assert together[i]["num_valid"] == alone["num_valid"] == again[i]["num_valid"]
        assert rect.stats() == {"calls": 7, "allocations": 1}  # the handle is reused: a call that fits allocates nothing
        for k, n in enumerate(names):
            check_map(rect, k, n)
        more = rect.run(frames * 4, valid=False)                  # twenty frames: larger than the blocks were made for
        assert rect.stats() == {"calls": 8, "allocations": 2}  # ... grows them once
        assert all(more[i]["image"].tobytes() == more[i + 5]["image"].tobytes() == together[i]["image"].tobytes() for i in range(5))
        assert "valid" not in more[0]
        rect.run(frames)
        assert rect.stats() == {"calls": 9, "allocations": 2}
        assert rect.run([]) == [] and rect.stats() == {"calls": 10, "allocations": 2}
        # the one-shot entry point gives the same bytes
        once = capi.rectify_images([R.to_capi(c) for c in cams], frames, valid=True, border="replicate", border_value=9, smooth_sigma=sigma)
        assert all(once[i]["image"].tobytes() == together[i]["image"].tobytes() and once[i]["num_valid"] == together[i]["num_valid"]
                   for i in range(5))
        rect.close()


def test_a_strided_output_and_null_outputs():
    cam, image = T.gpu_cameras()["barrel_33x33"], T.gpu_image("barrel_33x33")
    cams = [R.to_capi(cam)]
    fr, res, keep = capi._rectify_frame(cams, 0, image, False)
    out = np.full((33, 50), 77, np.uint8)
    res.image, res.stride, res.num_valid = out.ctypes.data_as(capi.C.POINTER(capi.C.c_ubyte)), 50, None
    opt = capi.rectify_options()
    assert capi.lib().slslam_rectify_images(opt, 1, capi._camera_array(cams), 1, fr, res) == 0
    assert np.array_equal(out[:, :33], R.rectify(image, cam)["image"]) and (out[:, 33:] == 77).all()


def test_chain_from_raw_images():
    """capi.rectify_detect_describe_pair_and_track on synth.make_raw_stereo_pair: the reference chain's segments, matches and ids."""
    p, cams, want = T.raw_pair(), T.pair_cameras(), T.pair_chain()
    rect = capi.ImageRectifier([R.to_capi(cams["left"]), R.to_capi(cams["right"])], max_frames=2, max_pixels=160 * 224, border="replicate",
                               smooth_sigma=T.PAIR_SIGMA)
    det = capi.LineDetector(max_frames=2, max_pixels=160 * 224)
    dsc = capi.LineDescriptor(max_frames=2, max_pixels=160 * 224, max_segments=64)
    sm = capi.StereoMatcher(dsc.D, max_frames=1, max_segments=64, **T.PAIR_STEREO)
    lt = capi.LineTracker(dsc.D, max_frames=1, max_segments=64)
    out = capi.rectify_detect_describe_pair_and_track(rect, det, dsc, sm, lt, [(p["left"], p["right"])])
    assert len(out) == 1 and [x.stats()["calls"] for x in (rect, det, dsc, sm, lt)] == [1, 1, 1, 1, 1]
    o = out[0]
    for side in range(2):
        assert np.array_equal(o["rectified"][side], want["rectified"][side]), side
    for side, key in enumerate(("left", "right")):
        ref = want["found"][side]
        assert np.array_equal(o[key]["label"], ref["label"]) and o[key]["num_ok"] == ref["num_ok"], key
        assert np.abs(o[key]["segments"].astype(np.float64) - ref["segments"]).max() <= 1e-4, key
    assert o["left_rows"].tolist() == want["rows"][0].tolist() and o["right_rows"].tolist() == want["rows"][1].tolist()
    assert o["stereo"]["match"].tolist() == want["stereo"]["match"].tolist() and (o["stereo"]["match"] >= 0).sum() == T.PAIR_MATCHED
    assert o["track"]["id"].tolist() == want["track"]["id"].tolist() and o["ids"].tolist() == want["ids"].tolist()
    assert o["observations"].shape == want["observations"].shape and np.abs(o["observations"] - want["observations"]).max() <= 1e-5
    # the stereo options the chain passed on are the rectified intrinsics
    k = capi.stereo_rectify(p["rig"]["left"], p["rig"]["right"], p["rig"]["R"], p["rig"]["t"])
    assert (k["fx"], k["cx"], k["cy"]) == (rect.cameras[0].fx2, rect.cameras[0].cx2, rect.cameras[0].cy2)
    for x in (rect, det, dsc, sm, lt):
        x.close()

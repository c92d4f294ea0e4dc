"""The MSLD line descriptor on the device (include/slslam_hip.h: slslam_line_descriptor_*, slslam_describe_lines; csrc/line_descriptor.h)
against the fp64 numpy reference (tests/line_descriptor_reference.py).  The inputs and the reference results are made once by
tests/test_line_descriptor_cpu.py (gpu_inputs, reference); the tolerance is the one measured there: 8 x the largest difference between the
float32 and the float64 evaluation of the reference on these very inputs."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_descriptor_reference as R  # noqa: E402
import test_line_descriptor_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = R.DEVICE_TOLERANCE


def check(got, name):
    """One frame's device results against the reference of the input `name`."""
    ref = T.reference(name)
    assert got["status"] == ref["status"], name
    assert np.array_equal(got["num_samples"], ref["num_samples"]), name
    assert got["descriptors"].dtype == np.float32 and got["descriptors"].shape == ref["descriptors"].shape
    runs = np.array([s == R.OK for s in ref["status"]], dtype=bool)
    assert (got["descriptors"][~runs] == 0).all() and (got["polarity"][~runs] == 0).all(), name
    pol = ref["polarity"]
    assert (np.abs(got["polarity"] - pol) <= 1e-3 * np.maximum(1.0, np.abs(pol))).all(), name
    # the flip agrees wherever |polarity| >= 1 grey level; below it a segment may flip either way, its descriptor is compared where
    # the decision is the same, and at most 10 % of a frame's segments may be left out so
    same = runs & ((np.abs(pol) >= 1.0) | (np.sign(got["polarity"]) == np.sign(pol)))
    assert (runs & ~same).sum() <= 0.1 * max(runs.sum(), 1), name
    diff = np.abs(got["descriptors"].astype(np.float64) - ref["descriptors"])[same]
    worst = float(diff.max()) if diff.size else 0.0
    print("%s: largest difference %.3g (tolerance %.3g)" % (name, worst, TOL))
    assert worst <= TOL, name


def run(name):
    image, seg, opt = T.gpu_inputs()[name]
    return capi.describe_lines(image, seg, **opt)


@pytest.mark.parametrize("name", sorted(T.HAND))
def test_hand_computed(name):
    got = run("hand_" + name)
    T.check_hand(got, name, TOL)
    check(got, "hand_" + name)


def test_wave_edges_along_the_line():
    got = run("along")
    assert got["num_samples"].tolist() == [2, 3, 63, 64, 65, 128, 129, 150] and got["status"] == [R.OK] * 8
    check(got, "along")


@pytest.mark.parametrize("n", T.COUNTS)
def test_wave_edges_over_segments(n):
    got = run("count_%d" % n)
    assert len(got["status"]) == n
    check(got, "count_%d" % n)


@pytest.mark.parametrize("orient", [False, True])
@pytest.mark.parametrize("bands,band_width", T.DEVICE_OPTIONS)
def test_options(bands, band_width, orient):
    name = "options_%d_%d_%d" % (bands, band_width, orient)
    got = run(name)
    assert got["descriptors"].shape[1] == 8 * bands
    if not orient:
        assert (got["polarity"] < 0).any() and (got["polarity"] > 0).any()
    check(got, name)


def test_frames_of_different_sizes_in_one_call():
    inputs = [T.gpu_inputs()["frames_%d" % i] for i in range(3)]
    assert [(im.shape[1], im.shape[0]) for im, _, _ in inputs] == list(T.FRAME_SIZES) and len(inputs[1][1]) == 0
    wide = np.zeros((33, 160), np.uint8)
    wide[:, 11:108] = inputs[2][0]
    strided = wide[:, 11:108]                                   # the third frame as a view: rows 160 bytes apart
    assert not strided.flags["C_CONTIGUOUS"]
    d = capi.LineDescriptor(max_frames=3, max_pixels=320 * 240, max_segments=16)
    frames = [(inputs[0][0], inputs[0][1]), (inputs[1][0], inputs[1][1]), (strided, inputs[2][1])]
    together = d.run(frames)
    assert len(together[1]["status"]) == 0 and together[1]["descriptors"].shape == (0, 72)
    for i in range(3):
        check(together[i], "frames_%d" % i)
        alone = d.run([(inputs[i][0], inputs[i][1])])[0]
        for key in ("descriptors", "num_samples", "polarity"):
            assert together[i][key].tobytes() == alone[key].tobytes(), (i, key)
        assert together[i]["status"] == alone["status"]
    d.close()


def test_borders_and_refused_segments():
    got = run("border")
    assert got["status"] == T.BORDER_STATUS
    check(got, "border")
    image, seg, _ = T.gpu_inputs()["border"]
    runs = [i for i, s in enumerate(T.BORDER_STATUS) if s == R.OK]
    only = capi.describe_lines(image, seg[runs])                # the neighbours of the refused segments, without them
    for key in ("descriptors", "num_samples", "polarity"):
        assert got[key][runs].tobytes() == only[key].tobytes(), key
    check(run("statuses"), "statuses")
    flat = capi.describe_lines(np.full((40, 56), 200, np.uint8), seg)
    assert flat["status"] == [R.FLAT if s == R.OK else s for s in T.BORDER_STATUS]
    assert (flat["descriptors"] == 0).all() and (flat["polarity"] == 0).all()
    assert flat["num_samples"].tolist() == got["num_samples"].tolist()


def test_flip_decision():
    """The flip agrees with the reference on every segment of |polarity| >= 1 grey level, with either order of the end points."""
    image, seg, _ = T.gpu_inputs()["pair_a"]
    ref = T.reference("pair_a")
    ok = T.counted(ref["polarity"])
    unoriented = R.describe(image, seg, orient=False)
    assert (unoriented["polarity"] < -1).sum() >= 10 and (unoriented["polarity"] > 1).sum() >= 10           # both decisions are taken
    d = capi.LineDescriptor(max_frames=2, max_segments=64)
    a, b = d.run([(image, seg), (image, seg[:, [2, 3, 0, 1]])])
    d.close()
    for got in (a, b):
        assert got["status"] == [R.OK] * len(seg) and (got["polarity"][ok] > 0).all()
        assert (np.abs(got["polarity"] - ref["polarity"]) <= 1e-3 * np.maximum(1.0, np.abs(ref["polarity"]))).all()
        assert np.abs(got["descriptors"].astype(np.float64) - ref["descriptors"])[ok].max() <= TOL


def test_handle_behaviour():
    inputs = T.gpu_inputs()
    small, large = inputs["count_63"], inputs["count_130"]
    d = capi.LineDescriptor(max_frames=1, max_pixels=72 * 96, max_segments=64)
    assert d.stats() == {"calls": 0, "allocations": 0}
    first = d.run([small[:2]])[0]
    assert d.stats() == {"calls": 1, "allocations": 1}
    again = d.run([small[:2]])[0]
    assert d.stats() == {"calls": 2, "allocations": 1}          # a call that fits allocates nothing
    for key in ("descriptors", "num_samples", "polarity"):
        assert first[key].tobytes() == again[key].tobytes(), key
    check(d.run([large[:2], small[:2]])[0], "count_130")         # more frames and more segments than the blocks were made for
    assert d.stats() == {"calls": 3, "allocations": 2}
    check(d.run([small[:2]])[0], "count_63")
    assert d.stats() == {"calls": 4, "allocations": 2}
    assert d.run([]) == [] and d.stats() == {"calls": 5, "allocations": 2}
    d.close()


def test_end_to_end_with_the_matcher_and_the_recogniser():
    p = T.pair()
    d = capi.LineDescriptor(max_frames=2, max_pixels=320 * 240, max_segments=64)
    a, b = d.run([(p["image"], p["segments"]), (p["image2"], p["segments2"])])
    d.close()
    check(a, "pair_a")
    check(b, "pair_b")
    assert np.allclose(np.linalg.norm(a["descriptors"], axis=1), 1, atol=1e-5)
    m = capi.match_descriptors(a["descriptors"], b["descriptors"], ratio=T.PAIR_RATIO, max_distance=T.PAIR_MAX_DISTANCE)
    assert m["status"] == "OK" and m["num_matched"] == 60 and np.array_equal(m["match"], p["truth"])
    tree = capi.VocTree(4, 2, 72, nodes=synth.make_voctree(1, 4, 2, 72))
    db = capi.PlaceDB(tree, max_docs=8, max_words=64, max_frames=2)
    ins = db.insert(a["descriptors"])
    assert ins["status"] == "OK" and len(ins["words"]) == 60 and (ins["words"] >= 0).all() and (ins["words"] < 16).all()
    assert db.insert(b["descriptors"])["status"] == "OK" and db.size()["inserted"] == 2
    db.close()
    tree.close()

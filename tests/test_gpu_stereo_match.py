"""The stereo line matcher on the device against its numpy contract (tests/stereo_match_reference.py).  The inputs, their references
and the longdouble figure behind the tolerance of the doubles are those of tests/test_stereo_match_cpu.py: made once, shared, never
written to.  Integers, statuses and the float distances are compared bit for bit; observations and disparity may differ by 8 x the
reference's own fp64 rounding (its difference from the same formulas in np.longdouble on these inputs) - the device evaluates the same
operations in the same order, so the difference is expected to be 0 and the largest one seen is printed."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_match_reference as R  # noqa: E402
import test_stereo_match_cpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

BITWISE = ("match", "best", "num_admissible", "best_left", "best_distance", "second_distance")
WORST = {"observations": 0.0, "disparity": 0.0}


def compare(got, want, name):
    assert got["status"] == want["status"] and got["num_matched"] == want["num_matched"], name
    for k in BITWISE:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, k)
    assert got["segment_status"] == want["segment_status"], name
    tol = dict(zip(("observations", "disparity"), (8 * f for f in T.float64_figure())))
    matched = want["match"] >= 0
    for k in ("observations", "disparity"):
        assert np.isnan(got[k][~matched]).all(), (name, k)                      # rows that are not MATCHED stay as the caller made them
        if matched.any():
            d = float(np.abs(got[k][matched] - want[k][matched]).max())
            WORST[k] = max(WORST[k], d)
            assert d <= tol[k], (name, k, d, tol[k])


def run_one(name):
    ls, ld, rs, rd, opt = T.gpu_inputs()[name]
    return capi.match_stereo((ls, ld), (rs, rd), **opt)


@pytest.mark.parametrize("name", sorted(T.gpu_inputs()))
def test_one_frame(name):
    compare(run_one(name), T.reference(name), name)
    print("largest device difference so far: observations %.3g, disparity %.3g px" % (WORST["observations"], WORST["disparity"]))


def test_the_skip_path_and_every_status():
    got = run_one("skip")
    assert got["num_matched"] == 2 and got["match"][5] == 3 and got["match"][66] == 20 and got["num_admissible"].sum() == 2
    got = run_one("invalid_and_flat")
    assert {"MATCHED", "UNMATCHED", "FLAT", "INVALID"} == set(got["segment_status"])
    assert run_one("gated_out")["num_matched"] == 0


def test_batching_and_reuse():
    names = list(T.BATCH)
    frames = [((i[0], i[1]), (i[2], i[3])) for i in (T.gpu_inputs()[n] for n in names)]
    sm = capi.StereoMatcher(8, max_frames=3, max_segments=129)
    alone = [sm.run([f])[0] for f in frames]
    assert sm.stats() == {"calls": 3, "allocations": 1}
    together = sm.run(frames)
    for n, a, t in zip(names, alone, together):
        compare(a, T.reference(n), n)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == t[k].tobytes(), (n, k)                 # (NaN rows included: byte for byte)
            else:
                assert a[k] == t[k], (n, k)
    assert sm.stats() == {"calls": 4, "allocations": 1}                         # a call that fits allocates nothing
    sm.run(frames * 2)                                                          # more frames, but fewer segments than 3 x 129 a side
    assert sm.stats() == {"calls": 5, "allocations": 1}
    i = T.gpu_inputs()["size_129_129_8"]
    many = sm.run([((i[0], i[1]), (i[2], i[3]))] * 4)                           # four full frames: one growth
    assert sm.stats() == {"calls": 6, "allocations": 2}
    for r in many:
        compare(r, T.reference("size_129_129_8"), "size_129_129_8")
    sm.run(frames + frames[1:])
    assert sm.stats() == {"calls": 7, "allocations": 2}
    # options per run; timing by events
    sm.set_timing(True)
    g = sm.run([frames[1]], min_disparity=-90.0, max_disparity=-1.0)[0]
    assert g["num_matched"] == 0 and sm.kernel_ms() > 0.0
    sm.close()


def test_the_chain_from_images():
    """detect_describe_and_pair on make_stereo_line_pair images gives the reference chain's matches; its observations pass through
    match_lines and the triangulator."""
    p = T.pair()
    a, b, ka, kb, want = T.chain_reference()
    det = capi.LineDetector(max_frames=2, max_pixels=160 * 224)
    dsc = capi.LineDescriptor(max_frames=2, max_pixels=160 * 224, max_segments=64)
    sm = capi.StereoMatcher(dsc.D, max_frames=1, max_segments=64, **T.PAIR_OPTIONS)
    out = capi.detect_describe_and_pair(det, dsc, sm, [(p["left"], p["right"])])[0]
    assert out["left_rows"].tolist() == ka.tolist() and out["right_rows"].tolist() == kb.tolist()
    # the device's MSLD descriptors differ from the reference's in their last bits: the decisions are the same, the distances close
    assert out["stereo"]["match"].tolist() == want["match"].tolist() and out["stereo"]["segment_status"] == want["segment_status"]
    has = want["best"] >= 0
    assert np.abs(out["stereo"]["best_distance"][has] - want["best_distance"][has]).max() < 1e-4
    k = want["num_matched"]
    assert out["observations"].shape == (k, 8) and k == T.CHAIN_TRUE_MATCHES + 1
    assert np.array_equal(out["left_index"], ka[np.nonzero(want["match"] >= 0)[0]])
    assert np.abs(out["observations"] - R.observations(want)[0]).max() <= 1e-5   # (float segments from the device's detector)
    # pixels -> a camera: the same pairs under intrinsics are what the back end takes
    K = dict(fx=200.0, fy=200.0, cx=112.0, cy=80.0)
    obs = capi.detect_describe_and_pair(det, dsc, sm, [(p["left"], p["right"])], **K)[0]["observations"]
    assert np.allclose(obs[:, 0::2] * 200.0 + 112.0, out["observations"][:, 0::2], atol=1e-9)
    lines = np.tile(np.array([0.0, 0.0, 5.0, 1.0, 0.0, 0.0]), (k, 1))
    pose = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    m = capi.match_lines(dict(pose=pose, observations=obs, lines=lines))
    assert m["status"] == "OK" and len(m["match"]) == k
    # ... and each alone is a stereo pair the triangulator makes a line from: a finite line in front of the camera
    for o8 in obs:
        t = capi.triangulate_host(o8[None, :], np.zeros((1, 6)), baseline=0.12)
        assert t["status"] in (capi.TRI_MULTIVIEW, capi.TRI_STEREO) and np.isfinite(t["av"]).all(), t
    for x in (det, dsc, sm):
        x.close()

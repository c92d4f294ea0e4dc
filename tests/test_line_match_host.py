"""Host-side checks of the line matcher's entry points (include/slslam_hip.h: slslam_line_matcher_*, slslam_match_lines): the answer
without a device and argument validation, which comes before the device is asked.  No device needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_match_reference as M  # noqa: E402

THR = 5.0 / 406.05


@pytest.fixture(scope="module")
def nodevice():
    capi.lib()
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible: the no-device answer cannot be observed here")
    return capi


def test_every_compute_entry_point_without_device_is_no_device(nodevice):
    fr = M.make_frame(601, 20, 30, extents=True)
    m = capi.LineMatcher(max_frames=2, max_observations=64, max_lines=64)
    with pytest.raises(capi.SlslamError) as ei:
        m.run([fr, fr])
    assert ei.value.status == 2
    assert m.stats() == {"calls": 0, "allocations": 0}
    m.close()
    with pytest.raises(capi.SlslamError) as ei:
        capi.match_lines(fr)
    assert ei.value.status == 2


def _raw(fr):
    mf, keep = capi._match_frame(fr)
    r, b = capi._match_buffers(mf.num_observations, mf.num_lines)
    r.status, r.num_matched = 91, 92
    return mf, r, (keep, b)


@pytest.mark.parametrize("what", ["negative_k", "negative_l", "null_observations", "null_lines", "null_pose", "k_beyond", "l_beyond",
                                  "nan_thr", "nan_ratio", "negative_margin", "negative_frames", "null_frames", "null_out"])
def test_validation_before_device_check(what):
    L = capi.lib()
    good = M.make_frame(602, 20, 30)
    mf0, r0, keep0 = _raw(good)
    mf1, r1, keep1 = _raw(M.make_frame(603, 64, 64))
    if what == "negative_k":
        mf1.num_observations = -1
    if what == "negative_l":
        mf1.num_lines = -1
    if what == "null_observations":
        mf1.observations = C.POINTER(C.c_double)()
    if what == "null_lines":
        mf1.lines = C.POINTER(C.c_double)()
    if what == "null_pose":
        mf1.pose = C.POINTER(C.c_double)()
    if what == "k_beyond":
        mf1.num_observations = 65
    if what == "l_beyond":
        mf1.num_lines = 65
    frames, outs = (capi.MatchFrame * 2)(mf0, mf1), (capi.MatchResult * 2)(r0, r1)
    thr, ratio, margin, n = THR, 1.5, 0.0, 2
    if what == "nan_thr":
        thr = float("nan")
    if what == "nan_ratio":
        ratio = float("nan")
    if what == "negative_margin":
        margin = -0.1
    if what == "negative_frames":
        n = -1
    m = capi.LineMatcher(max_frames=2, max_observations=64, max_lines=64)
    rc = L.slslam_line_matcher_run(m._h, n, None if what == "null_frames" else frames, 0.12, thr, ratio, margin,
                                   None if what == "null_out" else outs)
    assert rc == 1                                                         # SLSLAM_ERR_INVALID_ARGUMENT, not NO_DEVICE
    assert all((o.status, o.num_matched) == (91, 92) for o in outs)
    assert all((b["match"] == -2).all() and (b["best_observation"] == -2).all() for b in (keep0[1], keep1[1]))
    assert m.stats()["calls"] == 0
    m.close()
    # the one-shot form takes any size, and validates the rest in the same way
    if what not in ("k_beyond", "l_beyond", "negative_frames", "null_frames", "null_out"):
        assert L.slslam_match_lines(C.byref(mf1), 0.12, thr, ratio, margin, C.byref(r1)) == 1


def test_null_handles_and_create_arguments():
    L = capi.lib()
    h = C.c_void_p()
    assert L.slslam_line_matcher_create(-1, 0, 64, 64, C.byref(h)) == 1
    assert L.slslam_line_matcher_create(-1, 2, 0, 64, C.byref(h)) == 1
    assert L.slslam_line_matcher_create(-1, 2, 64, 0, C.byref(h)) == 1
    assert L.slslam_line_matcher_create(-1, 2, 64, 64, None) == 1
    assert L.slslam_line_matcher_create(-1, 2, 64, 64, C.byref(h)) == 0
    assert L.slslam_line_matcher_stats(None, None, None) == 1
    assert L.slslam_line_matcher_stats(h, None, None) == 0
    L.slslam_line_matcher_destroy(h)
    L.slslam_line_matcher_destroy(None)
    assert L.slslam_line_matcher_run(None, 0, None, 0.12, THR, 1.5, 0.0, None) == 1
    assert L.slslam_match_lines(None, 0.12, THR, 1.5, 0.0, None) == 1


def test_empty_frames_need_no_arrays():
    """K = 0 or L = 0: the arrays of the zero count and the pose may be NULL - validation passes (the device is asked next)"""
    L = capi.lib()
    mf = capi.MatchFrame(0, 0, None, None, None, None)
    r = capi.MatchResult()
    assert L.slslam_match_lines(C.byref(mf), 0.12, THR, 1.5, 0.0, C.byref(r)) in (0, 2)


def test_matched_trials_aligns_the_pairs():
    fr = M.make_frame(604, 40, 40)
    res = M.match(fr)
    tr = capi.matched_trials(fr, res, fr["obs0"], num_trials=30)
    k = np.nonzero(res["match"] >= 0)[0]
    assert len(k) >= 5 and np.array_equal(tr["observation_index"], k) and np.array_equal(tr["line_index"], res["match"][k])
    assert np.array_equal(tr["obs1"], fr["observations"][k]) and np.array_equal(tr["obs0"], fr["obs0"][res["match"][k]])
    assert np.array_equal(tr["lines"], fr["lines"][res["match"][k]])
    s = tr["samples"]
    assert s.shape == (30, 5) and s.dtype == np.int32 and s.min() >= 0 and s.max() < len(k)
    assert all(len(set(row)) == 5 for row in s.tolist())
    few = capi.matched_trials(fr, dict(match=np.where(np.arange(40) < 3, res["match"], -1)), fr["obs0"], num_trials=4)
    assert few["samples"].shape == (4, 5) and few["samples"].max() < max(len(few["obs1"]), 1)

"""The numpy reference of the lines' 3-D segments (tests/lba_segments_reference.py) against geometry it must satisfy, without a GPU.

On a noise-free window at its true parameters every observation of a line is the projection of the same 3-D segment, so
  - every observation of a line gives the same (lo, hi): to 1e-10 (measured spread 2e-14 on this window; the cut of a plane with a
    line at |m^ . dc| >= 0.07 and |pc| < 20 m carries eps |pc| / |m^ . dc| ~ 6e-14);
  - p_min and p_max project onto the line's observed left endpoints in every observing camera: to 1e-10 in normalised image coordinates.
And the reference's Pluecker construction equals the contract's closed form to 1e-12 (measured 7e-15), with and without the range clamp."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_segments_reference as S  # noqa: E402
from lba_report_reference import with_extra_line  # noqa: E402


@pytest.fixture(scope="module")
def clean():
    w = synth.make_window(3, num_lines=60, num_kf=8, num_free=4, noise_px=0)
    x = np.asarray(w["true_parameters"], dtype=np.float64)
    return w, x, S.segments(w, x)


def test_every_observation_of_a_line_gives_the_same_interval(clean):
    w, x, ref = clean
    line = np.asarray(w["line_index"])
    assert (ref["obs_status"] == S.USED).all() and (ref["status"] == S.OK).all()
    spread = 0.0
    for l in range(int(w["num_lines"])):
        rg = ref["obs_range"][line == l]
        assert len(rg) >= 2
        spread = max(spread, np.abs(rg - rg[0]).max())
        assert ref["num_observations"][l] == ref["num_used"][l] == len(rg) and ref["num_clamped"][l] == 0
        assert ref["t_min"][l] == rg[:, 0].min() and ref["t_max"][l] == rg[:, 1].max()
    print("largest spread of (lo, hi) over a line's observations %.3g" % spread)
    assert spread <= 1e-10


def test_segment_ends_project_onto_the_observed_endpoints(clean):
    w, x, ref = clean
    poses, cp, dv = S.geometry(w, x)
    cam, line = np.asarray(w["camera_index"]), np.asarray(w["line_index"])
    obs = np.asarray(w["observations"]).reshape(-1, 8)
    worst = 0.0
    for i in range(len(cam)):
        R, t = poses[cam[i]]
        ends = []
        for P in (ref["p_min"][line[i]], ref["p_max"][line[i]]):
            pc = R @ P + t
            ends.append(pc[:2] / pc[2])
        a, b = obs[i, 0:2], obs[i, 2:4]
        d = min(max(np.abs(ends[0] - a).max(), np.abs(ends[1] - b).max()), max(np.abs(ends[0] - b).max(), np.abs(ends[1] - a).max()))
        worst = max(worst, d)
    print("largest distance of a projected segment end from its observed endpoint %.3g" % worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("max_range", [0.0, 5.0, 8.0])
def test_pluecker_construction_equals_the_closed_form(max_range):
    worst = 0.0
    for w in (synth.make_window(3, num_lines=60, num_kf=8, num_free=4, noise_px=0), synth.make_window(3, num_lines=60, num_kf=8, num_free=4)):
        for x in (w["true_parameters"], w["parameters"]):
            a, c = S.segments(w, x, max_range), S.closed_form(w, x, max_range)
            for k in ("obs_status", "status", "num_observations", "num_used", "num_clamped"):
                assert np.array_equal(a[k], c[k]), k
            for k in ("obs_range", "t_min", "t_max", "p_min", "p_max"):
                worst = max(worst, np.abs(a[k] - c[k]).max())
    print("max_range %g: Pluecker construction against the closed form, max |d| %.3g" % (max_range, worst))
    assert worst <= 1e-12


def test_statuses_of_handmade_observations():
    """The skip rules on observations made to trigger them (the GPU test's case 3 uses the same)."""
    w = synth.make_window(3, num_lines=60, num_kf=8, num_free=4)
    for name, (w2, want_obs, want_line) in handmade(w).items():
        for ref in (S.segments(w2, w2["parameters"]), S.closed_form(w2, w2["parameters"])):
            if want_obs is not None:
                assert ref["obs_status"][-1] == want_obs, name
            assert ref["status"][-1] == want_line, name
            if want_line != S.OK:
                assert not ref["t_min"][-1] and not ref["t_max"][-1] and not ref["p_min"][-1].any() and not ref["p_max"][-1].any()
    ref = S.segments(w, w["parameters"], 5.0)
    assert {S.OUT_OF_RANGE, S.USED_CLAMPED, S.USED} <= set(ref["obs_status"].tolist()) and {S.NONE, S.OK} <= set(ref["status"].tolist())


def handmade(w):
    """name -> (w with one more line, the status its one observation must get - None without one -, the line's status).  The new line is seen by the window's
    identity camera (the newest free keyframe: parameters exactly zero), so that camera-frame and world coordinates coincide."""
    C = int(w["num_cameras"])
    ident = int(w["num_free_cameras"]) - 1
    assert not np.asarray(w["parameters"])[6 * ident:6 * ident + 6].any()
    # a = b = g = 0: dv = (0, 1, 0) and cp = (0, 0, -cot t) exactly; t = 3 pi / 4: the line x = 0, z = 1 (up to the rounding of cot)
    u = np.array([0.0, 0.0, 0.0, 0.75 * np.pi])

    def obs(x0, y0, x1, y1):
        return np.array([x0, y0, x1, y1, x0 - synth.BASELINE, y0, x1 - synth.BASELINE, y1])

    out = {
        "seen_once": (with_extra_line(w, u, ident, obs(0.0, -0.5, 0.0, 0.5)), S.USED, S.OK),
        "same_endpoints": (with_extra_line(w, u, ident, obs(0.1, 0.2, 0.1, 0.2)), S.DEGENERATE, S.NONE),
        "nan": (with_extra_line(w, u, ident, obs(np.nan, -0.5, 0.0, 0.5)), S.DEGENERATE, S.NONE),
        # a horizontal image line: ln = (0, +-1), the endpoint planes hold the direction (0, 1, 0): m . dc = lx = 0 exactly
        "parallel_plane": (with_extra_line(w, u, ident, obs(-0.5, 0.25, 0.5, 0.25)), S.DEGENERATE, S.NONE),
    }
    # the line x = 0, z = -1, behind the identity camera: its endpoint planes cut it at z = -1
    out["behind"] = (with_extra_line(w, np.array([0.0, 0.0, 0.0, 0.25 * np.pi]), ident, obs(0.0, -0.5, 0.0, 0.5)), S.BEHIND, S.NONE)
    # a line nobody sees
    nobody = dict(w)
    nobody["num_lines"] = int(w["num_lines"]) + 1
    nobody["parameters"] = np.append(np.asarray(w["parameters"], dtype=np.float64), u)
    assert len(nobody["parameters"]) == 6 * C + 4 * nobody["num_lines"]
    out["no_observation"] = (nobody, None, S.NO_OBSERVATIONS)
    return out

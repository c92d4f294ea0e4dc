"""The report on LBA windows (include/slslam_hip.h: slslam_lba_batch_report), what can be checked without a device: the numpy reference
tests/lba_report_reference.py against the oracle, the degenerate-line fixture the GPU tests plant, the Huber margin of every fixture,
and the C ABI's argument checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle
from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_covariance_reference as R  # noqa: E402
import lba_report_reference as P  # noqa: E402

INVALID, NO_DEVICE = 1, 2
CASES = R.cases()


def degenerate_window():
    """free10 plus one line that is depth-degenerate by construction: a single observation from the identity keyframe (camera 9 of
    free10: the newest free one), direction (1, 0, 0) in that camera's frame = parallel to the stereo baseline.  Both images see the
    same image line y = Y / Z, so the depth along the ray is exactly unobservable and H_ll has rank <= 3.  Returns (window, line)."""
    w = CASES["free10"][0]
    cam = int(w["num_free_cameras"]) - 1
    assert not np.asarray(w["parameters"])[6 * cam:6 * cam + 6].any()             # the identity keyframe
    Y, Z = 0.5, 4.0
    u = synth.av_to_orth(np.array([[0.0, Y, Z, 1.0, 0.0, 0.0]]))[0]
    obs = np.array([-0.2, Y / Z, 0.3, Y / Z, -0.2 - synth.BASELINE / Z, Y / Z, 0.3 - synth.BASELINE / Z, Y / Z])
    return P.with_extra_line(w, u, cam, obs), int(w["num_lines"])


@pytest.fixture(scope="module")
def solved():
    """name -> (window, huber_delta, the oracle's solved point, the reference there)."""
    out = {}
    items = {k: (v[0], v[1]) for k, v in CASES.items()}
    items["degenerate"] = (degenerate_window()[0], R.HUBER)
    for k, (w, hd) in items.items():
        x, _, _ = pyoracle.lba_solve(w, huber_delta=hd, linear_solver=1)
        out[k] = (w, hd, x, P.report(w, x, hd))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_reference_costs_and_weights_match_the_oracle(solved, name):
    w, hd, x, rep = solved[name]
    total = pyoracle.lba_cost(w, x, hd)                                            # fixed part included
    assert abs(rep["lines"]["cost"].sum() - total) <= 1e-13 * total
    assert abs(rep["cameras"]["cost"].sum() - total) <= 1e-13 * total
    # the weight is the square of the oracle's corrector: its robustified residuals are sqrt(rho') r
    _, r, _, _ = pyoracle.lba_cost(w, x, hd, want_jac=True)
    s_rob = (r * r).sum(1)
    # (two evaluations of the same residuals, jets and plain: 1e-14 absolute on each of four components, so |ds| <= 2 |r| |dr|)
    assert (np.abs(s_rob - rep["weight"] * rep["sq_norm"]) <= 4e-14 * np.sqrt(rep["sq_norm"]) + 1e-27).all()
    if hd > 0:
        for s, wt in zip(rep["sq_norm"], rep["weight"]):
            assert wt == pyoracle.huber(s, hd)[1]
        assert (rep["weight"] < 1.0).any() and (rep["weight"] == 1.0).any()        # the fixture exercises both branches
    else:
        assert (rep["weight"] == 1.0).all()
    assert rep["lines"]["num_observations"].sum() == len(w["camera_index"]) == rep["cameras"]["num_observations"].sum()
    assert rep["lines"]["num_downweighted"].sum() == int((rep["weight"] < 1.0).sum())


@pytest.mark.parametrize("name", list(CASES) + ["degenerate"])
def test_singular_with_well_posed_S_iff_a_line_pivot_falls(solved, name):
    w, hd, x, rep = solved[name]
    jc, jl = R.oracle_jacobians(w, x, hd)
    _, _, piv_s, piv_l = R.cov_schur(w, jc, jl, want_cov=False)
    free = rep["lines"]["status"] == P.FREE
    piv = np.append(rep["lines"]["min_pivot"][free], np.inf)                       # (a window without a free line: inf, as cov_schur says)
    assert piv.min() == piv_l                                                      # the same number, line by line
    line_singular = piv_l <= R.PIVOT_MIN
    assert line_singular == bool((piv <= R.PIVOT_MIN).any())
    print("%s: smallest pivot of S %.3g, of the lines %.3g" % (name, piv_s, piv_l))
    assert line_singular == (name == "degenerate")
    if name == "degenerate":                                                       # S itself is well-posed
        assert P.schur_pivot_without_degenerate_lines(w, x, hd, np.where(free, rep["lines"]["min_pivot"], 1.0)) > R.PIVOT_MIN


def test_degenerate_fixture_has_two_orders_of_margin(solved):
    """(a) of the issue alone: pushing a well-observed line out in depth (b) was not pursued."""
    w, hd, x, rep = solved["degenerate"]
    _, planted = degenerate_window()
    for point in (np.asarray(w["parameters"], dtype=np.float64), x):
        lines = P.report(w, point, hd)["lines"]
        free = np.nonzero(lines["status"] == P.FREE)[0]
        print("planted line: min_pivot %.3g; smallest of the others %.3g" % (
            lines["min_pivot"][planted], lines["min_pivot"][free[free != planted]].min()))
        assert lines["status"][planted] == P.FREE and lines["num_observations"][planted] == 1
        assert lines["min_pivot"][planted] <= 1e-12
        assert (lines["min_pivot"][free[free != planted]] >= 1e-8).all()


@pytest.mark.parametrize("name", list(CASES) + ["degenerate"])
def test_huber_margin_at_the_solved_point(solved, name):
    """No observation sits within 1e-6 a^2 of the corner of the loss: no weight comparison needs excluding."""
    w, hd, x, rep = solved[name]
    m = P.huber_margin(rep["sq_norm"], hd)
    print("%s: smallest |s - a^2| / a^2 = %.3g" % (name, m))
    assert m > 1e-6


# ---- the C ABI without a device
def test_symbols_exist():
    for name in ("slslam_lba_batch_report", "slslam_lba_batch_get_report", "slslam_lba_batch_report_stats", "slslam_lba_report"):
        assert name in capi.EXPORTS
        getattr(capi.lib(), name)
    for name in ("report", "get_report", "report_stats"):
        assert callable(getattr(capi.LBABatch, name)) and callable(getattr(capi._BatchView, name))
    assert capi.LINE_REPORT_DTYPE.itemsize == 40 and capi.CAMERA_REPORT_DTYPE.itemsize == 32


def test_bad_arguments_are_invalid():
    L = capi.lib()
    assert L.slslam_lba_batch_report(None, None) == INVALID
    assert L.slslam_lba_batch_get_report(None, 0, None, None, None, None) == INVALID
    assert L.slslam_lba_batch_report_stats(None, None, None) == INVALID
    assert L.slslam_lba_report(None, None, None, None, None, None) == INVALID
    w = CASES["free2"][0]
    arr = capi._WindowArrays(w)
    o = capi.default_options()
    arr.c.num_observations = -1                                                    # a negative count
    assert L.slslam_lba_report(C.byref(arr.c), C.byref(o), None, None, None, None) == INVALID
    bad = dict(w)
    bad["camera_index"] = np.array(w["camera_index"], dtype=np.int32)
    bad["camera_index"][0] = int(w["num_cameras"])                                 # an index out of range
    arr = capi._WindowArrays(bad)
    assert L.slslam_lba_report(C.byref(arr.c), C.byref(o), None, None, None, None) == INVALID


def test_one_shot_needs_a_device_after_validation():
    """A valid window: NO_DEVICE on a machine without one (with one, the call runs: tests/test_gpu_lba_report.py)."""
    w = CASES["free2"][0]
    if capi.device_count() == 0:
        with pytest.raises(capi.SlslamError) as ei:
            capi.lba_report(w)
        assert ei.value.status == NO_DEVICE
        h = C.c_void_p()                                                           # (an out-of-range index needs a batch, a batch a device)
        assert capi.lib().slslam_lba_batch_create(-1, C.byref(h)) == NO_DEVICE
    else:
        rep = capi.lba_report(w)
        assert rep["sq_norm"].shape == (len(w["camera_index"]),) and rep["lines"].shape == (int(w["num_lines"]),)

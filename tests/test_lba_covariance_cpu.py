"""Host-side checks of the LBA covariances (include/slslam_hip.h: slslam_lba_batch_covariance, _get_covariance, slslam_lba_covariance):
the numpy reference the GPU tests compare against agrees with itself on the windows they use, those windows keep their distance from
the SINGULAR threshold on either side, the new symbols resolve, and what can be refused without a device is.  No device needed.
The checks of the reference against itself and of the windows' margins need only numpy and the oracle: they guard the yardstick and pass
with or without the library's covariance entry points; the symbol and validation tests below them fail without those."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_covariance_reference as R  # noqa: E402

INVALID, NO_DEVICE = 1, 2
CASES = R.cases()
WELL_POSED = [k for k, v in CASES.items() if v[2]]


@pytest.fixture(scope="module")
def refs():
    return {k: R.reference(CASES[k][0], np.asarray(CASES[k][0]["parameters"], dtype=np.float64), CASES[k][1]) for k in WELL_POSED}


@pytest.mark.parametrize("name", WELL_POSED)
def test_reference_routes_agree(refs, name):
    """QR of J and the Schur route give the same covariance; the measured differences (d_route, the GPU tests' yardstick) are
    2e-13 ... 6e-10 for the cameras and 3e-13 ... 6e-9 for the lines - 1e-7 is two orders above the worst and still far below any
    mistake in the algebra, which shows in the first digit."""
    r = refs[name]
    print(name, "d_route cameras %.3g lines %.3g" % (r["d_route_cam"], r["d_route_line"]))
    assert r["d_route_cam"] < 1e-7 and r["d_route_line"] < 1e-7


@pytest.mark.parametrize("name", WELL_POSED)
def test_reference_is_the_inverse_of_the_normal_matrix(refs, name):
    """The camera block and the lines' diagonal blocks of (J^T J)^-1: rebuilt as a full inverse through the Schur complement and multiplied
    back.  ||Σ H - I||_max is bounded by cond(H) eps ~ 1e-16 / (smallest pivots ~ 6e-7 of a line block x 1.4e-2 of S, as the margin test
    below prints them) ~ 1e-8, and the entries of H reach ~1e3 x its diagonal scaling: 1e-5."""
    w, hd, _ = CASES[name]
    jc, jl = R.oracle_jacobians(w, np.asarray(w["parameters"], dtype=np.float64), hd)
    H = R.hessian(w, jc, jl)
    n = 6 * len(refs[name]["free_cameras"])
    Scc = refs[name]["qr"][0]
    Hcc, Hcl, Hll = H[:n, :n], H[:n, n:], H[n:, n:]
    if Hll.size:
        K = np.linalg.solve(Hll, Hcl.T)                   # H_ll^-1 H_lc
        full = np.block([[Scc, -Scc @ K.T], [-K @ Scc, np.linalg.inv(Hll) + K @ Scc @ K.T]])
        ql = refs[name]["qr"][1]
        for s, l in enumerate(refs[name]["free_lines"]):
            blk = full[n + 4 * s:n + 4 * s + 4, n + 4 * s:n + 4 * s + 4]
            assert np.abs(blk - ql[l]).max() <= 1e-6 * np.abs(ql[l]).max()
    else:
        full = Scc
    assert np.abs(full @ H - np.eye(H.shape[0])).max() < 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_windows_keep_their_margin_around_the_singular_threshold(name):
    """SINGULAR is a unit-diagonal Cholesky pivot <= 1e-10: every well-posed test window stays above 1e-7, the all-free one (6-dimensional
    gauge null space) has an S pivot below 1e-11 - a change of the generator cannot silently move a window across the line."""
    w, hd, well_posed = CASES[name]
    jc, jl = R.oracle_jacobians(w, np.asarray(w["parameters"], dtype=np.float64), hd)
    _, _, piv_s, piv_l = R.cov_schur(w, jc, jl, want_cov=False)
    print(name, "smallest pivot of S %.3g, of the line blocks %.3g" % (piv_s, piv_l))
    assert piv_l >= 1e-7
    if well_posed:
        assert piv_s >= 1e-7
    else:
        assert piv_s <= 1e-11


def test_free_sets_follow_the_solve_rule():
    w = CASES["constant_lines"][0]
    fc, fl = R.free_sets(w)
    assert list(fc) == [0, 1, 2]
    assert all(l % 4 != 1 for l in fl) and len(fl) < w["num_lines"]
    fc, fl = R.free_sets(CASES["motion_only"][0])
    assert len(fc) == 1 and len(fl) == 0


def test_symbols_resolve():
    L = capi.lib()
    for name in ("slslam_lba_batch_covariance", "slslam_lba_batch_get_covariance", "slslam_lba_batch_covariance_stats", "slslam_lba_covariance"):
        assert name in capi.EXPORTS
        getattr(L, name)
    assert hasattr(capi.LBABatch, "covariance") and hasattr(capi.LBABatch, "get_covariance") and hasattr(capi, "lba_covariance")
    assert (capi.COV_OK, capi.COV_SINGULAR) == (0, 1)


def test_null_arguments_are_invalid():
    L = capi.lib()
    st = C.c_int(-7)
    assert L.slslam_lba_batch_covariance(None, None, 1) == INVALID
    assert L.slslam_lba_batch_get_covariance(None, 0, C.byref(st), None, None, None, None) == INVALID
    assert L.slslam_lba_batch_covariance_stats(None, None, None) == INVALID
    assert L.slslam_lba_covariance(None, None, C.byref(st), None, None, None, None) == INVALID
    assert st.value == -7


@pytest.mark.parametrize("what", ["camera_high", "line_negative", "nan_parameter", "nan_observation"])
def test_one_shot_validates_before_it_looks_for_a_device(what):
    """slslam_lba_covariance refuses what slslam_lba_solve refuses, on any machine."""
    w = dict(CASES["free2"][0])
    if what == "camera_high":
        w["camera_index"] = np.array(w["camera_index"]).copy(); w["camera_index"][3] = w["num_cameras"]
    elif what == "line_negative":
        w["line_index"] = np.array(w["line_index"]).copy(); w["line_index"][5] = -1
    elif what == "nan_parameter":
        w["parameters"] = np.array(w["parameters"], dtype=np.float64).copy(); w["parameters"][7] = np.nan
    else:
        w["observations"] = np.array(w["observations"], dtype=np.float64).copy(); w["observations"].reshape(-1)[11] = np.nan
    with pytest.raises(capi.SlslamError) as ei:
        capi.lba_solve(w)
    assert ei.value.status == INVALID
    with pytest.raises(capi.SlslamError) as ei:
        capi.lba_covariance(w)
    assert ei.value.status == INVALID
    with pytest.raises(capi.SlslamError) as ei:
        capi.lba_covariance(CASES["free2"][0], max_num_iterations=-1)
    assert ei.value.status == INVALID


def test_one_shot_without_device_is_no_device():
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible: the no-device answer cannot be observed here")
    with pytest.raises(capi.SlslamError) as ei:
        capi.lba_covariance(CASES["free2"][0])
    assert ei.value.status == NO_DEVICE

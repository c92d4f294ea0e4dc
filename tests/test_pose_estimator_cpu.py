"""Host-side checks of the per-frame pose estimator (include/slslam_hip.h: slslam_pose_estimator_*) and of its input merge
(slslam_pose_estimation_inputs, slslam_amd/host/window_packer.h: SLAM::pose_estimation, reference src/slam.cpp:250-272).
No device needed."""
import ctypes as C
import os

import numpy as np
import pytest

from slslam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "slslam_amd", "_lib", "libslslam_host.so")


class Pose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class Keyframe(C.Structure):
    _fields_ = [("id", C.c_int), ("ba_rank", C.c_int), ("T", Pose), ("member_lms", C.POINTER(C.c_int)), ("num_member_lms", C.c_int)]


class Observation(C.Structure):
    _fields_ = [("kf_id", C.c_int), ("obs", C.c_double * 8)]


class Landmark(C.Structure):
    _fields_ = [("id", C.c_int), ("line", C.c_double * 6), ("init_kf_id", C.c_int), ("obs", C.POINTER(Observation)), ("num_obs", C.c_int)]


class FeatureObs(C.Structure):
    _fields_ = [("id", C.c_int), ("obs", C.c_double * 8)]


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(HOST_LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(HOST_LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.slslam_pose_estimation_inputs.argtypes = [C.POINTER(FeatureObs), C.c_int, C.POINTER(FeatureObs), C.c_int, C.POINTER(Landmark), C.c_int,
                                                C.POINTER(Keyframe), C.c_int, ip, dp, dp, dp, ip]
    return L


@pytest.fixture(scope="module")
def nodevice():
    capi.lib()
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible: the no-device answer cannot be observed here")
    return capi


def _frames():
    return [synth.make_ransac_pair(3100 + i, num_lines=k, num_trials=40) for i, k in enumerate((40, 150))]


def test_run_without_device_is_no_device(nodevice):
    est = capi.PoseEstimator(max_frames=4, max_lines=200)
    with pytest.raises(capi.SlslamError) as ei:
        est.run(_frames())
    assert ei.value.status == 2
    assert est.stats()["calls"] == 0
    est.close()


@pytest.mark.parametrize("what", ["sample", "null_lines", "sample_size", "negative_lines"])
def test_validation_before_device_check(what):
    frames = _frames()
    trs = (capi.RansacTrials * 2)()
    lns = (C.POINTER(C.c_double) * 2)()
    keep = []
    for i, fr in enumerate(frames):
        smp = fr["samples"].copy()
        if what == "sample" and i == 1:
            smp[7, 3] = len(fr["lines"])                                  # one past the last common line
        tr, k = capi._trials(fr["obs0"], fr["obs1"], smp)
        ln = np.ascontiguousarray(fr["lines"])
        keep += [k, ln, smp]
        trs[i] = tr
        lns[i] = capi._dp(ln)
    if what == "null_lines":
        lns[0] = C.POINTER(C.c_double)()
    if what == "sample_size":
        trs[1].sample_size = 17
    if what == "negative_lines":
        trs[0].num_lines = -1
    out = (capi.PoseEstimate * 2)()
    for o in out:
        o.status, o.trial_cnt, o.num_inliers = 91, 92, 93
    est = capi.PoseEstimator(max_frames=2, max_lines=200)
    rc = capi.lib().slslam_pose_estimator_run(est._h, 2, trs, lns, 0.12, 5.0 / 406.05, 0.999, 1000, out)
    assert rc == 1                                                         # SLSLAM_ERR_INVALID_ARGUMENT, not NO_DEVICE
    assert all((o.status, o.trial_cnt, o.num_inliers) == (91, 92, 93) for o in out)
    assert capi.lib().slslam_pose_estimator_run(None, 0, None, None, 0.12, 0.01, 0.999, 1000, None) == 1
    est.close()


def test_create_arguments():
    h = C.c_void_p()
    L = capi.lib()
    assert L.slslam_pose_estimator_create(-1, None, 0, 100, C.byref(h)) == 1
    assert L.slslam_pose_estimator_create(-1, None, 4, 4, C.byref(h)) == 1
    assert L.slslam_pose_estimator_create(-1, None, 4, 100, C.byref(h)) == 0
    L.slslam_pose_estimator_destroy(h)


# ---- the merge by feature id (slam.cpp:250-272), restated in numpy

def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _reference_merge(ids0, o0, ids1, o1, lm_line, lm_kf, kf_T):
    """ob_map walk of SLAM::pose_estimation; line = gc_line_from_pose(lm.line, kfs[lm.init_kfid].T) = (R^T (cp - t), R^T dv)"""
    m0, m1 = dict(zip(ids0, o0)), dict(zip(ids1, o1))
    ids = sorted(set(ids0) & set(ids1))
    lines = []
    for i in ids:
        R, t = kf_T[lm_kf[i]]
        cp, dv = lm_line[i][:3], lm_line[i][3:]
        lines.append(np.concatenate([R.T @ cp + (-(R.T @ t)), R.T @ dv]))
    return ids, np.array([m0[i] for i in ids]).reshape(-1, 8), np.array([m1[i] for i in ids]).reshape(-1, 8), np.array(lines).reshape(-1, 6)


@pytest.mark.parametrize("case", ["disjoint", "overlap", "identical"])
def test_pose_estimation_inputs_merge(host, case):
    rng = np.random.default_rng({"disjoint": 1, "overlap": 2, "identical": 3}[case])
    if case == "disjoint":
        ids0, ids1 = list(range(0, 40, 2)), list(range(1, 41, 2))
    elif case == "overlap":
        ids0 = sorted(rng.choice(200, 80, replace=False).tolist())
        ids1 = sorted(rng.choice(200, 90, replace=False).tolist())
    else:
        ids0 = ids1 = sorted(rng.choice(100, 30, replace=False).tolist())
    o0, o1 = rng.normal(size=(len(ids0), 8)), rng.normal(size=(len(ids1), 8))
    # keyframes 10, 11, 12 with their own poses; every landmark's line lives in its init keyframe's frame
    kf_T = {10 + j: (_rodrigues(rng.normal(size=3) * 0.3), rng.normal(size=3)) for j in range(3)}
    all_ids = sorted(set(ids0) | set(ids1))
    lm_line = {i: np.concatenate([rng.normal(size=3), rng.normal(size=3)]) for i in all_ids}
    lm_kf = {i: 10 + (i % 3) for i in all_ids}
    kfs = (Keyframe * 3)()
    for j, (kid, (R, t)) in enumerate(sorted(kf_T.items())):
        kfs[j].id = kid; kfs[j].ba_rank = -1
        kfs[j].T.R[:] = R.reshape(-1).tolist(); kfs[j].T.t[:] = t.tolist()
    lms = (Landmark * len(all_ids))()
    for j, i in enumerate(all_ids):
        lms[j].id = i; lms[j].line[:] = lm_line[i].tolist(); lms[j].init_kf_id = lm_kf[i]
    f0, f1 = (FeatureObs * max(len(ids0), 1))(), (FeatureObs * max(len(ids1), 1))()
    for j, i in enumerate(ids0):
        f0[j].id = i; f0[j].obs[:] = o0[j].tolist()
    for j, i in enumerate(ids1):
        f1[j].id = i; f1[j].obs[:] = o1[j].tolist()
    cap = min(len(ids0), len(ids1)) or 1
    ids = np.zeros(cap, dtype=np.int32)
    b0, b1, bl = np.zeros((cap, 8)), np.zeros((cap, 8)), np.zeros((cap, 6))
    k = C.c_int(-1)
    assert host.slslam_pose_estimation_inputs(f0, len(ids0), f1, len(ids1), lms, len(all_ids), kfs, 3, capi._ip(ids), capi._dp(b0),
                                              capi._dp(b1), capi._dp(bl), C.byref(k)) == 0
    rid, r0, r1, rl = _reference_merge(ids0, o0, ids1, o1, lm_line, lm_kf, kf_T)
    assert k.value == len(rid)
    assert ids[:k.value].tolist() == rid
    assert np.array_equal(b0[:k.value], r0) and np.array_equal(b1[:k.value], r1)
    assert np.abs(bl[:k.value] - rl).max(initial=0.0) < 1e-12
    if case == "disjoint":
        assert k.value == 0
    # unsorted input is refused
    if len(ids0) > 1:
        f0[0].id, f0[1].id = f0[1].id, f0[0].id
        assert host.slslam_pose_estimation_inputs(f0, len(ids0), f1, len(ids1), lms, len(all_ids), kfs, 3, capi._ip(ids), capi._dp(b0),
                                                  capi._dp(b1), capi._dp(bl), C.byref(k)) == 1

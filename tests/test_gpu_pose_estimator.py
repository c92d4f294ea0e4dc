"""GPU tests: the per-frame pose estimator (slslam_pose_estimator_*: SLAM::pose_estimation, reference src/slam.cpp:244-319) - RANSAC,
motion-only BA on its inliers and the final inlier set for many frames in one call - against the chain of the existing entry points
(slslam_ransac_motion_batch with best_score -1, a fresh fused motion-only batch of the host-packed window, slslam_ransac_score under
the refined pose) and against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from slslam_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "slslam_amd", "_lib", "libslslam_host.so")
MAX_TRIALS = 1000
FUSED = 1          # SLSLAM_PATH_FUSED_MOTION_ONLY


class Pose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class PackedWindow(C.Structure):
    _fields_ = [("num_cameras", C.c_int), ("num_lines", C.c_int), ("num_observations", C.c_int), ("num_parameters", C.c_int),
                ("camera_index", C.POINTER(C.c_int)), ("line_index", C.POINTER(C.c_int)), ("fixed_index", C.POINTER(C.c_int)),
                ("observations", C.POINTER(C.c_double)), ("parameters", C.POINTER(C.c_double)),
                ("camera_kf_id", C.POINTER(C.c_int)), ("line_lm_id", C.POINTER(C.c_int))]


@pytest.fixture(scope="module")
def host():
    L = C.CDLL(HOST_LIB)
    dp = C.POINTER(C.c_double)
    L.slslam_pack_motion_only.argtypes = [C.POINTER(Pose), dp, dp, dp, C.c_int, C.POINTER(PackedWindow)]
    L.slslam_free_packed_window.argtypes = [C.POINTER(PackedWindow)]
    L.slslam_free_packed_window.restype = None
    L.slslam_gc_wt_to_Rt.argtypes = [dp, C.POINTER(Pose)]
    L.slslam_gc_Rt_to_wt.argtypes = [C.POINTER(Pose), dp]
    L.slslam_gc_av_to_orth.argtypes = [dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _pose(T):
    p = Pose()
    p.R[:] = list(T[:9]); p.t[:] = list(T[9:])
    return p


def wt_to_Rt(host, wt):
    wt = np.ascontiguousarray(wt, dtype=np.float64)
    p = Pose()
    host.slslam_gc_wt_to_Rt(_dp(wt), C.byref(p))
    return np.array(list(p.R) + list(p.t))


def host_pack(host, T, obs1, obs0, lines):
    """slslam_pack_motion_only of the inliers -> window dict in the LBA array contract"""
    o1, o0, ln = (np.ascontiguousarray(a, dtype=np.float64) for a in (obs1, obs0, lines))
    pw = PackedWindow()
    assert host.slslam_pack_motion_only(C.byref(_pose(T)), _dp(o1), _dp(o0), _dp(ln), len(ln), C.byref(pw)) == 0
    M = pw.num_observations
    w = {"num_cameras": pw.num_cameras, "num_lines": pw.num_lines, "num_observations": M,
         "camera_index": np.ctypeslib.as_array(pw.camera_index, (M,)).copy(), "line_index": np.ctypeslib.as_array(pw.line_index, (M,)).copy(),
         "fixed_index": np.ctypeslib.as_array(pw.fixed_index, (2 * M,)).copy(),
         "observations": np.ctypeslib.as_array(pw.observations, (8 * M,)).copy().reshape(-1, 8),
         "parameters": np.ctypeslib.as_array(pw.parameters, (pw.num_parameters,)).copy()}
    host.slslam_free_packed_window(C.byref(pw))
    return w


def make_frames(seed0, specs):
    """specs: (K, outlier fraction, trials)"""
    out = []
    for i, (k, of, t) in enumerate(specs):
        if k == 0:
            out.append({"obs0": np.zeros((0, 8)), "obs1": np.zeros((0, 8)), "lines": np.zeros((0, 6)), "samples": np.zeros((t, 5), np.int32)})
            continue
        if k < 5:
            fr = synth.make_ransac_pair(seed0 + i, num_lines=8, outlier_frac=of, num_trials=t)
            smp = (np.arange(5 * t, dtype=np.int32).reshape(t, 5)) % k
            out.append({"obs0": fr["obs0"][:k], "obs1": fr["obs1"][:k], "lines": fr["lines"][:k], "samples": smp})
            continue
        out.append(synth.make_ransac_pair(seed0 + i, num_lines=k, outlier_frac=of, num_trials=t))
    return out


def composed(hip, host, frames, max_trials=MAX_TRIALS):
    """The chain of existing entry points: RANSAC batch (best_score -1), a fresh fused motion-only batch of the host-packed windows,
    one ransac_score per frame under the refined pose"""
    rs = hip.ransac_motion_batch(frames, max_trials=max_trials, best_score=-1)
    res = []
    solv = []
    for i, (fr, (tc, bs, pose, mask)) in enumerate(zip(frames, rs)):
        k = len(fr["lines"])
        st = "TOO_FEW_FEATURES" if k < 5 else "RANSAC_FAILED" if bs < 5 else "OK"
        if k < 5:
            tc, bs, mask = 0, -1, np.zeros(k, dtype=bool)
        res.append({"status": st, "trial_cnt": tc, "ransac_score": bs, "ransac_pose": pose, "ransac_mask": mask})
        if st == "OK":
            solv.append(i)
    if solv:
        b = hip.LBABatch()
        for i in solv:
            fr, m = frames[i], res[i]["ransac_mask"]
            b.add(host_pack(host, res[i]["ransac_pose"], fr["obs1"][m], fr["obs0"][m], fr["lines"][m]))
        b.finalize()
        assert b.path() == FUSED
        b.solve(); b.download()
        for j, i in enumerate(solv):
            x = b.parameters(j)
            T = wt_to_Rt(host, x[:6])
            _, mask = hip.ransac_score(T, frames[i]["obs1"], frames[i]["lines"])
            res[i].update(summary=b.summary(j), pose=T, mask=mask[0], wt=x[:6].copy())
        b.close()
    return res


SPECS = [(5, 0.1, 200), (40, 0.3, 1001), (150, 0.2, 1001), (400, 0.4, 1001), (40, 0.5, 600), (150, 0.1, 300),
         (400, 0.2, 1001), (5, 0.3, 50), (150, 0.5, 1001), (40, 0.1, 1001), (400, 0.3, 800), (150, 0.4, 1001),
         (5, 0.2, 1001), (40, 0.2, 100), (400, 0.1, 1001), (150, 0.3, 500), (40, 0.4, 1001), (400, 0.5, 1001),
         (150, 0.2, 64), (5, 0.4, 1001), (40, 0.3, 300), (150, 0.1, 1001), (400, 0.2, 700), (40, 0.5, 1001)]


def _same_frame(a, b, exact_pose=False):
    assert a["status"] == b["status"], (a["status"], b["status"])
    assert a["trial_cnt"] == b["trial_cnt"] and a["ransac_score"] == b["ransac_score"]
    if a["ransac_score"] >= 0:
        assert np.array_equal(a["ransac_pose"], b["ransac_pose"])
    assert np.array_equal(a["ransac_mask"], b["ransac_mask"])
    if a["status"] == "OK":
        for key in ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks"):
            assert a["summary"][key] == b["summary"][key], (key, a["summary"], b["summary"])
        if exact_pose:
            assert np.array_equal(a["pose"], b["pose"]) and a["summary"] == b["summary"]
        else:
            assert np.abs(a["pose"] - b["pose"]).max() < 1e-10
        assert np.array_equal(a["mask"], b["mask"])


def test_equals_composed_path(hip, host):
    frames = make_frames(9100, SPECS)
    est = hip.PoseEstimator(max_frames=len(frames), max_lines=400)
    got = est.run(frames, max_trials=MAX_TRIALS)
    ref = composed(hip, host, frames)
    assert sum(r["status"] == "OK" for r in ref) >= 20
    for g, r in zip(got, ref):
        _same_frame(g, r)
        if g["status"] == "OK":
            assert g["num_inliers"] == int(r["mask"].sum())
            assert np.isclose(g["summary"]["final_cost"], r["summary"]["final_cost"], rtol=1e-9, atol=1e-18)
    est.close()


def test_against_oracle(hip, oracle):
    frames = make_frames(9300, [(150, 0.2, 1001), (40, 0.3, 1001), (400, 0.3, 1001), (5, 0.1, 300)])
    est = hip.PoseEstimator(max_frames=4, max_lines=400)
    got = est.run(frames, max_trials=MAX_TRIALS)
    assert sum(g["status"] == "OK" for g in got) >= 3
    for f, (fr, g) in enumerate(zip(frames, got)):
        tc, bs, pose, inl = oracle.ransac_motion(fr["obs0"], fr["obs1"], fr["lines"], fr["samples"], max_trials=MAX_TRIALS, best_score=-1)
        assert (g["trial_cnt"], g["ransac_score"]) == (tc, bs)
        assert np.array_equal(g["ransac_mask"], inl)
        assert g["status"] == ("OK" if bs >= 5 else "RANSAC_FAILED")
        if g["status"] != "OK":
            continue
        # the motion-only window of the oracle's inliers, packed as the reference does (slam.cpp:590-640)
        w = est.window(f)
        n = int(inl.sum())
        ln = fr["lines"][inl]
        win = {"num_cameras": 2, "num_lines": n, "num_observations": 2 * n,
               "camera_index": np.tile([0, 1], n).astype(np.int32), "line_index": np.repeat(np.arange(n), 2).astype(np.int32),
               "fixed_index": np.tile([0, 1, 1, 1], n).astype(np.int32),
               "observations": np.stack([fr["obs1"][inl], fr["obs0"][inl]], axis=1).reshape(-1, 8),
               "parameters": np.concatenate([w["parameters"][:12]] + [oracle.av_to_orth(l) for l in ln])}
        x, s, _ = oracle.lba_solve(win, linear_solver=1)
        assert s["num_successful_steps"] == g["summary"]["num_successful_steps"]
        T = np.concatenate([synth.rodrigues(x[:3]).reshape(-1), x[3:6]])
        assert np.abs(T - g["pose"]).max() < 1e-7
        sc, fin = oracle.ransac_score(g["pose"], fr["obs1"], fr["lines"])
        assert np.array_equal(fin[0], g["mask"]) and g["num_inliers"] == int(fin[0].sum())
    est.close()


def test_statuses_in_one_call(hip, host):
    good = make_frames(9500, [(150, 0.2, 1001), (40, 0.3, 400)])
    # K = 0, K = 4, a frame whose best score stays below 5 (scattered correspondences: every sample degenerate or far off), and one
    # that only reaches 0: its lines are all far off under every hypothesis
    rng = np.random.default_rng(9512)
    low = synth.make_ransac_pair(9510, num_lines=12, outlier_frac=0.0, num_trials=200)
    low = dict(low, obs1=rng.uniform(-1, 1, size=(12, 8)))
    zero = synth.make_ransac_pair(9511, num_lines=30, outlier_frac=0.0, num_trials=300)
    zero = dict(zero, obs1=rng.uniform(-5, 5, size=(30, 8)))
    bad = make_frames(9520, [(0, 0.0, 10), (4, 0.2, 10)]) + [low, zero]
    frames = [good[0]] + bad[:2] + [good[1]] + bad[2:]
    est = hip.PoseEstimator(max_frames=8, max_lines=200)
    got = est.run(frames, max_trials=MAX_TRIALS)
    assert [g["status"] for g in got[:3]] == ["OK", "TOO_FEW_FEATURES", "TOO_FEW_FEATURES"]
    assert got[1]["trial_cnt"] == 0 and got[2]["trial_cnt"] == 0
    assert got[3]["status"] == "OK"
    assert got[4]["status"] == "RANSAC_FAILED" and got[4]["ransac_score"] < 5
    z = got[5]
    assert z["status"] == "RANSAC_FAILED"
    if z["ransac_score"] == 0:
        # -1 start: a trial scoring 0 becomes the best, ransac_trial jumps to ~6.9 M, the loop runs to max_trials
        assert z["trial_cnt"] == min(len(zero["samples"]), MAX_TRIALS + 1)
    ref = composed(hip, host, frames)
    for g, r in zip(got, ref):
        _same_frame(g, r)
    alone = hip.PoseEstimator(max_frames=8, max_lines=200).run(good, max_trials=MAX_TRIALS)
    for g, a in zip([got[0], got[3]], alone):
        _same_frame(g, a, exact_pose=True)
        assert g["num_inliers"] == a["num_inliers"]
    est.close()


def test_reuse_and_growth(hip):
    sets = [make_frames(9700, [(150, 0.2, 1001)] * 6 + [(400, 0.3, 1001)] * 2),
            make_frames(9720, [(40, 0.3, 500), (150, 0.1, 1001)]),
            make_frames(9740, [(400, 0.2, 800)] * 3 + [(5, 0.1, 100)]),
            make_frames(9760, [(150, 0.4, 1001)] * 5)]
    est = hip.PoseEstimator(max_frames=8, max_lines=400)
    runs = [est.run(sets[0], max_trials=MAX_TRIALS)]
    st1 = est.stats()
    runs += [est.run(s, max_trials=MAX_TRIALS) for s in sets[1:]]
    st = est.stats()
    assert st["allocations"] == st1["allocations"] and st["refills"] == 4, (st1, st)
    assert st["finalizes"] == 1 and st["calls"] == 4
    runs.append(est.run(sets[0], max_trials=MAX_TRIALS))
    st2 = est.stats()
    assert st2["allocations"] == st["allocations"] and st2["finalizes"] == 1, (st, st2)
    for s, r in zip(sets + [sets[0]], runs):
        fresh = hip.PoseEstimator(max_frames=8, max_lines=400).run(s, max_trials=MAX_TRIALS)
        for g, f in zip(r, fresh):
            _same_frame(g, f, exact_pose=True)
            assert np.array_equal(g["mask"], f["mask"])
    # beyond capacity: more frames and more lines than the estimator was made for
    big = make_frames(9800, [(500, 0.2, 1001)] * 3 + [(150, 0.2, 1001)] * 8)
    got = est.run(big, max_trials=MAX_TRIALS)
    assert est.stats()["finalizes"] == 2
    fresh = hip.PoseEstimator(max_frames=11, max_lines=500).run(big, max_trials=MAX_TRIALS)
    for g, f in zip(got, fresh):
        _same_frame(g, f, exact_pose=True)
    est.close()


def test_validation_leaves_outputs_untouched(hip):
    import ctypes as C
    frames = make_frames(9900, [(40, 0.2, 50), (40, 0.2, 50)])
    frames[1] = dict(frames[1], samples=frames[1]["samples"].copy())
    frames[1]["samples"][3, 2] = 40                                  # out of range
    est = hip.PoseEstimator(max_frames=2, max_lines=64)
    with pytest.raises(hip.SlslamError) as ei:
        est.run(frames)
    assert ei.value.status == 1
    # raw call: a NULL lines pointer, outputs keep their sentinel
    L = hip.lib()
    tr0, keep = hip._trials(frames[0]["obs0"], frames[0]["obs1"], frames[0]["samples"])
    trs = (hip.RansacTrials * 1)(tr0)
    lns = (C.POINTER(C.c_double) * 1)()
    out = (hip.PoseEstimate * 1)()
    out[0].status = 77; out[0].trial_cnt = 77
    assert L.slslam_pose_estimator_run(est._h, 1, trs, lns, 0.12, 5.0 / 406.05, 0.999, 1000, out) == 1
    assert out[0].status == 77 and out[0].trial_cnt == 77
    est.close()


def test_device_conversions(hip, host):
    frames = make_frames(9950, [(150, 0.2, 1001), (400, 0.3, 1001)])
    est = hip.PoseEstimator(max_frames=2, max_lines=400)
    got = est.run(frames, max_trials=MAX_TRIALS)
    for f, (fr, g) in enumerate(zip(frames, got)):
        assert g["status"] == "OK"
        w = est.window(f)
        wt = np.zeros(6)
        host.slslam_gc_Rt_to_wt(C.byref(_pose(g["ransac_pose"])), _dp(wt))
        assert np.abs(w["parameters"][:6] - wt).max() < 1e-14
        assert np.array_equal(w["parameters"][6:12], np.zeros(6))
        ln = fr["lines"][g["ransac_mask"]]
        for i, l in enumerate(ln):
            o = np.zeros(4)
            host.slslam_gc_av_to_orth(_dp(np.ascontiguousarray(l)), _dp(o))
            assert np.abs(w["parameters"][12 + 4 * i:16 + 4 * i] - o).max() < 1e-14
        assert np.array_equal(w["observations"][0::2], fr["obs1"][g["ransac_mask"]])
        assert np.array_equal(w["observations"][1::2], fr["obs0"][g["ransac_mask"]])
        n = len(ln)
        words = w["index_words"].astype(np.int64)
        assert np.array_equal(words & 0xffff, np.repeat(np.arange(n), 2))
        assert np.array_equal((words >> 16) & 0xff, np.tile([0, 1], n))
        assert np.abs(wt_to_Rt(host, w["solved_camera"]) - g["pose"]).max() < 1e-14

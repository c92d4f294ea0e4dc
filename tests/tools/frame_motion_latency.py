"""Developer tool: SLAM::pose_estimation (RANSAC, motion-only BA on its inliers, final inliers) for F frames of K = 150 common lines and
1001 pre-drawn trials - the chain of the existing entry points (slslam_ransac_motion_batch, a refilled fused motion-only batch of the
host-packed windows, one slslam_ransac_score per frame) against one slslam_pose_estimator_run call.  Prints one line per F and a JSON
summary."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from slslam_amd import capi, synth  # noqa: E402

HOST = C.CDLL(os.path.join(os.getcwd(), "slslam_amd", "_lib", "libslslam_host.so"))


class Pose(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class Packed(C.Structure):
    _fields_ = [("num_cameras", C.c_int), ("num_lines", C.c_int), ("num_observations", C.c_int), ("num_parameters", C.c_int),
                ("camera_index", C.POINTER(C.c_int)), ("line_index", C.POINTER(C.c_int)), ("fixed_index", C.POINTER(C.c_int)),
                ("observations", C.POINTER(C.c_double)), ("parameters", C.POINTER(C.c_double)),
                ("camera_kf_id", C.POINTER(C.c_int)), ("line_lm_id", C.POINTER(C.c_int))]


dp = C.POINTER(C.c_double)
HOST.slslam_pack_motion_only.argtypes = [C.POINTER(Pose), dp, dp, dp, C.c_int, C.POINTER(Packed)]
HOST.slslam_free_packed_window.argtypes = [C.POINTER(Packed)]
HOST.slslam_free_packed_window.restype = None
HOST.slslam_gc_wt_to_Rt.argtypes = [dp, C.POINTER(Pose)]


def pack(T, o1, o0, ln):
    """slslam_pack_motion_only (the host packer) -> window dict"""
    p = Pose()
    p.R[:] = list(T[:9]); p.t[:] = list(T[9:])
    o1, o0, ln = (np.ascontiguousarray(a) for a in (o1, o0, ln))
    pw = Packed()
    HOST.slslam_pack_motion_only(C.byref(p), capi._dp(o1), capi._dp(o0), capi._dp(ln), len(ln), C.byref(pw))
    M = pw.num_observations
    w = {"num_cameras": 2, "num_lines": pw.num_lines, "num_observations": M,
         "camera_index": np.ctypeslib.as_array(pw.camera_index, (M,)).copy(), "line_index": np.ctypeslib.as_array(pw.line_index, (M,)).copy(),
         "fixed_index": np.ctypeslib.as_array(pw.fixed_index, (2 * M,)).copy(),
         "observations": np.ctypeslib.as_array(pw.observations, (8 * M,)).copy(),
         "parameters": np.ctypeslib.as_array(pw.parameters, (pw.num_parameters,)).copy()}
    HOST.slslam_free_packed_window(C.byref(pw))
    return w


def composed(frames, batch):
    """pose_estimation of every frame through the existing entry points; batch = [LBABatch or None], refilled in place when it can be"""
    rs = capi.ransac_motion_batch(frames, max_trials=1000, best_score=-1)
    wins = [pack(pose, fr["obs1"][m], fr["obs0"][m], fr["lines"][m]) for fr, (tc, bs, pose, m) in zip(frames, rs)]
    b = batch[0]
    try:
        if b is None:
            raise capi.SlslamError(4, "no batch yet")
        b.refill(wins)
    except capi.SlslamError:
        if b is not None:
            b.close()
        b = capi.LBABatch()
        for w in wins:
            b.add(w)
        b.finalize(refill_headroom_percent=25)
        batch[0] = b
    b.solve()
    b.download()
    out = []
    for i, fr in enumerate(frames):
        x = np.ascontiguousarray(b.parameters(i)[:6])
        p = Pose()
        HOST.slslam_gc_wt_to_Rt(capi._dp(x), C.byref(p))
        out.append(capi.ransac_score(np.array(list(p.R) + list(p.t)), fr["obs1"], fr["lines"]))
    return out


def main():
    res = {}
    for F in (1, 256):
        frames = [synth.make_ransac_pair(40000 + i, num_lines=150, outlier_frac=0.2, num_trials=1001) for i in range(F)]
        reps = 20 if F == 1 else 5
        batch = [None]
        composed(frames, batch)                     # warm: the batch is built, its solve captured
        t = time.perf_counter()
        for _ in range(reps):
            composed(frames, batch)
        tc = (time.perf_counter() - t) / reps * 1e3
        est = capi.PoseEstimator(max_frames=F, max_lines=150)
        est.run(frames)                             # warm: buffers, batch, capture
        t = time.perf_counter()
        for _ in range(reps):
            got = est.run(frames)
        te = (time.perf_counter() - t) / reps * 1e3
        ok = sum(g["status"] == "OK" for g in got)
        print("F = %3d (K = 150, 1001 trials, %d solved): composed %.3f ms per call (%.3f per frame), estimator %.3f ms per call (%.3f per frame)"
              % (F, ok, tc, tc / F, te, te / F), flush=True)
        res["F%d" % F] = {"composed_ms": round(tc, 3), "estimator_ms": round(te, 3), "stats": est.stats()}
        est.close()
        batch[0].close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

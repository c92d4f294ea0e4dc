"""Developer tool: what the covariance of the estimated motion costs.  PoseEstimator.run with covariance off and on for F = 1 and
F = 256 frames of K = 150 common lines and 1001 pre-drawn trials (the frames of frame_motion_latency.py), and po_constraint_covariance
for n = 1 and n = 4096 items.  With SLSLAM_HIP_LIBRARY naming a library built before the covariance existed (the parent commit: the
yardstick) only the run without it is timed.  The "on" time includes the Python binding's one get_covariance call per solved frame.
Prints one line per case (median and fastest of the repetitions, after a warm-up call) and a JSON summary."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from slslam_amd import capi, synth  # noqa: E402


def timed(fn, reps):
    fn()                                            # warm: buffers, batch, capture
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts))


def main():
    has_cov = hasattr(capi.lib(), "slslam_pose_estimator_set_covariance")
    res = {"library": os.environ.get("SLSLAM_HIP_LIBRARY") or "in-tree", "covariance": has_cov}
    for F in (1, 256):
        frames = [synth.make_ransac_pair(40000 + i, num_lines=150, outlier_frac=0.2, num_trials=1001) for i in range(F)]
        reps = 30 if F == 1 else 7
        row = {}
        for mode in (("off", "on") if has_cov else ("off",)):
            est = capi.PoseEstimator(max_frames=F, max_lines=150, **({"covariance": True} if mode == "on" else {}))
            got = []
            med, best = timed(lambda: got.append(est.run(frames)), reps)
            ok = sum(g["status"] == "OK" for g in got[-1])
            row[mode] = {"median_ms": round(med, 4), "min_ms": round(best, 4), "solved": ok, "stats": est.stats()}
            print("F = %3d (K = 150, 1001 trials, %d solved) covariance %-3s: %.3f ms per call median, %.3f fastest" % (F, ok, mode, med, best), flush=True)
            est.close()
        if has_cov:
            row["on_over_off"] = round(row["on"]["median_ms"] / row["off"]["median_ms"], 4)
            print("F = %3d: on / off = %.3f" % (F, row["on_over_off"]), flush=True)
        res["F%d" % F] = row
    if has_cov:
        import po_gate_reference as gref
        import pose_covariance_reference as pref
        for n in (1, 4096):
            it = gref.primitive_items(n)
            sig = pref.random_spd(n)
            med, best = timed(lambda: capi.po_constraint_covariance(it["pose_a"], it["pose_b"], it["constraints"], sig, 1.0), 30)
            print("po_constraint_covariance n = %4d: %.3f ms per call median, %.3f fastest" % (n, med, best), flush=True)
            res["constraint_n%d" % n] = {"median_ms": round(med, 4), "min_ms": round(best, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

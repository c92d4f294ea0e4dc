"""Time of slslam_line_matcher_run, with and without extents, beside the only way the same pairs could be scored before it existed: one
slslam_ransac_score call per frame with the frame's K x L pairs flattened into K L "common lines" under one hypothesis.

    python tools/line_match_bench.py [--frames 64] [--observations 512] [--lines 4096] [--repeats 15] [--baseline-frames 4]
                                     [--parent-lib slslam_amd/_lib/libslslam_hip.parent.so] [--out profiles/line_match_bench.txt]

Frames: tests/line_match_reference.make_frame (one synthetic stereo pair per frame, shuffled observations, a perturbed pose; extents = the
interval each line's own observation cuts out of it).  Warm (three untimed calls first), median and spread of `repeats` calls.  Two figures
per variant: HIP events on the null stream around the call - the call is synchronous on the matcher's own stream, so this is upload +
three launches + download as the device clock sees them - and the wall time of the call.  The baseline is timed in the same two ways on
--parent-lib (a build of the commit before the matcher; without the file the row is left out and says so), for --baseline-frames frames;
it yields one inlier bit per pair at one threshold, no errors, minima or matches, and repeating the observations and tiling the lines
on the host is not in its time.  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--observations", type=int, default=512)
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--baseline-frames", type=int, default=4)
    ap.add_argument("--distinct", type=int, default=4, help="distinct synthetic frames (the call repeats them)")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "slslam_amd", "_lib", "libslslam_hip.parent.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_match_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from slslam_amd import capi
    import line_match_reference as M
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    F, K, L = a.frames, a.observations, a.lines
    base = [M.make_frame(8800 + i, K, L, extents=True) for i in range(min(a.distinct, F))]
    with_ext = [base[i % len(base)] for i in range(F)]
    without = [{k: v for k, v in fr.items() if k != "extents"} for fr in with_ext]
    lines = ["line_match_bench: %d frames x %d observations x %d lines = %.3g pairs per call (%d distinct frames), error_thr 5 / 406.05, ratio 1.5, margin 0.05"
             % (F, K, L, float(F) * K * L, len(base))]

    def timed(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(); call(); e1.record()
            e1.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(e0.elapsed_time(e1))
        return ev, wall

    def row(name, ms, per):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ns per pair" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), 1e6 * statistics.median(ms) / per)

    # the matcher: the raw entry point on prepared arrays, so that the binding's conversions are not in the time
    m = capi.LineMatcher(max_frames=F, max_observations=K, max_lines=L)
    for name, frames in (("without extents", without), ("with extents", with_ext)):
        mfs, outs, keep = (capi.MatchFrame * F)(), (capi.MatchResult * F)(), []
        for i, fr in enumerate(frames):
            mfs[i], k = capi._match_frame(fr)
            outs[i], b = capi._match_buffers(K, L)
            keep += [k, b]

        def call():
            rc = capi.lib().slslam_line_matcher_run(m._h, F, mfs, 0.12, 5.0 / 406.05, 1.5, 0.05, outs)
            assert rc == 0, rc

        ev, wall = timed(call)
        lines.append(row("matcher %s, HIP events around the call" % name, ev, float(F) * K * L))
        lines.append(row("matcher %s, wall" % name, wall, float(F) * K * L))
        lines.append("  matched %d of %d observations; admissible pairs %d" % (
            sum(o.num_matched for o in outs), F * K, sum(int(keep[2 * i + 1]["num_admissible"].sum()) for i in range(F))))
    lines.append("matcher buffers: %s" % m.stats())
    m.close()

    # the baseline on the parent's library
    if os.path.exists(a.parent_lib) and a.baseline_frames > 0:
        P = C.CDLL(a.parent_lib)
        P.slslam_ransac_score.argtypes = [C.POINTER(capi.RansacFrame), C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        assert not hasattr(P, "slslam_match_lines"), "--parent-lib holds the matcher: not a build of the parent commit"
        fr = without[0]
        obs = np.ascontiguousarray(np.repeat(fr["observations"], L, axis=0))
        lns = np.ascontiguousarray(np.tile(fr["lines"], (K, 1)))
        pose = np.ascontiguousarray(fr["pose"])
        score = np.zeros(1, dtype=np.int32)
        bits = np.zeros((K * L + 63) // 64, dtype=np.uint64)
        rf = capi.RansacFrame(1, K * L, capi._dp(pose), capi._dp(obs), capi._dp(lns))

        def one():
            rc = P.slslam_ransac_score(C.byref(rf), 0.12, 5.0 / 406.05, capi._ip(score), bits.ctypes.data_as(C.POINTER(C.c_ulonglong)))
            assert rc == 0, rc

        rep, a.repeats = a.repeats, a.baseline_frames
        ev, wall = timed(one)
        a.repeats = rep
        lines.append(row("slslam_ransac_score of one frame's %d pairs (parent library), HIP events around the call" % (K * L), ev, float(K) * L))
        lines.append(row("slslam_ransac_score of one frame's %d pairs (parent library), wall" % (K * L), wall, float(K) * L))
        lines.append("  a loop over %d frames at the median: %.1f ms by events, %.1f ms wall (extrapolated from %d timed calls; inlier bits %d)" % (
            F, F * statistics.median(ev), F * statistics.median(wall), len(ev), int(score[0])))
    else:
        lines.append("baseline (a loop of slslam_ransac_score calls on the parent's library): not measured - %s is missing" % os.path.relpath(a.parent_lib, ROOT))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the register counts kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Resources of the matcher's kernels")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

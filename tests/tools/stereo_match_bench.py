"""Time of slslam_stereo_matcher_run beside the same pairs through the ungated descriptor matcher (slslam_descriptor_matcher_run: the
right image's descriptors as a stored keyframe) and beside the numpy contract (tests/stereo_match_reference.py) on one host thread.

    python tests/tools/stereo_match_bench.py [--segments 300] [--dim 72] [--frames 64] [--repeats 15] [--out profiles/stereo_match_bench.txt]

Frames: test_stereo_match_cpu.stereo_frame - segments of a 752 x 480 pair, 80 % of them seen by both images with disparities in
2 .. 100 px, the rest unrelated; unit descriptors; the default options (disparity 0 .. 128 px, max_tan2 0.03, min_rows 3, min_overlap
0.5, ratio 1.5, max_distance 0.25).  Shapes: 1 frame and `frames` frames per call.  Warm (three untimed calls first), one process,
median and spread of `repeats` calls.  Per shape the three launches by events on the matcher's stream (slslam_stereo_matcher_timing)
and the wall time of the call (host fill of the upload block, upload, launches, download, scatter).  The descriptor matcher's row is
the wall time of its run call alone (its keyframes are inserted before).  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=300)
    ap.add_argument("--dim", type=int, default=72)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_match_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")                # (the host row: one thread; set before numpy loads its BLAS)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    import numpy as np
    from slslam_amd import capi
    import stereo_match_reference as R
    import test_stereo_match_cpu as T
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    N, D, F = a.segments, a.dim, a.frames
    raw = [T.stereo_frame(7000 + i, N, N, D, common=(4 * N) // 5) for i in range(F)]
    frames = [((f[0], f[1]), (f[2], f[3])) for f in raw]
    o = R.options()
    geo = np.mean([R.gate(f[0], f[2], o)[0].mean() for f in raw[:8]])
    lines = ["stereo_match_bench: n = m = %d segments, D = %d, %d x %d pairs per frame; disparities drawn from 2 .. 100 px, gate 0 .. 128 px"
             % (N, D, N, N),
             "the gate removes %.2f %% of the pairs before a descriptor is read (mean of 8 frames)" % (100.0 * (1.0 - geo))]

    def stats(name, ms, per):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ms per frame" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), statistics.median(ms) / per)

    sm = capi.StereoMatcher(D, max_frames=F, max_segments=max(N, 1))
    sm.set_timing(True)
    dm = capi.DescriptorMatcher(D, max_keyframes=F, max_descriptors=max(N, 1), max_frames=F, max_candidates=1)
    for f in raw:
        dm.insert(f[3])
    matched = None
    for count in (1, F):
        batch = frames[:count]
        for _ in range(3):
            res = sm.run(batch)
        kern, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = sm.run(batch)
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(sm.kernel_ms())
        matched = sum(r["num_matched"] for r in res)
        lines.append("--- %d frame(s) per call, %d matches" % (count, matched))
        lines.append(stats("  stereo matcher, three launches by events", kern, count))
        lines.append(stats("  stereo matcher, the call (wall)", wall, count))
        queries = [(raw[i][1], [i]) for i in range(count)]
        for _ in range(3):
            dm.run(queries, ratio=o["ratio"], max_distance=o["max_distance"])
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            dm.run(queries, ratio=o["ratio"], max_distance=o["max_distance"])
            wall.append(1e3 * (time.perf_counter() - t0))
        lines.append(stats("  descriptor matcher without a gate, the call (wall)", wall, count))
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = R.match(*raw[0])
        host.append(1e3 * (time.perf_counter() - t0))
    got = sm.run(frames[:1])[0]
    assert got["match"].tolist() == want["match"].tolist()
    lines.append("--- the numpy contract, one host thread, one frame: median %.1f ms of %d calls" % (statistics.median(host), len(host)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

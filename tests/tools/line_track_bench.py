"""Time of slslam_line_tracker_run beside the numpy contract (tests/line_track_reference.py) on one host thread, with the stereo
matcher's kernel time at the same n, m, D as a yardstick (the same chains, another gate).

    python tests/tools/line_track_bench.py [--segments 300] [--dim 72] [--frames 512] [--repeats 9] [--out profiles/line_track_bench.txt]

The sequence: `frames` frames of `segments` segments of a 752 x 480 image with unit descriptors; from frame to frame the scene moves by
up to 5 px, every end point by a further 0.5 px (sigma), a tenth of the segments is replaced by unrelated ones and the rows are
shuffled; the default options.  First the whole sequence goes through the numpy contract and through the device cut into runs of 1,
64 and `frames` frames: any difference in id, age, match, status or a distance ends the program with a non-zero status before
anything is timed.  Then, warm, one process, median and spread: per run the launches by events on the tracker's stream
(slslam_line_tracker_timing) and the wall time of the call (host fill of the upload block, upload, launches, download, scatter), for
runs of 1 frame (the carried frame from the run before), of 64 and of `frames` frames.  A measurement, not a gate: needs a GPU and
fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_sequence(np, seed, T, N, D):
    rng = np.random.default_rng(seed)

    def segs(k):
        c = np.stack([rng.uniform(60, 690, k), rng.uniform(60, 420, k)], axis=1)
        a, h = rng.uniform(0, np.pi, k), rng.uniform(12, 45, k)
        d = np.stack([h * np.cos(a), h * np.sin(a)], axis=1)
        return np.concatenate([c - d, c + d], axis=1)

    def descs(k):
        v = rng.normal(size=(k, D))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    seg, desc, frames = segs(N), descs(N), []
    for _ in range(T):
        seg = seg + np.tile(rng.uniform(-5.0, 5.0, 2), 2) + rng.normal(0.0, 0.5, (N, 4))
        seg[:, 0::2] = np.clip(seg[:, 0::2], 5.0, 747.0)
        seg[:, 1::2] = np.clip(seg[:, 1::2], 5.0, 475.0)
        desc = desc + 0.05 * descs(N)
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        fresh = rng.permutation(N)[:N // 10]
        seg[fresh], desc[fresh] = segs(len(fresh)), descs(len(fresh))
        p = rng.permutation(N)
        seg, desc = seg[p], desc[p]
        frames.append((seg.astype(np.float32), desc.astype(np.float32)))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=300)
    ap.add_argument("--dim", type=int, default=72)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_track_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")                # (the host row: one thread; set before numpy loads its BLAS)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    import numpy as np
    from slslam_amd import capi
    import line_track_reference as R
    import test_stereo_match_cpu as TS
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    N, D, F = a.segments, a.dim, a.frames
    frames = make_sequence(np, 9000, F, N, D)
    t0 = time.perf_counter()
    want = R.track(frames)
    host_ms = 1e3 * (time.perf_counter() - t0) / F
    lt = capi.LineTracker(D, max_frames=F, max_segments=max(N, 1))
    shapes = sorted({1, min(64, F), F})
    keys = ("id", "age", "match", "best", "num_admissible", "best_row", "best_distance", "second_distance")
    for count in shapes:                                         # ---- the inputs against the reference, before any timing
        lt.reset(0)
        got = []
        for at in range(0, F, count):
            got += lt.run(frames[at:at + count])
        for t, (g, w) in enumerate(zip(got, want)):
            bad = [k for k in keys if g[k].tobytes() != w[k].tobytes()] + (["segment_status"] if g["segment_status"] != w["segment_status"] else [])
            if bad:
                raise SystemExit("runs of %d: frame %d differs from the numpy contract in %s" % (count, t, bad))
    cont, new = sum(w["num_continued"] for w in want), sum(w["num_new"] for w in want)
    lines = ["line_track_bench: %d frames of %d segments, D = %d; %d continued, %d new; equal to the numpy contract in runs of %s"
             % (F, N, D, cont, new, ", ".join(str(c) for c in shapes)),
             "the gate admits %.2f %% of the pairs (mean of frames 1 .. 8)"
             % (100.0 * np.mean([R.gate(frames[t][0], frames[t - 1][0], R.options()).mean() for t in range(1, min(9, F))]))]

    def stats(name, ms, per):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d runs) = %.4f ms per frame" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), statistics.median(ms) / per)

    lt.set_timing(True)
    for count in shapes:
        kern, wall = [], []
        runs = max(a.repeats, min(64, F // count))
        lt.reset(0)
        at = 0
        for rep in range(-3, runs):                              # (three untimed runs first)
            if at + count > F or count == F:                     # (the sequence is over: a new one)
                lt.reset(0)
                at = 0
            t0 = time.perf_counter()
            lt.run(frames[at:at + count])
            if rep >= 0:
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(lt.kernel_ms())
            at += count
        lines.append("--- %d frame(s) per run" % count)
        lines.append(stats("  line tracker, the launches by events", kern, count))
        lines.append(stats("  line tracker, the call (wall)", wall, count))
    lt.close()
    # ---- the yardstick: the stereo matcher's three launches at the same n, m, D
    raw = [TS.stereo_frame(7000 + i, N, N, D, common=(4 * N) // 5) for i in range(min(64, F))]
    pairs = [((f[0], f[1]), (f[2], f[3])) for f in raw]
    sm = capi.StereoMatcher(D, max_frames=len(pairs), max_segments=max(N, 1))
    sm.set_timing(True)
    for count in sorted({1, len(pairs)}):
        kern = []
        for rep in range(-3, a.repeats):
            sm.run(pairs[:count])
            if rep >= 0:
                kern.append(sm.kernel_ms())
        lines.append(stats("--- stereo matcher, %d frame(s) per call, three launches by events" % count, kern, count))
    sm.close()
    lines.append("--- the numpy contract, one host thread: %.1f ms per frame (one pass over the %d frames)" % (host_ms, F))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

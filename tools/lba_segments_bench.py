"""Time of slslam_lba_batch_segments on the bench batch, beside slslam_lba_batch_report on the same batch.

    python tools/lba_segments_bench.py [--windows 1024] [--lines 2000] [--repeats 15] [--max-range 5.0] [--out profiles/lba_segments_bench.txt]

The batch is bench.py's: window i = synth.make_window(i, num_lines=2000) (10 + 10 keyframes), default options, solved once so that the
segments are taken at the solved point.  Two figures per call, warm (three untimed calls first), median and spread of `repeats` calls:
the device time of the launches alone (HIP events on the null stream), and the wall time of call + download, which is what a caller
waits for - the download brings the parameters and summaries back as well, for both calls alike.  Segments do the report's sweep
without Jacobians or the 4 x 4 factor: the report is the sanity check.  Also printed: the statuses the bench batch gives, and - for the
first windows - the largest deviation from the numpy reference.  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--max-range", type=float, default=5.0)
    ap.add_argument("--check", type=int, default=2, help="windows compared with the numpy reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_segments_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from slslam_amd import capi, synth
    import lba_segments_reference as S
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    ws = [synth.make_window(i, num_lines=a.lines) for i in range(a.windows)]
    b = capi.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    b.solve(); b.download()
    M, L = sum(len(w["camera_index"]) for w in ws), a.windows * a.lines
    lines = ["lba_segments_bench: %d windows x %d lines, %d observations, %d cameras of which %d free, path %d, max_range %g" % (
        a.windows, a.lines, M, ws[0]["num_cameras"], ws[0]["num_free_cameras"], b.path(), a.max_range)]

    def device_ms(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def wall_ms(call):
        for _ in range(3):
            call(); b.download()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call(); b.download()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    def row(name, ms):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.2f us per window" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), 1e3 * statistics.median(ms) / a.windows)

    def segments():
        b.segments(a.max_range)

    lines.append(row("segments, device (1 launch)", device_ms(segments)))
    lines.append(row("report, device (2 launches)", device_ms(b.report)))
    b.download()
    lines.append(row("download alone", wall_ms(lambda: None)))
    lines.append(row("segments + download", wall_ms(segments)))
    lines.append(row("report + download", wall_ms(b.report)))
    read, written = 72 * M + 32 * L, 20 * M + 80 * L
    lines.append("byte model: %.1f MB read, %.1f MB written per call" % (read / 1e6, written / 1e6))
    lines.append("segments buffers: %s" % b.segments_stats())
    segments(); b.download()
    segs = [b.get_segments(i) for i in range(a.windows)]
    st = np.bincount(np.concatenate([s["obs_status"] for s in segs]), minlength=6)
    ln = np.bincount(np.concatenate([s["status"] for s in segs]), minlength=3)
    lines.append("observations USED %d, USED_CLAMPED %d, DEGENERATE %d, BEHIND %d, OUT_OF_RANGE %d, COLLAPSED %d; lines OK %d, NO_OBSERVATIONS %d, NONE %d" % (
        tuple(st[:6]) + tuple(ln[:3])))
    worst = 0.0
    for i in range(min(a.check, a.windows)):
        ref = S.segments(ws[i], b.parameters(i), a.max_range)
        assert all(np.array_equal(ref[k], segs[i][k]) for k in ("obs_status", "status", "num_observations", "num_used", "num_clamped"))
        for k in ("obs_range", "t_min", "t_max", "p_min", "p_max"):
            worst = max(worst, float((np.abs(ref[k] - segs[i][k]) / (1.0 + np.abs(ref[k]))).max()))
    lines.append("largest |d| / (1 + |.|) against the numpy reference over %d windows: %.3g (bound 1e-9); statuses and counts equal" % (min(a.check, a.windows), worst))
    b.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the register counts kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Resources of the segments' kernels")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

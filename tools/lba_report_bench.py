"""Device time of slslam_lba_batch_report on the bench batch, beside one elimination sweep and the covariance call of the same batch.

    python tools/lba_report_bench.py [--windows 1024] [--lines 2000] [--repeats 15] [--out profiles/lba_report_bench.txt]

The batch is bench.py's: window i = synth.make_window(i, num_lines=2000) (10 + 10 keyframes), default options, solved once so that the
report is taken at the solved point.  Times are HIP events on the null stream around the call's two launches, warm (three untimed calls
first), median and spread of `repeats` calls; the covariance call (cameras + lines) the same way.  The elimination sweep: the batch
solved once more with profiling on (eager launches, events around each; slslam_lba_batch_kernel_times), the `linearise_schur` family's time
per launch.  Also printed: how many windows the report names a degenerate line in (min_pivot <= 1e-10) beside the covariance's SINGULAR
count, and - for the first windows - the largest deviation of min_pivot from the numpy reference on the device's own Jacobians.
A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--check", type=int, default=2, help="windows compared with the numpy reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_report_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from slslam_amd import capi, synth
    import lba_covariance_reference as R
    import lba_report_reference as P
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    ws = [synth.make_window(i, num_lines=a.lines) for i in range(a.windows)]
    b = capi.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    b.solve(); b.download()
    lines = ["lba_report_bench: %d windows x %d lines, %d cameras of which %d free, path %d, sweep %d" % (
        a.windows, a.lines, ws[0]["num_cameras"], ws[0]["num_free_cameras"], b.path(), b.elimination())]

    def timed(call):
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

    for name, call in (("report (2 launches)", b.report), ("covariance, cameras + lines (1 launch)", b.covariance)):
        ms = timed(call)
        lines.append("%s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.2f us per window" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), 1e3 * statistics.median(ms) / a.windows))
    lines.append("report buffers: %s" % b.report_stats())
    b.report(); b.covariance(); b.download()
    reps = [b.get_report(i) for i in range(a.windows)]
    named = [int(((r["lines"]["status"] == 0) & (r["lines"]["min_pivot"] <= R.PIVOT_MIN)).any()) for r in reps]
    singular = [b.get_covariance(i)[0] for i in range(a.windows)]
    lines.append("windows with a line of min_pivot <= 1e-10: %d; covariance SINGULAR: %d; the same windows: %s" % (
        sum(named), sum(singular), named == singular))
    worst = 0.0
    for i in range(min(a.check, a.windows)):
        jl = b.linearise(i, len(ws[i]["camera_index"]))[3]
        own = P.report(ws[i], b.parameters(i), R.HUBER, jl=jl, sq_norm=reps[i]["sq_norm"])["lines"]["min_pivot"]
        worst = max(worst, float(np.abs(own - reps[i]["lines"]["min_pivot"]).max()))
    lines.append("largest |min_pivot - reference on the device's own Jacobians| over %d windows: %.3g (bound 1e-12)" % (min(a.check, a.windows), worst))
    b.set_profiling(True)
    b.reset(); b.solve(); b.download()
    kt = b.kernel_times()
    b.set_profiling(False)
    b.close()
    lin = kt["linearise_schur"]
    lines.append("elimination sweep of the same batch: %.3f ms per launch (%.3f ms over %d launches)" % (lin[0] / max(1, lin[1]), lin[0], lin[1]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the register counts and accuracy figures kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Resources of the report's kernels")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

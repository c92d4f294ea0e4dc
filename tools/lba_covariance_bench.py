"""Device time of slslam_lba_batch_covariance on the bench batch, beside one LM iteration of the same batch and the numpy reference.

    python tools/lba_covariance_bench.py [--windows 1024] [--lines 2000] [--repeats 15] [--out profiles/lba_covariance_bench.txt]

The batch is bench.py's: window i = synth.make_window(i, num_lines=2000) (10 + 10 keyframes), default options, solved once so that the
covariance is taken at the solved point.  Times are HIP events on the null stream around the one launch, warm (three untimed calls
first), median and spread of `repeats` calls, with and without the lines' blocks.  The LM iteration: the batch solved once more with
profiling on (eager launches, events around each; slslam_lba_batch_kernel_times), all families summed, divided by the number of
lock-step iterations (launches of the LM update).  The numpy figure is the Schur route of tests/lba_covariance_reference.py on
window 0 from the oracle's Jacobians (the dense QR route would need a 80 000 x 8 060 matrix).  A measurement, not a gate: needs a GPU
and fails without one."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_covariance_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from slslam_amd import capi, synth
    import lba_covariance_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    ws = [synth.make_window(i, num_lines=a.lines) for i in range(a.windows)]
    b = capi.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    b.solve(); b.download()
    lines = ["lba_covariance_bench: %d windows x %d lines, %d cameras of which %d free, path %d, sweep %d" % (
        a.windows, a.lines, ws[0]["num_cameras"], ws[0]["num_free_cameras"], b.path(), b.elimination())]

    def timed(with_lines):
        for _ in range(3):
            b.covariance(with_lines=with_lines)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); b.covariance(with_lines=with_lines); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    for with_lines in (True, False):
        ms = timed(with_lines)
        lines.append("covariance, %s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.2f us per window" % (
            "cameras + lines" if with_lines else "cameras only  ", statistics.median(ms), min(ms), max(ms), len(ms),
            1e3 * statistics.median(ms) / a.windows))
    b.covariance(); b.download()
    status = [b.get_covariance(i)[0] for i in range(a.windows)]
    lines.append("status: %d OK, %d SINGULAR" % (status.count(0), status.count(1)))
    b.set_profiling(True)
    b.reset(); b.solve(); b.download()
    kt = b.kernel_times()
    total = sum(v[0] for v in kt.values())
    its = max(1, kt["lm_update"][1])
    lines.append("one LM iteration of the same batch: %.3f ms (%.3f ms over %d lock-step iterations: %s)" % (
        total / its, total, its, ", ".join("%s %.3f" % (k, v[0]) for k, v in kt.items() if v[1])))
    b.set_profiling(False)
    st, free, cc, cl = b.get_covariance(0)
    x = b.parameters(0)
    b.close()
    jc, jl = R.oracle_jacobians(ws[0], x, R.HUBER)
    t0 = time.perf_counter()
    sc, sl, piv_s, piv_l = R.cov_schur(ws[0], jc, jl)
    t1 = time.perf_counter()
    lines.append("numpy reference (Schur route, one window, Jacobians given): %.1f ms; smallest pivots S %.3g, lines %.3g" % (1e3 * (t1 - t0), piv_s, piv_l))
    lines.append("window 0 against it: cameras %.3g, lines %.3g (relative, tests/lba_covariance_reference.py rel_cameras / rel_lines)" % (
        R.rel_cameras(cc, sc), R.rel_lines(cl, sl)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the accuracy figures and register counts kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Accuracy of slslam_lba_batch_covariance")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

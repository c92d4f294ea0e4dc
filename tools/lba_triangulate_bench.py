#!/usr/bin/env python3
"""Throughput of the line triangulator (capi.LineTriangulator) on the bench population: 1024 windows x 2000 lines.  Writes what the
device gives; nothing is asserted.

  python tools/lba_triangulate_bench.py [--windows 1024] [--lines 2000] [--distinct 1024] [--reps 5] [--out profiles/lba_triangulate_bench.txt]

The parent runs every step as a child process of its own under its own time limit and stops at the first one that fails:
  device   methods 0 and 1: per-call time of slslam_line_triangulator_run, lines / s, and the split of the last call into host layout,
           upload, kernel, download and result scatter (slslam_line_triangulator_timing);
  oracle   the numpy reference loop (tests/lba_triangulate_reference.py) on one host thread over a subset of one window, scaled.
The population is --distinct different windows (synth.make_window, seeds 0 ..), repeated to --windows when that is smaller.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _population(a):
    from slslam_amd import synth
    base = [synth.make_window(i, num_lines=a.lines, line_init="triangulate") for i in range(min(a.distinct, a.windows))]
    return [base[i % len(base)] for i in range(a.windows)]


def step_device(a):
    from slslam_amd import capi
    ws = _population(a)
    L = sum(int(w["num_lines"]) for w in ws)
    M = sum(len(w["camera_index"]) for w in ws)
    print("line triangulator, %d windows x %d lines (%d distinct): %d lines, %d observations" % (a.windows, a.lines, min(a.distinct, a.windows), L, M))
    tr = capi.LineTriangulator(L, M + M // 2)
    arrs = [capi._WindowArrays(w) for w in ws]
    cw = (capi.LBAWindow * len(arrs))(*[x.c for x in arrs])
    res = [np.zeros(int(w["num_lines"]), dtype=np.dtype(capi.TriangulatedLine)) for w in ws]
    rp = (C.POINTER(capi.TriangulatedLine) * len(ws))(*[r.ctypes.data_as(C.POINTER(capi.TriangulatedLine)) for r in res])
    for method in (0, 1):
        times = []
        for rep in range(a.reps + 1):                         # the first call allocates
            t0 = time.perf_counter()
            capi._check(capi.lib().slslam_line_triangulator_run(tr.h, len(arrs), cw, method, 0.1, 0.0, rp, None), "slslam_line_triangulator_run")
            times.append(time.perf_counter() - t0)
        best, tm = min(times[1:]), tr.timing()
        made = sum(int((r["status"] <= capi.TRI_STEREO).sum()) for r in res)
        print("method %d: slslam_line_triangulator_run best of %d  %.2f ms, median %.2f ms (first call, allocating: %.2f ms);  %.3e lines / s"
              % (method, a.reps, 1e3 * best, 1e3 * float(np.median(times[1:])), 1e3 * times[0], made / best))
        print("method %d: last call: host layout %.2f ms, upload %.2f ms, kernel %.2f ms, download %.2f ms, scatter %.2f ms"
              % (method, tm["layout"], tm["upload"], tm["kernel"], tm["download"], tm["scatter"]))
        st = np.bincount(np.concatenate([r["status"] for r in res]), minlength=5)
        print("method %d: lines " % method + ", ".join("%s %d" % (capi.TRI_STATUS[k], int(st[k])) for k in range(5) if st[k])
              + "; clamped %d" % sum(int(r["clamped"].sum()) for r in res))
    s = tr.stats()
    print("calls %d, buffer allocations %d (all in the first call)" % (s["calls"], s["allocations"]))
    tr.close()


def step_oracle(a):
    import lba_triangulate_reference as T
    from slslam_amd import synth
    w = synth.make_window(0, num_lines=a.lines, line_init="triangulate")
    n = min(a.oracle_lines, int(w["num_lines"]))
    keep = np.asarray(w["line_index"]) < n
    v = dict(w, num_lines=n, camera_index=np.asarray(w["camera_index"])[keep], line_index=np.asarray(w["line_index"])[keep],
             fixed_index=np.asarray(w["fixed_index"]).reshape(-1, 2)[keep].reshape(-1), observations=w["observations"][keep],
             parameters=w["parameters"][:6 * w["num_cameras"] + 4 * n])
    for method in (0, 1):
        t0 = time.perf_counter()
        T.reference(v, method=method, yardstick=False)
        t = (time.perf_counter() - t0) / n
        print("method %d: numpy reference loop, one host thread: %.3f ms per line over %d lines -> %.1f s for %d lines"
              % (method, 1e3 * t, n, t * a.windows * a.lines, a.windows * a.lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-lines", type=int, default=200)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", choices=["device", "oracle"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_triangulate_bench.txt"))
    a = ap.parse_args()
    if a.step:
        return {"device": step_device, "oracle": step_oracle}[a.step](a)
    out = []
    for step in ("device", "oracle"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step] + \
            [x for k in ("windows", "lines", "distinct", "reps", "oracle_lines") for x in ("--" + k.replace("_", "-"), str(getattr(a, k)))]
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        out.append(r.stdout)
        if r.returncode:
            print(r.stderr[-2000:])
            print("step %s ended with status %d: stopping" % (step, r.returncode))
            return r.returncode
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)

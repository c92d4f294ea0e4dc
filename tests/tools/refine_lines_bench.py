"""Throughput of the structure-only refinement (capi.LineRefiner) on the bench population: 1024 windows x 2000 lines
(synth.make_window defaults).  Writes what the device gives; nothing is asserted.

  python tests/tools/refine_lines_bench.py [--windows 1024] [--lines 2000] [--reps 5] [--out profiles/lba_refine_lines_bench.txt]

Reports: ms per run and lines / s; the same work through (a) the per-line oracle loop on one host thread (a subset, scaled) and
(b) capi.LBABatch on the same windows with every camera flagged constant, if the general path takes them; bytes / s from the byte
model (M 72 + L 32 per pass over the observations) against 8 TB/s; LM iterations, initial and final cost of the ordinary window solve
with and without a preceding refinement on 32 of the windows.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_lines_reference as R  # noqa: E402
from slslam_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=1024)
    ap.add_argument("--lines", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-lines", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lba_refine_lines_bench.txt"))
    a = ap.parse_args()
    out = []

    def say(s):
        print(s, flush=True)
        out.append(s)

    ws = [synth.make_window(i, num_lines=a.lines) for i in range(a.windows)]
    L = sum(int(w["num_lines"]) for w in ws)
    M = sum(len(w["camera_index"]) for w in ws)
    say("structure-only refinement, %d windows x %d lines: %d lines, %d observations, default options" % (a.windows, a.lines, L, M))

    rf = capi.LineRefiner(L, 2 * M)
    xs, rs, ts = rf.run(ws)                                   # warm-up: allocates
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        xs, rs, ts = rf.run(ws)
        times.append(time.perf_counter() - t0)
    # the Python binding copies every window's arrays per run; time the C call alone as well
    import ctypes as C
    arrs = [capi._WindowArrays(w) for w in ws]
    cw = (capi.LBAWindow * len(arrs))(*[x.c for x in arrs])
    starts = [x.params.copy() for x in arrs]
    ctimes = []
    for _ in range(a.reps):
        for x, s in zip(arrs, starts):
            x.params[:] = s
        t0 = time.perf_counter()
        capi._check(capi.lib().slslam_line_refiner_run(rf.h, len(arrs), cw, None, None), "slslam_line_refiner_run")
        ctimes.append(time.perf_counter() - t0)
    st = rf.stats()
    rf.close()
    ms = 1e3 * min(ctimes)
    steps = sum(int(r["num_successful_steps"].sum() + r["num_unsuccessful_steps"].sum()) for r in rs)
    accepted = sum(int(r["num_successful_steps"].sum()) for r in rs)
    refined = sum(int((r["status"] == capi.LINE_REFINED).sum()) for r in rs)
    say("slslam_line_refiner_run (host layout + upload + one launch + download): best of %d  %.2f ms, median %.2f ms;  %.3e lines / s"
        % (a.reps, ms, 1e3 * float(np.median(ctimes)), refined / min(ctimes)))
    say("through capi.LineRefiner.run (adds the binding's per-window array copies): best %.2f ms" % (1e3 * min(times)))
    say("lines refined %d, LM steps %d (%.2f per line), accepted %d; calls %d, buffer allocations %d (all in the first run)"
        % (refined, steps, steps / max(refined, 1), accepted, st["calls"], st["allocations"]))
    term = np.bincount(np.concatenate([r["termination_type"][r["status"] == 0] for r in rs]), minlength=6)
    say("terminations: " + ", ".join("%s %d" % (capi.TERMINATION[k], int(term[k])) for k in range(6) if term[k]))
    say("cost: initial %.6e -> final %.6e (sum over the windows)" % (sum(t["initial_cost"] for t in ts), sum(t["final_cost"] for t in ts)))
    # byte model: every LM step is one pass for the candidate cost, every accepted step (and the first evaluation) one more to linearise
    passes_per_line = (steps + accepted + refined) / max(refined, 1)
    model_bytes = passes_per_line * (M * 72.0 + L * 32.0)
    say("byte model (M 72 + L 32 per pass, %.2f passes per line): %.3e bytes per run -> %.3e bytes / s = %.2f %% of 8 TB/s (whole call, host work included)"
        % (passes_per_line, model_bytes, model_bytes / min(ctimes), 100.0 * model_bytes / min(ctimes) / 8e12))

    # (a) the per-line oracle loop on one host thread, a subset scaled to the whole
    w0 = ws[0]
    n = min(a.oracle_lines, int(w0["num_lines"]))
    t0 = time.perf_counter()
    for l in range(n):
        R.solve_line(w0, l)
    t_or = (time.perf_counter() - t0) / n
    say("(a) per-line oracle loop, one host thread: %.3f ms per line over %d lines (window extraction included) -> %.1f s for %d lines; %.0f x the device call"
        % (1e3 * t_or, n, t_or * L, L, t_or * L / min(ctimes)))

    # (b) the general path on the same windows with every camera flagged constant
    try:
        b = capi.LBABatch()
        for w in ws:
            b.add(R.all_cameras_constant(w))
        b.finalize()
        t0 = time.perf_counter()
        b.solve(); b.download()
        t_first = time.perf_counter() - t0
        b.reset()
        t0 = time.perf_counter()
        b.solve(); b.download()
        t_b = time.perf_counter() - t0
        fin = sum(b.summary(i)["final_cost"] for i in range(len(ws)))
        say("(b) capi.LBABatch, every camera constant (one trust region per window): solve + download %.2f ms (first %.2f ms), path %d, final cost %.6e"
            % (1e3 * t_b, 1e3 * t_first, b.path(), fin))
        b.close()
    except capi.SlslamError as e:
        say("(b) capi.LBABatch does not take windows whose cameras are all constant: %s" % e)

    # the ordinary window solve with and without a preceding refinement, 32 windows
    picks = sorted(set(int(round(x)) for x in np.linspace(0, len(ws) - 1, 32)))
    for label, start in (("without", [None] * len(picks)), ("with   ", [xs[i] for i in picks])):
        b = capi.LBABatch()
        for i, p in zip(picks, start):
            b.add(ws[i], p)
        b.finalize()
        b.solve(); b.download()
        ss = [b.summary(k) for k in range(len(picks))]
        its = [s["num_successful_steps"] + s["num_unsuccessful_steps"] for s in ss]
        say("window solve %s refinement, %d windows: LM iterations mean %.2f (min %d, max %d), initial cost mean %.6e, final cost mean %.6e"
            % (label, len(picks), float(np.mean(its)), min(its), max(its), float(np.mean([s["initial_cost"] for s in ss])),
               float(np.mean([s["final_cost"] for s in ss]))))
        b.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time and accuracy of the pose-graph covariances (slslam_po_covariance, slslam_po_batch_covariance) on the 260-pose / 8-loop graph.
   python tools/po_covariance_bench.py [--out profiles/po_covariance_bench.txt] [--reps 15]
HIP events on the default stream, warm, median of --reps (>= 10) with min and max: the one-graph call (uploads and download included),
the batch call at G = 1, 16, 64, beside one batched solve of the same graphs and numpy.linalg.inv of the same H on the host.  Matrix-core
utilisation = (2/3) n^3 flops per graph / time / 78.6 TF (fp64 MFMA peak).  Also the accuracy ratios d / y of tests/test_gpu_po_covariance.py's
graphs (d: device against the numpy reference, y: the reference's own yardstick).  Not bench.py: nothing here is a pass / fail figure."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from slslam_amd import capi, synth  # noqa: E402
import po_covariance_reference as cref  # noqa: E402

PEAK = 78.6e12


class Events:
    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.rt.hipEventCreate(C.byref(self.a)) == 0 and self.rt.hipEventCreate(C.byref(self.b)) == 0

    def time(self, fn):
        assert self.rt.hipEventRecord(self.a, None) == 0
        fn()
        assert self.rt.hipEventRecord(self.b, None) == 0 and self.rt.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.rt.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def stats(samples):
    s = sorted(samples)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "po_covariance_bench.txt"))
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    reps = max(a.reps, 10)
    ev = Events()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from oracle import pyoracle
    say("# pose-graph covariances: accuracy (d / y per graph, seed 7, at the oracle's solved poses)")
    worst = 0.0
    for shape in [(4, 1), (12, 2), (24, 3), (33, 2), (60, 4)]:
        g = synth.make_pose_graph(7, *shape)
        x, _, _ = pyoracle.po_solve(g, linear_solver=2)
        N = shape[0]
        pairs = [(int(p), int(q)) for p, q in zip(g["pose_index_1"], g["pose_index_2"]) if q - p > 1] + [(1, N - 1), (2, 2), (0, N - 1)]
        for delta in (0.0, 0.001):
            ref = cref.covariance(g, x, delta)
            cp0, cq0 = cref.blocks(ref, N, pairs)
            st, cp, cq = capi.po_covariance(g, pairs, delta, params=x)
            d = max(np.abs(cp - cp0).max(), np.abs(cq - cq0).max()) / np.abs(ref["sigma"]).max()
            worst = max(worst, d / ref["y"])
            say("N %3d loops %d delta %-5g n %3d  pivot %.3e  y %.3e  d %.3e  d/y %6.3f  status %d" % (N, shape[1], delta, ref["n"], ref["pivot"], ref["y"], d, d / ref["y"], st))
    say("worst d / y %.3f" % worst)

    say()
    say("# time: 260 poses / 8 loops (n = 1554), ms: median  min  max over %d warm repetitions" % reps)
    g = synth.make_pose_graph(7, 260, 8)
    x, _, _ = capi.po_solve(g)
    N = 260
    pairs = [(int(p), int(q)) for p, q in zip(g["pose_index_1"], g["pose_index_2"]) if q - p > 1] + [(1, N - 1)]
    n = 6 * (N - 1)
    flops = (2.0 / 3.0) * n ** 3
    J = cref.jacobian(g, x, 0.0)
    H = J.T @ J
    t = []
    for _ in range(5):
        t0 = time.perf_counter(); np.linalg.inv(H); t.append(1e3 * (time.perf_counter() - t0))
    say("numpy.linalg.inv(H) on the host        %9.3f %9.3f %9.3f" % stats(t))
    capi.po_covariance(g, pairs, 0.0, params=x)
    t = [ev.time(lambda: capi.po_covariance(g, pairs, 0.0, params=x)) for _ in range(reps)]
    med = stats(t)
    say("slslam_po_covariance (one graph)       %9.3f %9.3f %9.3f   matrix-core utilisation %.2f%%" % (med + (100 * flops / (1e-3 * med[0]) / PEAK,)))
    for G in (1, 16, 64):
        b = capi.POBatch()
        for k in range(G):
            b.add(synth.make_pose_graph(7 if k == 0 else 100 + k, 260, 8))
            b.set_covariance_pairs(k, pairs)
        b.finalize()
        b.solve(); b.download()
        ts = []
        for _ in range(3):
            b.reset(); ts.append(ev.time(b.solve))
        b.download()
        b.covariance(); b.download()
        t = [ev.time(b.covariance) for _ in range(reps)]
        b.download()
        st = [b.get_covariance(k)[0] for k in range(G)]
        med = stats(t)
        say("batch G = %2d: covariance               %9.3f %9.3f %9.3f   per graph %.3f ms, utilisation %.2f%%; one solve of the batch %.3f ms; statuses %s; %s" % (
            (G,) + med + (med[0] / G, 100 * G * flops / (1e-3 * med[0]) / PEAK, stats(ts)[0], sorted(set(st)), b.covariance_stats())))
        b.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

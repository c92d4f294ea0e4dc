"""Pose-graph batch vs a loop of one-shot solves (slslam_po_batch_* vs slslam_po_solve), BASELINE config-5 graphs: 260 poses,
8 loop closures, seeds 100, 101, ...  For each G it reports, median and spread (min .. max) over the repeats, per graph:
  end-to-end  create + add + finalize + solve + download (+ destroy)
  resident    reset + solve + download of a finalized batch, after one warm-up
  loop        capi.po_solve over the same G graphs, one after the other
Every timed section ends in a synchronise (download / po_solve), so the host clock covers the device work.
    python tools/po_batch_bench.py [--sizes 1,16,64,256] [--repeats 10] [--loop-only] [--profile-one G]
--loop-only runs the loop alone (for a library built from another commit: SLSLAM_HIP_LIBRARY); --profile-one G finalizes one batch
of G graphs and solves it once (for rocprofv3 --kernel-trace --stats)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slslam_amd import capi, synth  # noqa: E402


def graphs(G):
    return [synth.make_pose_graph(s, num_poses=260, num_loops=8) for s in range(100, 100 + G)]


def clock(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def fmt(name, ms, G):
    per = ms / G
    return "%-11s %9.3f ms/graph  (min %.3f max %.3f; whole call median %.2f ms)" % (name, np.median(per), per.min(), per.max(), np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--profile-one", type=int, default=0)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("no HIP device")
    if a.profile_one:
        gs = graphs(a.profile_one)
        b = capi.POBatch()
        for g in gs:
            b.add(g)
        b.finalize()
        b.solve(); b.download()
        steps = [b.summary(i)["num_successful_steps"] + b.summary(i)["num_unsuccessful_steps"] for i in range(len(gs))]
        print("profiled one G = %d solve: steps per graph min %d max %d" % (a.profile_one, min(steps), max(steps)))
        b.close()
        return
    for G in [int(s) for s in a.sizes.split(",")]:
        gs = graphs(G)
        for g in gs[:2]:
            capi.po_solve(g)                                            # warm-up: module load, the one-shot path's cached block
        loop = clock(lambda: [capi.po_solve(g) for g in gs], a.repeats)
        print("G = %d" % G)
        print("  " + fmt("loop", loop, G))
        if a.loop_only:
            continue

        def end_to_end():
            b = capi.POBatch()
            for g in gs:
                b.add(g)
            b.finalize()
            b.solve(); b.download()
            b.close()
        end_to_end()
        e2e = clock(end_to_end, a.repeats)
        b = capi.POBatch()
        for g in gs:
            b.add(g)
        b.finalize()
        b.solve(); b.download()

        def resident():
            b.reset(); b.solve(); b.download()
        res = clock(resident, a.repeats)
        b.close()
        print("  " + fmt("end-to-end", e2e, G))
        print("  " + fmt("resident", res, G))
        print("  loop / end-to-end %.2fx, loop / resident %.2fx" % (np.median(loop) / np.median(e2e), np.median(loop) / np.median(res)))
        sys.stdout.flush()


if __name__ == "__main__":
    main()

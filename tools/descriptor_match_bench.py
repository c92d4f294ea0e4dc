"""Time of slslam_descriptor_matcher_run beside the two ways a caller could find the same pairs on the host: the numpy reference
(tests/descriptor_match_reference.py: the contract's ordered float chain) and an unordered `q @ k.T` - which does not give the contract's
bits - on one host thread.

    python tools/descriptor_match_bench.py [--dim 72] [--descriptors 300] [--repeats 15] [--out profiles/descriptor_match_bench.txt]

Shapes: D = 72, n = m = 300 at frames x candidates = 1 x 1, 1 x 3 and 64 x 3; descriptors from synth.make_descriptor_pair, ratio 1.5,
max_distance 0.25.  Warm (three untimed calls first), median and spread of `repeats` calls.  Two figures per shape: HIP events on the null
stream around the call - the call is synchronous on the matcher's own stream, so this is upload + two launches + download as the device
clock sees them, not separated - and the wall time of the call.  The host rows are wall times of one pair, times the pairs of the
shape.  A measurement, not a gate: needs a GPU and fails without one."""
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
    ap.add_argument("--dim", type=int, default=72)
    ap.add_argument("--descriptors", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "descriptor_match_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")                # (the host rows: one thread; set before numpy loads its BLAS)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    os.environ.setdefault("MKL_NUM_THREADS", "1")
    import numpy as np
    import torch
    from slslam_amd import capi, synth
    import descriptor_match_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    D, N = a.dim, a.descriptors
    ratio, max_distance = 1.5, 0.25
    views = [synth.make_descriptor_pair(9900 + i, n=N, dim=D, noise=0.03, outliers=0) for i in range(3)]
    lines = ["descriptor_match_bench: D = %d, n = m = %d (%d distances per pair), ratio %.1f, max_distance %.2f"
             % (D, N, N * N, ratio, max_distance)]

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

    def row(name, ms, pairs):
        return "%s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ms per pair, %.3f ns per distance" % (
            name, statistics.median(ms), min(ms), max(ms), len(ms), statistics.median(ms) / pairs, 1e6 * statistics.median(ms) / (pairs * N * N))

    m = capi.DescriptorMatcher(D, max_keyframes=3, max_descriptors=N, max_frames=64, max_candidates=3)
    for v in views:
        m.insert(v["keyframe"])
    for F, Cn in ((1, 1), (1, 3), (64, 3)):
        # the raw entry point on prepared arrays, so that the binding's conversions are not in the time
        cand = np.arange(Cn, dtype=np.int32)
        qs, outs, keep = (capi.DescriptorQuery * F)(), (capi.DescriptorResult * (F * Cn))(), []
        for f in range(F):
            q = views[f % 3]["query"]
            qs[f] = capi.DescriptorQuery(N, capi._fp(q), Cn, capi._ip(cand))
            for c in range(Cn):
                outs[f * Cn + c], b = capi._desc_buffers(N, N)
                keep.append(b)

        def call():
            rc = capi.lib().slslam_descriptor_matcher_run(m._h, F, qs, ratio, max_distance, F * Cn, outs)
            assert rc == 0, rc

        ev, wall = timed(call)
        lines.append(row("matcher %d x %d, HIP events around the call" % (F, Cn), ev, F * Cn))
        lines.append(row("matcher %d x %d, wall" % (F, Cn), wall, F * Cn))
        lines.append("  matched %d descriptors in %d pairs" % (sum(o.num_matched for o in outs), F * Cn))
    lines.append("matcher buffers: %s" % m.stats())
    m.close()

    # the host, one thread, one pair
    q, k = views[0]["query"], views[0]["keyframe"]
    t_ref, t_mm = [], []
    for _ in range(5):
        t0 = time.perf_counter(); R.match(q, k, ratio, max_distance); t_ref.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); r = np.float32(1.0) - q @ k.T; r.argmin(axis=1); r.argmin(axis=0); t_mm.append(1e3 * (time.perf_counter() - t0))
    for name, t in (("numpy reference (ordered chain, all outputs)", t_ref), ("numpy 1 - q @ k.T and the two argmins (unordered, not the contract's bits)", t_mm)):
        md = statistics.median(t)
        lines.append("%s, one pair, wall: median %.3f ms (min %.3f, max %.3f, %d calls); x 3 = %.3f ms, x 192 = %.1f ms" % (
            name, md, min(t), max(t), len(t), 3 * md, 192 * md))
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

"""Time of the vocabulary-tree trainer at the place bench's tree shape, beside the numpy reference on one host thread.

    python tools/voctree_train_bench.py [--n 600000] [--iterations 10] [--repeats 5] [--numpy-n 200000] [--out profiles/voctree_train_bench.txt]

Tree (40, 3, 72); N random unit descriptors; seed 1.  Warm (one untimed call first), the median of `repeats` calls.  The times are the
call's own (slslam_voctree_train_report: wall clock on the host around phases that each end in a stream synchronisation): per level the
host set-up (partition by node, initial centres, their upload), the assign-and-accumulate launches, the accumulator downloads, the host
centre() pass and the centre uploads; the rest of the total is validation, the keys, the descriptors' upload and the allocations.  The
numpy reference (tests/voctree_train_reference.py) is timed once at --numpy-n descriptors, where its nodes and words must equal the
device's.  A measurement, not a gate: needs a GPU and fails without one."""
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
    ap.add_argument("--n", type=int, default=600000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-n", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voctree_train_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    from slslam_amd import capi
    import voctree_train_reference as V
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    K, L, D, seed = 40, 3, 72, 1
    rng = np.random.default_rng(78)
    desc = rng.standard_normal((a.n, D))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    lines = ["voctree_train_bench: tree (%d, %d, %d), N = %d random unit descriptors, max_iterations %d, seed %d" % (K, L, D, a.n, a.iterations, seed)]

    capi.train_voctree(desc, K, L, max_iterations=a.iterations, seed=seed)
    runs = [capi.train_voctree(desc, K, L, max_iterations=a.iterations, seed=seed, timing=True) for _ in range(a.repeats)]
    med = lambda f: statistics.median(f(r) for r in runs)
    tot = [r["total_ms"] for r in runs]
    lines.append("total: median %.1f ms (min %.1f, max %.1f, %d warm calls); leaves reached %d of %d"
                 % (statistics.median(tot), min(tot), max(tot), a.repeats, len(np.unique(runs[0]["words"])), K ** L))
    phases = ("setup_ms", "kernel_ms", "download_ms", "centre_ms", "upload_ms")
    inside = 0.0
    for l in range(L):
        its = runs[0]["iterations"][l]
        t = {p: med(lambda r, p=p: r[p][l]) for p in phases}
        level = med(lambda r: sum(r[p][l] for p in phases))
        inside += level
        lines.append("level %d: %d rows of accumulators (%.1f MB), %d updates, %d assignments: median %.1f ms" %
                     (l, K ** (l + 1), 8e-6 * K ** (l + 1) * D, its, its + 1, level))
        lines.append("  set-up on the host (partition, initial centres, uploads) %.2f ms" % t["setup_ms"])
        lines.append("  assign-and-accumulate launches %.2f ms = %.3f ms per assignment" % (t["kernel_ms"], t["kernel_ms"] / (its + 1)))
        lines.append("  accumulator downloads (and labels, counts at the end) %.2f ms = %.3f ms per update" % (t["download_ms"], t["download_ms"] / max(its, 1)))
        lines.append("  host centre() pass %.2f ms = %.3f ms per update" % (t["centre_ms"], t["centre_ms"] / max(its, 1)))
        lines.append("  centre uploads %.2f ms = %.3f ms per update" % (t["upload_ms"], t["upload_ms"] / max(its, 1)))
    lines.append("outside the levels (validation, keys, allocations, descriptor upload of %.0f MB, copies out): median %.1f ms"
                 % (4e-6 * a.n * D, statistics.median(tot) - inside))

    m = min(a.numpy_n, a.n)
    t0 = time.perf_counter()
    ref = V.train(desc[:m], K, L, max_iterations=a.iterations, seed=seed)
    t_ref = time.perf_counter() - t0
    got = capi.train_voctree(desc[:m], K, L, max_iterations=a.iterations, seed=seed, timing=True)
    same = got["nodes"].tobytes() == ref["nodes"].tobytes() and got["words"].tolist() == ref["words"].tolist()
    lines.append("numpy reference, one host thread, N = %d: %.1f s; the device at that N: %.1f ms; nodes and words equal: %s"
                 % (m, t_ref, got["total_ms"], same))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

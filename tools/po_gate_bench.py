#!/usr/bin/env python3
"""Time and accuracy of the edge statistics (slslam_po_edge_statistics, slslam_po_gate, slslam_po_batch_gate).
   python tools/po_gate_bench.py [--out profiles/po_gate_bench.txt] [--reps 15] [--parent-library libslslam_hip.so of the parent commit]
HIP events on the default stream, warm, median of --reps (>= 10) with min .. max.  The graph is 260 poses / 8 loops with 8 candidates.
  gate against the old route   slslam_po_gate against slslam_po_covariance with the same pairs followed by INTEGRATION.md's formula on the
                               host (numpy, the Jacobians from the oracle's functor), one graph and batches of 16 and 64
  primitive throughput         slslam_po_edge_statistics alone at n = 9216 (1024 windows x 9 consecutive pairs)
  existing calls               with --parent-library: slslam_po_covariance and slslam_po_batch_covariance (G = 16), parent library and
                               this one in alternating child processes - the figures must lie inside the parent's own spread
Also the accuracy ratios d / y of tests/test_gpu_po_gate.py's cases.  Not bench.py: nothing here is a pass / fail figure."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from slslam_amd import capi, synth  # noqa: E402
import po_gate_reference as gref  # noqa: E402


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


def bench_graph(seed=7):
    g = synth.make_pose_graph(seed, 260, 8)
    x, _, _ = capi.po_solve(g)
    loops = [(int(p), int(q)) for p, q in zip(g["pose_index_1"], g["pose_index_2"]) if q - p > 1]
    rng = np.random.default_rng(41)
    sd = np.array([2e-3] * 3 + [1e-2] * 3)
    X = x.reshape(-1, 6)
    cons = np.array([gref.relative_pose(X[a], X[b]) + rng.normal(size=6) * sd for a, b in loops])
    cand = dict(pose_a=[p[0] for p in loops], pose_b=[p[1] for p in loops], constraints=cons, cov_meas=np.tile(np.diag(sd * sd), (len(loops), 1, 1)), sigma2=1.0)
    return g, x, loops, cand


def host_snippet(x, pairs, cand, cp, cq):
    X = x.reshape(-1, 6)
    out = []
    for k, (a, b) in enumerate(pairs):
        te, ja, jb = gref.jet(X[a], X[b], cand["constraints"][k])
        out.append(gref.snippet(te, ja, jb, cp[a], cp[b], cq[k], cand["cov_meas"][k], cand["sigma2"])[1])
    return out


def child_existing(reps):
    """Times the two existing covariance calls with whatever library SLSLAM_HIP_LIBRARY names; one JSON line."""
    ev = Events()
    g, x, loops, _ = bench_graph()
    capi.po_covariance(g, loops, 0.0, params=x)
    one = [ev.time(lambda: capi.po_covariance(g, loops, 0.0, params=x)) for _ in range(reps)]
    b = capi.POBatch()
    for k in range(16):
        b.add(synth.make_pose_graph(7 if k == 0 else 100 + k, 260, 8))
        b.set_covariance_pairs(k, loops)
    b.finalize()
    b.solve(); b.covariance(); b.download()
    bat = [ev.time(b.covariance) for _ in range(reps)]
    b.download()
    b.close()
    print(json.dumps(dict(one=stats(one), batch=stats(bat))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "po_gate_bench.txt"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child-existing", action="store_true")
    ap.add_argument("--skip-accuracy", action="store_true")
    a = ap.parse_args()
    reps = max(a.reps, 10)
    if a.child_existing:
        return child_existing(reps)
    ev = Events()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if not a.skip_accuracy:
        from oracle import pyoracle
        say("# edge statistics: accuracy, worst d / y per quantity (tests/test_gpu_po_gate.py's cases; K = 100 is the bound)")

        def worst(label, got, refs):
            w = dict.fromkeys(gref.QUANTITIES, 0.0)
            for k, ref in enumerate(refs):
                if ref["status"] == gref.COV_OK:
                    for q, r in gref.deviations(ref, {q: got[q][k] for q in gref.QUANTITIES}).items():
                        w[q] = max(w[q], r)
            say("%-44s " % label + "  ".join("%s %7.3f" % (q, w[q]) for q in gref.QUANTITIES))
        for n in (1, 5, 6, 65):
            it = gref.primitive_items(n)
            got = capi.po_edge_statistics(it["pose_a"], it["pose_b"], it["constraints"], it["cov_aa"], it["cov_bb"], it["cov_ab"], it["cov_meas"], it["sigma2"])
            worst("primitive n %d" % n, got, gref.primitive_reference(it))
        for shape in [(4, 1), (12, 2), (24, 3)]:
            g = synth.make_pose_graph(7, *shape)
            x, _, _ = pyoracle.po_solve(g, linear_solver=2)
            cand = gref.graph_candidates(g, x)
            pairs = list(zip(cand["pose_a"], cand["pose_b"]))
            ia, ib = [p[0] for p in pairs], [p[1] for p in pairs]
            for delta in (0.0, 0.001):
                _, got = capi.po_gate(g, cand, delta, params=x)
                st, cp, cq = capi.po_covariance(g, pairs, delta, params=x)
                worst("gate N %d loops %d delta %g, device Sigma" % (shape + (delta,)), got, gref.gate(g, x, cand, delta, blocks=(st, cp[ia], cp[ib], cq))[1])
                worst("gate N %d loops %d delta %g, end to end" % (shape + (delta,)), got, gref.gate(g, x, cand, delta)[1])
        say()

    say("# time, ms: median  min .. max over %d warm repetitions; 260 poses / 8 loops, 8 candidates" % reps)
    g, x, loops, cand = bench_graph()
    capi.po_gate(g, cand, 0.0, params=x)
    t = [ev.time(lambda: capi.po_gate(g, cand, 0.0, params=x)) for _ in range(reps)]
    say("slslam_po_gate (one graph)                          %9.3f %9.3f .. %9.3f" % stats(t))
    t, th = [], []
    for _ in range(reps):
        res = []
        t.append(ev.time(lambda: res.append(capi.po_covariance(g, loops, 0.0, params=x))))
        t0 = time.perf_counter()
        host_snippet(x, loops, cand, res[0][1], res[0][2])
        th.append(1e3 * (time.perf_counter() - t0))
    say("old route: slslam_po_covariance, the same pairs      %9.3f %9.3f .. %9.3f" % stats(t))
    say("           + the formula on the host (numpy, wall)   %9.3f %9.3f .. %9.3f" % stats(th))
    for G in (16, 64):
        b = capi.POBatch()
        for k in range(G):
            b.add(synth.make_pose_graph(7 if k == 0 else 100 + k, 260, 8))
            b.set_covariance_pairs(k, loops)
            b.set_candidates(k, cand)
        b.finalize()
        b.solve(); b.gate(); b.download()
        tg = [ev.time(b.gate) for _ in range(reps)]
        tc = [ev.time(b.covariance) for _ in range(reps)]
        tg2 = [ev.time(b.gate) for _ in range(reps)]
        b.gate(); b.download()
        ok = sorted(set(int(s) for k in range(G) for s in b.get_gate(k)["status"]))
        say("batch G = %2d: gate                                  %9.3f %9.3f .. %9.3f" % ((G,) + stats(tg)))
        say("batch G = %2d: covariance (the old route's device part)%7.3f %9.3f .. %9.3f   + %d x the host formula" % ((G,) + stats(tc) + (G,)))
        say("batch G = %2d: gate again                            %9.3f %9.3f .. %9.3f   statuses %s; %s" % ((G,) + stats(tg2) + (ok, b.covariance_stats())))
        b.close()
    n = 9216
    it = gref.primitive_items(n)
    args = (it["pose_a"], it["pose_b"], it["constraints"], it["cov_aa"], it["cov_bb"], it["cov_ab"], it["cov_meas"], it["sigma2"])
    capi.po_edge_statistics(*args)
    t = [ev.time(lambda: capi.po_edge_statistics(*args)) for _ in range(reps)]
    med = stats(t)
    say("slslam_po_edge_statistics n = %d (upload, launch, download) %9.3f %9.3f .. %9.3f   %.2f M items / s" % ((n,) + med + (n / med[0] / 1e3,)))

    if a.parent_library:
        say()
        say("# existing calls, parent library and this one in alternating child processes (ms: median  min .. max of %d)" % reps)
        for rnd in range(3):
            for name, path in (("parent", a.parent_library), ("this  ", None)):
                env = dict(os.environ)
                env.pop("SLSLAM_HIP_LIBRARY", None)
                if path:
                    env["SLSLAM_HIP_LIBRARY"] = os.path.abspath(path)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-existing", "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    say("%s round %d: child failed (%d) %s" % (name, rnd, p.returncode, p.stderr[-300:]))
                    break
                r = json.loads(p.stdout.strip().splitlines()[-1])
                say("%s round %d: slslam_po_covariance %8.3f %8.3f .. %8.3f   slslam_po_batch_covariance G = 16 %8.3f %8.3f .. %8.3f" % ((name, rnd) + tuple(r["one"]) + tuple(r["batch"])))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

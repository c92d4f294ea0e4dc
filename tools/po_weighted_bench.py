#!/usr/bin/env python3
"""Cost of the pose graph's per-edge square-root information (slslam_po_graph.sqrt_information): the solve without weights against the
parent commit's, and what the weights cost when given.  260 poses / 8 loop closures (BASELINE config 5), one graph and a 64-graph batch.
   python tools/po_weighted_bench.py --parent <checkout of the parent commit, built> [--out profiles/po_weighted_bench.txt] [--pairs 4]
The two libraries alternate in ONE session with the order balanced (P B | B P | B P | P B), every line a fresh process that imports the
package of its own tree: 3 warm-up and 40 timed capi.po_solve calls (host clock around calls that end in a synchronise), then a resident
batch of 64 (reset + solve + download, 3 warm-up and 10 timed).  'null' is the solve without weights - it has to sit inside the parent's
own run-to-run spread, which is printed beside it -, 'weighted' the same graphs with synth.make_edge_information's matrices (this tree
only); its extra cost is reported, not capped.  Not bench.py: nothing here is a pass / fail figure."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(root, weighted):
    sys.path.insert(0, root)
    import numpy as np
    from slslam_amd import capi, synth

    def graph(seed):
        g = synth.make_pose_graph(seed, 260, 8)
        return dict(g, sqrt_information=synth.make_edge_information(seed, g)) if weighted else g

    g = graph(7)
    for _ in range(3):
        x, s, _ = capi.po_solve(g)
    t = []
    for _ in range(40):
        t0 = time.perf_counter(); x, s, _ = capi.po_solve(g); t.append(1e3 * (time.perf_counter() - t0))
    b = capi.POBatch()
    for k in range(64):
        b.add(graph(7 if k == 0 else 100 + k))
    b.finalize()
    tb = []
    for r in range(13):
        b.reset()
        t0 = time.perf_counter(); b.solve(); b.download(); dt = 1e3 * (time.perf_counter() - t0)
        if r >= 3:
            tb.append(dt / 64)
    steps = [b.summary(k)["num_successful_steps"] + b.summary(k)["num_unsuccessful_steps"] for k in range(64)]
    b.close()
    print(json.dumps(dict(one=sorted(t), batch=sorted(tb), steps="%d+%d" % (s["num_successful_steps"], s["num_unsuccessful_steps"]),
                          cost=s["final_cost"], batch_steps=[min(steps), max(steps)], x=float(np.abs(x).sum()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "po_weighted_bench.txt"))
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--child", nargs=2, metavar=("ROOT", "WEIGHTED"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1] == "1")
    if not a.parent:
        ap.error("--parent is required")
    raw, res = [], {"parent null": [], "branch null": [], "branch weighted": []}

    def run(label, root, weighted):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "1" if weighted else "0"], capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit("%s failed (%d): %s" % (label, p.returncode, p.stderr[-2000:]))
        r = json.loads(p.stdout.strip().splitlines()[-1])
        res[label].append(r)
        o, q = r["one"], r["batch"]
        line = "%-15s one-graph median %.3f ms (min %.3f, max %.3f; 40 solves)  steps %s cost %.12e | batch 64 resident %.4f ms/graph (min %.4f, max %.4f; LM steps %d .. %d)" % (
            label, o[len(o) // 2], o[0], o[-1], r["steps"], r["cost"], q[len(q) // 2], q[0], q[-1], r["batch_steps"][0], r["batch_steps"][1])
        print(line, flush=True)
        raw.append(line)

    for k in range(a.pairs):
        order = "PB" if k % 4 in (0, 3) else "BP"
        raw.append("== pair %d: %s" % (k + 1, " ".join("parent" if c == "P" else "branch" for c in order)))
        print(raw[-1], flush=True)
        for c in order:
            if c == "P":
                run("parent null", os.path.abspath(a.parent), False)
            else:
                run("branch null", ROOT, False)
                run("branch weighted", ROOT, True)

    def med(v):
        v = sorted(v)
        return v[len(v) // 2]

    out = ["Pose-graph edge weights (sqrt_information): cost of the field when NULL, and of the whitening when given.  Parent commit against this",
           "change, one MI355X, one session, the two libraries alternating (%d pairs, order balanced); 260 poses, 8 loop closures." % a.pairs,
           "Every figure is a host clock around calls that end in a synchronise; per line a fresh process, 3 warm-up + 40 timed one-graph solves,",
           "then a resident batch of 64 (reset + solve + download; 3 warm-up + 10 timed).  tools/po_weighted_bench.py wrote this file.", "",
           "Summary (median of the per-process medians | min .. max of the per-process medians):"]
    for key, name, unit in (("one", "one-graph structured", "ms"), ("batch", "batch 64 resident", "ms/graph")):
        m = {lab: [r[key][len(r[key]) // 2] for r in rs] for lab, rs in res.items()}
        lo, hi = min(m["parent null"]), max(m["parent null"])
        bn = med(m["branch null"])
        verdict = "inside the parent's spread" if lo <= bn <= hi else ("BELOW the parent's spread" if bn < lo else "ABOVE the parent's spread")
        out.append("  %-22s [%s]  parent %.4f (%.4f .. %.4f, %d runs)   branch NULL %.4f (%.4f .. %.4f)   branch median %s" % (
            name, unit, med(m["parent null"]), lo, hi, len(m["parent null"]), bn, min(m["branch null"]), max(m["branch null"]), verdict))
        bw = med(m["branch weighted"])
        out.append("  %-22s [%s]  branch weighted %.4f (%.4f .. %.4f): %+.4f (%+.1f%%) against the branch's NULL solve of the same poses and edges" % (
            name, unit, bw, min(m["branch weighted"]), max(m["branch weighted"]), bw - bn, 100.0 * (bw - bn) / bn))
    def agree(labels):
        rs = [r for lab in labels for r in res[lab]]
        return "yes" if all((r["cost"], r["x"], r["steps"]) == (rs[0]["cost"], rs[0]["x"], rs[0]["steps"]) for r in rs) else "no"

    # (E = 267 edges are 54 waves adding into one matrix with fp64 atomics: the order of the sums, and with it the last bits, can differ from run to run)
    out.append("  NULL solves agree bit for bit (steps, final cost, sum |x|): the parent's runs among themselves %s, the branch's %s, parent and branch %s;"
               " final costs %.15e (parent) %.15e (branch)" % (agree(["parent null"]), agree(["branch null"]), agree(["parent null", "branch null"]),
                                                              res["parent null"][0]["cost"], res["branch null"][0]["cost"]))
    out.append("  (the weighted graphs are a different problem - other costs, possibly another number of LM steps: compare the step counts in the raw lines)")
    out += ["", "==== raw output"] + raw
    print("\n".join(out[5:5 + 8]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

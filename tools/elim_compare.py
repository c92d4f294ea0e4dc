"""A/B of the elimination sweeps on the bench batch (same windows, one process): per-kernel hipEvent times and it/s.
usage: python tools/elim_compare.py [--windows 1024] [--lines 2000] [--modes 1,2,3] [--steps 5]"""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slslam_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--lines", type=int, default=2000)
ap.add_argument("--modes", default="1,3,2")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--chunks", type=int, default=0)
args = ap.parse_args()
wins = [synth.make_window(i, num_lines=args.lines) for i in range(args.windows)]
ref = None
for mode in [int(m) for m in args.modes.split(",")]:
    bt = capi.LBABatch()
    for w in wins:
        bt.add(w)
    bt.finalize(use_graph=0, lba_elimination=mode, chunks_per_window=args.chunks)
    bt.set_profiling(True)
    for _ in range(2):
        bt.reset(); bt.solve()
    torch.cuda.synchronize()
    bt.iterations(clear=True)
    bt.set_profiling(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        bt.reset(); bt.solve()
    its = bt.iterations()
    dt = time.perf_counter() - t0
    bt.download()
    kt = bt.kernel_times()
    x0 = bt.parameters(0)
    s0 = bt.summary(0)
    if ref is None:
        ref = (x0, s0)
    out = {"mode": mode, "it_per_s": its / dt, "ms_per_step": 1e3 * dt / args.steps, "lm_iterations": its,
           "kernel_ms_per_launch": {k: v[0] / v[1] for k, v in kt.items() if v[1] > 0},
           "win0": {"steps": (s0["num_successful_steps"], s0["num_unsuccessful_steps"]), "final_cost": s0["final_cost"],
                    "max_param_diff_vs_first_mode": float(np.abs(x0 - ref[0]).max())}}
    print(json.dumps(out), flush=True)
    bt.close()

"""Records what every device LM loop computes on one tiny problem each: tests/golden/lm_traces_parent.npz.

    python tools/record_lm_traces.py [--out tests/golden/lm_traces_parent.npz]
    python tools/record_lm_traces.py --sweeps [--out tests/golden/lm_traces_sweeps_parent.npz]

Run on the GPU at the commit whose behaviour is to be kept; tests/test_gpu_lm_policy_parity.py replays the recorded inputs and
demands equal integers and bit-equal doubles (the pose graphs, whose sums go through fp64 atomics, to the oracle-parity tolerances).
The file holds, per case (CASES below has its solver options), the input arrays and the solved parameters, the summary and the full
iteration trace (refine-lines: the per-line results - that loop keeps no trace).

The start values of every case are perturbed (Gaussian, the smallest scale of SCALES that does it) until the trace of every loop has
at least one accepted and one rejected step; the tool refuses to write the file otherwise.

--sweeps records SWEEP_CASES instead: the LBA kernels CASES does not reach (the matrix-core sweeps, the slab reduction of a window cut
into many chunks, the reduced solve of a batch with more windows than CUs, the wider k_big_solve), replayed by
tests/test_gpu_sweep_parity.py.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from slslam_amd import capi, synth  # noqa: E402

SCALES = (0.0, 0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4, 0.8, 1.5, 3.0)
SEEDS = range(8)
WINDOW_KEYS = ("camera_index", "line_index", "fixed_index", "observations", "parameters")
GRAPH_KEYS = ("pose_index_1", "pose_index_2", "constraints", "parameters")
SUMMARY_INT = ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks")
SUMMARY_DBL = ("initial_cost", "final_cost", "fixed_cost")
TRACE_INT = ("iteration", "step_is_valid", "step_is_successful")
TRACE_DBL = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change")
LINE_INT = ("status", "termination_type", "num_successful_steps", "num_unsuccessful_steps", "num_observations")
LINE_DBL = ("initial_cost", "final_cost")
PATH_TILED, PATH_FUSED_MOTION_ONLY, PATH_GLOBAL_MEMORY = 0, 1, 2

# case -> (kind, expected slslam_lba_batch_path or None, solver options)
CASES = {
    "lba_fused": ("lba", PATH_TILED, {}),                         # the first sweep doubles as the initial evaluation (k_reduced_solve)
    "lba_split": ("lba", PATH_TILED, {"reuse_elimination": 1}),   # a separate initial pass (k_lm_init), then k_lm_update
    "lba_big": ("lba", PATH_GLOBAL_MEMORY, {}),                   # lba_big.h
    "motion_only": ("lba", PATH_FUSED_MOTION_ONLY, {}),
    "refine_lines": ("refine", None, {}),
    "po_single": ("po", None, {}),
    "po_batch": ("po_batch", None, {}),
}

# case -> (kind, expected path, solver options); an lba_elimination among the options is also what elimination() must report.  Inputs
# with "copies" are solved as a batch of that many copies of the window, and the windows listed in "record" are kept (keys "<field>_<i>")
SWEEP_CASES = {
    "elim2": ("lba", PATH_TILED, {"lba_elimination": 2}),          # k_eliminate_mfma<1>
    "elim3": ("lba", PATH_TILED, {"lba_elimination": 3}),          # k_eliminate_mfma<2>, k_backsub with two waves
    "elim4": ("lba", PATH_TILED, {"lba_elimination": 4}),          # k_eliminate_grouped
    "elim4_keep": ("lba", PATH_TILED, {"lba_elimination": 4, "lba_keep_jacobian": 1}),
    "elim4_mixed": ("lba", PATH_TILED, {"lba_elimination": 4, "lba_precision": 1}),
    "two_chunks": ("lba", PATH_TILED, {"chunks_per_window": 2}),   # the 70-line window in two chunks (no slab reduction: that takes more than 8)
    "many_chunks": ("lba", PATH_TILED, {"chunks_per_window": 64}),  # one tile per chunk, more than 8 of them: k_slab_reduce, k_lm_update_wave
    "batch257": ("lba", PATH_TILED, {}),                           # more windows than CUs: k_reduced_solve<4>
    "big_wide": ("lba", PATH_GLOBAL_MEMORY, {}),                   # 42 free cameras, 252 reduced unknowns: k_big_solve<kBsvSlots>
}
MANY_CHUNKS = 9      # what "many_chunks" must be cut into at least (k_slab_reduce runs for windows of more than 8 chunks)


def _window(w, params=None):
    d = {k: np.array(w[k]) for k in WINDOW_KEYS}
    d["sizes"] = np.array([w["num_cameras"], w["num_lines"]], dtype=np.int64)
    if params is not None:
        d["parameters"] = np.array(params)
    return d


def _graph(g, params=None):
    d = {k: np.array(g[k]) for k in GRAPH_KEYS}
    d["sizes"] = np.array([g["num_poses"]], dtype=np.int64)
    if params is not None:
        d["parameters"] = np.array(params)
    return d


def as_window(d, suffix=""):
    w = {k: d[k + suffix] for k in WINDOW_KEYS}
    w["num_cameras"], w["num_lines"] = (int(v) for v in d["sizes" + suffix])
    return w


def as_graph(d, suffix=""):
    g = {k: d[k + suffix] for k in GRAPH_KEYS}
    g["num_poses"] = int(d["sizes" + suffix][0])
    return g


def oversize(w):
    """The window with the observations of line 0 repeated until it has 65 of them: a line beyond one wave's 64 lanes takes the
    batch to the global-memory path.  There is no option that selects that path for a window the tiled sweeps can hold."""
    li = np.asarray(w["line_index"])
    rows = np.nonzero(li == 0)[0]
    extra = np.resize(rows, 65 - len(rows))
    order = np.concatenate([rows, extra, np.nonzero(li != 0)[0]])
    out = dict(w)
    out["camera_index"] = np.asarray(w["camera_index"])[order]
    out["line_index"] = li[order]
    out["fixed_index"] = np.asarray(w["fixed_index"]).reshape(-1, 2)[order].reshape(-1)
    out["observations"] = np.asarray(w["observations"]).reshape(-1, 8)[order]
    return out


def _pack(summary, trace):
    return {"summary_int": np.array([summary[k] for k in SUMMARY_INT], dtype=np.int64),
            "summary_dbl": np.array([summary[k] for k in SUMMARY_DBL], dtype=np.float64),
            "trace_int": np.array([[r[k] for k in TRACE_INT] for r in trace], dtype=np.int64).reshape(-1, len(TRACE_INT)),
            "trace_dbl": np.array([[r[k] for k in TRACE_DBL] for r in trace], dtype=np.float64).reshape(-1, len(TRACE_DBL))}


def solve(kind, path, opts, inp):
    """One case: the recorded outputs as a dict of arrays."""
    if kind == "lba":
        w = as_window(inp)
        b = capi.LBABatch()
        try:
            for _ in range(int(inp["copies"]) if "copies" in inp else 1):
                b.add(w)
            b.finalize(**opts)
            b.solve(); b.download()
            assert b.path() == path, (b.path(), path)
            if "lba_elimination" in opts:
                assert b.elimination() == opts["lba_elimination"], (b.elimination(), opts)
            if opts.get("chunks_per_window", 0) > 8:
                assert b.window_chunks(0) >= MANY_CHUNKS, b.window_chunks(0)
            if "copies" in inp:
                out = {}
                for i in inp["record"]:
                    for k, v in _pack(b.summary(int(i)), b.trace(int(i))).items():
                        out["%s_%d" % (k, i)] = v
                    out["parameters_%d" % i] = b.parameters(int(i)).copy()
            else:
                out = _pack(b.summary(0), b.trace(0))
                out["parameters"] = b.parameters(0).copy()
        finally:
            b.close()
        return out
    if kind == "refine":
        x, res, tot = capi.lba_refine_lines(as_window(inp), **opts)
        out = _pack(tot, [])
        out["parameters"] = np.array(x)
        out["line_int"] = np.array([[r[k] for k in LINE_INT] for r in res], dtype=np.int64)
        out["line_dbl"] = np.array([[r[k] for k in LINE_DBL] for r in res], dtype=np.float64)
        return out
    if kind == "po":
        x, s, t = capi.po_solve(as_graph(inp), **opts)
        out = _pack(s, t)
        out["parameters"] = np.array(x)
        return out
    out = {}
    for i, (x, s, t) in enumerate(capi.po_solve_batch([as_graph(inp, "_%d" % i) for i in range(2)], **opts)):
        for k, v in _pack(s, t).items():
            out["%s_%d" % (k, i)] = v
        out["parameters_%d" % i] = np.array(x)
    return out


def walks_both(out):
    """At least one accepted and one rejected step in every trace of the case."""
    if "line_int" in out:
        li = out["line_int"]
        return bool(((li[:, 2] > 0) & (li[:, 3] > 0)).any())
    ok = True
    for k, t in out.items():
        if k.startswith("trace_int"):
            steps = t[t[:, 0] > 0]
            ok = ok and bool((steps[:, 2] == 1).any()) and bool((steps[:, 2] == 0).any())
    return ok


def perturbed(x, scale, seed, first=0):
    x = np.array(x, dtype=np.float64)
    if scale > 0.0:
        x[first:] += scale * np.random.default_rng([17, seed]).normal(size=x[first:].shape)
    return x


def search(names, make_inputs, cases=None):
    """The inputs at the smallest perturbation at which every case of `names` walks both branches, and the outputs."""
    cases = CASES if cases is None else cases
    for scale in SCALES:
        for seed in SEEDS:
            inputs = make_inputs(scale, seed)
            outs = {n: solve(*cases[n], inputs[n]) for n in names}
            if all(walks_both(o) for o in outs.values()):
                print("%s: start perturbation %g (seed %d)" % (", ".join(names), scale, seed))
                return {n: (inputs[n], outs[n]) for n in names}
            if scale == 0.0:
                break
    raise SystemExit("no start perturbation gives %s an accepted and a rejected step: nothing written" % ", ".join(names))


def record():
    w = synth.make_window(3, num_lines=12, num_kf=3, num_free=2, mean_track=3.0)
    mo = synth.make_motion_only(5, num_lines=12)
    rl = synth.make_window(7, num_lines=70, num_kf=3, num_free=2, mean_track=3.0)
    g6 = synth.make_pose_graph(2, num_poses=6, num_loops=3)
    g4 = synth.make_pose_graph(3, num_poses=4, num_loops=2)
    assert len(g6["pose_index_1"]) == 8, len(g6["pose_index_1"])
    done = {}

    def lba_inputs(scale, seed):
        x = perturbed(w["parameters"], scale, seed)
        return {"lba_fused": _window(w, x), "lba_split": _window(w, x), "lba_big": _window(oversize(w), x)}
    done.update(search(["lba_fused", "lba_split", "lba_big"], lba_inputs))
    done.update(search(["motion_only"], lambda scale, seed: {"motion_only": _window(mo, perturbed(mo["parameters"], scale, seed))}))
    done.update(search(["refine_lines"], lambda scale, seed: {"refine_lines": _window(rl, perturbed(rl["parameters"], scale, seed, first=6 * 3))}))
    done.update(search(["po_single"], lambda scale, seed: {"po_single": _graph(g6, perturbed(g6["parameters"], scale, seed, first=6))}))

    def batch_inputs(scale, seed):
        d = {}
        for i, g in enumerate((g6, g4)):
            for k, v in _graph(g, perturbed(g["parameters"], scale, seed + i, first=6)).items():
                d["%s_%d" % (k, i)] = v
        return {"po_batch": d}
    done.update(search(["po_batch"], batch_inputs))
    return _flat(done)


def wide_window():
    """42 free cameras of 44 (252 reduced unknowns, beyond the 240 of k_big_solve<15>), few lines on long tracks."""
    return oversize(synth.make_window(12, num_lines=60, num_kf=44, num_free=42, mean_track=10.0))


def record_sweeps():
    w = synth.make_window(3, num_lines=12, num_kf=3, num_free=2, mean_track=3.0)
    w70 = synth.make_window(7, num_lines=70, num_kf=3, num_free=2, mean_track=3.0)
    w240 = synth.make_window(9, num_lines=240, num_kf=3, num_free=2, mean_track=3.0)
    wide = wide_window()
    done = {}
    for name, base in (("elim2", w), ("elim3", w), ("elim4", w), ("elim4_keep", w), ("elim4_mixed", w), ("two_chunks", w70), ("many_chunks", w240),
                       ("big_wide", wide)):
        done.update(search([name], lambda scale, seed: {name: _window(base, perturbed(base["parameters"], scale, seed))}, SWEEP_CASES))

    def copies(scale, seed):
        d = _window(w, perturbed(w["parameters"], scale, seed))
        d["copies"], d["record"] = np.array(257, dtype=np.int64), np.array([0, 256], dtype=np.int64)
        return {"batch257": d}
    done.update(search(["batch257"], copies, SWEEP_CASES))
    return _flat(done)


def _flat(done):
    flat = {}
    for name, (inp, out) in done.items():
        for k, v in inp.items():
            flat["%s/in/%s" % (name, k)] = v
        for k, v in out.items():
            flat["%s/out/%s" % (name, k)] = v
    return flat


def load(path):
    """{case: (inputs, outputs)} of a recorded file."""
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            name, side, k = key.split("/")
            cases.setdefault(name, ({}, {}))[0 if side == "in" else 1][k] = z[key]
    return cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sweeps", action="store_true", help="record SWEEP_CASES (tests/golden/lm_traces_sweeps_parent.npz) instead of CASES")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "tests", "golden", "lm_traces_sweeps_parent.npz" if a.sweeps else "lm_traces_parent.npz")
    flat = record_sweeps() if a.sweeps else record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **flat)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(flat), os.path.getsize(a.out)))

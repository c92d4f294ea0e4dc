"""Reference for the structure-only refinement (include/slslam_hip.h: slslam_line_refiner_run, slslam_lba_refine_lines): THE ORACLE
APPLIED TO EACH LINE'S OWN PROBLEM.  For line l of a window: oracle.pyoracle.lba_solve on the one-line window made of the window's
cameras, all flagged constant, and l's observations in their original order, from l's start value.

The yardstick of a line is the oracle's own movement when that line's start value is scaled by (1 + 1e-13) - what
tests/test_gpu_lba.py::test_headline_path_matches_oracle measures a deviation against: initial cost, final cost and the four
parameters of the perturbed solve against the unperturbed one, and whether the accept / reject sequence of the two solves is the same.
TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

PERTURB = 1e-13
MARGIN = 10.0              # fused multiply-add and summation-order differences between the C oracle and the device
PARAM_FLOOR = 1e-10        # absolute, parameters
COST_FLOOR = 1e-12         # relative, costs


def all_cameras_constant(w):
    """The window with every camera flagged constant (line flags kept)."""
    v = dict(w)
    f = np.array(w["fixed_index"], dtype=np.int32).reshape(-1, 2).copy()
    f[:, 0] = 1
    v["fixed_index"] = f.reshape(-1)
    return v


def one_line_window(w, l, params=None):
    """Line l alone: the window's cameras, all constant, l's observations in their original order; line index 0."""
    C = int(w["num_cameras"])
    li = np.asarray(w["line_index"])
    sel = np.nonzero(li == l)[0]
    x = np.asarray(w["parameters"] if params is None else params, dtype=np.float64).reshape(-1)
    f = np.array(w["fixed_index"], dtype=np.int32).reshape(-1, 2)[sel].copy()
    f[:, 0] = 1
    v = {"num_cameras": C, "num_lines": 1,
         "camera_index": np.asarray(w["camera_index"], dtype=np.int32)[sel].copy(),
         "line_index": np.zeros(len(sel), dtype=np.int32), "fixed_index": f.reshape(-1),
         "observations": np.asarray(w["observations"], dtype=np.float64).reshape(-1, 8)[sel].copy(),
         "parameters": np.concatenate([x[:6 * C], x[6 * C + 4 * l:6 * C + 4 * l + 4]])}
    if "baseline" in w:
        v["baseline"] = w["baseline"]
    return v


def _decisions(trace):
    return [(t["iteration"], t["step_is_valid"], t["step_is_successful"]) for t in trace]


def solve_line(w, l, params=None, perturb=0.0, **opt):
    """(line[4], summary, trace) of the oracle on line l's own problem; perturb: the line's start scaled by (1 + perturb)."""
    from oracle import pyoracle
    v = one_line_window(w, l, params)
    if perturb:
        v["parameters"] = v["parameters"].copy()
        v["parameters"][-4:] *= 1.0 + perturb
    x, s, tr = pyoracle.lba_solve(v, **opt)
    return x[-4:].copy(), s, tr


def reference(w, params=None, yardstick=True, **opt):
    """Per line of the window: dict(line, initial_cost, final_cost, num_successful_steps, num_unsuccessful_steps, termination_type,
    num_observations) and, with yardstick, move_param / move_initial / move_final (the oracle's own movement under PERTURB) and
    stable (its accept / reject sequence and termination did not change).  opt: oracle options (max_num_iterations, huber_delta, ...)."""
    out = []
    li = np.asarray(w["line_index"])
    for l in range(int(w["num_lines"])):
        n = int((li == l).sum())
        x, s, tr = solve_line(w, l, params, **opt)
        r = dict(line=x, initial_cost=s["initial_cost"], final_cost=s["final_cost"], num_successful_steps=s["num_successful_steps"],
                 num_unsuccessful_steps=s["num_unsuccessful_steps"], termination_type=s["termination_type"], num_observations=n)
        if yardstick:
            xp, sp, trp = solve_line(w, l, params, perturb=PERTURB, **opt)
            r["move_param"] = float(np.abs(xp - x).max())
            r["move_initial"] = abs(sp["initial_cost"] - s["initial_cost"])
            r["move_final"] = abs(sp["final_cost"] - s["final_cost"])
            r["stable"] = _decisions(tr) == _decisions(trp) and sp["termination_type"] == s["termination_type"]
        out.append(r)
    return out


def check_parity(ref, params, res, num_cameras, lines=None, label=""):
    """The issue's rule, per line: step counts and termination identical (lines whose oracle decisions move under PERTURB left out, at
    most 5 % of them), costs and parameters within MARGIN x the oracle's own movement (floors PARAM_FLOOR absolute / COST_FLOOR relative).
    Prints the worst ratio; returns it."""
    lines = range(len(ref)) if lines is None else lines
    worst, left_out, n = 0.0, 0, 0
    for l in lines:
        r, g = ref[l], res[l]
        n += 1
        if r["stable"]:
            assert (int(g["num_successful_steps"]), int(g["num_unsuccessful_steps"]), int(g["termination_type"])) == \
                (r["num_successful_steps"], r["num_unsuccessful_steps"], r["termination_type"]), (label, l, g, r)
        else:
            left_out += 1
        x = np.asarray(params[6 * num_cameras + 4 * l:6 * num_cameras + 4 * l + 4])
        tol_p = max(MARGIN * r["move_param"], PARAM_FLOOR)
        tol_i = max(MARGIN * r["move_initial"], COST_FLOOR * abs(r["initial_cost"]))
        tol_f = max(MARGIN * r["move_final"], COST_FLOOR * abs(r["final_cost"]))
        ratios = (float(np.abs(x - r["line"]).max()) / tol_p, abs(float(g["initial_cost"]) - r["initial_cost"]) / tol_i,
                  abs(float(g["final_cost"]) - r["final_cost"]) / tol_f)
        worst = max(worst, *ratios)
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0 and ratios[2] <= 1.0, (label, l, ratios, x, r)
    print("%s: %d lines, worst deviation / tolerance %.3g, left out of the count check %d" % (label, n, worst, left_out))
    assert left_out <= 0.05 * n, (label, left_out, n)
    return worst

"""CPU reference of the pose-graph solve with per-edge square-root information matrices (slslam_po_graph.sqrt_information), for the tests.

The pattern of tests/po_robust_reference.py, whose trust-region driver (oracle_lm_minimize through ctypes callbacks, the dense numpy
Jacobian, the oracle's Cholesky) is reused as it is: every block - the six residuals of oracle_pose_residual_jet and both 6 x 6 Jacobian
blocks - is multiplied by the edge's W_e BEFORE the Huber corrector (oracle_huber), so s = |W_e Te|^2, the corrector scales the whitened
block and the block cost is rho(s) / 2: the weight inside the functor, as Ceres has it.  W = None is tests/po_robust_reference.py.
Also the per-edge report and the covariance of the whitened system, on tests/po_covariance_reference.py's two routes and yardstick.
TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C
import os
import sys

import numpy as np

from oracle import pyoracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402
import po_robust_reference as robust  # noqa: E402


def weights(g, W=None):
    """[E, 6, 6] from W, else from g["sqrt_information"], else None."""
    if W is None:
        W = g.get("sqrt_information")
    return None if W is None else np.asarray(W, dtype=np.float64).reshape(-1, 6, 6)


def _block(p1, p2, c, w, delta, want_jac=True):
    """One whitened residual block: (s = |W Te|^2, rho', robustified r, J1, J2, block cost).  w = None: identity."""
    if w is None:
        return robust._block(p1, p2, c, delta, want_jac)
    if want_jac:
        r, j1, j2 = pyoracle.pose_residual_jet(p1, p2, c)
        j1, j2 = w @ j1, w @ j2
    else:
        r = np.zeros(6)
        p1, p2, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (p1, p2, c))
        pyoracle.lib().oracle_pose_residual(pyoracle._dp(p1), pyoracle._dp(p2), pyoracle._dp(c), pyoracle._dp(r))
        j1 = j2 = None
    r = w @ r
    s = 0.0
    for q in range(6):
        s += r[q] * r[q]
    if delta > 0.0:
        rho = pyoracle.huber(s, delta)
        sr = np.sqrt(rho[1])
        r = r * sr
        if want_jac:
            j1, j2 = j1 * sr, j2 * sr
        return s, rho[1], r, j1, j2, 0.5 * rho[0]
    return s, 1.0, r, j1, j2, 0.5 * s


class _Problem(robust._Problem):
    def __init__(self, g, params, delta, W):
        super().__init__(g, params, delta)
        self.W = W
        kept = set(self.kept)
        self.fixed_cost = sum(_block(self.params[self.i1[e]], self.params[self.i2[e]], self.cons[e], self._w(e), self.delta, False)[5]
                              for e in range(self.E) if e not in kept)

    def _w(self, e):
        return None if self.W is None else self.W[e]

    def evaluate(self, _ctx, xp, costp, want_jac, gradp):
        x = np.ctypeslib.as_array(xp, shape=(self.n,))
        self.scatter(x)
        total = 0.0
        if want_jac:
            self.J[:] = 0.0
        for row, e in enumerate(self.kept):
            a, b = self.i1[e], self.i2[e]
            _, _, r, j1, j2, c = _block(self.params[a], self.params[b], self.cons[e], self._w(e), self.delta, bool(want_jac))
            total += c
            if want_jac:
                self.r[6 * row:6 * row + 6] = r
                if self.slot[a] >= 0:
                    self.J[6 * row:6 * row + 6, self.slot[a]:self.slot[a] + 6] = j1
                if self.slot[b] >= 0:
                    self.J[6 * row:6 * row + 6, self.slot[b]:self.slot[b] + 6] = j2
        costp[0] = total
        if want_jac and gradp:
            np.ctypeslib.as_array(gradp, shape=(self.n,))[:] = self.J.T @ self.r
        return 1 if np.isfinite(total) else 0


def po_solve(g, po_huber_delta=0.0, W=None, params=None, trace_cap=256, **opt):
    """The pose graph with blocks whitened by W ([E, 6, 6]; default g["sqrt_information"]; None: identity) through oracle_lm_minimize,
    HuberLoss(po_huber_delta) on |W_e Te|^2 (0: no loss).  Returns (params_out, summary dict, trace list) as po_robust_reference.po_solve."""
    L = pyoracle.lib()
    L.oracle_dense_cholesky.argtypes = [robust._DP, C.c_int]
    L.oracle_dense_cholesky_solve.argtypes = [robust._DP, C.c_int, robust._DP]
    L.oracle_lm_minimize.argtypes = [C.POINTER(robust._NLLS), C.POINTER(pyoracle.LMOptions), robust._DP, C.POINTER(pyoracle.Summary),
                                     C.POINTER(pyoracle.Iteration), C.c_int, C.POINTER(C.c_int)]
    x0 = np.array(g["parameters"] if params is None else params, dtype=np.float64).reshape(-1).copy()
    P = _Problem(g, x0, po_huber_delta, weights(g, W))
    s = pyoracle.Summary()
    tr = (pyoracle.Iteration * trace_cap)()
    nt = C.c_int(0)
    s.fixed_cost = P.fixed_cost
    s.num_free_parameters = P.n
    s.num_residual_blocks = len(P.kept)
    if P.E == 0 or P.n == 0:
        s.initial_cost = s.final_cost = P.fixed_cost
        s.termination_type = 2
        return x0, dict(pyoracle._summary_dict(s), rc=0), []
    x = np.zeros(P.n)
    for k in range(P.N):
        if P.slot[k] >= 0:
            x[P.slot[k]:P.slot[k] + 6] = x0[6 * k:6 * k + 6]
    cbs = (robust._EVAL(P.evaluate), robust._VEC(P.sq_col_norm), robust._VEC(P.scale_cols), robust._SOLVE(P.solve), robust._MODEL(P.model_cost_change))
    nl = robust._NLLS(P.n, None, *cbs)
    o = pyoracle.default_options(**opt)
    rc = L.oracle_lm_minimize(C.byref(nl), C.byref(o), pyoracle._dp(x), C.byref(s), tr, trace_cap, C.byref(nt))
    out = x0.copy()
    if s.termination_type != 4:
        for k in range(P.N):
            if P.slot[k] >= 0:
                out[6 * k:6 * k + 6] = x[P.slot[k]:P.slot[k] + 6]
    return out, dict(pyoracle._summary_dict(s), rc=rc), pyoracle._trace_list(tr, min(nt.value, trace_cap))


def edge_report(g, params, po_huber_delta=0.0, W=None):
    """(sq_norm[E], weight[E]) at params: |W_e Te|^2 of every edge and rho' of it (1 for inliers and when there is no loss)."""
    W = weights(g, W)
    x = np.asarray(params, dtype=np.float64).reshape(-1, 6)
    cons = np.asarray(g["constraints"], dtype=np.float64).reshape(-1, 6)
    sq, w = [], []
    for e, (a, b, c) in enumerate(zip(g["pose_index_1"], g["pose_index_2"], cons)):
        s, rho1 = _block(x[a], x[b], c, None if W is None else W[e], float(po_huber_delta), False)[:2]
        sq.append(s); w.append(rho1)
    return np.array(sq), np.array(w)


def jacobian(g, params, delta=0.0, W=None):
    """po_covariance_reference.jacobian with every edge's block whitened: J [6 E, n] at params."""
    W = weights(g, W)
    slot, n = cref.slots(g)
    x = np.asarray(params, dtype=np.float64).reshape(-1, 6)
    cons = np.asarray(g["constraints"], dtype=np.float64).reshape(-1, 6)
    J = np.zeros((6 * len(cons), n))
    for e, (a, b) in enumerate(zip(g["pose_index_1"], g["pose_index_2"])):
        _, _, _, j1, j2, _ = _block(x[a], x[b], cons[e], None if W is None else W[e], float(delta), True)
        if slot[a] >= 0:
            J[6 * e:6 * e + 6, slot[a]:slot[a] + 6] = j1
        if slot[b] >= 0:
            J[6 * e:6 * e + 6, slot[b]:slot[b] + 6] = j2
    return J


def covariance(g, params, delta=0.0, W=None):
    """po_covariance_reference.covariance of the whitened system: the same dict, routes and yardstick y = max(r, c)."""
    slot, n = cref.slots(g)
    J = jacobian(g, params, delta, W)
    piv = cref.smallest_pivot(J.T @ J)
    out = dict(slot=slot, n=n, pivot=piv, sigma=None, r=None, c=None, y=None)
    if not piv > cref.PIVOT_MIN:
        return out
    s1 = cref._route1(J)
    out["sigma"] = s1
    top = np.abs(s1).max()
    out["r"] = np.abs(s1 - cref._route2(J)).max() / top
    rng = np.random.default_rng(2024)
    eps = np.finfo(np.float64).eps
    out["c"] = max(np.abs(cref._route1(J * (1.0 + eps * rng.choice([-1.0, 1.0], size=J.shape))) - s1).max() for _ in range(5)) / top
    out["y"] = max(out["r"], out["c"])
    return out


# ---------------------------------------------------------------------------------------------- the tests' graphs
# Those of tests/test_gpu_po_robust.py (k_po_linearise packs 5 edges of 12 lanes per wave): e1, e5, e10 - one lane group, one full wave,
# two full waves -, e6 - a 7-pose chain: the second wave holds one edge -, c24 (E = 26) and c60 (E = 63) with one false loop closure,
# gauge24 with the false constraint on the gauge edge, clean24 / clean60 without one.
WEIGHT_SEED = 3


def corrupt(g, e=None):
    """One loop constraint off by (1.5, 0, -1) m and 0.4 rad: the first loop edge unless an edge is named.  Returns (graph, edge)."""
    g = dict(g, constraints=np.array(g["constraints"], dtype=np.float64).copy())
    if e is None:
        e = int(np.nonzero(np.asarray(g["pose_index_2"]) - np.asarray(g["pose_index_1"]) > 1)[0][0])
    g["constraints"][e, 3:6] += (1.5, 0.0, -1.0)
    g["constraints"][e, 1] += 0.4
    return g, e


def chain(seed, n):
    """A chain without loops, its free poses perturbed (a tree: every constraint can be met exactly)."""
    from slslam_amd import synth
    g = synth.make_pose_graph(seed, num_poses=n, num_loops=0)
    rng = np.random.default_rng(seed)
    return dict(g, parameters=g["parameters"] + rng.normal(0, 2e-3, g["parameters"].shape) * (np.arange(len(g["parameters"])) >= 6))


def graph(name):
    """(graph without weights, index of its false edge or -1)."""
    from slslam_amd import synth
    if name in ("c24", "c60", "clean24", "clean60"):
        g = synth.make_pose_graph(7, *((24, 3) if name.endswith("24") else (60, 4)))
        return (g, -1) if name.startswith("clean") else corrupt(g)
    if name == "gauge24":
        return corrupt(synth.make_pose_graph(7, 24, 3), 0)
    if name == "e1":
        g = synth.make_pose_graph(27, num_poses=2, num_loops=0)
        g = dict(g, constraints=g["constraints"].copy()); g["constraints"][0, 3] += 0.5
        return g, 0
    if name in ("e5", "e6", "e10"):
        return chain({"e5": 31, "e6": 33, "e10": 32}[name], int(name[1:]) + 1), -1
    raise KeyError(name)


def weighted(name, seed=WEIGHT_SEED):
    """(the graph with synth.make_edge_information's full, non-symmetric W_e as g["sqrt_information"], its false edge or -1)."""
    from slslam_amd import synth
    g, bad = graph(name)
    return dict(g, sqrt_information=synth.make_edge_information(seed, g)), bad

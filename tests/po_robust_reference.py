"""CPU reference of the ROBUST pose-graph solve (reference src/po_problem.cpp:27,55: robustify ? HuberLoss(0.001) : NULL), for the tests.

The oracle's pose-graph solve (oracle/po_oracle.c) restates the reference as it ships, without a loss.  This helper drives the same
trust-region loop - oracle_lm_minimize (oracle/lm_core.h) - through ctypes callbacks, with the oracle's own residual functor
(oracle_pose_residual_jet) and loss (oracle_huber), and keeps the Jacobian as a dense numpy matrix: per edge both 6 x 6 blocks and the
residuals are scaled by sqrt(rho') (Ceres 1.7's corrector for rho'' <= 0, as oracle/lba_oracle.c does for line blocks) and the block cost
is rho / 2.  With delta = 0 it is oracle.po_solve (tests/test_po_robust_cpu.py holds it to that).

Conventions of lm_core.c: evaluate returns non-zero on success; solve returns 0 on success and writes y with
(J^T J + diag(d)^2) y = J^T r; the free poses are all referenced poses except pose_index_1[0].  TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C

import numpy as np

from oracle import pyoracle

_DP = C.POINTER(C.c_double)
_EVAL = C.CFUNCTYPE(C.c_int, C.c_void_p, _DP, _DP, C.c_int, _DP)
_VEC = C.CFUNCTYPE(None, C.c_void_p, _DP)
_SOLVE = C.CFUNCTYPE(C.c_int, C.c_void_p, _DP, _DP)
_MODEL = C.CFUNCTYPE(C.c_double, C.c_void_p, _DP)


class _NLLS(C.Structure):
    _fields_ = [("n", C.c_int), ("ctx", C.c_void_p), ("evaluate", _EVAL), ("sq_col_norm", _VEC), ("scale_cols", _VEC),
                ("solve", _SOLVE), ("model_cost_change", _MODEL)]


def _block(p1, p2, c, delta, want_jac=True):
    """One residual block: (s = |Te|^2, rho', robustified r, J1, J2, block cost)."""
    if want_jac:
        r, j1, j2 = pyoracle.pose_residual_jet(p1, p2, c)
    else:
        r = np.zeros(6)
        p1, p2, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (p1, p2, c))
        pyoracle.lib().oracle_pose_residual(pyoracle._dp(p1), pyoracle._dp(p2), pyoracle._dp(c), pyoracle._dp(r))
        j1 = j2 = None
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


class _Problem:
    def __init__(self, g, params, delta):
        self.i1 = np.asarray(g["pose_index_1"], dtype=np.int64)
        self.i2 = np.asarray(g["pose_index_2"], dtype=np.int64)
        self.cons = np.asarray(g["constraints"], dtype=np.float64).reshape(-1, 6)
        self.N, self.E = int(g["num_poses"]), len(self.i1)
        self.delta = float(delta)
        self.params = np.array(params, dtype=np.float64).reshape(-1, 6).copy()
        used = np.zeros(self.N, bool)
        used[self.i1] = True; used[self.i2] = True
        self.slot = np.full(self.N, -1)
        n = 0
        for k in range(self.N):                       # po_problem.cpp:62-63: pose1 of edge 0 is constant
            if used[k] and k != self.i1[0]:
                self.slot[k] = n; n += 6
        self.n = n
        self.kept = [e for e in range(self.E) if self.slot[self.i1[e]] >= 0 or self.slot[self.i2[e]] >= 0]
        self.fixed_cost = sum(_block(self.params[self.i1[e]], self.params[self.i2[e]], self.cons[e], self.delta, False)[5]
                              for e in range(self.E) if e not in set(self.kept))
        self.J = np.zeros((6 * len(self.kept), max(n, 1)))
        self.r = np.zeros(6 * len(self.kept))

    def scatter(self, x):
        for k in range(self.N):
            if self.slot[k] >= 0:
                self.params[k] = x[self.slot[k]:self.slot[k] + 6]

    def evaluate(self, _ctx, xp, costp, want_jac, gradp):
        x = np.ctypeslib.as_array(xp, shape=(self.n,))
        self.scatter(x)
        total = 0.0
        if want_jac:
            self.J[:] = 0.0
        for row, e in enumerate(self.kept):
            a, b = self.i1[e], self.i2[e]
            _, _, r, j1, j2, c = _block(self.params[a], self.params[b], self.cons[e], self.delta, bool(want_jac))
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

    def sq_col_norm(self, _ctx, outp):
        np.ctypeslib.as_array(outp, shape=(self.n,))[:] = (self.J * self.J).sum(axis=0)

    def scale_cols(self, _ctx, sp):
        self.J *= np.ctypeslib.as_array(sp, shape=(self.n,))[None, :]

    def solve(self, _ctx, dp, yp):
        d = np.ctypeslib.as_array(dp, shape=(self.n,))
        H = np.ascontiguousarray(self.J.T @ self.J + np.diag(d * d))
        if pyoracle.lib().oracle_dense_cholesky(pyoracle._dp(H), self.n):
            return 1
        y = np.ascontiguousarray(self.J.T @ self.r)
        pyoracle.lib().oracle_dense_cholesky_solve(pyoracle._dp(H), self.n, pyoracle._dp(y))
        np.ctypeslib.as_array(yp, shape=(self.n,))[:] = y
        return 0

    def model_cost_change(self, _ctx, sp):
        m = self.J @ np.ctypeslib.as_array(sp, shape=(self.n,))
        return -float(m @ (self.r + 0.5 * m))


def po_solve(g, po_huber_delta=0.0, params=None, trace_cap=256, **opt):
    """The pose graph through oracle_lm_minimize with HuberLoss(po_huber_delta) on every edge (0: no loss).
    Returns (params_out, summary dict, trace list) as pyoracle.po_solve does."""
    L = pyoracle.lib()
    L.oracle_dense_cholesky.argtypes = [_DP, C.c_int]
    L.oracle_dense_cholesky_solve.argtypes = [_DP, C.c_int, _DP]
    L.oracle_lm_minimize.argtypes = [C.POINTER(_NLLS), C.POINTER(pyoracle.LMOptions), _DP, C.POINTER(pyoracle.Summary),
                                     C.POINTER(pyoracle.Iteration), C.c_int, C.POINTER(C.c_int)]
    x0 = np.array(g["parameters"] if params is None else params, dtype=np.float64).reshape(-1).copy()
    P = _Problem(g, x0, po_huber_delta)
    s = pyoracle.Summary()
    tr = (pyoracle.Iteration * trace_cap)()
    nt = C.c_int(0)
    s.fixed_cost = P.fixed_cost
    s.num_free_parameters = P.n
    s.num_residual_blocks = len(P.kept)
    if P.E == 0 or P.n == 0:
        s.initial_cost = s.final_cost = P.fixed_cost
        s.termination_type = 2                       # ORACLE_FUNCTION_TOLERANCE, as oracle_po_solve answers
        return x0, dict(pyoracle._summary_dict(s), rc=0), []
    x = np.zeros(P.n)
    for k in range(P.N):
        if P.slot[k] >= 0:
            x[P.slot[k]:P.slot[k] + 6] = x0[6 * k:6 * k + 6]
    cbs = (_EVAL(P.evaluate), _VEC(P.sq_col_norm), _VEC(P.scale_cols), _SOLVE(P.solve), _MODEL(P.model_cost_change))
    nl = _NLLS(P.n, None, *cbs)
    o = pyoracle.default_options(**opt)
    rc = L.oracle_lm_minimize(C.byref(nl), C.byref(o), pyoracle._dp(x), C.byref(s), tr, trace_cap, C.byref(nt))
    out = x0.copy()
    if s.termination_type != 4:                      # ORACLE_NUMERICAL_FAILURE leaves the parameters untouched
        for k in range(P.N):
            if P.slot[k] >= 0:
                out[6 * k:6 * k + 6] = x[P.slot[k]:P.slot[k] + 6]
    return out, dict(pyoracle._summary_dict(s), rc=rc), pyoracle._trace_list(tr, min(nt.value, trace_cap))


def edge_report(g, params, po_huber_delta=0.0):
    """(sq_norm[E], weight[E]) at params: |Te|^2 of every edge and rho'(s) (1 for inliers and when there is no loss)."""
    x = np.asarray(params, dtype=np.float64).reshape(-1, 6)
    cons = np.asarray(g["constraints"], dtype=np.float64).reshape(-1, 6)
    sq, w = [], []
    for a, b, c in zip(g["pose_index_1"], g["pose_index_2"], cons):
        s, rho1 = _block(x[a], x[b], c, float(po_huber_delta), False)[:2]
        sq.append(s); w.append(rho1)
    return np.array(sq), np.array(w)

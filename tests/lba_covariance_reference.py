"""numpy reference for the posterior covariances of an LBA window (include/slslam_hip.h: slslam_lba_batch_covariance).

With J the Jacobian of all residual blocks w.r.t. the free parameter blocks (after the Huber corrector, no Jacobi scaling, no damping)
and H = J^T J split into cameras (c) and lines (l), the library returns Σ_cc = (H_cc - Σ_l H_cl H_ll^-1 H_lc)^-1 and, per free line,
Σ_ll = H_ll^-1 + K Σ_cc K^T with K = H_ll^-1 H_lc: the camera block and the lines' diagonal blocks of (J^T J)^-1.  Two routes to the
same numbers, so that their difference says how well the numbers are determined at all:
  (a) cov_qr:    QR of the dense J, (J^T J)^-1 = R^-1 R^-T - never forms J^T J;
  (b) cov_schur: the Schur route above, every H_ll and S factored by Cholesky after symmetric scaling to unit diagonal (the
                 route the device takes), which also yields
  (c) the smallest unit-diagonal pivots of S and of the lines' blocks (the quantity the SINGULAR rule tests against 1e-10);
  (d) either route on caller-supplied Jacobian blocks (the device's own, from slslam_lba_batch_linearise) instead of the oracle's.
A camera / line is free iff it is observed and no observation flags it constant (oracle/lba_oracle.c, the rule of the solve).
"""
import numpy as np

from oracle import pyoracle

PIVOT_MIN = 1e-10        # the library's SINGULAR threshold


def free_sets(w):
    """(free cameras, free lines): ascending caller indices."""
    cam = np.asarray(w["camera_index"], dtype=np.int64)
    line = np.asarray(w["line_index"], dtype=np.int64)
    fixed = np.asarray(w["fixed_index"], dtype=np.int64).reshape(-1, 2)
    fc = sorted(set(cam.tolist()) - set(cam[fixed[:, 0] != 0].tolist()))
    fl = sorted(set(line.tolist()) - set(line[fixed[:, 1] != 0].tolist()))
    return np.array(fc, dtype=np.int64), np.array(fl, dtype=np.int64)


def oracle_jacobians(w, x, huber_delta):
    """(jc [M, 4, 6], jl [M, 4, 4]) of the oracle at x, after the Huber corrector."""
    _, _, jc, jl = pyoracle.lba_cost(w, x, huber_delta, want_jac=True)
    return jc, jl


def _slots(w):
    fc, fl = free_sets(w)
    cslot = -np.ones(int(w["num_cameras"]), dtype=np.int64)
    cslot[fc] = np.arange(len(fc))
    lslot = -np.ones(int(w["num_lines"]), dtype=np.int64)
    lslot[fl] = np.arange(len(fl))
    return fc, fl, cslot, lslot


def dense_jacobian(w, jc, jl):
    """J [4M, 6F + 4Lf]: cameras first (free_camera order), then the free lines (ascending)."""
    fc, fl, cslot, lslot = _slots(w)
    cam = np.asarray(w["camera_index"], dtype=np.int64)
    line = np.asarray(w["line_index"], dtype=np.int64)
    M, F = len(cam), len(fc)
    J = np.zeros((4 * M, 6 * F + 4 * len(fl)))
    for i in range(M):
        if cslot[cam[i]] >= 0:
            J[4 * i:4 * i + 4, 6 * cslot[cam[i]]:6 * cslot[cam[i]] + 6] = jc[i]
        if lslot[line[i]] >= 0:
            c0 = 6 * F + 4 * lslot[line[i]]
            J[4 * i:4 * i + 4, c0:c0 + 4] = jl[i]
    return J


def _line_blocks(full, w, F, fl):
    out = np.zeros((int(w["num_lines"]), 4, 4))
    for s, l in enumerate(fl):
        c0 = 6 * F + 4 * s
        out[l] = full[c0:c0 + 4, c0:c0 + 4]
    return out


def cov_qr(w, jc, jl):
    """Route (a) / (d): (Σ_cc [6F, 6F], Σ_ll [L, 4, 4] with zeros for lines that are not free) from the QR factor of J."""
    fc, fl = free_sets(w)
    J = dense_jacobian(w, jc, jl)
    R = np.linalg.qr(J, mode="r")
    Rinv = np.linalg.solve(R, np.eye(R.shape[0]))
    full = Rinv @ Rinv.T
    F = len(fc)
    return full[:6 * F, :6 * F].copy(), _line_blocks(full, w, F, fl)


def scaled_cholesky(A):
    """Cholesky of A scaled to unit diagonal.  Returns (d, L, pivots): d = 1 / sqrt(diag A), L the factor of d A d as far as it got,
    pivots the values under the square roots, up to and including the first that is not positive."""
    n = A.shape[0]
    diag = np.diag(A).copy()
    if n and diag.min() <= 0.0:
        return None, None, np.array([diag.min()])
    d = 1.0 / np.sqrt(diag)
    B = A * d[:, None] * d[None, :]
    L = np.zeros_like(B)
    piv = []
    for k in range(n):
        p = B[k, k] - L[k, :k] @ L[k, :k]
        piv.append(p)
        if p <= 0.0:
            break
        L[k, k] = np.sqrt(p)
        L[k + 1:, k] = (B[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return d, L, np.array(piv)


def _inverse_from(d, L):
    X = np.linalg.solve(L, np.eye(L.shape[0]))           # L^-1
    return (X.T @ X) * d[:, None] * d[None, :]


def cov_schur(w, jc, jl, want_cov=True):
    """Route (b) and (c): (Σ_cc, Σ_ll [L, 4, 4], smallest pivot of S, smallest pivot over the lines' blocks).  Σ are None when a
    factorisation broke down (a pivot <= 0) or want_cov is False."""
    fc, fl, cslot, lslot = _slots(w)
    cam = np.asarray(w["camera_index"], dtype=np.int64)
    line = np.asarray(w["line_index"], dtype=np.int64)
    F, n = len(fc), 6 * len(fc)
    Hcc = np.zeros((n, n))
    Hll = np.zeros((len(fl), 4, 4))
    Hlc = np.zeros((len(fl), 4, n))
    for i in range(len(cam)):
        cs, ls = cslot[cam[i]], lslot[line[i]]
        if cs >= 0:
            Hcc[6 * cs:6 * cs + 6, 6 * cs:6 * cs + 6] += jc[i].T @ jc[i]
        if ls >= 0:
            Hll[ls] += jl[i].T @ jl[i]
            if cs >= 0:
                Hlc[ls][:, 6 * cs:6 * cs + 6] += jl[i].T @ jc[i]
    S = Hcc.copy()
    Hinv = np.zeros_like(Hll)
    piv_l, ok = np.inf, True
    for s in range(len(fl)):
        d, L, piv = scaled_cholesky(Hll[s])
        piv_l = min(piv_l, piv.min())
        if piv.min() <= 0.0:
            ok = False
            continue
        Hinv[s] = _inverse_from(d, L)
        S -= Hlc[s].T @ Hinv[s] @ Hlc[s]
    d, L, piv = scaled_cholesky(S)
    piv_s = piv.min() if n else np.inf
    if not ok or (n and piv.min() <= 0.0) or not want_cov:
        return None, None, piv_s, piv_l
    Scc = _inverse_from(d, L) if n else np.zeros((0, 0))
    Sll = np.zeros((int(w["num_lines"]), 4, 4))
    for s, l in enumerate(fl):
        K = Hinv[s] @ Hlc[s]
        Sll[l] = Hinv[s] + K @ Scc @ K.T
    return Scc, Sll, piv_s, piv_l


def hessian(w, jc, jl):
    J = dense_jacobian(w, jc, jl)
    return J.T @ J


def rel_cameras(a, b):
    """Largest entry of a - b relative to the largest entry of b."""
    return float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0


def rel_lines(a, b):
    """Largest over the lines' 4 x 4 blocks of (largest entry of a_l - b_l relative to the largest entry of b_l); blocks of b that are
    zero (lines that are not free) must be zero in a too."""
    worst = 0.0
    for al, bl in zip(a, b):
        m = np.abs(bl).max()
        if m == 0.0:
            worst = max(worst, 0.0 if not np.abs(al).max() else np.inf)
        else:
            worst = max(worst, float(np.abs(al - bl).max() / m))
    return worst


def perturbed(x, rel=1e-13, seed=0):
    """x with every entry moved by a relative `rel`, random signs (fixed seed): the yardstick tests/test_gpu_lba.py uses for solves."""
    rng = np.random.default_rng(seed)
    return np.asarray(x, dtype=np.float64) * (1.0 + rel * rng.choice([-1.0, 1.0], size=np.shape(x)))


def reference(w, x, huber_delta, with_perturb=False):
    """Everything the tests need for window w at point x: free sets, both routes on the oracle's Jacobians, their difference
    (d_route, floor 1e-13), the pivots, and - with_perturb - the movement of route (a) under a 1e-13 relative change of x."""
    jc, jl = oracle_jacobians(w, x, huber_delta)
    fc, fl = free_sets(w)
    qc, ql = cov_qr(w, jc, jl)
    sc, sl, piv_s, piv_l = cov_schur(w, jc, jl)
    out = dict(free_cameras=fc, free_lines=fl, qr=(qc, ql), schur=(sc, sl), piv_s=piv_s, piv_l=piv_l,
               d_route_cam=max(rel_cameras(sc, qc), 1e-13), d_route_line=max(rel_lines(sl, ql), 1e-13))
    if with_perturb:
        pc, pl = cov_qr(w, *oracle_jacobians(w, perturbed(x), huber_delta))
        out["d_perturb_cam"], out["d_perturb_line"] = rel_cameras(pc, qc), rel_lines(pl, ql)
    return out


def with_constant_lines(w, every=4):
    """w with every `every`-th line flagged constant in all its observations (a line of the map that the window does not move)."""
    out = dict(w)
    fixed = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    fixed[np.asarray(w["line_index"]) % every == 1, 1] = 1
    out["fixed_index"] = fixed.reshape(-1)
    return out


HUBER = 1.0 / 406.05


def cases():
    """The windows of tests/test_gpu_lba_covariance.py: name -> (window, huber_delta, well posed)."""
    from slslam_amd import synth
    return {
        "free2": (synth.make_window(1, num_lines=40, num_kf=4, num_free=2), HUBER, True),             # the smallest general case
        "free10": (synth.make_window(3, num_lines=300, num_kf=20, num_free=10), HUBER, True),          # the bench shape's 60 x 60
        "free12": (synth.make_window(5, num_lines=200, num_kf=24, num_free=12), HUBER, True),          # 72 > 64: past a wave and a tile
        "free20": (synth.make_window(8, num_lines=200, num_kf=24, num_free=20), HUBER, True),          # the LDS ceiling, 120 x 120
        "motion_only": (synth.make_motion_only(6, num_lines=30), HUBER, True),                        # the fused path
        "all_free": (synth.make_window(4, num_lines=40, num_kf=4, num_free=4, all_free=True), HUBER, False),    # gauge-singular
        "constant_lines": (with_constant_lines(synth.make_window(2, num_lines=60, num_kf=6, num_free=3)), HUBER, True),
        "no_huber": (synth.make_window(9, num_lines=50, num_kf=5, num_free=3), 0.0, True),
    }

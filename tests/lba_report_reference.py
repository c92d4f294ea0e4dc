"""numpy reference for the report on an LBA window (include/slslam_hip.h: slslam_lba_batch_report).

Per observation s = |r|^2 of the four raw residuals and the Huber weight rho'(s); per line and per camera the counts, sum s and
cost = sum rho(s) / 2; per free line min_pivot, the smallest value under the square roots of the Cholesky factorisation of
H_ll = sum J_l^T J_l (J_l after the corrector) scaled to unit diagonal - lba_covariance_reference.scaled_cholesky's `pivots`.
Built on the oracle: pyoracle.line_residual for the raw residuals, pyoracle.huber for rho, pyoracle.lba_cost(..., want_jac=True) for
the Jacobians (or caller-supplied ones: the device's own from LBABatch.linearise)."""
import numpy as np

from oracle import pyoracle
import lba_covariance_reference as ref

FREE, CONSTANT, NO_OBSERVATIONS = 0, 1, 2


def raw_sq_norms(w, x):
    """s [M]: |r|^2 of every observation's four raw residuals at x."""
    x = np.asarray(x, dtype=np.float64)
    cam = np.asarray(w["camera_index"], dtype=np.int64)
    line = np.asarray(w["line_index"], dtype=np.int64)
    obs = np.asarray(w["observations"], dtype=np.float64).reshape(-1, 8)
    C = int(w["num_cameras"])
    base = float(w.get("baseline", 0.12))
    s = np.zeros(len(cam))
    for i in range(len(cam)):
        r = pyoracle.line_residual(x[6 * cam[i]:6 * cam[i] + 6], x[6 * C + 4 * line[i]:6 * C + 4 * line[i] + 4], obs[i], base)
        s[i] = float(r @ r)
    return s


def huber_weights(s, a):
    """(weight rho'(s), cost rho(s) / 2) per observation, from the oracle's loss (a <= 0: none)."""
    s = np.asarray(s, dtype=np.float64)
    if a <= 0.0:
        return np.ones_like(s), 0.5 * s
    rho = np.array([pyoracle.huber(v, a) for v in s]).reshape(-1, 3)
    return rho[:, 1].copy(), 0.5 * rho[:, 0]


def huber_margin(s, a):
    """Smallest |s - a^2| / a^2 over the observations (inf without a loss): how far every observation is from the corner."""
    if a <= 0.0 or len(s) == 0:
        return np.inf
    return float(np.abs(np.asarray(s) - a * a).min() / (a * a))


def report(w, x, huber_delta, jl=None, sq_norm=None):
    """dict(sq_norm, weight, cost_obs, lines, cameras): lines / cameras are dicts of arrays status, num_observations, num_downweighted,
    sq_norm_sum, cost (+ min_pivot for the lines).  jl [M, 4, 4]: the line Jacobians after the corrector (default: the oracle's at x);
    sq_norm [M]: the observations' |r|^2 (default: the oracle's at x) - with the device's own, the sums are sums of the device's terms."""
    cam = np.asarray(w["camera_index"], dtype=np.int64)
    line = np.asarray(w["line_index"], dtype=np.int64)
    fixed = np.asarray(w["fixed_index"], dtype=np.int64).reshape(-1, 2)
    C, L = int(w["num_cameras"]), int(w["num_lines"])
    s = raw_sq_norms(w, x) if sq_norm is None else np.asarray(sq_norm, dtype=np.float64)
    wt, cost = huber_weights(s, huber_delta)
    if jl is None:
        _, jl = ref.oracle_jacobians(w, x, huber_delta)

    def sums(index, n, flag):
        out = dict(status=np.zeros(n, dtype=np.int64), num_observations=np.zeros(n, dtype=np.int64), num_downweighted=np.zeros(n, dtype=np.int64),
                   sq_norm_sum=np.zeros(n), cost=np.zeros(n))
        for k in range(n):
            sel = index == k
            out["num_observations"][k] = int(sel.sum())
            out["num_downweighted"][k] = int((wt[sel] < 1.0).sum())
            out["sq_norm_sum"][k] = float(s[sel].sum())
            out["cost"][k] = float(cost[sel].sum())
            out["status"][k] = NO_OBSERVATIONS if not sel.any() else CONSTANT if flag[sel].any() else FREE
        return out

    lines = sums(line, L, fixed[:, 1] != 0)
    cams = sums(cam, C, fixed[:, 0] != 0)
    lines["min_pivot"] = np.zeros(L)
    for l in range(L):
        if lines["status"][l] != FREE:
            continue
        H = np.zeros((4, 4))
        for i in np.nonzero(line == l)[0]:
            H += jl[i].T @ jl[i]
        lines["min_pivot"][l] = ref.scaled_cholesky(H)[2].min()
    return dict(sq_norm=s, weight=wt, cost_obs=cost, lines=lines, cameras=cams)


def with_extra_line(w, u, cam, obs, fixed=(0, 0)):
    """w with one more line (parameters u[4]) observed once by camera `cam` with observation obs[8]; the new line's index is the old L."""
    out = dict(w)
    C, L = int(w["num_cameras"]), int(w["num_lines"])
    out["num_lines"] = L + 1
    out["camera_index"] = np.append(np.asarray(w["camera_index"]), cam).astype(np.int32)
    out["line_index"] = np.append(np.asarray(w["line_index"]), L).astype(np.int32)
    out["fixed_index"] = np.append(np.asarray(w["fixed_index"]).reshape(-1), fixed).astype(np.int32)
    out["observations"] = np.append(np.asarray(w["observations"], dtype=np.float64).reshape(-1), obs)
    out["parameters"] = np.append(np.asarray(w["parameters"], dtype=np.float64), u)
    return out


def schur_pivot_without_degenerate_lines(w, x, huber_delta, min_pivot):
    """Smallest unit-diagonal pivot of S when the lines whose min_pivot[l] <= PIVOT_MIN are held constant (they add to H_cc only, as the
    report's reader would flag them): is S itself well-posed?  (cov_schur inverts a block whose pivot is tiny but positive, which
    says nothing about S.)"""
    out = dict(w)
    fixed = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    bad = np.nonzero(np.asarray(min_pivot) <= ref.PIVOT_MIN)[0]
    fixed[np.isin(np.asarray(w["line_index"]), bad), 1] = 1
    out["fixed_index"] = fixed.reshape(-1)
    jc, jl = ref.oracle_jacobians(out, x, huber_delta)
    return ref.cov_schur(out, jc, jl, want_cov=False)[2]

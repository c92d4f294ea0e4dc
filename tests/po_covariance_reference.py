"""numpy reference for the posterior covariances of a pose graph (include/slslam_hip.h: slslam_po_covariance, slslam_po_batch_covariance).

J is assembled from the oracle's own residual functor (oracle_pose_residual_jet) with the corrector of tests/po_robust_reference._block:
the Jacobian of every edge's six residuals w.r.t. the free poses (referenced and not pose_index_1[0]), free poses in index order, no
Jacobi scaling, no damping.  Sigma = (J^T J)^-1 by two routes - the inverse of the normal matrix, and R^-1 R^-T from the QR factorisation of
J, which never forms J^T J - and a yardstick y per graph for what an independent evaluation may differ by.  TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_robust_reference as robust  # noqa: E402

PIVOT_MIN = 1e-10                                    # the singular rule of the C ABI


def slots(g):
    """(slot[N], n): offset of every free pose among the unknowns, -1 for the constant pose and poses no edge references."""
    i1, i2 = np.asarray(g["pose_index_1"], dtype=np.int64), np.asarray(g["pose_index_2"], dtype=np.int64)
    N = int(g["num_poses"])
    used = np.zeros(N, bool)
    used[i1] = True; used[i2] = True
    slot = np.full(N, -1)
    n = 0
    for k in range(N):
        if used[k] and len(i1) and k != i1[0]:
            slot[k] = n; n += 6
    return slot, n


def jacobian(g, params, delta=0.0):
    """J [6 E, n] at params, after the Huber corrector of delta (0: none)."""
    slot, n = slots(g)
    x = np.asarray(params, dtype=np.float64).reshape(-1, 6)
    cons = np.asarray(g["constraints"], dtype=np.float64).reshape(-1, 6)
    E = len(cons)
    J = np.zeros((6 * E, n))
    for e, (a, b) in enumerate(zip(g["pose_index_1"], g["pose_index_2"])):
        _, _, _, j1, j2, _ = robust._block(x[a], x[b], cons[e], float(delta), True)
        if slot[a] >= 0:
            J[6 * e:6 * e + 6, slot[a]:slot[a] + 6] = j1
        if slot[b] >= 0:
            J[6 * e:6 * e + 6, slot[b]:slot[b] + 6] = j2
    return J


def smallest_pivot(H):
    """The smallest pivot of the Cholesky factorisation of H scaled to unit diagonal; the factorisation stops at the first pivot
    <= PIVOT_MIN and returns it (what follows a vanished pivot means nothing)."""
    d = 1.0 / np.sqrt(np.diag(H))
    A = H * d[:, None] * d[None, :]
    n = len(A)
    least = np.inf
    for k in range(n):
        piv = A[k, k]
        least = min(least, piv)
        if not piv > PIVOT_MIN:
            return piv
        col = A[k + 1:, k] / piv
        A[k + 1:, k + 1:] -= np.outer(col, A[k + 1:, k])
    return least


def _route1(J):
    return np.linalg.inv(J.T @ J)


def _route2(J):
    R = np.linalg.qr(J, mode="r")
    Ri = np.linalg.solve(R, np.eye(R.shape[0]))
    return Ri @ Ri.T


def covariance(g, params, delta=0.0, want_yardstick=True):
    """dict(sigma [n, n] (route 1), slot, n, pivot, r, c, y).  r: the two routes' difference, c: the largest change of route 1 over five
    random +-1 ulp relative perturbations of J's entries, both relative to max |Sigma|; y = max(r, c).  A graph whose pivot is
    <= PIVOT_MIN has sigma = None."""
    slot, n = slots(g)
    J = jacobian(g, params, delta)
    piv = smallest_pivot(J.T @ J)
    out = dict(slot=slot, n=n, pivot=piv, sigma=None, r=None, c=None, y=None)
    if not piv > PIVOT_MIN:
        return out
    s1 = _route1(J)
    out["sigma"] = s1
    if want_yardstick:
        top = np.abs(s1).max()
        out["r"] = np.abs(s1 - _route2(J)).max() / top
        rng = np.random.default_rng(2024)
        eps = np.finfo(np.float64).eps
        out["c"] = max(np.abs(_route1(J * (1.0 + eps * rng.choice([-1.0, 1.0], size=J.shape))) - s1).max() for _ in range(5)) / top
        out["y"] = max(out["r"], out["c"])
    return out


def blocks(ref, num_poses, pairs):
    """(cov_poses [N, 6, 6], cov_pairs [P, 6, 6]) of a covariance() result, as the C ABI lays them out (zeros for a singular graph)."""
    slot, S = ref["slot"], ref["sigma"]
    cp, cq = np.zeros((num_poses, 6, 6)), np.zeros((len(pairs), 6, 6))
    if S is None:
        return cp, cq
    for k in range(num_poses):
        if slot[k] >= 0:
            cp[k] = S[slot[k]:slot[k] + 6, slot[k]:slot[k] + 6]
    for q, (a, b) in enumerate(pairs):
        if slot[a] >= 0 and slot[b] >= 0:
            cq[q] = S[slot[a]:slot[a] + 6, slot[b]:slot[b] + 6]
    return cp, cq

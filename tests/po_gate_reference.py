"""numpy reference for the statistics of a pose-graph edge under the posterior covariance of its two poses (include/slslam_hip.h:
slslam_po_edge_statistics, slslam_po_gate, slslam_po_batch_gate).

Te, Ja, Jb come from the oracle's own residual functor (oracle_pose_residual_jet), Sigma from tests/po_covariance_reference.covariance
(tests/po_weighted_reference.covariance for a weighted graph).  S = sigma2 (Ja Saa Ja^T + Jb Sbb Jb^T + Ja Sab Jb^T + Jb Sab^T Ja^T) + R;
W by the C ABI's rule (Cholesky after scaling to unit diagonal, a scaled pivot <= 1e-10: singular); m2 independently by np.linalg.solve.

The yardstick y per quantity, as po_covariance_reference builds it: the larger of (r) the difference between two routes - S as the four
terms against [Ja|Jb] Sigma12 [Ja|Jb]^T, W by the scaled Cholesky against the inverse of numpy's unscaled factor, m2 = |W Te|^2 against
Te . solve(S, Te) - and (c) the largest movement of the first route over five random +-1 ulp perturbations of the entries of J and
Sigma (the edge error itself is moved by +-1 ulp on the entries of the poses and the constraint it is a difference of).  No yardstick
is below one ulp.  Deviations and yardsticks are relative to TOPS: max |S|, max |W|, m2 and, for the error, the largest input entry.
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402

PIVOT_MIN = cref.PIVOT_MIN
COV_OK, COV_SINGULAR = 0, 1
QUANTITIES = ("error", "cov", "sqrt_information", "mahalanobis2")


def jet(xa, xb, c):
    """(Te[6], Ja[6, 6], Jb[6, 6]) of the oracle's functor at T1 = xa, T2 = xb."""
    from oracle import pyoracle
    r, ja, jb = pyoracle.pose_residual_jet(np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64), np.asarray(c, dtype=np.float64))
    return np.array(r, dtype=np.float64), np.array(ja, dtype=np.float64).reshape(6, 6), np.array(jb, dtype=np.float64).reshape(6, 6)


def residual(xa, xb, c):
    from oracle import pyoracle
    r = np.zeros(6)
    xa, xb, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (xa, xb, c))
    pyoracle.lib().oracle_pose_residual(pyoracle._dp(xa), pyoracle._dp(xb), pyoracle._dp(c), pyoracle._dp(r))
    return r


def scaled_pivot(S):
    """The smallest pivot of the Cholesky factorisation of S scaled to unit diagonal (the first one <= PIVOT_MIN, when there is one);
    a diagonal entry <= 0 counts as that entry (at or below zero)."""
    dg = np.diag(S)
    if not (dg > 0.0).all():
        return float(min(dg.min(), 0.0))
    return cref.smallest_pivot(np.array(S, dtype=np.float64))


def sqrt_information(S):
    """W lower triangular with W^T W = S^-1, by the rule of slslam_po_sqrt_information; None when singular."""
    if not scaled_pivot(S) > PIVOT_MIN:
        return None
    d = 1.0 / np.sqrt(np.diag(S))
    Lc = np.linalg.cholesky(S * d[:, None] * d[None, :])
    return np.linalg.solve(Lc, np.eye(6)) * d[None, :]


def _s_terms(ja, jb, saa, sbb, sab, R, sigma2):
    return sigma2 * (ja @ saa @ ja.T + jb @ sbb @ jb.T + ja @ sab @ jb.T + jb @ sab.T @ ja.T) + R


def _s_joint(ja, jb, saa, sbb, sab, R, sigma2):
    J = np.hstack([ja, jb])
    return sigma2 * (J @ np.block([[saa, sab], [sab.T, sbb]]) @ J.T) + R


def _route1(te, S):
    W = sqrt_information(S)
    y = W @ te
    return W, float(y @ y)


def snippet(te, ja, jb, saa, sbb, sab, R, sigma2):
    """INTEGRATION.md's formula, verbatim: (S_e, m2)."""
    S_e = ja @ saa @ ja.T + jb @ sbb @ jb.T + ja @ sab @ jb.T + jb @ sab.T @ ja.T
    S_e = sigma2 * S_e + R
    return S_e, float(te @ np.linalg.solve(S_e, te))


def edge_statistics(xa, xb, c, saa=None, sbb=None, sab=None, R=None, sigma2=1.0, want_yardstick=True):
    """One item: dict(status, error, cov, sqrt_information, mahalanobis2, pivot, tops{quantity}, y{quantity}) - zeros but for the error
    (and no yardstick) when singular."""
    z = np.zeros((6, 6))
    saa, sbb, sab, R = (z if a is None else np.asarray(a, dtype=np.float64).reshape(6, 6) for a in (saa, sbb, sab, R))
    R = np.tril(R) + np.tril(R, -1).T                                  # (the lower triangle is what the C ABI reads)
    xa, xb, c = (np.asarray(a, dtype=np.float64).reshape(6) for a in (xa, xb, c))
    te, ja, jb = jet(xa, xb, c)
    S = _s_terms(ja, jb, saa, sbb, sab, R, sigma2)
    S = 0.5 * (S + S.T)
    piv = scaled_pivot(S)
    out = dict(status=COV_OK, error=te, cov=S, sqrt_information=z.copy(), mahalanobis2=0.0, pivot=piv, tops=None, y=None)
    if not piv > PIVOT_MIN:
        out.update(status=COV_SINGULAR, cov=z.copy())
        return out
    W, m2 = _route1(te, S)
    out.update(sqrt_information=W, mahalanobis2=m2)
    if not want_yardstick:
        return out
    in_top = max(np.abs(xa).max(), np.abs(xb).max(), np.abs(c).max(), 1e-300)
    tops = dict(error=in_top, cov=np.abs(S).max(), sqrt_information=np.abs(W).max(), mahalanobis2=max(m2, 1e-300))
    # (r) the second routes
    S2 = _s_joint(ja, jb, saa, sbb, sab, R, sigma2)
    W2 = np.linalg.inv(np.linalg.cholesky(S))
    m22 = float(te @ np.linalg.solve(S, te))
    y = dict(error=np.finfo(np.float64).eps,
             cov=np.abs(S2 - S).max() / tops["cov"],
             sqrt_information=np.abs(W2 - W).max() / tops["sqrt_information"],
             mahalanobis2=abs(m22 - m2) / tops["mahalanobis2"])
    # (c) +-1 ulp on the inputs
    rng = np.random.default_rng(2024)
    eps = np.finfo(np.float64).eps

    def jig(a):
        return a * (1.0 + eps * rng.choice([-1.0, 1.0], size=a.shape))
    for _ in range(5):
        te_p = residual(jig(xa), jig(xb), jig(c))
        S_p = _s_terms(jig(ja), jig(jb), jig(saa), jig(sbb), jig(sab), R, sigma2)
        S_p = 0.5 * (S_p + S_p.T)
        W_p, m2_p = _route1(te_p, S_p)
        y["error"] = max(y["error"], np.abs(te_p - te).max() / tops["error"])
        y["cov"] = max(y["cov"], np.abs(S_p - S).max() / tops["cov"])
        y["sqrt_information"] = max(y["sqrt_information"], np.abs(W_p - W).max() / tops["sqrt_information"])
        y["mahalanobis2"] = max(y["mahalanobis2"], abs(m2_p - m2) / tops["mahalanobis2"])
    y = {q: max(v, eps) for q, v in y.items()}                          # (one ulp of the top: what the number format itself resolves)
    out.update(tops=tops, y=y)
    return out


def deviations(ref, got):
    """{quantity: d / y} of one non-singular item: got = dict(error, cov, sqrt_information, mahalanobis2) of that item."""
    return {q: float(np.abs(np.asarray(got[q]) - np.asarray(ref[q])).max() / ref["tops"][q] / ref["y"][q]) for q in QUANTITIES}


def graph_blocks(g, x, pairs, delta=0.0):
    """(cov_status, Saa[P], Sbb[P], Sab[P]) of the pairs of a graph at x: the reference covariance (the weighted one when the graph has
    sqrt_information), zeros for a singular graph."""
    if g.get("sqrt_information") is not None:
        import po_weighted_reference as wref
        ref = wref.covariance(g, x, delta)
    else:
        ref = cref.covariance(g, x, delta, want_yardstick=False)
    cp, cq = cref.blocks(ref, int(g["num_poses"]), pairs)
    a = [p[0] for p in pairs]
    b = [p[1] for p in pairs]
    return (COV_SINGULAR if ref["sigma"] is None else COV_OK), cp[a], cp[b], cq


def gate(g, x, cand, delta=0.0, blocks=None, want_yardstick=True):
    """The candidates dict(pose_a, pose_b, constraints, cov_meas?, sigma2?) against graph g at x: (cov_status, [edge_statistics ...]).
    blocks = (cov_status, Saa, Sbb, Sab): Sigma blocks to use instead of the reference covariance (e.g. the device's own)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    pairs = list(zip(cand["pose_a"], cand["pose_b"]))
    cs, saa, sbb, sab = blocks if blocks is not None else graph_blocks(g, x, pairs, delta)
    cons = np.asarray(cand["constraints"], dtype=np.float64).reshape(-1, 6)
    R = cand.get("cov_meas")
    out = []
    for k, (a, b) in enumerate(pairs):
        if cs != COV_OK:
            te = residual(x[a], x[b], cons[k])
            out.append(dict(status=COV_SINGULAR, error=te, cov=np.zeros((6, 6)), sqrt_information=np.zeros((6, 6)), mahalanobis2=0.0, pivot=0.0, tops=None, y=None))
            continue
        out.append(edge_statistics(x[a], x[b], cons[k], saa[k], sbb[k], sab[k], None if R is None else np.asarray(R).reshape(-1, 6, 6)[k],
                                   float(cand.get("sigma2", 1.0)), want_yardstick))
    return cs, out


# ------------------------------------------------------------------------------------------------ the cases the GPU tests use
def primitive_items(n, seed=31):
    """n items for slslam_po_edge_statistics: dict(pose_a, pose_b, constraints, cov_aa, cov_bb, cov_ab, cov_meas, sigma2, singular[n]).
    Random poses a few metres apart, a joint 12 x 12 covariance A A^T / 12 scaled to centimetres and milliradians, R likewise.  Item 0
    has pose_a at exactly zero rotation (the small-angle branch); item 3 (when there is one) has every covariance zero: singular."""
    rng = np.random.default_rng(np.random.SeedSequence([17, int(seed), int(n)]))
    xa = np.concatenate([rng.uniform(-0.8, 0.8, (n, 3)), rng.uniform(-4, 4, (n, 3))], axis=1)
    xb = np.concatenate([rng.uniform(-0.8, 0.8, (n, 3)), rng.uniform(-4, 4, (n, 3))], axis=1)
    xa[0, :3] = 0.0
    cons = np.concatenate([rng.uniform(-0.6, 0.6, (n, 3)), rng.uniform(-3, 3, (n, 3))], axis=1)
    sc = np.array([2e-3] * 3 + [1e-2] * 3)
    saa, sbb, sab, R = (np.zeros((n, 6, 6)) for _ in range(4))
    for k in range(n):
        A = rng.normal(size=(12, 12)) * np.concatenate([sc, sc])[:, None]
        Sig = A @ A.T / 12.0
        saa[k], sbb[k], sab[k] = Sig[:6, :6], Sig[6:, 6:], Sig[:6, 6:]
        B = rng.normal(size=(6, 6)) * sc[:, None]
        R[k] = B @ B.T / 6.0 + np.diag(sc * sc)
    singular = np.zeros(n, bool)
    if n > 3:
        saa[3] = sbb[3] = sab[3] = R[3] = 0.0
        singular[3] = True
    return dict(pose_a=xa, pose_b=xb, constraints=cons, cov_aa=saa, cov_bb=sbb, cov_ab=sab, cov_meas=R, sigma2=1.7, singular=singular)


def primitive_reference(items, use=("cov_aa", "cov_bb", "cov_ab", "cov_meas")):
    """[edge_statistics ...] of primitive_items(), with only the covariance arrays named in `use` (the others: None)."""
    n = len(items["pose_a"])
    pick = {k: (items[k] if k in use else [None] * n) for k in ("cov_aa", "cov_bb", "cov_ab", "cov_meas")}
    return [edge_statistics(items["pose_a"][k], items["pose_b"][k], items["constraints"][k], pick["cov_aa"][k], pick["cov_bb"][k],
                            pick["cov_ab"][k], pick["cov_meas"][k], items["sigma2"]) for k in range(n)]


def relative_pose(xa, xb):
    """The constraint an edge (a, b) meets exactly: Te(xa, xb, C) = 0, C = T_b o T_a^-1 (reference src/slam.cpp:1410-1412)."""
    from slslam_amd import capi
    return capi.se3_compose(xb, capi.se3_inverse(xa))


def graph_candidates(g, x, seed=5):
    """Candidates for a solved graph: one touching the constant pose, one between two poses that share no edge, the loop closures'
    endpoints reversed - each C the solved relative pose plus noise of a centimetre / two milliradians -, R = diag of that noise."""
    N = int(g["num_poses"])
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    edges = set(zip(map(int, g["pose_index_1"]), map(int, g["pose_index_2"])))
    apart = next((a, b) for a in range(1, N) for b in range(N - 1, a, -1) if (a, b) not in edges and (b, a) not in edges)
    pairs = [(int(g["pose_index_1"][0]), N - 1), apart] + [(b, a) for a, b in sorted(edges) if b - a > 1]
    rng = np.random.default_rng(np.random.SeedSequence([23, int(seed), N]))
    sd = np.array([2e-3] * 3 + [1e-2] * 3)
    cons = np.array([relative_pose(x[a], x[b]) + rng.normal(size=6) * sd for a, b in pairs])
    R = np.tile(np.diag(sd * sd), (len(pairs), 1, 1))
    return dict(pose_a=[p[0] for p in pairs], pose_b=[p[1] for p in pairs], constraints=cons, cov_meas=R, sigma2=1.0)


def residual_variance(g, final_cost):
    """sigma2 of a solved unweighted graph: 2 final_cost / (6 E - 6 (N - 1))."""
    E, N = len(g["pose_index_1"]), int(g["num_poses"])
    return 2.0 * final_cost / (6 * E - 6 * (N - 1))


SCENARIO_SEED = 3


def scenario(g, x, final_cost, seed=SCENARIO_SEED):
    """The gating scenario on a solved graph: sigma2 its residual variance, R = sigma2 I; candidate 0 between the first loop closure's
    poses with C the solved relative pose plus seeded noise of that variance, candidate 1 the same C off by (1.5, 0, -1) m and 0.4 rad."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    s2 = residual_variance(g, final_cost)
    a, b = next((int(a), int(b)) for a, b in zip(g["pose_index_1"], g["pose_index_2"]) if b - a > 1)
    rng = np.random.default_rng(np.random.SeedSequence([29, int(seed)]))
    good = relative_pose(x[a], x[b]) + rng.normal(size=6) * np.sqrt(s2)
    bad = good.copy()
    bad[3:6] += (1.5, 0.0, -1.0)
    bad[1] += 0.4
    return dict(pose_a=[a, a], pose_b=[b, b], constraints=np.array([good, bad]), cov_meas=np.tile(s2 * np.eye(6), (2, 1, 1)), sigma2=s2)

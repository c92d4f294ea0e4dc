"""numpy reference for the covariance of an estimated frame motion and its map into an edge error's coordinates (include/slslam_hip.h:
slslam_pose_estimator_get_covariance, slslam_po_constraint_covariance).

Estimator covariance: tests/lba_covariance_reference.reference on the motion-only window the estimator packed (window_dict), at its
solved parameters - its camera block and its yardstick (d_route, d_perturb); sigma2 = 2 (cost of the kept blocks) / (4 n - 6).

J_C = dTe/dC: the oracle's pose_residual_jet gives only Ja and Jb, so the functor (reference src/po_problem.h:27-108: gc_T_inv, gc_w_20
through quaternions, gc_T_20, PoseConstraintError, with the first-order branches at zero angle) is restated here on a forward-mode dual
number with an 18-wide gradient (x_a | x_b | C); tests/test_pose_covariance_cpu.py anchors its Te, Ja, Jb to the oracle's.
R_ref = sigma2 J_C Sigma J_C^T.

The yardstick y per quantity, as po_gate_reference.edge_statistics builds it: the larger of (a) a second route - (J_C L)(J_C L)^T with L
the Cholesky factor of Sigma, against the direct product - and (b) the largest movement over five +-1 ulp jiggles of J_C and Sigma (for
J_C and the error: of the poses and the constraint they are functions of).  No yardstick is below one ulp of the quantity's top entry.
TEST INFRASTRUCTURE ONLY.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EPS = np.finfo(np.float64).eps
QUANTITIES = ("error", "jacobian", "cov_meas")


# ------------------------------------------------------------------------------------------------ forward-mode duals, 18 directions
class Dual:
    __slots__ = ("v", "g")
    WIDTH = 18

    def __init__(self, v, g=None):
        self.v = float(v)
        self.g = np.zeros(self.WIDTH) if g is None else g

    @staticmethod
    def lift(a):
        return a if isinstance(a, Dual) else Dual(a)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.v + o.v, self.g + o.g)
    __radd__ = __add__

    def __sub__(self, o):
        o = Dual.lift(o)
        return Dual(self.v - o.v, self.g - o.g)

    def __rsub__(self, o):
        return Dual.lift(o) - self

    def __neg__(self):
        return Dual(-self.v, -self.g)

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.v * o.v, self.v * o.g + o.v * self.g)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.v / o.v
        return Dual(q, (self.g - q * o.g) / o.v)


def _sin(a):
    return Dual(np.sin(a.v), np.cos(a.v) * a.g)


def _cos(a):
    return Dual(np.cos(a.v), -np.sin(a.v) * a.g)


def _sqrt(a):
    s = np.sqrt(a.v)
    return Dual(s, a.g / (2.0 * s))


def _atan2(y, x):
    return Dual(np.arctan2(y.v, x.v), (x.v * y.g - y.v * x.g) / (x.v * x.v + y.v * y.v))


def _aa_rotate(w, p):
    """ceres::AngleAxisRotatePoint: Rodrigues, first order at zero angle."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2.v > 0.0:
        th = _sqrt(th2)
        u = [w[0] / th, w[1] / th, w[2] / th]
        c, s = _cos(th), _sin(th)
        x = [u[1] * p[2] - u[2] * p[1], u[2] * p[0] - u[0] * p[2], u[0] * p[1] - u[1] * p[0]]
        dot = u[0] * p[0] + u[1] * p[1] + u[2] * p[2]
        omc = 1.0 - c
        return [p[k] * c + x[k] * s + u[k] * omc * dot for k in range(3)]
    return [p[0] + (w[1] * p[2] - w[2] * p[1]), p[1] + (w[2] * p[0] - w[0] * p[2]), p[2] + (w[0] * p[1] - w[1] * p[0])]


def _aa_to_quat(a):
    t2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    if t2.v > 0.0:
        th = _sqrt(t2)
        half = th * 0.5
        k = _sin(half) / th
        return [_cos(half), a[0] * k, a[1] * k, a[2] * k]
    return [Dual(1.0), a[0] * 0.5, a[1] * 0.5, a[2] * 0.5]


def _quat_to_aa(q):
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if s2.v > 0.0:
        st = _sqrt(s2)
        two = 2.0 * (_atan2(-st, -q[0]) if q[0].v < 0.0 else _atan2(st, q[0]))
        k = two / st
        return [q[1] * k, q[2] * k, q[3] * k]
    return [q[1] * 2.0, q[2] * 2.0, q[3] * 2.0]


def _compose(t21, t10):
    a, b = _aa_to_quat(t21[:3]), _aa_to_quat(t10[:3])
    q = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
         a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
         a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
    w = _quat_to_aa(q)
    t = _aa_rotate(t21[:3], t10[3:])
    return w + [t[k] + t21[3 + k] for k in range(3)]


def _inverse(p):
    w = [-p[0], -p[1], -p[2]]
    return w + _aa_rotate(w, [-p[3], -p[4], -p[5]])


def functor_jet(xa, xb, c):
    """(Te[6], Ja[6, 6], Jb[6, 6], Jc[6, 6]) of Te = T_b^-1 o (C o T_a): one evaluation on duals seeded on all 18 inputs."""
    vals = np.concatenate([np.asarray(a, dtype=np.float64).reshape(6) for a in (xa, xb, c)])
    seeds = np.eye(18)
    d = [Dual(vals[k], seeds[k].copy()) for k in range(18)]
    te = _compose(_inverse(d[6:12]), _compose(d[12:18], d[0:6]))
    J = np.array([t.g for t in te])
    return np.array([t.v for t in te]), J[:, 0:6].copy(), J[:, 6:12].copy(), J[:, 12:18].copy()


def functor_value(xa, xb, c):
    return functor_jet(xa, xb, c)[0]


# ------------------------------------------------------------------------------------------------ R = sigma2 J_C Sigma J_C^T
def _sym_lower(a):
    a = np.asarray(a, dtype=np.float64).reshape(6, 6)
    return np.tril(a) + np.tril(a, -1).T                         # (the lower triangle is what the C ABI reads)


def _product(jc, sig, sigma2):
    R = sigma2 * (jc @ sig @ jc.T)
    return 0.5 * (R + R.T)


def constraint_covariance(xa, xb, c, cov_constraint=None, sigma2=1.0, want_yardstick=True):
    """One item: dict(error, jacobian, cov_meas, tops{quantity}, y{quantity})."""
    xa, xb, c = (np.asarray(a, dtype=np.float64).reshape(6) for a in (xa, xb, c))
    sig = np.zeros((6, 6)) if cov_constraint is None else _sym_lower(cov_constraint)
    te, _, _, jc = functor_jet(xa, xb, c)
    R = _product(jc, sig, sigma2)
    out = dict(error=te, jacobian=jc, cov_meas=R, tops=None, y=None)
    if not want_yardstick:
        return out
    tiny = 1e-300
    tops = dict(error=max(np.abs(xa).max(), np.abs(xb).max(), np.abs(c).max(), tiny), jacobian=max(np.abs(jc).max(), tiny),
                cov_meas=max(np.abs(R).max(), tiny))
    y = dict(error=EPS, jacobian=EPS, cov_meas=EPS)
    if sig.any():                                                 # (a) the second route
        L = np.linalg.cholesky(sig)
        JL = jc @ L
        y["cov_meas"] = max(y["cov_meas"], np.abs(sigma2 * (JL @ JL.T) - R).max() / tops["cov_meas"])
    rng = np.random.default_rng(2025)

    def jig(a):
        return a * (1.0 + EPS * rng.choice([-1.0, 1.0], size=a.shape))
    for _ in range(5):                                            # (b) +-1 ulp on the inputs
        te_p, _, _, jc_p = functor_jet(jig(xa), jig(xb), jig(c))
        R_p = _product(jig(jc), _sym_lower(jig(sig)), sigma2)
        y["error"] = max(y["error"], np.abs(te_p - te).max() / tops["error"])
        y["jacobian"] = max(y["jacobian"], np.abs(jc_p - jc).max() / tops["jacobian"])
        y["cov_meas"] = max(y["cov_meas"], np.abs(R_p - R).max() / tops["cov_meas"])
    out.update(tops=tops, y=y)
    return out


def deviations(ref, got):
    """{quantity: d / y} of one item: got = dict(error, jacobian, cov_meas) of that item."""
    return {q: float(np.abs(np.asarray(got[q]) - np.asarray(ref[q])).max() / ref["tops"][q] / ref["y"][q]) for q in QUANTITIES}


def random_spd(n, seed=41, scale=1.0):
    """n covariances of (w_C, t_C): A A^T / 6 scaled to `scale` x (2 milliradians, 1 centimetre), plus that scale's diagonal."""
    rng = np.random.default_rng(np.random.SeedSequence([19, int(seed), int(n)]))
    sc = scale * np.array([2e-3] * 3 + [1e-2] * 3)
    out = np.zeros((n, 6, 6))
    for k in range(n):
        B = rng.normal(size=(6, 6)) * sc[:, None]
        out[k] = B @ B.T / 6.0 + np.diag(sc * sc)
    return out


# ------------------------------------------------------------------------------------------------ the estimator's covariance
def window_dict(num_lines, observations, parameters, camera0=None):
    """The motion-only window of n lines in the LBA array contract (reference src/slam.cpp:590-640): camera 0 free, camera 1 and every
    line constant, per line (camera 0, obs1) then (camera 1, obs0).  camera0: replaces the first six parameters (the solved camera)."""
    n = int(num_lines)
    par = np.array(parameters, dtype=np.float64).reshape(-1)[:12 + 4 * n].copy()
    if camera0 is not None:
        par[:6] = camera0
    return {"num_cameras": 2, "num_lines": n, "num_observations": 2 * n,
            "camera_index": np.tile([0, 1], n).astype(np.int32), "line_index": np.repeat(np.arange(n), 2).astype(np.int32),
            "fixed_index": np.tile([0, 1, 1, 1], n).astype(np.int32),
            "observations": np.asarray(observations, dtype=np.float64).reshape(-1, 8)[:2 * n].copy(), "parameters": par}


def motion_covariance(win, huber_delta, with_perturb=True):
    """dict(cov [6, 6] (route (a) of lba_covariance_reference), y: that file's END TO END yardstick max(d_route, d_perturb), dof, sigma2,
    ref) of a motion-only window at win["parameters"].  sigma2 = 2 (cost of the kept blocks) / dof: the oracle's cost over the blocks
    of camera 0 (after the loss), dof = 4 n - 6."""
    import lba_covariance_reference as lref
    from oracle import pyoracle
    x = np.asarray(win["parameters"], dtype=np.float64)
    ref = lref.reference(win, x, huber_delta, with_perturb=with_perturb)
    n = int(win["num_lines"])
    kept = dict(win, num_observations=n, camera_index=win["camera_index"][0::2], line_index=win["line_index"][0::2],
                fixed_index=np.asarray(win["fixed_index"]).reshape(-1, 2)[0::2].reshape(-1), observations=win["observations"][0::2])
    cost = pyoracle.lba_cost(kept, x, huber_delta)
    dof = 4 * n - 6
    y = max(ref["d_route_cam"], ref.get("d_perturb_cam", 0.0))
    return dict(cov=ref["qr"][0], y=y, dof=dof, sigma2=2.0 * cost / dof, ref=ref)


# ------------------------------------------------------------------------------------------------ the end-to-end gating scenario
SCENARIO_SEED = 3
SCENARIO_SCALE = 10.0            # the constraints' standard deviations: decimetres and 20 milliradians, above the solved graphs' own uncertainty
SCENARIO_SIGMA2 = 0.5            # the residual variance the constraints' unit-variance covariances are scaled by


def scenario(g, x, final_cost, seed=SCENARIO_SEED):
    """Loop-closure candidates for a solved graph as a motion estimator would deliver them: the pairs of po_gate_reference.graph_candidates,
    each C the solved relative pose of its two poses displaced by a draw from N(0, sigma2_c Sigma_C) (Sigma_C: random_spd), and a last
    candidate - the second pair again - displaced by 20 standard deviations along Sigma_C's best-determined axis instead.
    dict(pose_a, pose_b, constraints [M, 6], cov_constraint [M, 6, 6], sigma2_c, sigma2 (the graph's residual variance), outlier)."""
    import po_gate_reference as gref
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    base = gref.graph_candidates(g, x)
    pairs = list(zip(base["pose_a"], base["pose_b"]))
    pairs.append(pairs[1])
    M = len(pairs)
    sig = random_spd(M, seed, SCENARIO_SCALE)
    rng = np.random.default_rng(np.random.SeedSequence([37, int(seed), int(g["num_poses"])]))
    cons = np.zeros((M, 6))
    for k, (a, b) in enumerate(pairs):
        c0 = gref.relative_pose(x[a], x[b])
        if k < M - 1:
            cons[k] = c0 + np.sqrt(SCENARIO_SIGMA2) * (np.linalg.cholesky(sig[k]) @ rng.normal(size=6))
        else:
            lam, vec = np.linalg.eigh(SCENARIO_SIGMA2 * sig[k])
            cons[k] = c0 + 20.0 * np.sqrt(lam[0]) * vec[:, 0]
    return dict(pose_a=[p[0] for p in pairs], pose_b=[p[1] for p in pairs], constraints=cons, cov_constraint=sig, sigma2_c=SCENARIO_SIGMA2,
                sigma2=gref.residual_variance(g, final_cost), outlier=M - 1)


def scenario_reference(g, x, sc):
    """(candidates dict with cov_meas = R_ref, [constraint_covariance ...], (cov_status, [edge_statistics ...]) of po_gate_reference.gate)."""
    import po_gate_reference as gref
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    items = [constraint_covariance(x[a], x[b], sc["constraints"][k], sc["cov_constraint"][k], sc["sigma2_c"])
             for k, (a, b) in enumerate(zip(sc["pose_a"], sc["pose_b"]))]
    cand = dict(pose_a=sc["pose_a"], pose_b=sc["pose_b"], constraints=sc["constraints"], cov_meas=np.array([it["cov_meas"] for it in items]),
                sigma2=sc["sigma2"])
    return cand, items, gref.gate(g, x, cand)

"""The motion covariances of include/slslam_hip.h (slslam_pose_estimator_set_covariance / _get_covariance, slslam_po_constraint_covariance)
without a device: the numpy reference of tests/pose_covariance_reference.py anchored to the oracle, the definition calibrated on the
oracle alone, and the argument validation of the new C entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_gate_reference as gref  # noqa: E402
import pose_covariance_reference as pref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, STATE = 0, 1, 5
K = 100.0
EPS = np.finfo(np.float64).eps


def _anchor_items():
    """The random items of po_gate_reference.primitive_items(65), one with x_a = 0 and one with Te = 0 exactly (every zero-angle branch)."""
    it = gref.primitive_items(65)
    items = list(zip(it["pose_a"], it["pose_b"], it["constraints"]))
    items.append((np.zeros(6), it["pose_b"][1], it["constraints"][1]))
    items.append((np.zeros(6), np.zeros(6), np.zeros(6)))
    return items


def test_dual_functor_matches_the_oracle(oracle):
    worst = 0.0
    for k, (a, b, c) in enumerate(_anchor_items()):
        te, ja, jb, _ = pref.functor_jet(a, b, c)
        r, oa, ob = gref.jet(a, b, c)
        ref = gref.edge_statistics(a, b, c, R=np.eye(6))               # (R: only to have a regular S; the error's yardstick is what is used)
        y, top = ref["y"]["error"], ref["tops"]["error"]
        d = max(np.abs(te - r).max(), np.abs(ja - oa).max(), np.abs(jb - ob).max()) / top / y
        worst = max(worst, d)
        assert d <= K, (k, d)
    te = pref.functor_value(np.zeros(6), np.zeros(6), np.zeros(6))
    assert not te.any()                                                  # Te = 0 exactly
    print("dual functor against the oracle: worst d / y %.3f" % worst)


def test_jc_matches_central_differences(oracle):
    """Central differences of the oracle's residual at h = 1e-6 are accurate to their truncation h^2 M3 (M3: the largest third
    derivative, estimated below by differences at H = 1e-2 and printed; the usual 1/6 is left out) plus their rounding: the two
    residuals each carry an evaluation error of up to K y top - what test_dual_functor_matches_the_oracle accepts between two
    evaluations of Te - divided by h.  At h = 1e-6 the rounding term is the larger one (measured: deviation 1.5e-9, h^2 M3 5e-12)."""
    h, H = 1e-6, 1e-2
    it = gref.primitive_items(65)
    m3, rows = 0.0, []
    for a, b, c in zip(it["pose_a"], it["pose_b"], it["constraints"]):
        jc = pref.functor_jet(a, b, c)[3]
        ref = gref.edge_statistics(a, b, c, R=np.eye(6))
        for d in range(6):
            e = np.zeros(6); e[d] = 1.0
            cd = (gref.residual(a, b, c + h * e) - gref.residual(a, b, c - h * e)) / (2 * h)
            f3 = (gref.residual(a, b, c + 2 * H * e) - 2 * gref.residual(a, b, c + H * e) + 2 * gref.residual(a, b, c - H * e)
                  - gref.residual(a, b, c - 2 * H * e)) / (2 * H ** 3)
            m3 = max(m3, np.abs(f3).max())
            rows.append((np.abs(cd - jc[:, d]).max(), K * ref["y"]["error"] * ref["tops"]["error"] / h))
    worst = max(r[0] for r in rows)
    print("J_C against central differences: largest third derivative %.3f, h^2 M3 %.3e, worst deviation %.3e, rounding term >= %.3e" % (
        m3, h * h * m3, worst, min(r[1] for r in rows)))
    for dev, rounding in rows:
        assert dev <= h * h * m3 + rounding


def test_identity_constraint_has_zero_error():
    it = gref.primitive_items(11)
    for c in it["constraints"]:
        te = pref.functor_value(np.zeros(6), c, c)
        assert np.abs(te).max() <= K * EPS * np.abs(c).max()             # x_a = 0, x_b = C: Te = 0 up to rounding


def test_covariance_definition_is_calibrated(oracle):
    """N outlier-free synthetic frames with Gaussian endpoint noise, Huber off, solved by the oracle from the true motion: the parameter
    error e of the solved camera under sigma2 Sigma is chi-square with 6 degrees of freedom, and sigma2 estimates the injected variance."""
    N, lines, noise_px, focal = 120, 60, 0.5, 406.05
    m2, s2 = [], []
    for i in range(N):
        fr = synth.make_ransac_pair(5000 + i, num_lines=lines, noise_px=noise_px, outlier_frac=0.0, num_trials=1)
        T = fr["true_pose"]
        truth = np.concatenate([synth.log_so3(T[:9].reshape(3, 3)), T[9:]])
        par = np.concatenate([truth, np.zeros(6)] + [oracle.av_to_orth(l) for l in fr["lines"]])
        win = pref.window_dict(lines, np.stack([fr["obs1"], fr["obs0"]], axis=1).reshape(-1, 8), par)
        x, s, _ = oracle.lba_solve(win, huber_delta=0.0, linear_solver=1)
        ref = pref.motion_covariance(dict(win, parameters=x), 0.0, with_perturb=False)
        assert abs(ref["sigma2"] - 2.0 * (s["final_cost"] - s["fixed_cost"]) / ref["dof"]) <= 1e-9 * ref["sigma2"]
        e = x[:6] - truth
        m2.append(float(e @ np.linalg.solve(ref["sigma2"] * ref["cov"], e)))
        s2.append(ref["sigma2"])
    injected = (noise_px / focal) ** 2
    print("calibration: N %d  mean m2 %.3f (6 +- %.3f)  mean sigma2 / injected %.4f" % (N, np.mean(m2), 5 * np.sqrt(12.0 / N), np.mean(s2) / injected))
    assert abs(np.mean(m2) - 6.0) <= 5.0 * np.sqrt(12.0 / N)
    assert abs(np.mean(s2) / injected - 1.0) <= 0.10


def test_scenario_separates_on_the_reference(oracle):
    """The end-to-end scenario of tests/test_gpu_pose_covariance.py, on the reference alone: the candidate displaced by 20 standard
    deviations is beyond the 99 % point of chi-square(6), the honest ones are below it."""
    for shape in ((4, 1), (12, 2)):
        g = synth.make_pose_graph(7, *shape)
        x, s, _ = oracle.po_solve(g, linear_solver=2)
        sc = pref.scenario(g, x, s["final_cost"])
        _, _, (cs, refs) = pref.scenario_reference(g, x, sc)
        m2 = np.array([r["mahalanobis2"] for r in refs])
        print("scenario N %d loops %d: m2 %s" % (shape + (np.round(m2, 2),)))
        assert cs == 0 and all(r["status"] == 0 for r in refs)
        assert m2[sc["outlier"]] > 16.8 and (np.delete(m2, sc["outlier"]) < 16.8).all()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_symbols_and_struct_layout(tmp_path):
    L = capi.lib()
    for name in ("slslam_po_constraint_covariance", "slslam_pose_estimator_set_covariance", "slslam_pose_estimator_get_covariance"):
        assert name in capi.EXPORTS and hasattr(L, name)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "slslam_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(slslam_po_constraint_items), offsetof(slslam_po_constraint_items, cov_constraint),'
                   ' offsetof(slslam_po_constraint_items, sigma2), sizeof(slslam_pose_estimate), sizeof(slslam_po_candidates)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off_cov, off_s2, size_est, size_cand = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(capi.POConstraintItems)
    assert off_cov == capi.POConstraintItems.cov_constraint.offset and off_s2 == capi.POConstraintItems.sigma2.offset
    assert size_est == C.sizeof(capi.PoseEstimate) and size_cand == C.sizeof(capi.POCandidates)      # (the existing structs did not move)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_constraint_covariance_validates_before_it_writes():
    L = capi.lib()
    it = gref.primitive_items(3)
    xa, xb, cc = (np.ascontiguousarray(it[k]).reshape(-1) for k in ("pose_a", "pose_b", "constraints"))
    sc = np.ascontiguousarray(pref.random_spd(3)).reshape(-1)
    outs = [np.full(18, 7.0), np.full(108, 7.0), np.full(108, 7.0)]

    def call(n=3, a=xa, b=xb, c=cc, s=sc, sigma2=1.0, null_items=False):
        items = capi.POConstraintItems(n, None if a is None else _dp(a), None if b is None else _dp(b), None if c is None else _dp(c),
                                       None if s is None else _dp(s), sigma2)
        rc = L.slslam_po_constraint_covariance(None if null_items else C.byref(items), *[_dp(o) for o in outs])
        assert all((o == 7.0).all() for o in outs)
        return rc

    assert call(null_items=True) == INVALID
    assert call(n=-1) == INVALID
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert call(sigma2=bad) == INVALID
    assert call(a=None) == INVALID and call(b=None) == INVALID and call(c=None) == INVALID
    for which in range(4):
        arrays = [xa.copy(), xb.copy(), cc.copy(), sc.copy()]
        arrays[which][5] = np.nan if which % 2 else np.inf
        assert call(a=arrays[0], b=arrays[1], c=arrays[2], s=arrays[3]) == INVALID
    assert call(n=0) == OK                                                # succeeds and does nothing
    assert call(n=0, a=None, b=None, c=None, s=None) == OK
    with pytest.raises(capi.SlslamError) as ei:
        capi.po_constraint_covariance(it["pose_a"], it["pose_b"], it["constraints"], sigma2=-2.0)
    assert ei.value.status == INVALID
    empty = capi.po_constraint_covariance(np.zeros((0, 6)), np.zeros((0, 6)), np.zeros((0, 6)))
    assert empty["cov_meas"].shape == (0, 6, 6)


def test_estimator_covariance_validates_before_a_run():
    L = capi.lib()
    st, dof, s2 = C.c_int(77), C.c_int(77), C.c_double(77.0)
    cons, cov = np.full(6, 7.0), np.full(36, 7.0)

    def get(handle, frame):
        rc = L.slslam_pose_estimator_get_covariance(handle, frame, C.byref(st), _dp(cons), _dp(cov), C.byref(s2), C.byref(dof))
        assert st.value == 77 and dof.value == 77 and s2.value == 77.0 and (cons == 7.0).all() and (cov == 7.0).all()
        return rc

    assert L.slslam_pose_estimator_set_covariance(None, 1) == INVALID
    assert get(None, 0) == INVALID
    est = capi.PoseEstimator(max_frames=2, max_lines=16)
    try:
        assert get(est._h, -1) == INVALID
        assert get(est._h, 0) == STATE                                    # no run yet
        est.set_covariance(True)                                          # host only: no device is asked
        assert get(est._h, 0) == STATE and get(est._h, -1) == INVALID
        est.set_covariance(False)
        assert L.slslam_pose_estimator_get_covariance(est._h, 0, None, None, None, None, None) == STATE
        with pytest.raises(capi.SlslamError) as ei:
            est.get_covariance(0)
        assert ei.value.status == STATE
    finally:
        est.close()
    assert capi.PoseEstimator(max_frames=1, max_lines=8, covariance=True)._covariance


def test_motion_candidates_leaves_out_what_has_no_covariance():
    """Host-side part of capi.motion_candidates: nothing left to send, so no device is asked."""
    x = np.zeros((3, 6))
    est = [dict(status="RANSAC_FAILED"), dict(status="OK", cov_status=capi.COV_SINGULAR, constraint=np.zeros(6), covariance=np.zeros((6, 6)), sigma2=1.0)]
    cand, skipped = capi.motion_candidates(est, [0, 1], [1, 2], x)
    assert skipped == [0, 1] and len(cand["pose_a"]) == 0 and cand["constraints"].shape == (0, 6) and cand["cov_meas"].shape == (0, 6, 6)
    with pytest.raises(ValueError):
        capi.motion_candidates(est, [0], [1, 2], x)

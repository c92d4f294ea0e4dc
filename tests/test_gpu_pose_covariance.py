"""The covariance of an estimated frame motion and its map into an edge error's coordinates on the device (include/slslam_hip.h:
slslam_pose_estimator_set_covariance / _get_covariance, slslam_po_constraint_covariance; capi.motion_candidates) against the numpy
reference of tests/pose_covariance_reference.py.  Needs a real MI355X.

Deviations d of the primitive and of the gate are relative to the quantity's top and held to K * y with y the reference's own yardstick
and K = 100, the bound of tests/test_gpu_po_gate.py and tests/test_gpu_po_covariance.py.  The estimator's covariance is held to
tests/test_gpu_lba_covariance.py's rules: SAME_POINT against slslam_lba_covariance of the same window at the same parameters, 10 x
max(d_route, d_perturb) against the reference.  Each comparison prints its figures; the worst measured on the MI355X are listed in
profiles/pose_covariance_bench.txt."""
import functools
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_covariance_reference as lref  # noqa: E402
import po_gate_reference as gref  # noqa: E402
import pose_covariance_reference as pref  # noqa: E402

pytestmark = pytest.mark.gpu
K = 100.0
SAME_POINT = 1e-12                 # tests/test_gpu_lba_covariance.py: the same kernel at the same point, relative to the block's largest entry
COV_OK = 0
STATE = 5
CHI2_6_99 = 16.8
TRIALS = 64


def _mixed_frames():
    """Four frames for one call: K = 5 without outliers (the smallest solvable frame), K = 65 (a second inlier word), four lines
    (TOO_FEW_FEATURES), twelve lines with scattered correspondences (RANSAC fails)."""
    five = synth.make_ransac_pair(9611, num_lines=5, outlier_frac=0.0, num_trials=TRIALS)
    many = synth.make_ransac_pair(9612, num_lines=65, outlier_frac=0.1, num_trials=TRIALS)
    few = synth.make_ransac_pair(9613, num_lines=8, outlier_frac=0.0, num_trials=10)
    few = {"obs0": few["obs0"][:4], "obs1": few["obs1"][:4], "lines": few["lines"][:4], "samples": (np.arange(50, dtype=np.int32).reshape(10, 5)) % 4}
    low = synth.make_ransac_pair(9614, num_lines=12, outlier_frac=0.0, num_trials=TRIALS)
    low = dict(low, obs1=np.random.default_rng(9615).uniform(-1, 1, size=(12, 8)))
    return [five, many, few, low]


def _same_estimate(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "summary":
            assert a[k] == b[k]
        else:
            assert np.array_equal(a[k], b[k]), k


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


def test_estimator_reports_the_covariance_of_every_solved_frame(hip):
    frames = _mixed_frames()
    est = hip.PoseEstimator(max_frames=4, max_lines=80, covariance=True)
    plain = hip.PoseEstimator(max_frames=4, max_lines=80)
    try:
        got = est.run(frames, max_trials=TRIALS)
        assert [g["status"] for g in got] == ["OK", "OK", "TOO_FEW_FEATURES", "RANSAC_FAILED"]
        for f in (0, 1):
            g, w = got[f], est.window(f)
            n = len(w["index_words"]) // 2
            assert g["constraint"].tobytes() == w["solved_camera"].tobytes()
            cov = g["covariance"]
            assert g["cov_status"] == COV_OK and (cov == cov.T).all() and (np.diag(cov) > 0).all()
            assert g["summary"]["num_residual_blocks"] == n and g["dof"] == 4 * n - 6
            want = 2.0 * (g["summary"]["final_cost"] - g["summary"]["fixed_cost"]) / g["dof"]
            assert _ulps(g["sigma2"], want) <= 4, (g["sigma2"], want)
            win = pref.window_dict(n, w["observations"], w["parameters"], camera0=w["solved_camera"])
            st, free, cc, _ = hip.lba_covariance(win, with_lines=False)
            assert st == COV_OK and [int(c) for c in free] == [0]
            same = lref.rel_cameras(cov, cc[:6, :6])
            ref = pref.motion_covariance(win, lref.HUBER)
            d = lref.rel_cameras(cov, ref["cov"])
            print("frame %d: %d lines, dof %d, sigma2 %.6e (%.2f ulp from the summary's; reference %.6e)  cov: same point %.3g, reference %.3g "
                  "(d_route %.3g, d_perturb %.3g)" % (f, n, g["dof"], g["sigma2"], _ulps(g["sigma2"], want), ref["sigma2"], same, d,
                                                       ref["ref"]["d_route_cam"], ref["ref"]["d_perturb_cam"]))
            assert same <= SAME_POINT
            assert d <= 10 * ref["y"]
            assert ref["dof"] == g["dof"] and abs(g["sigma2"] - ref["sigma2"]) <= 1e-8 * ref["sigma2"]
        assert got[0]["dof"] == 14                                        # five inliers: the smallest solvable frame
        assert len(est.window(1)["index_words"]) // 2 <= 65 and frames[1]["obs0"].shape[0] == 65
        for f in (2, 3):
            assert "covariance" not in got[f]
            with pytest.raises(hip.SlslamError) as ei:
                est.get_covariance(f)
            assert ei.value.status == STATE
        with pytest.raises(hip.SlslamError) as ei:
            est.get_covariance(4)
        assert ei.value.status == 1
        # off means untouched: every field of every estimate is what the enabled run returned
        off = plain.run(frames, max_trials=TRIALS)
        keys = ("status", "trial_cnt", "ransac_score", "ransac_pose", "ransac_mask", "summary", "pose", "num_inliers", "mask")
        for a, b in zip(off, got):
            assert "covariance" not in a
            _same_estimate(a, {k: b[k] for k in keys})
        with pytest.raises(hip.SlslamError) as ei:
            plain.get_covariance(0)
        assert ei.value.status == STATE
        # a second run of the same size allocates nothing, neither in the estimator nor in its batch
        before = est.stats()
        again = est.run(frames, max_trials=TRIALS)
        after = est.stats()
        # (with covariance enabled the estimator's count includes the buffers slslam_lba_batch_covariance made in its batch)
        assert after["allocations"] == before["allocations"] > plain.stats()["allocations"] and after["refills"] == before["refills"] + 1
        for a, b in zip(again, got):
            # (k_lba_covariance sums a window's blocks by LDS atomics: the covariance repeats to SAME_POINT, everything else to the bit)
            _same_estimate({k: v for k, v in a.items() if k != "covariance"}, {k: v for k, v in b.items() if k != "covariance"})
            assert ("covariance" in a) == ("covariance" in b)
            if "covariance" in a:
                assert lref.rel_cameras(a["covariance"], b["covariance"]) <= SAME_POINT
        # switching it off on the same estimator: the run it was, and nothing to read
        est.set_covariance(False)
        for a, b in zip(est.run(frames, max_trials=TRIALS), off):
            _same_estimate(a, b)
        with pytest.raises(hip.SlslamError) as ei:
            est.get_covariance(0)
        assert ei.value.status == STATE
    finally:
        est.close(); plain.close()


# ---------------------------------------------------------------------------------------------- the primitive
def _hold(label, got, refs):
    worst = dict.fromkeys(pref.QUANTITIES, 0.0)
    for k, ref in enumerate(refs):
        for q, r in pref.deviations(ref, {q: got[q][k] for q in pref.QUANTITIES}).items():
            worst[q] = max(worst[q], r)
    print("%s: worst d / y  " % label + "  ".join("%s %.3f" % (q, worst[q]) for q in pref.QUANTITIES))
    for q in pref.QUANTITIES:
        assert worst[q] <= K, (label, q)
    return worst


@pytest.mark.parametrize("n", [1, 10, 11, 65])
def test_primitive_matches_reference(hip, n):
    items = gref.primitive_items(n)
    xa, xb, cc, s2 = items["pose_a"], items["pose_b"], items["constraints"], items["sigma2"]
    sig = pref.random_spd(n)
    got = hip.po_constraint_covariance(xa, xb, cc, sig, s2)
    refs = [pref.constraint_covariance(xa[k], xb[k], cc[k], sig[k], s2) for k in range(n)]
    _hold("constraint covariance n %d" % n, got, refs)
    R = got["cov_meas"]
    assert (R == np.transpose(R, (0, 2, 1))).all() and (np.linalg.eigvalsh(R) > 0).all()
    again = hip.po_constraint_covariance(xa, xb, cc, sig, s2)
    assert all(again[q].tobytes() == got[q].tobytes() for q in got)          # no atomics: the same bits
    none = hip.po_constraint_covariance(xa, xb, cc, None, s2)
    assert not none["cov_meas"].any() and none["error"].tobytes() == got["error"].tobytes() and none["jacobian"].tobytes() == got["jacobian"].tobytes()
    twice = hip.po_constraint_covariance(xa, xb, cc, sig, 2.0 * s2)
    assert (twice["cov_meas"] == 2.0 * R).all()
    upper = sig.copy()
    upper[:, np.triu_indices(6, 1)[0], np.triu_indices(6, 1)[1]] = 123.0        # only the lower triangle is read
    assert hip.po_constraint_covariance(xa, xb, cc, upper, s2)["cov_meas"].tobytes() == R.tobytes()
    # the error is the gate's own
    stat = hip.po_edge_statistics(xa, xb, cc, cov_meas=R, sigma2=1.0)
    assert stat["error"].tobytes() == got["error"].tobytes()


# ---------------------------------------------------------------------------------------------- end to end, smallest graphs
@functools.lru_cache(maxsize=None)
def _solved(shape):
    """(graph, the oracle's solved poses, its summary): computed once, shared, never modified (as tests/test_gpu_po_gate.py)."""
    from oracle import pyoracle
    g = synth.make_pose_graph(7, *shape)
    x, s, _ = pyoracle.po_solve(g, linear_solver=2)
    x.setflags(write=False)
    return g, x, s


@pytest.mark.parametrize("shape", [(4, 1), (12, 2)])
def test_gate_fed_by_the_constraint_covariance(hip, shape):
    g, x, s = _solved(shape)
    X = np.asarray(x).reshape(-1, 6)
    sc = pref.scenario(g, x, s["final_cost"])
    ref_cand, ref_items, (ref_cs, refs) = pref.scenario_reference(g, x, sc)
    a, b = np.array(sc["pose_a"]), np.array(sc["pose_b"])
    got_r = hip.po_constraint_covariance(X[a], X[b], sc["constraints"], sc["cov_constraint"], sc["sigma2_c"])
    _hold("scenario N %d loops %d: constraint covariance" % shape, got_r, ref_items)
    cand = dict(pose_a=sc["pose_a"], pose_b=sc["pose_b"], constraints=sc["constraints"], cov_meas=got_r["cov_meas"], sigma2=sc["sigma2"])
    cs, got = hip.po_gate(g, cand, 0.0, params=x)
    assert cs == COV_OK == ref_cs
    worst = dict.fromkeys(gref.QUANTITIES, 0.0)
    for k, ref in enumerate(refs):
        assert got["status"][k] == COV_OK == ref["status"] and ref["pivot"] >= 1e3 * gref.PIVOT_MIN
        for q, r in gref.deviations(ref, {q: got[q][k] for q in gref.QUANTITIES}).items():
            worst[q] = max(worst[q], r)
    print("scenario N %d loops %d: gate, worst d / y  " % shape + "  ".join("%s %.3f" % (q, worst[q]) for q in gref.QUANTITIES))
    assert all(worst[q] <= K for q in gref.QUANTITIES)
    m2, m2_ref = got["mahalanobis2"], np.array([r["mahalanobis2"] for r in refs])
    print("scenario N %d loops %d: m2 %s (reference %s)" % (shape + (np.round(m2, 3), np.round(m2_ref, 3))))
    out = sc["outlier"]
    assert m2_ref[out] > CHI2_6_99 and (np.delete(m2_ref, out) < CHI2_6_99).all()
    assert m2[out] > CHI2_6_99 and (np.delete(m2, out) < CHI2_6_99).all()
    # capi.motion_candidates on hand-made estimates reproduces the same arrays (and leaves out what has no covariance)
    est = [dict(status="OK", cov_status=COV_OK, constraint=sc["constraints"][k], covariance=sc["cov_constraint"][k], sigma2=sc["sigma2_c"])
           for k in range(len(a))]
    est.insert(1, dict(status="RANSAC_FAILED"))
    est.append(dict(status="OK", cov_status=1, constraint=np.zeros(6), covariance=np.zeros((6, 6)), sigma2=1.0))
    pa, pb = np.insert(a, 1, 0), np.insert(b, 1, 1)
    mc, skipped = hip.motion_candidates(est, np.append(pa, 0), np.append(pb, 1), X)
    assert skipped == [1, len(est) - 1]
    assert np.array_equal(mc["pose_a"], a) and np.array_equal(mc["pose_b"], b) and np.array_equal(mc["constraints"], sc["constraints"])
    direct = hip.po_constraint_covariance(X[a], X[b], sc["constraints"], sc["sigma2_c"] * sc["cov_constraint"], 1.0)
    assert mc["cov_meas"].tobytes() == direct["cov_meas"].tobytes() and "sigma2" not in mc
    for k, it in enumerate(ref_items):
        assert np.abs(mc["cov_meas"][k] - it["cov_meas"]).max() <= K * it["y"]["cov_meas"] * it["tops"]["cov_meas"]
    cs2, got2 = hip.po_gate(g, dict(mc, sigma2=sc["sigma2"]), 0.0, params=x)
    assert cs2 == COV_OK and (got2["mahalanobis2"][out] > CHI2_6_99) and (np.delete(got2["mahalanobis2"], out) < CHI2_6_99).all()

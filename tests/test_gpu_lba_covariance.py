"""Posterior covariances of LBA windows on the device (include/slslam_hip.h: slslam_lba_batch_covariance / _get_covariance,
slslam_lba_covariance; csrc/lba_covariance.h) against the numpy reference tests/lba_covariance_reference.py.  Needs a real MI355X.

Yardsticks (none taken from what the device returns):
  d_route   = the relative difference of the reference's two routes - QR of J against the Schur complement - on the oracle's Jacobians at
              the point in question, per window, floor 1e-13: how well fp64 determines these numbers at all.  Cameras: largest entry of
              the difference over the largest entry of Σ_cc; lines: the worst 4 x 4 block, each relative to its own largest entry.
  d_perturb = the movement of the reference covariance when the point is perturbed by a relative 1e-13 with random signs (fixed seed),
              the yardstick tests/test_gpu_lba.py::test_headline_path_matches_oracle uses for solves.
  ALGEBRA:    the device's covariance lies within 10 x d_route of route (a) fed with the device's OWN Jacobians (slslam_lba_batch_linearise at
              the same point), so that nothing but the covariance algebra is compared.
  END TO END: ... within 10 x max(d_route, d_perturb) of route (a) on the oracle's Jacobians.
The factor 10 is the project's rule for judging a deviation against the reference's own movement.
  SAME POINT: two device results at the same point to the bit (with and without the lines; a window in company and alone) may differ by the
              order of the LDS atomic sums into S only.  An entry of S sums at most ~2500 terms (every observation of a camera), so
              its relative rounding spread is ~sqrt(2500) x 1.1e-16 = 5.5e-15; the inverse amplifies that by at most 1 / (smallest
              unit-diagonal pivot of S) <= 1 / 8.5e-3 = 118 (the smallest in the issue's table of well-posed windows; tests/test_lba_covariance_cpu.py
              prints 1.4e-2 ... 9.7e-2 for the windows used here): 6.5e-13, bound 1e-12 of the block's largest entry.  The lines' blocks
              H_ll^-1 + K Σ_cc K^T inherit it from Σ_cc (H_ll^-1 and K come from fixed-order wave sums), both terms being positive.
Measured on MI355X (deviation / bound, solved point): see profiles/lba_covariance_bench.txt."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_covariance_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID, STATE = 4, 1, 5
SAME_POINT = 1e-12
CASES = R.cases()
# the mixed batch of eight: every Huber window of the cases (the singular one among them) and two more small ones
MIXED = ["free2", "free10", "all_free", "free12", "constant_lines", "free20", "extra_a", "extra_b"]
CHECKED = ["free2", "free10", "free12", "free20", "constant_lines"]


def _window(name):
    if name == "extra_a":
        return synth.make_window(11, num_lines=40, num_kf=4, num_free=2)
    if name == "extra_b":
        return synth.make_window(12, num_lines=60, num_kf=6, num_free=3)
    return CASES[name][0]


def _grab(b, i, w):
    """Everything about window i of a downloaded batch: parameters, covariance, and the device's Jacobians at the same point."""
    st, free, cc, cl = b.get_covariance(i)
    _, _, jc, jl = b.linearise(i, len(w["camera_index"]))
    return dict(x=b.parameters(i).copy(), status=st, free=free, cc=cc, cl=cl, jc=jc, jl=jl)


def _deviation(got_c, got_l, ref_c, ref_l):
    return R.rel_cameras(got_c, ref_c), (R.rel_lines(got_l, ref_l) if got_l is not None else 0.0)


def _assert_algebra(tag, w, hd, g, x):
    """Assertion 1 at point x (where g's Jacobians and covariance were taken)."""
    ref = R.reference(w, x, hd)
    dc, dl = R.cov_qr(w, g["jc"], g["jl"])
    ec, el = _deviation(g["cc"], g["cl"], dc, dl)
    print("%s ALGEBRA cameras %.3g (d_route %.3g) lines %.3g (d_route %.3g)" % (tag, ec, ref["d_route_cam"], el, ref["d_route_line"]))
    assert g["status"] == 0
    assert ec <= 10 * ref["d_route_cam"] and el <= 10 * ref["d_route_line"]
    return ref


@pytest.fixture(scope="module")
def mixed(hip):
    """Eight windows in one batch: covariance at the solved point (with lines, then without), then after a reset."""
    ws = [_window(k) for k in MIXED]
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    with pytest.raises(hip.SlslamError) as ei:                  # nothing enqueued yet
        b.get_covariance(0)
    assert ei.value.status == INVALID
    b.solve(); b.covariance(); b.download()
    out = {"solved": {k: _grab(b, i, ws[i]) for i, k in enumerate(MIXED)}, "stats1": b.covariance_stats()}
    b.covariance(with_lines=False); b.download()
    out["no_lines"] = {k: b.get_covariance(i) for i, k in enumerate(MIXED)}
    b.covariance(); b.download()
    out["stats3"] = b.covariance_stats()
    b.reset(); b.covariance(); b.download()
    out["initial"] = {k: _grab(b, i, ws[i]) for i, k in enumerate(MIXED)}
    b.close()
    return out


@pytest.fixture(scope="module")
def refs_solved(mixed):
    """The reference at the solved points of the mixed batch, computed once."""
    return {k: R.reference(CASES[k][0], mixed["solved"][k]["x"], CASES[k][1], with_perturb=True) for k in CHECKED}


@pytest.mark.parametrize("name", CHECKED)
def test_algebra_on_the_devices_own_jacobians(mixed, refs_solved, name):
    g, ref, w = mixed["solved"][name], refs_solved[name], CASES[name][0]
    dc, dl = R.cov_qr(w, g["jc"], g["jl"])
    ec, el = _deviation(g["cc"], g["cl"], dc, dl)
    print("%s ALGEBRA cameras %.3g (d_route %.3g) lines %.3g (d_route %.3g)" % (name, ec, ref["d_route_cam"], el, ref["d_route_line"]))
    assert g["status"] == 0
    assert ec <= 10 * ref["d_route_cam"]
    assert el <= 10 * ref["d_route_line"]


@pytest.mark.parametrize("name", CHECKED)
def test_end_to_end_against_the_oracle(mixed, refs_solved, name):
    g, ref = mixed["solved"][name], refs_solved[name]
    ec, el = _deviation(g["cc"], g["cl"], *ref["qr"])
    bc = 10 * max(ref["d_route_cam"], ref["d_perturb_cam"])
    bl = 10 * max(ref["d_route_line"], ref["d_perturb_line"])
    print("%s END TO END cameras %.3g (d_route %.3g, d_perturb %.3g) lines %.3g (d_route %.3g, d_perturb %.3g)" % (
        name, ec, ref["d_route_cam"], ref["d_perturb_cam"], el, ref["d_route_line"], ref["d_perturb_line"]))
    assert ec <= bc
    assert el <= bl


@pytest.mark.parametrize("name", CHECKED)
def test_structure(mixed, refs_solved, name):
    g, ref, w = mixed["solved"][name], refs_solved[name], CASES[name][0]
    n = 6 * len(ref["free_cameras"])
    assert g["cc"].shape == (n, n)
    assert np.array_equal(g["free"], ref["free_cameras"]) and np.all(np.diff(g["free"]) > 0)
    assert np.abs(g["cc"] - g["cc"].T).max() <= 1e-15 * np.abs(g["cc"]).max()          # symmetric to round-off
    np.linalg.cholesky(g["cc"])                                                      # positive definite
    free_lines = set(ref["free_lines"].tolist())
    for l in range(int(w["num_lines"])):
        if l in free_lines:
            assert np.abs(g["cl"][l] - g["cl"][l].T).max() <= 1e-15 * np.abs(g["cl"][l]).max()
            np.linalg.cholesky(g["cl"][l])
        else:
            assert not g["cl"][l].any()                                              # constant / unobserved: exactly zero
    st, free, cc, cl = mixed["no_lines"][name]
    assert st == 0 and cl is None
    # with_lines = 0 runs the same passes 1 and 2: the cameras' block may differ by the order of the LDS atomic sums only
    e0 = R.rel_cameras(cc, g["cc"])
    print("%s without lines against with: cameras %.3g" % (name, e0))
    assert e0 <= SAME_POINT


def test_constant_lines_are_really_there(refs_solved):
    w = CASES["constant_lines"][0]
    assert 0 < len(refs_solved["constant_lines"]["free_lines"]) < int(w["num_lines"])


def test_singular_window_is_reported_and_alone(mixed, refs_solved):
    g, w = mixed["solved"]["all_free"], CASES["all_free"][0]
    assert g["status"] == 1
    assert list(g["free"]) == [0, 1, 2, 3]
    assert not g["cc"].any() and not g["cl"].any()
    assert mixed["no_lines"]["all_free"][0] == 1 and not mixed["no_lines"]["all_free"][2].any()
    for k in CHECKED + ["extra_a", "extra_b"]:                                       # (their results: test_algebra_...)
        assert mixed["solved"][k]["status"] == 0


def test_second_call_allocates_nothing(mixed):
    assert mixed["stats1"]["calls"] == 1 and mixed["stats1"]["allocations"] > 0
    assert mixed["stats3"]["calls"] == 3 and mixed["stats3"]["allocations"] == mixed["stats1"]["allocations"]


@pytest.mark.parametrize("name", ["free2", "free10", "free20"])
def test_window_in_company_equals_window_alone(hip, mixed, name):
    """At the INITIAL parameters (after a reset of the mixed batch, after finalize of the window's own batch): the same point to the bit,
    so only the order of the atomic sums differs.  Also: the covariance after a reset is that of the initial parameters, and differs from
    the one at the solved point."""
    w, hd, _ = CASES[name]
    x0 = np.asarray(w["parameters"], dtype=np.float64)
    gi = mixed["initial"][name]
    assert np.array_equal(gi["x"], x0)
    ref = _assert_algebra(name + " initial", w, hd, gi, x0)
    b = hip.LBABatch()
    b.add(w); b.finalize(); b.covariance(); b.download()
    alone = _grab(b, 0, w)
    b.close()
    _assert_algebra(name + " alone", w, hd, alone, x0)
    ec, el = _deviation(gi["cc"], gi["cl"], alone["cc"], alone["cl"])
    print("%s in company against alone: cameras %.3g lines %.3g" % (name, ec, el))
    assert ec <= SAME_POINT and el <= SAME_POINT
    gs = mixed["solved"][name]
    assert R.rel_cameras(gs["cc"], gi["cc"]) > 1e-6                                   # the solve moved the point


def test_one_shot_agrees_with_the_batch(hip, mixed, refs_solved):
    for name in ("free2", "free12"):
        w, hd, _ = CASES[name]
        g, ref = mixed["solved"][name], refs_solved[name]
        st, free, cc, cl = hip.lba_covariance(w, params=g["x"], huber_delta=hd)
        assert st == 0 and np.array_equal(free, g["free"])
        # (not SAME POINT: the batch's sin / cos table of the solved lines comes from the solve's incremental updates, the one-shot call's
        # from sin / cos of the same parameters - the Jacobians differ in their last bits, which is what d_route measures)
        ec, el = _deviation(cc, cl, g["cc"], g["cl"])
        print("%s one-shot against batch: cameras %.3g lines %.3g" % (name, ec, el))
        assert ec <= 10 * ref["d_route_cam"] and el <= 10 * ref["d_route_line"]
        st, free, cc2, cl2 = hip.lba_covariance(w, params=g["x"], with_lines=False, huber_delta=hd)
        assert cl2 is None and R.rel_cameras(cc2, cc) <= SAME_POINT


def test_motion_only_batch(hip):
    """The fused path: S = H_cc, 6 x 6, no free line."""
    w, hd, _ = CASES["motion_only"]
    b = hip.LBABatch()
    b.add(w); b.add(synth.make_motion_only(7, num_lines=45)); b.finalize()
    assert b.path() == 1
    b.solve(); b.covariance(); b.download()
    g = _grab(b, 0, w)
    b.close()
    ref = _assert_algebra("motion_only", w, hd, g, g["x"])
    assert g["cc"].shape == (6, 6) and np.array_equal(g["free"], ref["free_cameras"]) and not g["cl"].any()
    np.linalg.cholesky(g["cc"])
    refp = R.reference(w, g["x"], hd, with_perturb=True)
    ec, _ = _deviation(g["cc"], None, *refp["qr"])
    print("motion_only END TO END cameras %.3g (d_route %.3g, d_perturb %.3g)" % (ec, refp["d_route_cam"], refp["d_perturb_cam"]))
    assert ec <= 10 * max(refp["d_route_cam"], refp["d_perturb_cam"])


def test_without_huber_loss(hip):
    w, hd, _ = CASES["no_huber"]
    assert hd == 0.0
    b = hip.LBABatch()
    b.add(w); b.finalize(huber_delta=0.0)
    b.solve(); b.covariance(); b.download()
    g = _grab(b, 0, w)
    b.close()
    _assert_algebra("no_huber", w, hd, g, g["x"])
    refp = R.reference(w, g["x"], hd, with_perturb=True)
    ec, el = _deviation(g["cc"], g["cl"], *refp["qr"])
    print("no_huber END TO END cameras %.3g lines %.3g" % (ec, el))
    assert ec <= 10 * max(refp["d_route_cam"], refp["d_perturb_cam"]) and el <= 10 * max(refp["d_route_line"], refp["d_perturb_line"])
    # the loss matters: the same point under the default loss gives another covariance
    st, _, cc_h, _ = hip.lba_covariance(w, params=g["x"])
    assert st == 0 and R.rel_cameras(cc_h, g["cc"]) > 1e-6


def test_refilled_batch(hip):
    """On a batch made for refills the covariance is that of the windows the batch holds NOW; what was downloaded before the refill is gone."""
    first = [_window("extra_a"), _window("extra_b")]
    second = [synth.make_window(21, num_lines=40, num_kf=4, num_free=2), synth.make_window(22, num_lines=60, num_kf=6, num_free=3)]
    b = hip.LBABatch()
    for w in first:
        b.add(w)
    b.finalize(refill_headroom_percent=50)
    b.solve(); b.covariance(); b.download()
    before = b.get_covariance(1)
    n_alloc = b.covariance_stats()["allocations"]
    b.refill(second)
    with pytest.raises(hip.SlslamError) as ei:
        b.get_covariance(1)
    assert ei.value.status == INVALID
    b.solve(); b.covariance(); b.download()
    assert b.covariance_stats()["allocations"] == n_alloc
    for i, w in enumerate(second):
        g = _grab(b, i, w)
        _assert_algebra("refilled %d" % i, w, R.HUBER, g, g["x"])
    assert R.rel_cameras(b.get_covariance(1)[2], before[2]) > 1e-6
    b.close()


def test_stream_batch(hip):
    """Through slslam_lba_stream_batch: no stream entry point of its own."""
    ws = hip.WindowSet([_window("extra_a"), _window("extra_b")])
    st = hip.LBAStream(depth=2, host_threads=1)
    t = st.submit(ws)
    st.collect(t)
    v = st.batch_of(t, ws)
    v.covariance(); v.download()
    for i, k in enumerate(("extra_a", "extra_b")):
        w = _window(k)
        g = _grab(v, i, w)
        assert np.array_equal(g["x"], ws.parameters(i))
        _assert_algebra("stream %s" % k, w, R.HUBER, g, g["x"])
    st.close(); ws.close()


def test_oversize_window_is_refused_and_still_solves(hip):
    w = synth.make_window(13, num_lines=120, num_kf=44, num_free=22)
    b = hip.LBABatch()
    b.add(w); b.finalize()
    assert b.path() == 2
    with pytest.raises(hip.SlslamError) as ei:
        b.covariance()
    assert ei.value.status == UNSUPPORTED
    b.solve(); b.download()
    s = b.summary(0)
    assert s["final_cost"] < s["initial_cost"] and s["num_successful_steps"] > 0
    with pytest.raises(hip.SlslamError) as ei:
        b.get_covariance(0)
    assert ei.value.status == INVALID
    b.close()
    with pytest.raises(hip.SlslamError) as ei:
        hip.lba_covariance(w)
    assert ei.value.status == UNSUPPORTED
    # a batch that mixes such a window with ordinary ones
    b = hip.LBABatch()
    b.add(w); b.add(_window("extra_a")); b.finalize()
    assert b.path() == 3
    with pytest.raises(hip.SlslamError) as ei:
        b.covariance()
    assert ei.value.status == UNSUPPORTED
    b.solve(); b.download()
    assert b.summary(1)["num_successful_steps"] > 0
    b.close()


def test_solve_is_untouched_by_an_interleaved_covariance(hip):
    ws = [_window("free10"), _window("free2"), _window("constant_lines")]
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    b.solve(); b.download()
    plain = [(b.parameters(i).copy(), b.summary(i), b.trace(i)) for i in range(len(ws))]
    b.reset(); b.covariance(); b.solve(); b.covariance(); b.download()
    for i in range(len(ws)):
        assert b.parameters(i).tobytes() == plain[i][0].tobytes()
        assert b.summary(i) == plain[i][1] and b.trace(i) == plain[i][2]
        assert b.get_covariance(i)[0] == 0
    b.close()

"""The report on the windows of a resident LBA batch (include/slslam_hip.h: slslam_lba_batch_report / _get_report, slslam_lba_report;
csrc/lba_report.h) against the numpy reference tests/lba_report_reference.py, evaluated at the device's own downloaded parameters.
Needs a real MI355X.

Bounds (none taken from what the device returns):
  per observation  |s - s0| <= 4e-14 sqrt(s0) + 1e-27: the 1e-14 bound on a residual component tests/test_gpu_lba.py holds, through
                   ds <= 2 |r| |dr| over four components; weight to 1e-12 relative; the Huber margin of tests/test_lba_report_cpu.py
                   (no observation within 1e-6 a^2 of the corner) is asserted again at this point, so no weight is excluded.
  sums             sq_norm_sum and cost to 1e-12 relative against the sums of the device's own per-observation terms (the order of
                   summation differs), and against the oracle's within the per-observation bound on top; counts and statuses exactly;
                   sum of the lines' cost = summary.final_cost (fixed cost included) to 1e-12 relative after a solve.
  min_pivot        against the reference on the device's OWN line Jacobians (LBABatch.linearise): |d| <= 1e-12 absolute - unit-diagonal
                   entries carry <= n_obs 4 eps (6e-14 at 64 observations), a pivot is 1 minus at most three products of such entries;
                   against the oracle's Jacobians: 10 x the reference's own change under lba_covariance_reference.perturbed(x),
                   floor 1e-12 (the yardstick of DESIGN.md 4.2).
Measured on MI355X: profiles/lba_report_bench.txt."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_covariance_reference as R  # noqa: E402
import lba_report_reference as P  # noqa: E402
from test_lba_report_cpu import degenerate_window  # noqa: E402

pytestmark = pytest.mark.gpu
UNSUPPORTED, INVALID = 4, 1
CASES = R.cases()
MIXED = ["free2", "free10", "all_free", "free12", "constant_lines", "free20", "extra_a", "extra_b"]
ROW_COUNTS = [1, 15, 16, 17, 32, 33, 64, 0]        # the row and tile boundaries of csrc/lba_types.h


def _window(name):
    if name == "extra_a":
        return synth.make_window(11, num_lines=40, num_kf=4, num_free=2)
    if name == "extra_b":
        return synth.make_window(12, num_lines=60, num_kf=6, num_free=3)
    if name == "degenerate":
        return degenerate_window()[0]
    return CASES[name][0]


def handmade(counts, num_kf):
    """A window whose line l is seen by cameras 0 .. counts[l] - 1 (4 free cameras, the rest constant): the cameras and lines of a synthetic
    window, every line projected into the cameras that are to see it, half a pixel of noise."""
    base = synth.make_window(21, num_lines=len(counts), num_kf=num_kf, num_free=4)
    rng = np.random.default_rng(5)
    C, L = num_kf, len(counts)
    xt = np.asarray(base["true_parameters"], dtype=np.float64)
    poses = [synth.wt_to_rt(xt[6 * c:6 * c + 6]) for c in range(C)]
    av = synth.orth_to_av(xt[6 * C:].reshape(L, 4))
    cam, line, obs = [], [], []
    for l, k in enumerate(counts):
        cp, dv = av[l, :3], av[l, 3:] / np.linalg.norm(av[l, 3:])
        best = max(np.linspace(-20, 20, 81), key=lambda s: min((R_ @ (cp + s * dv) + t_)[2] for R_, t_ in poses[:max(k, 1)]))
        ends = [cp + (best - 0.5) * dv, cp + (best + 0.5) * dv]
        for c in range(k):
            R_, t_ = poses[c]
            o = np.zeros(8)
            for e, Pw in enumerate(ends):
                pc = R_ @ Pw + t_
                assert pc[2] > 0.3
                o[2 * e], o[2 * e + 1] = pc[0] / pc[2], pc[1] / pc[2]
                o[4 + 2 * e], o[4 + 2 * e + 1] = (pc[0] - synth.BASELINE) / pc[2], pc[1] / pc[2]
            cam.append(c); line.append(l); obs.append(o + rng.normal(0, 0.5 / synth.FOCAL, 8))
    cam = np.array(cam, dtype=np.int32)
    fixed = np.zeros((len(cam), 2), dtype=np.int32)
    fixed[:, 0] = cam >= 4
    return {"num_cameras": C, "num_lines": L, "num_free_cameras": 4, "camera_index": cam, "line_index": np.array(line, dtype=np.int32),
            "fixed_index": fixed.reshape(-1), "observations": np.array(obs), "parameters": np.asarray(base["parameters"]).copy(),
            "baseline": synth.BASELINE}


def _grab(b, i, w, solved=True):
    g = dict(x=b.parameters(i).copy(), rep=b.get_report(i), jl=b.linearise(i, len(w["camera_index"]))[3])
    if solved:
        g["summary"] = b.summary(i)
    return g


def _batch(hip, ws, solve=True, **opt):
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(**opt)
    if solve:
        b.solve()
    b.report(); b.download()
    return b


def _same_bytes(a, c):
    return all(a[k].tobytes() == c[k].tobytes() for k in ("sq_norm", "weight", "lines", "cameras"))


def _check(tag, w, hd, g, solved=True):
    """Assertions 1 and 2 of the issue for one window, at the device's own point g['x']."""
    rep, x = g["rep"], g["x"]
    ref = P.report(w, x, hd)
    s0 = ref["sq_norm"]
    # 1. per observation, caller's order, constant-constant observations present
    assert rep["sq_norm"].shape == s0.shape
    ds = np.abs(rep["sq_norm"] - s0)
    print("%s: |s - s0| / (4e-14 sqrt(s0) + 1e-27) max %.3g" % (tag, (ds / (4e-14 * np.sqrt(s0) + 1e-27)).max() if len(s0) else 0.0))
    assert (ds <= 4e-14 * np.sqrt(s0) + 1e-27).all()
    margin = P.huber_margin(s0, hd)
    print("%s: Huber margin %.3g" % (tag, margin))
    assert margin > 1e-6
    dw = np.abs(rep["weight"] - ref["weight"]) / ref["weight"]
    print("%s: weight rel max %.3g" % (tag, dw.max() if len(dw) else 0.0))
    assert (dw <= 1e-12).all()
    # 2. per line and per camera: counts and statuses against the oracle's; the sums to 1e-12 relative against the reference summing the
    # SAME terms (the device's per-observation values, each checked above) - only the order of summation differs - and against the
    # oracle's terms within what the per-observation bound allows on top (a line whose one residual is ~0 has no relative accuracy)
    own = P.report(w, x, hd, jl=g["jl"], sq_norm=rep["sq_norm"])
    ob = 4e-14 * np.sqrt(s0) + 1e-27
    for kind, index in (("lines", np.asarray(w["line_index"])), ("cameras", np.asarray(w["camera_index"]))):
        got, want = rep[kind], ref[kind]
        assert np.array_equal(got["status"], want["status"])
        assert np.array_equal(got["num_observations"], want["num_observations"])
        assert np.array_equal(got["num_downweighted"], want["num_downweighted"])
        slack = np.bincount(index, weights=ob, minlength=len(got))
        for f in ("sq_norm_sum", "cost"):
            d = np.abs(got[f] - own[kind][f])
            print("%s: %s %s rel max %.3g" % (tag, kind, f, (d / np.maximum(own[kind][f], 1e-300)).max() if len(d) else 0.0))
            assert (d <= 1e-12 * own[kind][f]).all()
            assert (np.abs(got[f] - want[f]) <= 1e-12 * want[f] + slack).all()
    if solved:
        fc = g["summary"]["final_cost"]
        assert abs(rep["lines"]["cost"].sum() - fc) <= 1e-12 * fc
        assert abs(rep["cameras"]["cost"].sum() - fc) <= 1e-12 * fc
    free = ref["lines"]["status"] == P.FREE
    assert not rep["lines"]["min_pivot"][~free].any()
    own = own["lines"]["min_pivot"]
    d_own = np.abs(rep["lines"]["min_pivot"] - own).max() if len(own) else 0.0
    print("%s: min_pivot against the device's own Jacobians |d| max %.3g (bound 1e-12)" % (tag, d_own))
    assert d_own <= 1e-12
    moved = np.abs(P.report(w, R.perturbed(x), hd)["lines"]["min_pivot"] - ref["lines"]["min_pivot"])
    d_or = np.abs(rep["lines"]["min_pivot"] - ref["lines"]["min_pivot"])
    print("%s: min_pivot against the oracle's Jacobians |d| / max(10 moved, 1e-12) max %.3g" % (tag, (d_or / np.maximum(10 * moved, 1e-12)).max() if len(d_or) else 0.0))
    assert (d_or <= np.maximum(10 * moved, 1e-12)).all()
    return ref


@pytest.fixture(scope="module")
def mixed(hip):
    """The eight-window batch and the degenerate fixture, solved: report and covariance enqueued together, one download."""
    names = MIXED + ["degenerate"]
    ws = [_window(k) for k in names]
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    with pytest.raises(hip.SlslamError) as ei:                  # nothing enqueued yet
        b.get_report(0)
    assert ei.value.status == INVALID
    b.solve(); b.report(); b.covariance(); b.download()
    out = {"both": {k: _grab(b, i, ws[i]) for i, k in enumerate(names)}, "cov_both": [b.get_covariance(i) for i in range(len(ws))],
           "stats1": b.report_stats(), "path": b.path()}
    b.report(); b.download()
    out["alone"] = [b.get_report(i) for i in range(len(ws))]
    out["stats2"] = b.report_stats()
    b.covariance(); b.download()
    out["cov_alone"] = [b.get_covariance(i) for i in range(len(ws))]
    out["report_kept"] = [b.get_report(i) for i in range(len(ws))]   # a covariance call does not invalidate the report
    b.report()
    with pytest.raises(hip.SlslamError) as ei:                  # a newer report is still on the device
        b.get_report(0)
    assert ei.value.status == INVALID
    b.download()
    assert hip.lib().slslam_lba_batch_get_report(b._h, len(ws), None, None, None, None) == INVALID      # an index out of range
    assert hip.lib().slslam_lba_batch_get_report(b._h, -1, None, None, None, None) == INVALID
    b.close()
    out["names"], out["ws"] = names, ws
    return out


@pytest.mark.parametrize("name", MIXED + ["degenerate"])
def test_against_the_reference(mixed, name):
    w = _window(name)
    _check(name, w, R.HUBER, mixed["both"][name])


def test_agrees_with_the_covariance_and_names_the_planted_line(mixed):
    for i, k in enumerate(mixed["names"]):
        w, g = mixed["ws"][i], mixed["both"][k]
        lines = g["rep"]["lines"]
        free = lines["status"] == P.FREE
        ref_piv = P.report(w, g["x"], R.HUBER)["lines"]["min_pivot"]
        piv_s = P.schur_pivot_without_degenerate_lines(w, g["x"], R.HUBER, np.where(free, ref_piv, 1.0))
        named = bool((lines["min_pivot"][free] <= R.PIVOT_MIN).any())
        singular_line = mixed["cov_both"][i][0] == 1 and piv_s > R.PIVOT_MIN
        print("%s: covariance status %d, smallest pivot of S %.3g, of the lines %.3g" % (k, mixed["cov_both"][i][0], piv_s, lines["min_pivot"][free].min()))
        assert named == singular_line == (k == "degenerate")
    lines = mixed["both"]["degenerate"]["rep"]["lines"]
    piv = np.where(lines["status"] == P.FREE, lines["min_pivot"], np.inf)
    assert int(np.argmin(piv)) == degenerate_window()[1]


def test_report_and_covariance_do_not_disturb_each_other(mixed):
    assert mixed["path"] == 0
    for i, k in enumerate(mixed["names"]):
        assert _same_bytes(mixed["both"][k]["rep"], mixed["alone"][i]) and _same_bytes(mixed["alone"][i], mixed["report_kept"][i])
        # (the covariance is not reproducible to the bit from call to call, with or without a report beside it: its four waves add into S
        # by LDS atomics in arrival order - tests/test_gpu_lba_covariance.py, SAME POINT, whose yardstick is used here)
        a, c = mixed["cov_both"][i], mixed["cov_alone"][i]
        assert a[0] == c[0] and np.array_equal(a[1], c[1])
        if a[0] == 1:                                               # SINGULAR: zeros both times
            assert not a[2].any() and not c[2].any() and not a[3].any() and not c[3].any()
        else:
            assert R.rel_cameras(a[2], c[2]) <= 1e-12 and R.rel_lines(a[3], c[3]) <= 1e-12
    assert mixed["stats1"]["calls"] == 1 and mixed["stats1"]["allocations"] > 0
    assert mixed["stats2"] == {"calls": 2, "allocations": mixed["stats1"]["allocations"]}      # a second call allocates nothing


@pytest.mark.parametrize("name", ["free10", "constant_lines", "degenerate"])
def test_in_company_equals_alone(hip, mixed, name):
    w = _window(name)
    b = _batch(hip, [w])
    g = b.get_report(0)
    x = b.parameters(0)
    b.close()
    c = mixed["both"][name]
    assert x.tobytes() == c["x"].tobytes()
    assert g["sq_norm"].tobytes() == c["rep"]["sq_norm"].tobytes() and g["weight"].tobytes() == c["rep"]["weight"].tobytes()
    for kind in ("lines", "cameras"):
        assert np.array_equal(g[kind]["status"], c["rep"][kind]["status"]) and np.array_equal(g[kind]["num_downweighted"], c["rep"][kind]["num_downweighted"])
        for f in ("sq_norm_sum", "cost"):
            assert (np.abs(g[kind][f] - c["rep"][kind][f]) <= 1e-12 * c["rep"][kind][f]).all()


def test_motion_only_path(hip):
    w = synth.make_motion_only(6, num_lines=100)
    b = _batch(hip, [w])
    assert b.path() == 1
    _check("motion_only", w, R.HUBER, _grab(b, 0, w))
    b.close()


@pytest.mark.parametrize("counts,num_kf,path", [(ROW_COUNTS, 64, 0), (ROW_COUNTS + [65], 65, 2)])
def test_row_and_tile_boundaries(hip, counts, num_kf, path):
    w = handmade(counts, num_kf)
    b = _batch(hip, [w])
    assert b.path() == path
    g = _grab(b, 0, w)
    assert np.array_equal(g["rep"]["lines"]["num_observations"], counts)
    assert g["rep"]["lines"]["status"][7] == P.NO_OBSERVATIONS
    _check("handmade%d" % num_kf, w, R.HUBER, g)
    b.close()


def test_oversize_window_alone_and_in_a_mixed_batch(hip):
    """SLSLAM_PATH_GLOBAL_MEMORY and SLSLAM_PATH_MIXED report, where the covariance of the same batch is UNSUPPORTED."""
    big, small = synth.make_window(13, num_lines=120, num_kf=44, num_free=22), _window("extra_a")
    got = {}
    for ws, path in (([big], 2), ([small, big], 3)):
        b = _batch(hip, ws)
        assert b.path() == path
        with pytest.raises(hip.SlslamError) as ei:
            b.covariance()
        assert ei.value.status == UNSUPPORTED
        for i, w in enumerate(ws):
            got[(path, i)] = _grab(b, i, w)
            _check("path%d window %d" % (path, i), w, R.HUBER, got[(path, i)])
        b.report(); b.download()
        assert b.report_stats()["calls"] == 2 and _same_bytes(b.get_report(0), got[(path, 0)]["rep"])
        b.close()
    a, c = got[(2, 0)], got[(3, 1)]                                # the oversize window alone and in company
    assert a["x"].tobytes() == c["x"].tobytes() and _same_bytes(a["rep"], c["rep"])


def test_one_shot_equals_the_batch_at_the_initial_point(hip):
    for w in (_window("free2"), handmade(ROW_COUNTS + [65], 65)):
        b = _batch(hip, [w], solve=False)
        g = _grab(b, 0, w, solved=False)
        b.close()
        assert g["x"].tobytes() == np.asarray(w["parameters"], dtype=np.float64).tobytes()
        assert _same_bytes(hip.lba_report(w), g["rep"])
        _check("initial", w, R.HUBER, g, solved=False)


def test_refill_invalidates_and_interleaved_reports_leave_the_solve_alone(hip):
    ws1 = [synth.make_window(60 + i, num_lines=50 + 10 * i, num_kf=6, num_free=3) for i in range(3)]
    ws2 = [synth.make_window(70 + i, num_lines=55 + 10 * i, num_kf=6, num_free=3) for i in range(3)]
    plain = hip.LBABatch()
    for w in ws2:
        plain.add(w)
    plain.finalize(); plain.solve(); plain.download()
    undisturbed = [(plain.parameters(i).copy(), plain.summary(i)) for i in range(3)]
    plain.close()
    b = hip.LBABatch()
    for w in ws1:
        b.add(w)
    b.finalize(refill_headroom_percent=50)
    b.report(); b.solve(); b.report(); b.download()
    for i, w in enumerate(ws1):
        _check("before refill %d" % i, w, R.HUBER, _grab(b, i, w))
    stats = b.report_stats()
    b.refill(ws2)
    with pytest.raises(hip.SlslamError) as ei:                  # the refill replaced the windows
        b.get_report(0)
    assert ei.value.status == INVALID
    b.report(); b.solve(); b.report(); b.download()             # a report at the initial point, the solve, a report at the solved one
    assert b.report_stats() == {"calls": stats["calls"] + 2, "allocations": stats["allocations"]}
    for i, w in enumerate(ws2):
        g = _grab(b, i, w)
        assert g["x"].tobytes() == undisturbed[i][0].tobytes() and g["summary"] == undisturbed[i][1]
        _check("refilled %d" % i, w, R.HUBER, g)
    b.close()


def test_stream_batches_report(hip):
    """Through slslam_lba_stream_batch: the first set is packed on the host, the third is a device-built refill of the first slot."""
    sets = [hip.WindowSet([synth.make_window(80 + 4 * k + i, num_lines=40 + 10 * i, num_kf=6, num_free=3) for i in range(2)], pinned=True) for k in range(3)]
    wins = [[synth.make_window(80 + 4 * k + i, num_lines=40 + 10 * i, num_kf=6, num_free=3) for i in range(2)] for k in range(3)]
    st = hip.LBAStream(depth=2, host_threads=1)
    tk = [st.submit(sets[0]), st.submit(sets[1])]
    st.collect(tk[0])
    for k, t in ((0, tk[0]),):
        v = st.batch_of(t, sets[k])
        v.report(); v.download()
        for i, w in enumerate(wins[k]):
            _check("stream set %d window %d" % (k, i), w, R.HUBER, _grab(v, i, w))
    tk.append(st.submit(sets[2]))
    st.collect(tk[1]); st.collect(tk[2])
    assert st.build_stats()["device_builds"] == 1
    v = st.batch_of(tk[2], sets[2])
    v.report(); v.download()
    for i, w in enumerate(wins[2]):
        _check("stream set 2 (device-built) window %d" % i, w, R.HUBER, _grab(v, i, w))
    st.close()
    for s in sets:
        s.close()

"""Structure-only refinement on the device (slslam_line_refiner_run / slslam_lba_refine_lines, csrc/lba_refine_lines.h) against the
oracle applied to each line's own problem (tests/refine_lines_reference.py).

Parity rule, per line: step counts and termination type identical to the reference; initial cost, final cost and the four parameters
within 10 x the oracle's own movement when that line's start is scaled by (1 + 1e-13) (floors: 1e-10 absolute on parameters, 1e-12
relative on costs); a line whose ORACLE accept / reject sequence changes under that perturbation is left out of the count check, at
most 5 % of the lines.  Every test also checks that the camera parameters come back bitwise unchanged.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_lines_reference as R  # noqa: E402
from slslam_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def _window(name):
    if name not in _CACHE:
        if name == "A":
            w = synth.make_window(4, num_lines=60, num_kf=8, num_free=4)
        elif name == "B":
            w = synth.make_window(5, num_lines=40, num_kf=6, num_free=3)
            w["parameters"] = w["parameters"].copy()
            w["parameters"][6 * w["num_cameras"]:] += 0.05 * np.random.default_rng(5).standard_normal(4 * w["num_lines"])
        elif name == "B2":
            w = synth.make_window(6, num_lines=40, num_kf=6, num_free=3)
            w["parameters"] = w["parameters"].copy()
            w["parameters"][6 * w["num_cameras"]:] += 0.2 * np.random.default_rng(6).standard_normal(4 * w["num_lines"])
        elif name == "W150":
            w = synth.make_window(7, num_lines=150, num_kf=8, num_free=4)
        _CACHE[name] = w
    return _CACHE[name]


def _reference(name, **opt):
    key = ("ref", name, tuple(sorted(opt.items())))
    if key not in _CACHE:
        _CACHE[key] = R.reference(_window(name), **opt)
    return _CACHE[key]


def _run(hip, name):
    key = ("run", name)
    if key not in _CACHE:
        _CACHE[key] = hip.lba_refine_lines(_window(name))
    return _CACHE[key]


def _cameras_untouched(w, x):
    nc = 6 * int(w["num_cameras"])
    assert np.asarray(w["parameters"][:nc], dtype=np.float64).tobytes() == x[:nc].tobytes()


def _same_bytes(a, b):
    return a.tobytes() == b.tobytes()


def test_parity_one_wave(hip):
    w = _window("A")
    assert w["num_lines"] == 60 and len(w["camera_index"]) == 315
    ref = _reference("A")
    assert sum(r["num_unsuccessful_steps"] for r in ref) == 6 and sum(r["num_unsuccessful_steps"] > 0 for r in ref) == 3
    assert sum(r["termination_type"] == 2 for r in ref) == 46 and sum(r["termination_type"] == 0 for r in ref) == 14
    x, res, tot = _run(hip, "A")
    assert (res["status"] == hip.LINE_REFINED).all()
    R.check_parity(ref, x, res, w["num_cameras"], label="A")
    _cameras_untouched(w, x)
    assert tot["num_successful_steps"] == int(res["num_successful_steps"].sum())
    assert tot["num_residual_blocks"] == 315 and tot["num_free_parameters"] == 240
    assert abs(tot["final_cost"] - float(res["final_cost"].sum())) <= 1e-15 * 60


@pytest.mark.parametrize("name,rejected,lines", [("B", 21, 5), ("B2", 42, 9)])
def test_parity_many_rejections(hip, name, rejected, lines):
    w = _window(name)
    ref = _reference(name)
    assert sum(r["num_unsuccessful_steps"] for r in ref) == rejected
    assert sum(r["num_unsuccessful_steps"] > 0 for r in ref) == lines
    x, res, _ = _run(hip, name)
    R.check_parity(ref, x, res, w["num_cameras"], label=name)
    _cameras_untouched(w, x)


def test_wave_boundary_and_sorting(hip):
    """More lines than a wave: every line's result is, bit for bit, what the line alone gives - under the caller's numbering."""
    w = _window("W150")
    L, C = int(w["num_lines"]), int(w["num_cameras"])
    assert L > 64
    x, res, _ = _run(hip, "W150")
    _cameras_untouched(w, x)
    counts = np.bincount(np.asarray(w["line_index"]), minlength=L)
    assert len(set(counts.tolist())) > 1            # the sort by observation count permutes the lines
    for l in range(L):
        x1, r1, _ = hip.lba_refine_lines(R.one_line_window(w, l))
        assert _same_bytes(x1[-4:], x[6 * C + 4 * l:6 * C + 4 * l + 4]), l
        assert _same_bytes(r1[0:1], res[l:l + 1]), (l, r1[0], res[l])
        assert int(res[l]["num_observations"]) == counts[l]


def test_company_independence(hip):
    wa, wb = _window("A"), _window("W150")
    wc = R.one_line_window(wa, 7)
    rf = hip.LineRefiner(256, 2048)
    xs, rs, ts = rf.run([wa, wb, wc])
    rf.close()
    for w, x, r, t, solo in zip((wa, wb, wc), xs, rs, ts, (_run(hip, "A"), _run(hip, "W150"), hip.lba_refine_lines(wc))):
        assert _same_bytes(x, solo[0]) and _same_bytes(r, solo[1]) and t == solo[2]
        _cameras_untouched(w, x)


def test_edges(hip):
    wa = _window("A")
    C, L = int(wa["num_cameras"]), int(wa["num_lines"])
    x0, res0, _ = _run(hip, "A")
    li = np.asarray(wa["line_index"])
    counts = np.bincount(li, minlength=L)
    l_const, l_none, l_one, l_nan = 3, 11, 20, 31
    assert counts[l_one] >= 2
    f = np.array(wa["fixed_index"], dtype=np.int32).reshape(-1, 2).copy()
    f[np.nonzero(li == l_const)[0][-1], 1] = 1                       # ONE flagged observation makes the line constant
    obs = np.array(wa["observations"], dtype=np.float64).reshape(-1, 8).copy()
    obs[np.nonzero(li == l_nan)[0][1], 5] = np.nan
    keep = np.ones(len(li), dtype=bool)
    keep[li == l_none] = False
    keep[np.nonzero(li == l_one)[0][1:]] = False
    w = dict(wa)
    w["camera_index"] = np.asarray(wa["camera_index"])[keep]
    w["line_index"] = li[keep]
    w["fixed_index"] = f[keep].reshape(-1)
    w["observations"] = obs[keep]
    x, res, _ = hip.lba_refine_lines(w)
    _cameras_untouched(w, x)
    for l, st in ((l_const, hip.LINE_CONSTANT), (l_none, hip.LINE_NO_OBSERVATIONS), (l_nan, hip.LINE_INVALID)):
        assert int(res[l]["status"]) == st
        assert _same_bytes(x[6 * C + 4 * l:6 * C + 4 * l + 4], np.asarray(wa["parameters"], dtype=np.float64)[6 * C + 4 * l:6 * C + 4 * l + 4])
    assert int(res[l_one]["status"]) == hip.LINE_REFINED and int(res[l_one]["num_observations"]) == 1
    assert np.isfinite(x).all()
    x1, r1, _ = hip.lba_refine_lines(R.one_line_window(w, l_one))
    assert _same_bytes(x1[-4:], x[6 * C + 4 * l_one:6 * C + 4 * l_one + 4]) and _same_bytes(r1[0:1], res[l_one:l_one + 1])
    for l in range(L):
        if l in (l_const, l_none, l_one, l_nan):
            continue
        assert _same_bytes(x[6 * C + 4 * l:6 * C + 4 * l + 4], x0[6 * C + 4 * l:6 * C + 4 * l + 4]), l
        assert _same_bytes(res[l:l + 1], res0[l:l + 1]), l
    # an index out of range fails the whole call
    bad = dict(wa)
    bad["line_index"] = np.asarray(wa["line_index"]).copy()
    bad["line_index"][0] = L
    with pytest.raises(hip.SlslamError) as e:
        hip.lba_refine_lines(bad)
    assert e.value.status == 1


def test_zero_iterations_evaluates_the_costs(hip, oracle):
    w = _window("A")
    C = int(w["num_cameras"])
    x, res, _ = hip.lba_refine_lines(w, max_num_iterations=0)
    assert _same_bytes(x, np.asarray(w["parameters"], dtype=np.float64))
    ref = _reference("A")
    for l in range(int(w["num_lines"])):
        v = R.one_line_window(w, l)
        c = oracle.lba_cost(v, v["parameters"])
        tol = max(R.MARGIN * ref[l]["move_initial"], R.COST_FLOOR * abs(c))
        assert float(res[l]["initial_cost"]) == float(res[l]["final_cost"])
        assert abs(float(res[l]["initial_cost"]) - c) <= tol, (l, res[l], c, tol)
        assert int(res[l]["num_successful_steps"]) == 0 and int(res[l]["num_unsuccessful_steps"]) == 0


def test_parity_without_the_robust_loss(hip):
    w = _window("A")
    ref = _reference("A", huber_delta=0.0)
    x, res, _ = hip.lba_refine_lines(w, huber_delta=0.0)
    R.check_parity(ref, x, res, w["num_cameras"], label="A, huber_delta = 0")
    _cameras_untouched(w, x)


def test_reuse(hip):
    wa, wb = _window("A"), _window("W150")
    rf = hip.LineRefiner(64, 512)
    x1, r1, _ = rf.run([wa])
    a1 = rf.stats()
    x2, r2, _ = rf.run([wa])
    a2 = rf.stats()
    assert a2["allocations"] == a1["allocations"] and a2["calls"] == a1["calls"] + 1
    assert _same_bytes(x1[0], x2[0]) and _same_bytes(r1[0], r2[0])
    xs, rs, _ = rf.run([wb, wa, wb])                                   # beyond the capacities: succeeds, the buffers grew
    a3 = rf.stats()
    assert a3["allocations"] > a2["allocations"]
    assert _same_bytes(xs[1], x1[0]) and _same_bytes(xs[0], _run(hip, "W150")[0]) and _same_bytes(rs[2], _run(hip, "W150")[1])
    rf.close()

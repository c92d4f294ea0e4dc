"""The line triangulator on the device (slslam_line_triangulator_run / slslam_lba_triangulate_lines, csrc/lba_triangulate.h) against the
numpy reference (tests/lba_triangulate_reference.py).

Parity rule, per line: status, num_observations, num_planes, first_camera and clamped identical; (cp, v / |v|), the four orth parameters
(angles modulo 2 pi) and the eigenvalues within 10 x the reference's own movement when that line's observations are scaled by
(1 + 1e-13) (floors: 1e-12 absolute on unit vectors and angles - per metre on the closest point -, 1e-12 lambda1 on eigenvalues); a line
whose REFERENCE choice flips under that perturbation is left out of the status check - none on these windows, which every test asserts.
Every test also checks that the camera parameters come back bitwise unchanged.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_triangulate_reference as T  # noqa: E402
from slslam_amd import synth  # noqa: E402
from test_gpu_lba import _assert_summary_parity, _assert_trace_parity  # noqa: E402

pytestmark = pytest.mark.gpu

_CACHE = {}


def _window(name):
    if name not in _CACHE:
        if name == "A":
            w = synth.make_window(4, num_lines=60, num_kf=8, num_free=4, line_init="triangulate")
        elif name == "W150":
            w = synth.make_window(7, num_lines=150, num_kf=8, num_free=4, line_init="triangulate")
        _CACHE[name] = w
    return _CACHE[name]


def _reference(name, method, min_parallax=0.0):
    key = ("ref", name, method, min_parallax)
    if key not in _CACHE:
        _CACHE[key] = T.reference(_window(name), method=method, min_parallax=min_parallax)
    return _CACHE[key]


def _run(hip, name, method, min_parallax=0.0):
    key = ("run", name, method, min_parallax)
    if key not in _CACHE:
        _CACHE[key] = hip.lba_triangulate_lines(_window(name), method=method, min_parallax=min_parallax)
    return _CACHE[key]


def _cameras_untouched(w, x):
    nc = 6 * int(w["num_cameras"])
    assert np.asarray(w["parameters"][:nc], dtype=np.float64).tobytes() == x[:nc].tobytes()


def _line_bytes(w, x, res, av, l):
    C = int(w["num_cameras"])
    return x[6 * C + 4 * l:6 * C + 4 * l + 4].tobytes() + res[l:l + 1].tobytes() + av[l].tobytes()


def _parallax_gap(name):
    """A min_parallax between two adjacent sorted lambda2 / lambda1 of the reference, near the window's median, in a gap wider than
    100 x the ratios' own movement under the perturbation."""
    w = _window(name)
    li, ci = np.asarray(w["line_index"]), np.asarray(w["camera_index"])
    cams = [synth.wt_to_rt(c) for c in w["parameters"][:6 * w["num_cameras"]].reshape(-1, 6)]
    ratio, move = [], []
    for l in range(w["num_lines"]):
        sel = np.nonzero(li == l)[0]
        Rs, ts = [cams[c][0] for c in ci[sel]], [cams[c][1] for c in ci[sel]]
        a = T.triangulate_line(w["observations"][sel], Rs, ts)["ratio"]
        b = T.triangulate_line(w["observations"][sel] * (1.0 + T.PERTURB), Rs, ts)["ratio"]
        ratio.append(a); move.append(abs(a - b))
    order = np.argsort(ratio)
    mid = len(order) // 2
    for k in sorted(range(len(order) - 1), key=lambda k: abs(k + 1 - mid)):
        lo, hi = order[k], order[k + 1]
        if ratio[hi] - ratio[lo] > 100.0 * 2.0 * max(move[lo], move[hi], 1e-16):
            return 0.5 * (ratio[lo] + ratio[hi]), k + 1
    raise AssertionError("no gap")


@pytest.mark.parametrize("method", [0, 1])
def test_parity_one_wave(hip, method):
    w = _window("A")
    assert w["num_lines"] == 60 and len(w["camera_index"]) == 315
    ref = _reference("A", method)
    x, res, av = _run(hip, "A", method)
    _, left_out = T.check_parity(ref, w, x, res, av, label="A, method %d" % method)
    assert left_out == 0
    _cameras_untouched(w, x)
    assert (res["status"] == (hip.TRI_MULTIVIEW if method else hip.TRI_STEREO)).all()
    if method == 0:
        assert not res["eigenvalues"].any() and not res["num_planes"].any() and res["clamped"].sum() > 0
        # the (cp, v) output against the same header functions evaluated on the host: the same bits
        li, ci = np.asarray(w["line_index"]), np.asarray(w["camera_index"])
        cams = w["parameters"][:6 * w["num_cameras"]].reshape(-1, 6)
        for l in range(w["num_lines"]):
            sel = np.nonzero(li == l)[0]
            h = hip.triangulate_host(w["observations"][sel], cams[ci[sel]], method=0)
            assert h["av"].tobytes() == av[l].tobytes(), (l, h["av"], av[l])
            assert h["clamped"] == int(res[l]["clamped"]) and h["status"] == int(res[l]["status"])
    else:
        assert (res["num_planes"] == 2 * res["num_observations"]).all() and not res["clamped"].any()


@pytest.mark.parametrize("method", [0, 1])
def test_two_waves_and_a_ragged_tail(hip, method):
    w = _window("W150")
    counts = np.bincount(np.asarray(w["line_index"]), minlength=150)
    assert w["num_lines"] == 150 and counts.min() < counts.max()          # the sort by observation count permutes the lines
    ref = _reference("W150", method)
    x, res, av = _run(hip, "W150", method)
    _, left_out = T.check_parity(ref, w, x, res, av, label="W150, method %d" % method)
    assert left_out == 0
    _cameras_untouched(w, x)
    assert (res["num_observations"] == counts).all()


def test_a_lane_with_one_observation_beside_a_lane_with_eight(hip):
    w0 = _window("W150")
    li = np.asarray(w0["line_index"])
    counts = np.bincount(li, minlength=150)
    assert counts.max() >= 8
    keep = np.ones(len(li), dtype=bool)
    for l in (5, 70, 149):
        keep[np.nonzero(li == l)[0][1:]] = False
    w = dict(w0, camera_index=np.asarray(w0["camera_index"])[keep], line_index=li[keep],
             fixed_index=np.asarray(w0["fixed_index"]).reshape(-1, 2)[keep].reshape(-1), observations=w0["observations"][keep])
    ref = T.reference(w, method=1)
    x, res, av = hip.lba_triangulate_lines(w, method=1)
    _, left_out = T.check_parity(ref, w, x, res, av, label="W150 with three one-observation lines")
    assert left_out == 0
    for l in (5, 70, 149):
        assert int(res[l]["status"]) == hip.TRI_STEREO and int(res[l]["num_observations"]) == 1 and int(res[l]["num_planes"]) == 2
        assert not res[l]["eigenvalues"].any()
    _cameras_untouched(w, x)


def test_fallback_on_parallax(hip):
    w = _window("A")
    mp, below = _parallax_gap("A")
    ref = T.reference(w, method=1, min_parallax=mp)
    assert sum(r["status"] == T.STEREO for r in ref) == below and sum(r["status"] == T.MULTIVIEW for r in ref) == 60 - below
    assert 20 <= below <= 40
    x, res, av = hip.lba_triangulate_lines(w, method=1, min_parallax=mp)
    _, left_out = T.check_parity(ref, w, x, res, av, label="A, min_parallax %.4g" % mp)
    assert left_out == 0
    assert int((res["status"] == hip.TRI_STEREO).sum()) == below and int((res["status"] == hip.TRI_MULTIVIEW).sum()) == 60 - below
    assert not res["eigenvalues"][res["status"] == hip.TRI_STEREO].any()
    # a fallback line is, bit for bit, the method 0 line
    x0, _, av0 = _run(hip, "A", 0)
    for l in np.nonzero(res["status"] == hip.TRI_STEREO)[0]:
        assert x[48 + 4 * l:52 + 4 * l].tobytes() == x0[48 + 4 * l:52 + 4 * l].tobytes() and av[l].tobytes() == av0[l].tobytes()
    _cameras_untouched(w, x)


def _exact_pair(B=synth.BASELINE):
    """Two abscissae x with (x + B) - B == x: a right segment that is, in the kernel's arithmetic, the left one."""
    xs = [x for x in np.arange(-32, 33) / 64.0 if (x + B) - B == x]
    assert len(xs) >= 2
    return xs[0], xs[-1]


def test_statuses(hip):
    wa = _window("A")
    C, L = int(wa["num_cameras"]), int(wa["num_lines"])
    x0, res0, av0 = _run(hip, "A", 1)
    li, ci = np.asarray(wa["line_index"]), np.asarray(wa["camera_index"])
    counts = np.bincount(li, minlength=L)
    l_none, l_const, l_nan, l_zero, l_same = 11, 3, 31, 40, 20
    assert counts[l_zero] >= 3
    seen_by = [set(ci[li == l]) for l in range(L)]
    c_bad = next(c for c in range(C) if 0 < sum(c in s for s in seen_by) < L and all(c not in seen_by[l] for l in (l_zero, l_same, l_const)))
    f = np.array(wa["fixed_index"], dtype=np.int32).reshape(-1, 2).copy()
    f[np.nonzero(li == l_const)[0][-1], 1] = 1
    obs = np.array(wa["observations"], dtype=np.float64).reshape(-1, 8).copy()
    obs[np.nonzero(li == l_nan)[0][1], 5] = np.nan
    k = np.nonzero(li == l_zero)[0][1]
    obs[k, 2:4] = obs[k, 0:2]                                            # a left segment of zero length, not in the first observation
    k = np.nonzero(li == l_same)[0][0]
    xa, xb = _exact_pair()
    obs[k] = [xa, 0.25, xb, -0.125, xa, 0.25, xb, -0.125]                # right segment = left segment: parallel planes, v = 0
    keep = np.ones(len(li), dtype=bool)
    keep[li == l_none] = False
    keep[np.nonzero(li == l_same)[0][1:]] = False
    prm = np.array(wa["parameters"], dtype=np.float64)
    prm[6 * c_bad + 4] = np.nan
    w = dict(wa, camera_index=ci[keep], line_index=li[keep], fixed_index=f[keep].reshape(-1), observations=obs[keep], parameters=prm)
    ref = T.reference(w, method=1)
    l_cam = [l for l in range(L) if c_bad in seen_by[l] and l not in (l_none,)]
    assert l_cam and ref[l_same]["status"] == T.INVALID and ref[l_zero]["num_planes"] == 2 * counts[l_zero] - 1
    x, res, av = hip.lba_triangulate_lines(w, method=1)
    _, left_out = T.check_parity(ref, w, x, res, av, label="statuses")
    assert left_out == 0
    assert x[:6 * C].tobytes() == prm[:6 * C].tobytes()                  # the NaN camera included
    want = {l_none: hip.TRI_NO_OBSERVATIONS, l_const: hip.TRI_CONSTANT, l_nan: hip.TRI_INVALID, l_same: hip.TRI_INVALID,
            l_zero: hip.TRI_MULTIVIEW}
    want.update({l: hip.TRI_INVALID for l in l_cam if l not in (l_nan,)})
    for l in range(L):
        sl = slice(6 * C + 4 * l, 6 * C + 4 * l + 4)
        if l in want:
            assert int(res[l]["status"]) == want[l], (l, res[l])
            if want[l] != hip.TRI_MULTIVIEW:
                assert x[sl].tobytes() == prm[sl].tobytes() and np.isnan(av[l]).all(), l          # untouched
                assert int(res[l]["num_planes"]) == 0 and not res[l]["eigenvalues"].any() and int(res[l]["clamped"]) == 0
        else:
            assert _line_bytes(w, x, res, av, l) == _line_bytes(wa, x0, res0, av0, l), l          # the others: unaffected
    assert int(res[l_zero]["num_planes"]) == 2 * counts[l_zero] - 1
    assert int(res[l_none]["first_camera"]) == -1 and int(res[l_none]["num_observations"]) == 0
    assert int(res[l_const]["num_observations"]) == counts[l_const] and int(res[l_same]["num_observations"]) == 1


def test_independence_and_reuse(hip):
    wa, wb = _window("A"), _window("W150")
    L = int(wa["num_lines"])
    perm = np.random.default_rng(3).permutation(L)
    prm = np.array(wa["parameters"], dtype=np.float64)
    wp = dict(wa, line_index=perm[np.asarray(wa["line_index"])].astype(np.int32), parameters=prm)
    solo = _run(hip, "A", 1)
    tr = hip.LineTriangulator(64, 512)
    x1, r1, a1 = tr.run([wa])
    s1 = tr.stats()
    x2, r2, a2 = tr.run([wa])
    s2 = tr.stats()
    assert s2["allocations"] == s1["allocations"] and s2["calls"] == s1["calls"] + 1          # a run that fits allocates nothing
    xs, rs, avs = tr.run([wa, wb, wp])                                                         # beyond the capacities: the buffers grow
    assert tr.stats()["allocations"] > s2["allocations"]
    tr.close()
    big = _run(hip, "W150", 1)
    for l in range(L):
        b = _line_bytes(wa, solo[0], solo[1], solo[2], l)
        assert b == _line_bytes(wa, x1[0], r1[0], a1[0], l) == _line_bytes(wa, x2[0], r2[0], a2[0], l) == _line_bytes(wa, xs[0], rs[0], avs[0], l), l
        assert b == _line_bytes(wp, xs[2], rs[2], avs[2], int(perm[l])), l
    for l in range(int(wb["num_lines"])):
        assert _line_bytes(wb, big[0], big[1], big[2], l) == _line_bytes(wb, xs[1], rs[1], avs[1], l), l
    for w, x in zip((wa, wb, wp), xs):
        _cameras_untouched(w, x)


def _project(P, B=synth.BASELINE):
    return np.array([P[0][0] / P[0][2], P[0][1] / P[0][2], P[1][0] / P[1][2], P[1][1] / P[1][2],
                     (P[0][0] - B) / P[0][2], P[0][1] / P[0][2], (P[1][0] - B) / P[1][2], P[1][1] / P[1][2]])


def test_clamp_and_flip(hip):
    """A hand-made window, one identity camera, exact projections: the reference's stereo-first |cp| is < 0.1 for line 0, > 10 for line 1,
    cp.z < 0 for line 2, none of it for line 3 - each at least 1e-6 from its edge."""
    lines = [(np.array([0.03, 0.0, 0.04]), np.array([-4.0, 5.0, 3.0])), (np.array([12.0, 0.0, 1.0]), np.array([-0.05, 1.0, 0.6])),
             (np.array([0.2, 1.0, -0.5]), np.array([0.0, 0.5, 1.0])), (np.array([0.5, 1.0, 0.2]), np.array([-0.4, 0.0, 1.0]))]
    obs = np.array([_project([cp + s * d / np.linalg.norm(d) for s in (3.0, 5.0)]) for cp, d in lines])
    w = {"num_cameras": 1, "num_lines": 4, "camera_index": np.zeros(4, dtype=np.int32), "line_index": np.arange(4, dtype=np.int32),
         "fixed_index": np.zeros(8, dtype=np.int32), "observations": obs, "parameters": np.zeros(6 + 16), "baseline": synth.BASELINE}
    for method in (0, 1):
        ref = T.reference(w, method=method)
        assert ref[0]["cpn"] < 0.1 - 1e-6 and ref[1]["cpn"] > 10.0 + 1e-6 and 0.1 + 1e-6 < ref[2]["cpn"] < 10.0 - 1e-6
        assert ref[2]["cpz"] < -1e-6 and all(ref[i]["cpz"] > 1e-6 for i in (0, 1, 3))
        assert 0.1 + 1e-6 < ref[3]["cpn"] < 10.0 - 1e-6 and [r["clamped"] for r in ref] == [1, 1, 0, 0]
        assert ref[2]["av"][2] > 0                                       # flipped
        x, res, av = hip.lba_triangulate_lines(w, method=method)
        _, left_out = T.check_parity(ref, w, x, res, av, label="clamp and flip, method %d" % method)
        assert left_out == 0
        assert res["clamped"].tolist() == [1, 1, 0, 0] and (res["status"] == hip.TRI_STEREO).all()
        assert abs(np.linalg.norm(av[0][:3]) - 10.0) < 1e-9 and abs(np.linalg.norm(av[1][:3]) - 10.0) < 1e-9      # 1 / inverse_depth
        assert av[2][2] > 0
    x5, _, av5 = hip.lba_triangulate_lines(w, method=0, inverse_depth=0.2)
    assert abs(np.linalg.norm(av5[0][:3]) - 5.0) < 1e-9 and av5[3].tobytes() == av[3].tobytes()


@pytest.mark.parametrize("method,init", [(0, "triangulate"), (1, "multiview")])
def test_window_solve_from_the_device_start(hip, oracle, method, init):
    """End to end: hip.lba_solve of window A from the device's stereo-first and multi-view starts reproduces the oracle's runs of
    tests/test_lba_triangulate_cpu.py (from synth's starts), iteration by iteration (the helpers of tests/test_gpu_lba.py)."""
    w = _window("A")
    x, res, _ = _run(hip, "A", method)
    ws = synth.make_window(4, num_lines=60, num_kf=8, num_free=4, line_init=init)
    x0, s0, t0 = oracle.lba_solve(ws, linear_solver=1)
    x1, s1, t1 = hip.lba_solve(w, params=x)
    print("method %d: oracle %.9e -> %.9e (%d + %d steps), device %.9e -> %.9e (%d + %d steps)"
          % (method, s0["initial_cost"], s0["final_cost"], s0["num_successful_steps"], s0["num_unsuccessful_steps"],
             s1["initial_cost"], s1["final_cost"], s1["num_successful_steps"], s1["num_unsuccessful_steps"]))
    for a, b in zip(t0, t1):
        print("  it %2d  accepted %d/%d  cost %.12e / %.12e  radius %.6e / %.6e" % (a["iteration"], a["step_is_successful"],
              b["step_is_successful"], a["cost"], b["cost"], a["trust_region_radius"], b["trust_region_radius"]))
    _assert_trace_parity(t0, t1, n=4)
    _assert_summary_parity(s0, s1)

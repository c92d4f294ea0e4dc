"""Host side of the line triangulator, no GPU: the numpy reference (tests/lba_triangulate_reference.py) against synth and against a known
line, the device's header functions evaluated on the host, the host glue under the sanitizers (a stand-alone program), the C struct
against its ctypes mirror, argument checks, and what the multi-view start buys the window solve (oracle only)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_triangulate_reference as T  # noqa: E402
from slslam_amd import capi, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "slslam_amd", "csrc")


def _window_a(line_init="triangulate"):
    return synth.make_window(4, num_lines=60, num_kf=8, num_free=4, line_init=line_init)


def test_method_0_is_synths_stereo_start():
    """Window A: the reference's method 0 is synth._initialize_lm followed by the world transform - make_window's "triangulate" lines."""
    w = _window_a()
    C6 = 6 * w["num_cameras"]
    ref = T.reference(w, method=0, yardstick=False)
    assert all(r["status"] == T.STEREO and r["num_planes"] == 0 and not r["eigenvalues"].any() for r in ref)
    got = np.array([r["orth"] for r in ref])
    d = np.abs(T.angle_diff(got, w["parameters"][C6:].reshape(-1, 4))).max()
    print("method 0 against synth: largest angle difference %.3g" % d)
    assert d <= 1e-13
    assert sum(r["clamped"] for r in ref) > 0                       # window A has lines the clamp moves


def test_line_init_values_keep_their_bytes_and_multiview_is_the_reference():
    wt, wm, wp = _window_a(), _window_a("multiview"), synth.make_window(4, num_lines=60, num_kf=8, num_free=4)
    C6 = 6 * wt["num_cameras"]
    for k in ("camera_index", "line_index", "fixed_index", "observations", "true_parameters"):
        assert np.asarray(wt[k]).tobytes() == np.asarray(wm[k]).tobytes() == np.asarray(wp[k]).tobytes(), k
    assert wt["parameters"][:C6].tobytes() == wm["parameters"][:C6].tobytes() == wp["parameters"][:C6].tobytes()
    ref = T.reference(wt, method=1, min_parallax=0.0, yardstick=False)
    assert all(r["status"] == T.MULTIVIEW for r in ref)
    assert np.abs(T.angle_diff(np.array([r["orth"] for r in ref]), wm["parameters"][C6:].reshape(-1, 4))).max() <= 1e-13
    with pytest.raises(ValueError):
        _window_a("nonsense")


def test_multiview_recovers_a_known_line_from_three_cameras():
    """Exact projections (noise 0, true cameras) of known lines seen from 3 keyframes: the multi-view line is the line, within the
    reference's own movement under the (1 + 1e-13) perturbation of the observations x 10 (floor 1e-12, per metre on the closest point)."""
    w = synth.make_window(11, num_lines=40, num_kf=3, num_free=3, noise_px=0.0, pose_sigma_t=0.0, pose_sigma_r_deg=0.0, mean_track=50.0)
    ref = T.reference(w, method=1)
    truth = synth.orth_to_av(w["true_parameters"][18:].reshape(-1, 4))
    n, worst = 0, 0.0
    for l, r in enumerate(ref):
        if r["num_observations"] != 3:
            continue
        assert r["status"] == T.MULTIVIEW and r["num_planes"] == 6 and r["stable"]
        av, tr = T.unit_av(r["av"]), T.unit_av(truth[l])
        if np.dot(av[3:], tr[3:]) < 0:
            av[3:] = -av[3:]
        scale = max(1.0, float(np.linalg.norm(tr[:3])))
        tol = np.r_[[max(T.MARGIN * r["move_av"], T.UNIT_FLOOR * scale)] * 3, [max(T.MARGIN * r["move_av"], T.UNIT_FLOOR)] * 3]
        ratio = float((np.abs(av - tr) / tol).max())
        worst, n = max(worst, ratio), n + 1
        assert ratio <= 1.0, (l, av, tr, tol)
        # exact planes of one line span a pencil: the Gram matrix has rank 2
        assert r["eigenvalues"][2] <= 1e-9 * r["eigenvalues"][0]
    print("%d lines seen from 3 cameras, worst deviation / tolerance %.3g" % (n, worst))
    assert n >= 10


def test_header_functions_on_the_host_against_the_reference():
    """slslam_debug_triangulate_host - the kernel's functions compiled for the host - on every line of window A, methods 0 and 1, and
    with a min_parallax in the middle of the window's ratios: the parity rule of the device tests; the off-diagonal norm the Jacobi
    sweeps leave is printed (DESIGN.md 4.6 records it)."""
    w = _window_a()
    li, ci = np.asarray(w["line_index"]), np.asarray(w["camera_index"])
    cams = w["parameters"][:6 * w["num_cameras"]].reshape(-1, 6)
    ratios = sorted(r["ratio"] for r in T.reference(w, method=1, yardstick=False))
    mid = 0.5 * (ratios[29] + ratios[30])
    off = 0.0
    for method, mp in ((0, 0.0), (1, 0.0), (1, mid)):
        ref = T.reference(w, method=method, min_parallax=mp)
        res = np.zeros(w["num_lines"], dtype=np.dtype(capi.TriangulatedLine))
        av = np.full((w["num_lines"], 6), np.nan)
        x = w["parameters"].copy()
        for l in range(w["num_lines"]):
            sel = np.nonzero(li == l)[0]
            h = capi.triangulate_host(w["observations"][sel], cams[ci[sel]], method=method, min_parallax=mp)
            res[l] = (h["status"], len(sel), h["num_planes"], ci[sel[0]], tuple(h["eigenvalues"]), h["clamped"], 0)
            av[l] = h["av"]
            x[48 + 4 * l:48 + 4 * l + 4] = synth.av_to_orth(h["av"])
            off = max(off, h["offdiagonal"] / max(h["eigenvalues"][0], 1e-300) if h["status"] == T.MULTIVIEW else 0.0)
        _, left_out = T.check_parity(ref, w, x, res, av, label="host, method %d, min_parallax %.3g" % (method, mp))
        assert left_out == 0
    print("largest off-diagonal norm after %s sweeps, relative to lambda1: %.3g" % ("the kernel's", off))
    assert off <= 1e-15


def test_refine_layout_is_reused():
    """One layout, one plan: over all of csrc, refine_layout_build is called once - from the plan the refiner and the triangulator share
    (line_call_plan.h) -, and neither call nor the shared files bring a sort or placement of their own."""
    calls = {}
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        k = text.count("refine_layout_build(") - text.count("inline void refine_layout_build(")
        if k:
            calls[f] = k
    assert calls == {"line_call_plan.h": 1}, calls
    plan = open(os.path.join(CSRC, "line_call_plan.h")).read()
    assert '#include "lba_refine_layout.h"' in plan
    for f in ("lba_triangulate_host.h", "lba_triangulate.h", "triangulate_api.hip", "lba_refine_host.h", "lba_refine_lines.h", "lba_refine_api.h",
              "line_call_plan.h", "line_call_handle.h"):
        text = open(os.path.join(CSRC, f)).read()
        assert "bucket" not in text and "W.dest[" not in text.replace("W.dest[(size_t)k]", "") and "group_row.push_back" not in text, f
    for f in ("lba_triangulate_host.h", "lba_refine_host.h"):
        assert '#include "line_call_plan.h"' in open(os.path.join(CSRC, f)).read(), f


def test_host_glue_under_the_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "triangulate_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "triangulate_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triangulate host ok" in r.stdout


def test_struct_matches_the_header():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "triangulate_abi_probe")
    subprocess.check_call(["gcc", "-std=c99", os.path.join(ROOT, "tests", "host_cxx", "triangulate_abi_probe.c"), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert int(got.pop("slslam_triangulated_line")) == C.sizeof(capi.TriangulatedLine) == np.dtype(capi.TriangulatedLine).itemsize
    for f, _ in capi.TriangulatedLine._fields_:
        assert int(got.pop("slslam_triangulated_line.%s" % f)) == getattr(capi.TriangulatedLine, f).offset, f
    assert tuple(int(got.pop("SLSLAM_TRI_" + k)) for k in ("MULTIVIEW", "STEREO", "CONSTANT", "NO_OBSERVATIONS", "INVALID")) == \
        (capi.TRI_MULTIVIEW, capi.TRI_STEREO, capi.TRI_CONSTANT, capi.TRI_NO_OBSERVATIONS, capi.TRI_INVALID) == \
        (T.MULTIVIEW, T.STEREO, T.CONSTANT, T.NO_OBSERVATIONS, T.INVALID)
    assert not got, got


def test_symbols_and_argument_checks_without_a_device():
    L = capi.lib()
    for name in ("slslam_line_triangulator_create", "slslam_line_triangulator_destroy", "slslam_line_triangulator_run",
                 "slslam_line_triangulator_stats", "slslam_lba_triangulate_lines", "slslam_debug_triangulate_host"):
        assert name in capi.EXPORTS and hasattr(L, name)
    assert L.slslam_line_triangulator_create(-1, None, 1, 1, None) == 1
    assert L.slslam_line_triangulator_run(None, 0, None, 1, 0.1, 0.0, None, None) == 1
    assert L.slslam_lba_triangulate_lines(None, None, 1, 0.1, 0.0, None, None) == 1
    tr = capi.LineTriangulator(64, 512)
    assert tr.stats() == {"calls": 0, "allocations": 0}
    w = _window_a()
    x0 = np.asarray(w["parameters"], dtype=np.float64).copy()
    bad_line = dict(w, line_index=np.asarray(w["line_index"]).copy())
    bad_line["line_index"][0] = w["num_lines"]
    bad_cam = dict(w, camera_index=np.asarray(w["camera_index"]).copy())
    bad_cam["camera_index"][5] = -1
    calls = [(bad_line, {}), (bad_cam, {}), (w, dict(method=2)), (w, dict(method=-1)), (w, dict(min_parallax=float("nan"))),
             (w, dict(min_parallax=-1e-3)), (w, dict(inverse_depth=0.0)), (w, dict(inverse_depth=-0.1)),
             (w, dict(inverse_depth=float("inf"))), (w, dict(inverse_depth=float("nan")))]
    for v, kw in calls:
        for call in (lambda: tr.run([w, v], **kw), lambda: capi.lba_triangulate_lines(v, **kw)):
            with pytest.raises(capi.SlslamError) as e:
                call()
            assert e.value.status == 1, kw
    assert tr.stats() == {"calls": 0, "allocations": 0}
    assert np.asarray(w["parameters"]).tobytes() == x0.tobytes()
    # a run with nothing for the device needs none: no windows; a window whose lines are all constant
    assert tr.run([]) == ([], [], [])
    f = np.array(w["fixed_index"], dtype=np.int32).reshape(-1, 2).copy()
    f[:, 1] = 1
    xs, rs, avs = tr.run([dict(w, fixed_index=f.reshape(-1))])
    assert (rs[0]["status"] == capi.TRI_CONSTANT).all() and xs[0].tobytes() == x0.tobytes() and np.isnan(avs[0]).all()
    assert (rs[0]["num_observations"] == np.bincount(w["line_index"], minlength=60)).all() and (rs[0]["first_camera"] >= 0).all()
    assert tr.stats() == {"calls": 2, "allocations": 0}
    tr.close()


def test_multiview_start_pays_in_the_window_solve(oracle):
    """The two windows of the issue's table, oracle only, default options (the reference's 10 iterations): the multi-view start's
    initial cost and its cost after the solve, summed over the two windows, are below the stereo-first start's.
    Measured: see the printed values (the ratios are above 7)."""
    tot = {}
    for init in ("triangulate", "multiview"):
        ini = fin = 0.0
        for seed in (4, 7):
            w = synth.make_window(seed, num_lines=60, num_kf=8, num_free=4, line_init=init)
            _, s, _ = oracle.lba_solve(w)
            print("seed %d, %-11s: cost %.6e -> %.6e, %d accepted and %d rejected steps, termination %d"
                  % (seed, init, s["initial_cost"], s["final_cost"], s["num_successful_steps"], s["num_unsuccessful_steps"], s["termination_type"]))
            ini, fin = ini + s["initial_cost"], fin + s["final_cost"]
        tot[init] = (ini, fin)
    print("summed initial cost: stereo-first %.6e, multi-view %.6e (ratio %.1f); after the solve: %.6e, %.6e (ratio %.1f)"
          % (tot["triangulate"][0], tot["multiview"][0], tot["triangulate"][0] / tot["multiview"][0],
             tot["triangulate"][1], tot["multiview"][1], tot["triangulate"][1] / tot["multiview"][1]))
    assert tot["multiview"][0] < tot["triangulate"][0]
    assert tot["multiview"][1] < tot["triangulate"][1]

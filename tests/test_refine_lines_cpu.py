"""Host side of the structure-only refinement, no GPU: the reference helper (the per-line problems ARE the joint problem), the
lane-interleaved layout under the sanitizers (a stand-alone program), the C structs against their ctypes mirrors, argument checks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_lines_reference as R  # noqa: E402
from slslam_amd import capi, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")


def test_per_line_problems_are_the_joint_problem(oracle):
    """Window A: the sum of the per-line final costs is the joint optimum of the window with every camera constant, run to convergence.
    Tolerance from that solve's own last cost_change: it stopped because a step changed the cost by less than function_tolerance x cost,
    so its distance to the optimum is of that order; 10 x it (and the same for the per-line solves) is allowed."""
    w = synth.make_window(4, num_lines=60, num_kf=8, num_free=4)
    assert w["num_lines"] == 60 and len(w["camera_index"]) == 315
    ref = R.reference(w, yardstick=False, max_num_iterations=200)
    total = sum(r["final_cost"] for r in ref)
    _, s, tr = oracle.lba_solve(R.all_cameras_constant(w), max_num_iterations=200)
    assert s["termination_type"] != 0, s
    last = abs(tr[-1]["cost_change"]) if abs(tr[-1]["cost_change"]) > 0 else 1e-6 * s["final_cost"]
    rel = 10.0 * max(last / s["final_cost"], 1e-6)
    print("joint %.10e  per-line sum %.10e  last cost_change %.3e  relative tolerance %.3e  difference %.3e"
          % (s["final_cost"], total, last, rel, abs(total - s["final_cost"]) / s["final_cost"]))
    assert abs(total - s["final_cost"]) <= rel * s["final_cost"]
    assert abs(sum(r["initial_cost"] for r in ref) - s["initial_cost"]) <= 1e-12 * s["initial_cost"]


def test_layout_under_the_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "refine_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "refine_layout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine layout ok" in r.stdout


def test_host_side_under_the_sanitizers():
    """The plan, the upload image and the scatter of a refiner run (csrc/lba_refine_host.h over csrc/line_call_plan.h), no device."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "refine_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_cxx", "refine_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine host ok" in r.stdout


def test_structs_match_the_header():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "refine_abi_probe")
    subprocess.check_call(["gcc", "-std=c99", os.path.join(ROOT, "tests", "host_cxx", "refine_abi_probe.c"), "-o", exe])
    got = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    for name, T in (("slslam_line_result", capi.LineResult), ("slslam_summary", capi.Summary), ("slslam_lba_window", capi.LBAWindow)):
        assert int(got.pop(name)) == C.sizeof(T), name
        for f, _ in T._fields_:
            assert int(got.pop("%s.%s" % (name, f))) == getattr(T, f).offset, (name, f)
    assert np.dtype(capi.LineResult).itemsize == C.sizeof(capi.LineResult)
    assert (int(got.pop("SLSLAM_LINE_REFINED")), int(got.pop("SLSLAM_LINE_CONSTANT")), int(got.pop("SLSLAM_LINE_NO_OBSERVATIONS")),
            int(got.pop("SLSLAM_LINE_INVALID"))) == (capi.LINE_REFINED, capi.LINE_CONSTANT, capi.LINE_NO_OBSERVATIONS, capi.LINE_INVALID)
    assert not got, got                      # every field the header has is mirrored


def test_symbols_and_argument_checks_without_a_device():
    L = capi.lib()
    for name in ("slslam_line_refiner_create", "slslam_line_refiner_destroy", "slslam_line_refiner_run", "slslam_line_refiner_stats",
                 "slslam_lba_refine_lines"):
        assert name in capi.EXPORTS and hasattr(L, name)
    assert L.slslam_line_refiner_create(-1, None, 1, 1, None) == 1
    assert L.slslam_line_refiner_run(None, 0, None, None, None) == 1
    assert L.slslam_lba_refine_lines(None, None, None, None) == 1
    rf = capi.LineRefiner(64, 512)
    assert rf.stats() == {"calls": 0, "allocations": 0}
    w = synth.make_window(4, num_lines=60, num_kf=8, num_free=4)
    bad = dict(w)
    bad["camera_index"] = np.asarray(w["camera_index"]).copy()
    bad["camera_index"][5] = w["num_cameras"]
    x0 = np.asarray(bad["parameters"], dtype=np.float64).copy()
    try:
        rf.run([bad])
        raise AssertionError("an out-of-range camera index was accepted")
    except capi.SlslamError as e:
        assert e.status == 1
    assert rf.stats() == {"calls": 0, "allocations": 0}
    assert (np.asarray(bad["parameters"]) == x0).all()
    # a run with nothing to refine needs no device: no windows; a window whose lines are all constant
    assert rf.run([]) == ([], [], [])
    allc = dict(w)
    f = np.array(w["fixed_index"], dtype=np.int32).reshape(-1, 2).copy()
    f[:, 1] = 1
    allc["fixed_index"] = f.reshape(-1)
    xs, rs, ts = rf.run([allc])
    assert (rs[0]["status"] == capi.LINE_CONSTANT).all() and xs[0].tobytes() == x0.tobytes()
    assert ts[0]["num_free_parameters"] == 0 and ts[0]["termination_type"] == 2
    assert rf.stats()["allocations"] == 0
    rf.close()

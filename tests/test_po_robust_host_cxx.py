"""POProblem::set_robustify (slslam_amd/host/po_problem.h) reaches the C ABI: the facade's ceres::Solve passes po_huber_delta = 0.001
for a robust pose graph (reference src/po_problem.cpp:55: robustify ? new HuberLoss(0.001) : NULL) and 0 otherwise.  Observed by a C++
program that defines slslam_po_solve itself (tests/host_cxx/po_robustify_seam.cpp).  No device needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slslam_amd", "host")
LIBDIR = os.path.join(ROOT, "slslam_amd", "_lib")
EXE = os.path.join(ROOT, "tests", "_build", "po_robustify_seam")


def test_set_robustify_reaches_the_c_abi():
    subprocess.check_call(["make", "-s", "-C", HOST])
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-I", HOST, "-o", EXE, os.path.join(ROOT, "tests", "host_cxx", "po_robustify_seam.cpp"),
                           "-L", LIBDIR, "-lslslam_host", "-lslslam_hip", "-Wl,-rpath," + LIBDIR])
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "calls 3"                                       # every ceres::Solve went through the program's slslam_po_solve
    rows = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in lines[:3]]
    assert [r["robust"] for r in rows] == ["0", "1", "0"]
    assert [float(r["po_huber_delta"]) for r in rows] == [0.0, 0.001, 0.0]
    # the LBA loss is not what switches: existing callers see the same huber_delta as before, whatever robustify says
    assert len({r["huber_delta"] for r in rows}) == 1 and abs(float(rows[0]["huber_delta"]) - 1.0 / 406.05) < 1e-18
    assert all(r["backend"] == "0" and r["blocks"] == "2" for r in rows)

"""csrc/lm_policy.h on the host: the trust-region policy of every device LM loop against the oracle's lm_core.c, stopping rule by
stopping rule (tests/host_cxx/lm_policy_check.cpp, a stand-alone program under ASan + UBSan)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_policy_against_the_oracle_under_the_sanitizers():
    os.makedirs(BUILD, exist_ok=True)
    obj, exe = os.path.join(BUILD, "lm_core_asan.o"), os.path.join(BUILD, "lm_policy_check")
    subprocess.check_call(["gcc", "-std=c99"] + SAN + ["-c", os.path.join(ROOT, "oracle", "lm_core.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17"] + SAN + [os.path.join(ROOT, "tests", "host_cxx", "lm_policy_check.cpp"), obj, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lm policy ok" in r.stdout

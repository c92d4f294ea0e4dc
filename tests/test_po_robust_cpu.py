"""Host-side checks of the pose graph's robust loss (slslam_solver_options.po_huber_delta, slslam_po_edge_report): the CPU reference the
GPU tests compare with (tests/po_robust_reference.py) is the oracle when the loss is off; the option is the struct's last field and off
by default; a bad value is refused before any device is asked for.  No device needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_robust_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = 1, 2


@pytest.mark.parametrize("n,loops", [(24, 3), (60, 4)])
def test_reference_helper_without_loss_is_the_oracle(oracle, n, loops):
    g = synth.make_pose_graph(7, n, loops)
    x0, s0, t0 = oracle.po_solve(g)
    x1, s1, t1 = ref.po_solve(g, 0.0)
    assert np.abs(x0 - x1).max() < 1e-12
    for k in ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks"):
        assert s0[k] == s1[k], k
    assert len(t0) == len(t1) and abs(s0["final_cost"] - s1["final_cost"]) <= 1e-12 * s0["final_cost"]
    sq, w = ref.edge_report(g, x1, 0.0)
    assert np.all(w == 1.0) and abs(0.5 * sq.sum() - oracle.po_cost(g, x1)) <= 1e-12 * oracle.po_cost(g, x1)


def test_option_is_last_field_and_off_by_default(tmp_path):
    o = capi.default_options()
    assert o.po_huber_delta == 0.0
    assert capi.SolverOptions._fields_[-1][0] == "po_huber_delta"
    off = capi.SolverOptions.po_huber_delta.offset
    assert off + C.sizeof(C.c_double) == C.sizeof(capi.SolverOptions)
    # the C side: sizeof, the field's offset, and every earlier field where it was (device_build was the last one)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "slslam_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(slslam_solver_options), offsetof(slslam_solver_options, po_huber_delta),'
                   ' offsetof(slslam_solver_options, device_build)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, off_c, off_db = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(capi.SolverOptions) and off_c == off and off_c + 8 == size
    assert off_db == capi.SolverOptions.device_build.offset
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slslam_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct slslam_solver_options \{(.*?)\} slslam_solver_options;", text, re.S).group(1)
    assert [f.split()[-1] for f in body.split(";") if f.strip()] == [f[0] for f in capi.SolverOptions._fields_]


@pytest.mark.parametrize("delta", [-0.001, -np.inf, np.inf, np.nan])
def test_bad_delta_is_invalid_argument_everywhere(delta):
    g = synth.make_pose_graph(2, num_poses=12, num_loops=1)
    with pytest.raises(capi.SlslamError) as ei:
        capi.po_solve(g, po_huber_delta=delta)
    assert ei.value.status == INVALID
    b = capi.POBatch()
    b.add(g)
    with pytest.raises(capi.SlslamError) as ei:
        b.finalize(po_huber_delta=delta)
    assert ei.value.status == INVALID
    b.close()
    with pytest.raises(capi.SlslamError) as ei:
        capi.po_edge_report(g, po_huber_delta=delta)
    assert ei.value.status == INVALID


def test_edge_report_validates_then_asks_for_a_device():
    g = synth.make_pose_graph(2, num_poses=12, num_loops=1)
    bad = dict(g, pose_index_2=g["pose_index_2"].copy()); bad["pose_index_2"][1] = 99
    nan = dict(g, parameters=g["parameters"].copy()); nan["parameters"][7] = np.nan
    for gb in (bad, nan, dict(g, constraints=np.where(np.arange(g["constraints"].size).reshape(g["constraints"].shape) == 3, np.inf, g["constraints"]))):
        with pytest.raises(capi.SlslamError) as ei:
            capi.po_edge_report(gb, po_huber_delta=0.001)
        assert ei.value.status == INVALID
    L = capi.lib()
    assert L.slslam_po_edge_report(None, 0.0, None, None) == INVALID
    i1, i2, cons, x = capi._po_arrays(g)
    cg = capi.POGraph(int(g["num_poses"]), len(i1), capi._ip(i1), capi._ip(i2), None, capi._dp(x))
    assert L.slslam_po_edge_report(C.byref(cg), 0.0, None, None) == INVALID
    if capi.device_count() == 0:
        with pytest.raises(capi.SlslamError) as ei:
            capi.po_edge_report(g, po_huber_delta=0.001)
        assert ei.value.status == NO_DEVICE
        b = capi.POBatch()                                  # the batch getter: no results without a download
        b.add(g)
        with pytest.raises(capi.SlslamError) as ei:
            b.edge_report(0)
        assert ei.value.status == 5
        b.close()
    else:
        sq, w = capi.po_edge_report(g, po_huber_delta=0.001)
        assert sq.shape == w.shape == (len(i1),) and np.all(w > 0) and np.all(w <= 1)

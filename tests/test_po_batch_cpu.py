"""Host-side checks of the pose-graph batch (include/slslam_hip.h: slslam_po_batch_*): create and add need no device and validate
exactly as slslam_po_solve does; finalize is the first call that asks for one.  No device needed."""
import ctypes as C

import numpy as np
import pytest

from slslam_amd import capi, synth

INVALID, NO_DEVICE, STATE = 1, 2, 5


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def _graph(seed=2, n=40, loops=3):
    return synth.make_pose_graph(seed, num_poses=n, num_loops=loops)


def _bad_graphs():
    g = _graph()
    out = {}
    b = dict(g, pose_index_2=g["pose_index_2"].copy()); b["pose_index_2"][3] = 40
    out["index_high"] = b
    b = dict(g, pose_index_1=g["pose_index_1"].copy()); b["pose_index_1"][2] = -1
    out["index_negative"] = b
    b = dict(g, pose_index_2=g["pose_index_2"].copy()); b["pose_index_2"][5] = b["pose_index_1"][5]
    out["a_equals_b"] = b
    b = dict(g, constraints=g["constraints"].copy()); b["constraints"][4, 2] = np.nan
    out["nan_constraint"] = b
    b = dict(g, parameters=g["parameters"].copy()); b["parameters"][13] = np.nan
    out["nan_parameter"] = b
    b = dict(g, parameters=g["parameters"].copy()); b["parameters"][7] = np.inf
    out["inf_parameter"] = b
    return out


def test_create_and_add_return_indices(L):
    b = capi.POBatch()
    graphs = [_graph(1, 12, 1), _graph(2, 40, 3), _graph(7, 260, 8),
              dict(num_poses=3, pose_index_1=np.zeros(0, np.int32), pose_index_2=np.zeros(0, np.int32),
                   constraints=np.zeros((0, 6)), parameters=np.arange(18.0))]
    assert [b.add(g) for g in graphs] == [0, 1, 2, 3]
    assert len(b) == 4
    b.close()


@pytest.mark.parametrize("what", ["index_high", "index_negative", "a_equals_b", "nan_constraint", "nan_parameter", "inf_parameter"])
def test_add_rejects_what_po_solve_rejects(L, what):
    g = _bad_graphs()[what]
    b = capi.POBatch()
    assert b.add(_graph(1, 12, 1)) == 0
    with pytest.raises(capi.SlslamError) as ei:
        b.add(g)
    assert ei.value.status == INVALID
    assert b.add(_graph(3, 75, 4)) == 1                  # nothing was added by the refused call
    b.close()


@pytest.mark.parametrize("missing", ["pose_index_1", "pose_index_2", "constraints", "parameters"])
def test_add_rejects_null_arrays(L, missing):
    g = _graph()
    i1 = np.ascontiguousarray(g["pose_index_1"], np.int32)
    i2 = np.ascontiguousarray(g["pose_index_2"], np.int32)
    cons = np.ascontiguousarray(g["constraints"], np.float64).reshape(-1)
    x = np.ascontiguousarray(g["parameters"], np.float64).copy()
    ptrs = dict(pose_index_1=capi._ip(i1), pose_index_2=capi._ip(i2), constraints=capi._dp(cons), parameters=capi._dp(x))
    ptrs[missing] = None
    cg = capi.POGraph(int(g["num_poses"]), len(i1), ptrs["pose_index_1"], ptrs["pose_index_2"], ptrs["constraints"], ptrs["parameters"])
    h = C.c_void_p()
    assert L.slslam_po_batch_create(-1, C.byref(h)) == 0
    idx = C.c_int(-7)
    assert L.slslam_po_batch_add(h, C.byref(cg), C.byref(idx)) == INVALID
    assert idx.value == -7
    assert L.slslam_po_batch_add(h, None, C.byref(idx)) == INVALID
    assert L.slslam_po_batch_add(None, C.byref(cg), C.byref(idx)) == INVALID
    L.slslam_po_batch_destroy(h)


def test_getters_before_download_are_state(L):
    b = capi.POBatch()
    b.add(_graph())
    for call in (lambda: b.parameters(0), lambda: b.summary(0), lambda: b.trace(0)):
        with pytest.raises(capi.SlslamError) as ei:
            call()
        assert ei.value.status == STATE
    for call in (b.solve, b.reset, b.download):                       # before finalize
        with pytest.raises(capi.SlslamError) as ei:
            call()
        assert ei.value.status == STATE
    b.close()


def test_finalize_without_device_is_no_device(L):
    if capi.device_count() > 0:
        pytest.skip("a HIP device is visible: the no-device answer cannot be observed here")
    b = capi.POBatch()
    b.add(_graph())
    with pytest.raises(capi.SlslamError) as ei:
        b.finalize()
    assert ei.value.status == NO_DEVICE
    with pytest.raises(capi.SlslamError) as ei:                      # still unfinalized, still no results
        b.summary(0)
    assert ei.value.status == STATE
    assert b.add(_graph(1, 12, 1)) == 1
    b.close()

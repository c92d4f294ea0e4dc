"""Host-side checks of the pose-graph covariances (include/slslam_hip.h: slslam_po_covariance, slslam_po_batch_covariance and friends):
the numpy reference of tests/po_covariance_reference.py is held to itself - two routes to Sigma, the margin of the singular rule - and
the C ABI validates before it needs a device.  No device needed."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_covariance_reference as cref  # noqa: E402

INVALID, STATE = 1, 5
SHAPES = [(4, 1), (12, 2), (24, 3), (33, 2), (60, 4)]          # n = 18, 66, 138, 192, 354


@functools.lru_cache(maxsize=None)
def _solved(shape):
    from oracle import pyoracle
    g = synth.make_pose_graph(7, *shape)
    x, _, _ = pyoracle.po_solve(g, linear_solver=2)
    x.setflags(write=False)
    return g, x


def _cut_chain():
    """The 12-pose chain without edge (5, 6): poses 6 .. 11 are not connected to the constant pose."""
    g = synth.make_pose_graph(7, 12, 0)
    keep = [e for e, (a, b) in enumerate(zip(g["pose_index_1"], g["pose_index_2"])) if (a, b) != (5, 6)]
    assert len(keep) == len(g["pose_index_1"]) - 1
    return dict(g, pose_index_1=g["pose_index_1"][keep], pose_index_2=g["pose_index_2"][keep], constraints=g["constraints"][keep])


@pytest.mark.parametrize("delta", [0.0, 0.001])
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_routes_agree(shape, delta):
    g, x = _solved(shape)
    ref = cref.covariance(g, x, delta)
    print("N %d loops %d: n %d, pivot %.3e, r %.2e, c %.2e" % (shape + (ref["n"], ref["pivot"], ref["r"], ref["c"])))
    assert ref["n"] == 6 * (shape[0] - 1)
    assert ref["r"] <= 10 * ref["c"]
    assert ref["pivot"] >= 1e-3
    S = ref["sigma"]
    assert np.abs(S - S.T).max() <= 10 * ref["c"] * np.abs(S).max()


def test_disconnected_component_is_singular():
    g = _cut_chain()
    ref = cref.covariance(g, g["parameters"], 0.0)
    print("cut chain: pivot %.3e" % ref["pivot"])
    assert ref["pivot"] <= 1e-10 and ref["sigma"] is None


def _cgraph(g):
    i1, i2, cons, x = capi._po_arrays(g)
    return capi.POGraph(int(g["num_poses"]), len(i1), capi._ip(i1), capi._ip(i2), capi._dp(cons), capi._dp(x)), (i1, i2, cons, x)


def test_symbols_are_declared_and_exported():
    L = capi.lib()
    for name in ("slslam_po_covariance", "slslam_po_batch_set_covariance_pairs", "slslam_po_batch_covariance", "slslam_po_batch_get_covariance",
                 "slslam_po_batch_covariance_stats"):
        assert name in capi.EXPORTS and hasattr(L, name)


def test_one_shot_validates_without_a_device():
    L = capi.lib()
    g = synth.make_pose_graph(7, 12, 2)
    cg, keep = _cgraph(g)
    out = np.zeros(36 * 12)
    pq = np.zeros(36 * 2)
    st = C.c_int(-1)
    good = np.array([1, 2], np.int32)
    for bad in ([1, 12], [-1, 2]):
        pa = np.array(bad, np.int32)
        assert L.slslam_po_covariance(C.byref(cg), 0.0, 2, capi._ip(pa), capi._ip(good), C.byref(st), capi._dp(out), capi._dp(pq)) == INVALID
        assert L.slslam_po_covariance(C.byref(cg), 0.0, 2, capi._ip(good), capi._ip(pa), C.byref(st), capi._dp(out), capi._dp(pq)) == INVALID
    assert L.slslam_po_covariance(C.byref(cg), 0.0, -1, capi._ip(good), capi._ip(good), C.byref(st), capi._dp(out), capi._dp(pq)) == INVALID
    assert L.slslam_po_covariance(C.byref(cg), 0.0, 2, None, None, C.byref(st), capi._dp(out), capi._dp(pq)) == INVALID
    assert L.slslam_po_covariance(None, 0.0, 0, None, None, C.byref(st), capi._dp(out), None) == INVALID
    assert L.slslam_po_covariance(C.byref(cg), -1.0, 0, None, None, C.byref(st), capi._dp(out), None) == INVALID
    bad_g = dict(g, pose_index_2=g["pose_index_2"].copy()); bad_g["pose_index_2"][3] = 12
    cb, keep_b = _cgraph(bad_g)
    assert L.slslam_po_covariance(C.byref(cb), 0.0, 0, None, None, C.byref(st), capi._dp(out), None) == INVALID
    assert st.value == -1 and not out.any()
    del keep, keep_b


def test_batch_pairs_and_states_without_a_device():
    L = capi.lib()
    b = capi.POBatch()
    assert b.add(synth.make_pose_graph(7, 12, 2)) == 0
    b.set_covariance_pairs(0, [(1, 11), (3, 3)])                    # before finalize: host only
    b.set_covariance_pairs(0, [])                                    # replaces the list
    for pairs in ([(1, 12)], [(-1, 2)]):
        with pytest.raises(capi.SlslamError) as ei:
            b.set_covariance_pairs(0, pairs)
        assert ei.value.status == INVALID
    with pytest.raises(capi.SlslamError) as ei:
        b.set_covariance_pairs(1, [(1, 2)])
    assert ei.value.status == INVALID
    one = np.array([1], np.int32)
    assert L.slslam_po_batch_set_covariance_pairs(b._h, 0, -1, capi._ip(one), capi._ip(one)) == INVALID
    assert L.slslam_po_batch_set_covariance_pairs(b._h, 0, 1, None, capi._ip(one)) == INVALID
    assert L.slslam_po_batch_set_covariance_pairs(None, 0, 1, capi._ip(one), capi._ip(one)) == INVALID
    with pytest.raises(capi.SlslamError) as ei:
        b.covariance()
    assert ei.value.status == STATE
    with pytest.raises(capi.SlslamError) as ei:
        b.get_covariance(0)
    assert ei.value.status == INVALID
    assert b.covariance_stats() == dict(calls=0, allocations=0)
    b.close()

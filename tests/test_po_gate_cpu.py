"""The edge statistics of include/slslam_hip.h (slslam_po_edge_statistics, slslam_po_gate, slslam_po_batch_*gate*) without a device: the
numpy reference of tests/po_gate_reference.py against central differences and INTEGRATION.md's formula, the conditioning of every case
the GPU tests use, the gating scenario in the reference alone, and the argument checks of the C ABI (made before a device is needed)."""
import ctypes as C
import functools
import os
import sys

import numpy as np

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import po_gate_reference as gref  # noqa: E402

INVALID = 1
CHI2_6_95, CHI2_6_99 = 12.6, 16.8
GRAPHS = [(4, 1), (12, 2), (24, 3)]
PRIMITIVE_N = [1, 5, 6, 65]


@functools.lru_cache(maxsize=None)
def _solved(shape):
    from oracle import pyoracle
    g = synth.make_pose_graph(7, *shape)
    x, s, _ = pyoracle.po_solve(g, linear_solver=2)
    x.setflags(write=False)
    return g, x, s


def test_jacobians_agree_with_central_differences():
    items = gref.primitive_items(6)
    for k in range(6):
        xa, xb, c = items["pose_a"][k], items["pose_b"][k], items["constraints"][k]
        _, ja, jb = gref.jet(xa, xb, c)
        h = 1e-6
        for J, which in ((ja, 0), (jb, 1)):
            for i in range(6):
                step = np.zeros(6); step[i] = h
                hi = gref.residual(xa + step * (which == 0), xb + step * (which == 1), c)
                lo = gref.residual(xa - step * (which == 0), xb - step * (which == 1), c)
                # (central differences of a smooth function: O(h^2) truncation + eps / h rounding, both ~1e-10 here)
                assert np.abs((hi - lo) / (2 * h) - J[:, i]).max() < 1e-7 * max(1.0, np.abs(J).max()), (k, which, i)


def test_reference_equals_the_integration_formula():
    items = gref.primitive_items(6)
    for k, ref in enumerate(gref.primitive_reference(items)):
        if items["singular"][k]:
            assert ref["status"] == gref.COV_SINGULAR and not ref["cov"].any() and not ref["sqrt_information"].any() and ref["mahalanobis2"] == 0.0
            continue
        te, ja, jb = gref.jet(items["pose_a"][k], items["pose_b"][k], items["constraints"][k])
        S, m2 = gref.snippet(te, ja, jb, items["cov_aa"][k], items["cov_bb"][k], items["cov_ab"][k], items["cov_meas"][k], items["sigma2"])
        assert np.abs(S - ref["cov"]).max() <= 1e-12 * np.abs(S).max()
        assert abs(m2 - ref["mahalanobis2"]) <= 1e-9 * m2
        W = ref["sqrt_information"]
        assert not np.triu(W, 1).any()
        assert np.abs(W.T @ W @ ref["cov"] - np.eye(6)).max() < 1e-9
        st, W_lib = capi.po_sqrt_information(ref["cov"])                  # the host routine the definition names
        assert st == gref.COV_OK and np.abs(W_lib - W).max() <= 1e-10 * np.abs(W).max()


def test_se3_helpers_against_the_oracle_functor():
    """Te = T2^-1 (C T1): with T2 the identity it is the composition C T1, with T1 and C the identity it is the inverse of T2."""
    items = gref.primitive_items(6)
    zero = np.zeros(6)
    for k in range(6):
        p, q = items["pose_a"][k], items["constraints"][k]
        assert np.abs(capi.se3_compose(q, p) - gref.residual(p, zero, q)).max() < 1e-14 * max(1.0, np.abs(p).max())
        assert np.abs(capi.se3_inverse(p) - gref.residual(zero, p, zero)).max() < 1e-14 * max(1.0, np.abs(p).max())


def test_relative_pose_meets_its_edge_exactly():
    items = gref.primitive_items(5)
    for k in range(5):
        c = gref.relative_pose(items["pose_a"][k], items["pose_b"][k])
        assert np.abs(gref.residual(items["pose_a"][k], items["pose_b"][k], c)).max() < 1e-13


def _pivots_ok(refs, singular):
    for k, ref in enumerate(refs):
        if singular[k]:
            assert ref["pivot"] <= 0.0, k
        else:
            assert ref["pivot"] >= 1e3 * gref.PIVOT_MIN, (k, ref["pivot"])


def test_every_case_is_well_conditioned_or_exactly_singular():
    for n in PRIMITIVE_N:
        items = gref.primitive_items(n)
        _pivots_ok(gref.primitive_reference(items), items["singular"])
        only_r = gref.primitive_reference(items, use=("cov_meas",))
        _pivots_ok(only_r, items["singular"])
    for shape in GRAPHS:
        g, x, _ = _solved(shape)
        for delta in (0.0, 0.001):
            cs, refs = gref.gate(g, x, gref.graph_candidates(g, x), delta, want_yardstick=False)
            assert cs == gref.COV_OK
            _pivots_ok(refs, [False] * len(refs))
    g, x, _ = _solved((24, 3))
    gw = dict(g, sqrt_information=synth.make_edge_information(7, g))
    cs, refs = gref.gate(gw, x, gref.graph_candidates(g, x), want_yardstick=False)
    assert cs == gref.COV_OK
    _pivots_ok(refs, [False] * len(refs))
    g, x, _ = _solved((12, 2))                                 # the mirror program's graph: weighted, with the loss
    gw = dict(g, sqrt_information=synth.make_edge_information(7, g))
    cs, refs = gref.gate(gw, x, gref.graph_candidates(g, x), 0.001, want_yardstick=False)
    assert cs == gref.COV_OK
    _pivots_ok(refs, [False] * len(refs))
    # (the batch's own solved poses, the graph without edges and the LBA window need a device: tests/test_gpu_po_gate.py asserts the same
    # pivot bound on every reference it builds)


def test_scenario_separates_in_the_reference():
    g, x, s = _solved((24, 3))
    cand = gref.scenario(g, x, s["final_cost"])
    cs, refs = gref.gate(g, x, cand, want_yardstick=False)
    good, bad = refs[0]["mahalanobis2"], refs[1]["mahalanobis2"]
    print("scenario: sigma2 %.3e  m2 consistent %.3f  corrupted %.3e" % (cand["sigma2"], good, bad))
    assert cs == gref.COV_OK
    _pivots_ok(refs, [False, False])
    assert good < 0.75 * CHI2_6_95 and bad > 10.0 * CHI2_6_99      # with room


def test_symbols_are_declared_and_exported():
    L = capi.lib()
    for name in ("slslam_po_edge_statistics", "slslam_po_gate", "slslam_po_batch_set_candidates", "slslam_po_batch_gate", "slslam_po_batch_get_gate"):
        assert name in capi.EXPORTS and hasattr(L, name)


def _untouched(call, expect=INVALID):
    """call(status, error, cov, W, m2) must return `expect` and leave the sentinel-filled outputs as they are."""
    st = np.full(4, -7, dtype=np.int32)
    outs = [np.full(k, -7.5) for k in (24, 144, 144, 4)]
    rc = call(capi._ip(st), *[capi._dp(a) for a in outs])
    assert rc == expect
    assert (st == -7).all() and all((a == -7.5).all() for a in outs)


def test_edge_statistics_rejects_bad_arguments_without_a_device():
    L = capi.lib()
    items = gref.primitive_items(4)

    def call_with(n=4, sigma2=1.0, **repl):
        arrs = {k: np.ascontiguousarray(items[k], dtype=np.float64).reshape(-1).copy() for k in ("pose_a", "pose_b", "constraints", "cov_aa", "cov_bb", "cov_ab", "cov_meas")}
        for k, (idx, v) in repl.items():
            arrs[k][idx] = v
        it = capi.POEdgeItems(n, *[capi._dp(arrs[k]) for k in ("pose_a", "pose_b", "constraints", "cov_aa", "cov_bb", "cov_ab", "cov_meas")], sigma2)
        _untouched(lambda *o: L.slslam_po_edge_statistics(C.byref(it), *o))
    call_with(pose_a=(7, np.nan))
    call_with(pose_b=(0, np.inf))
    call_with(cov_ab=(100, np.nan))
    call_with(sigma2=0.0)
    call_with(sigma2=-1.0)
    call_with(sigma2=np.nan)
    call_with(n=-1)
    _untouched(lambda *o: L.slslam_po_edge_statistics(None, *o))
    it = capi.POEdgeItems(2, None, None, None, None, None, None, None, 1.0)
    _untouched(lambda *o: L.slslam_po_edge_statistics(C.byref(it), *o))
    it0 = capi.POEdgeItems(0, None, None, None, None, None, None, None, 1.0)          # n == 0 succeeds and does nothing
    _untouched(lambda *o: L.slslam_po_edge_statistics(C.byref(it0), *o), expect=0)


def test_gate_rejects_bad_arguments_without_a_device():
    L = capi.lib()
    g, x, _ = _solved((12, 2))
    cg, keep = capi._po_graph(g, x)
    base = gref.graph_candidates(g, x)

    def call_with(graph=cg, **repl):
        cand = dict(base, **{k: np.array(base[k], dtype=np.float64 if k in ("constraints", "cov_meas") else np.int32) for k in ("pose_a", "pose_b", "constraints", "cov_meas")})
        num = repl.pop("num", None)
        sigma2 = repl.pop("sigma2", None)
        for k, (idx, v) in repl.items():
            cand[k].reshape(-1)[idx] = v
        cc, keep2 = capi._po_candidates(cand)
        if num is not None:
            cc.num = num
        if sigma2 is not None:
            cc.sigma2 = sigma2
        cs = C.c_int(-7)
        _untouched(lambda *o: L.slslam_po_gate(C.byref(graph), 0.0, C.byref(cc), C.byref(cs), *o))
        assert cs.value == -7
    call_with(pose_a=(1, int(base["pose_b"][1])))          # a == b
    call_with(pose_b=(0, 12))                              # out of range
    call_with(pose_a=(2, -1))
    call_with(num=-1)
    call_with(sigma2=0.0)
    call_with(constraints=(5, np.nan))
    call_with(cov_meas=(40, np.inf))
    xn = np.array(x); xn[9] = np.nan
    cgn, keepn = capi._po_graph(g, xn)                     # NaN in a pose of the graph
    call_with(graph=cgn)
    cs = C.c_int(-7)
    _untouched(lambda *o: L.slslam_po_gate(C.byref(cg), 0.0, None, C.byref(cs), *o))
    _untouched(lambda *o: L.slslam_po_gate(C.byref(cg), -1.0, C.byref(capi._po_candidates(base)[0]), C.byref(cs), *o))


def test_batch_candidates_are_checked_on_the_host():
    g, x, _ = _solved((12, 2))
    base = gref.graph_candidates(g, x)
    b = capi.POBatch()
    try:
        b.add(g, x)
        b.set_candidates(0, base)
        b.set_candidates(0, None)
        for bad in (dict(base, pose_a=[12] + list(base["pose_a"][1:])), dict(base, pose_b=list(base["pose_a"])), dict(base, sigma2=0.0)):
            try:
                b.set_candidates(0, bad)
            except capi.SlslamError as e:
                assert e.status == INVALID
            else:
                raise AssertionError("accepted")
        try:
            b.get_gate(0)                                  # nothing downloaded
        except capi.SlslamError as e:
            assert e.status == INVALID
        else:
            raise AssertionError("accepted")
    finally:
        b.close()

"""GPU tests of the stream's submit-time copy contract (include/slslam_hip.h, stream and refill blocks): for arrays in ordinary (pageable)
memory the results depend only on what the arrays held when slslam_lba_stream_submit / slslam_lba_batch_refill was called.  The reference's
caller frees its five arrays per window with the LBAProblem that owns them (src/slam.cpp:899-920, src/lba_problem.cpp:46-52), so a drop-in
caller may reuse them at once; only `parameters` must stay allocated, and collect() writes it without reading it.

Every leg overwrites the caller's arrays right after submit / refill returns (_poison: NaN observations and parameters, indices -1, constant
flags 7, narrowed words 0xffffffff - values every packer refuses or that give visibly different bytes) and compares each window, to the
byte, with a fresh batch of what the arrays held.  The stats show that each leg took the path it names: the staging copy of a device-built
refill, the host path of a flagged window, the whole-set rebuild of a refill that did not fit the slot.  Page-locked sets are not poisoned:
for them the header asks for the arrays unmodified until collect."""
import copy

import numpy as np
import pytest

from slslam_amd import synth

pytestmark = pytest.mark.gpu


def _poison(ws):
    """Overwrites every pageable array of WindowSet `ws` in place (never frees it) and returns deep copies of what the arrays held, as
    window dicts."""
    saved = []
    for (nc, nl), a in zip(ws.sizes, ws.arrays):
        saved.append(dict(num_cameras=nc, num_lines=nl, camera_index=a.cam.copy(), line_index=a.line.copy(), fixed_index=a.fixed.copy(),
                          observations=a.obs.copy(), parameters=a.params.copy()))
        a.obs[:] = np.nan
        a.cam[:] = -1
        a.line[:] = -1
        a.fixed[:] = 7
        a.params[:] = np.nan
    for pk in getattr(ws, "packed_arrays", None) or []:
        pk[:] = np.uint32(0xffffffff)
    return saved


def _solve_fresh(hip, ws, **opt):
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(**opt)
    b.solve(); b.download()
    out = [(b.parameters(i).copy(), b.summary(i)) for i in range(len(ws))]
    b.close()
    return out


def _same_summary(a, b):
    """Equal summaries; a NaN cost (a window that fails numerically) equals a NaN."""
    return a.keys() == b.keys() and all(a[k] == b[k] or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def _assert_fresh(hip, ws, saved, res, what):
    fresh = _solve_fresh(hip, saved)
    for j in range(len(saved)):
        assert np.array_equal(ws.parameters(j), fresh[j][0]), (what, j)
        assert _same_summary(res[j], fresh[j][1]), (what, j, res[j], fresh[j][1])


def _assert_oracle(oracle, w, x, s):
    xo, so, _ = oracle.lba_solve(w, linear_solver=1)
    assert so["num_successful_steps"] == s["num_successful_steps"]
    assert abs(so["final_cost"] - s["final_cost"]) <= 1e-7 * so["final_cost"] and np.abs(xo - x).max() < 1e-5


def _with_duplicate(w):
    """`w` with one free camera seeing one line twice (the device build leaves such a window to the host path; the host packer takes it)."""
    w = copy.deepcopy(w)
    cam, line = np.asarray(w["camera_index"]).copy(), np.asarray(w["line_index"])
    fx = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    for q0 in np.flatnonzero(fx[:, 0] == 0):
        others = np.flatnonzero((line == line[q0]) & (cam != cam[q0]))
        if len(others):
            cam[others[0]] = cam[q0]
            fx[others[0], 0] = 0
            break
    else:
        raise AssertionError("no free camera to duplicate")
    w["camera_index"], w["fixed_index"] = cam, fx.reshape(-1)
    return w


def _long_track_sets(per=40):
    """The construction of test_gpu_device_build.py::test_stream_rebuilds_a_slot_whose_refill_did_not_fit: set 1 has fewer lines and
    observations than set 0 but long tracks, so it passes the host's size tests and needs ~15 % more tiles than a slot with 5 % headroom."""
    sets = [[synth.make_window(7700 + i, num_lines=300, num_kf=40, num_free=10, mean_track=5.0) for i in range(per)]]
    for k in (1, 2):
        sets.append([synth.make_window(7800 + 100 * k + i, num_lines=60, num_kf=40, num_free=10, mean_track=36.0) for i in range(per)])
    return sets


@pytest.mark.parametrize("packed", [False, True])
def test_device_built_refill_reads_only_the_staging_copy(hip, packed):
    """Leg 1: a depth-2 stream of four sets of six pageable windows, every set poisoned as soon as submit returns; sets 2 and 3 are refills
    built on the device from the staging copy, sets 0 and 1 are packed by the host at submit.  submit and submit_packed."""
    sets = [[synth.make_window(7000 + 10 * k + i, num_lines=220 + 15 * i) for i in range(6)] for k in range(4)]
    st = hip.LBAStream(depth=2, host_threads=2)
    wsets = [hip.WindowSet(s, packed=packed) for s in sets]
    tickets, saved, res = [], [], {}
    for k in range(4):
        if k >= 2:
            res[k - 2] = st.collect(tickets[k - 2])
        tickets.append(st.submit(wsets[k]))
        saved.append(_poison(wsets[k]))
    for k in (2, 3):
        res[k] = st.collect(tickets[k])
    ss, bs = st.stats(), st.build_stats()
    assert ss["builds"] == 2 and ss["refills"] == 2, ss
    assert bs["device_builds"] == 2 and bs["zero_copy"] == 0 and bs["fallback_windows"] == 0, bs
    for k in range(4):
        _assert_fresh(hip, wsets[k], saved[k], res[k], (packed, k))
    st.close()


def test_flagged_window_starts_from_the_staged_parameters(hip):
    """Leg 2: the duplicate-observation window of test_stream_hands_flagged_windows_to_the_host_path in a pageable set, poisoned after
    submit: the device build flags it, collect solves it through the host path from the staging copy - its initial parameters included."""
    per = 6
    base = [[synth.make_window(7000 + 10 * k + i, num_lines=220 + 15 * i) for i in range(per)] for k in range(5)]
    dup = dict(base[3][2])
    cam = np.asarray(dup["camera_index"]).copy()
    same = np.flatnonzero(np.asarray(dup["line_index"]) == dup["line_index"][0])
    cam[same[1]] = cam[same[0]]
    dup["camera_index"] = cam
    base[3][2] = dup
    st = hip.LBAStream(depth=2, host_threads=2)
    wsets = [hip.WindowSet(s) for s in base]
    tickets, saved, res = [], [], {}
    for k in range(5):
        if k >= 2:
            res[k - 2] = st.collect(tickets[k - 2])
        tickets.append(st.submit(wsets[k]))
        saved.append(_poison(wsets[k]))
    for k in (3, 4):
        res[k] = st.collect(tickets[k])
    ss, bs = st.stats(), st.build_stats()
    assert ss["builds"] == 2 and ss["refills"] == 3, ss
    assert bs["device_builds"] == 3 and bs["fallback_windows"] == 1, bs
    for k in range(5):
        keep = [j for j in range(per) if not (k == 3 and j == 2)]
        fresh = _solve_fresh(hip, [saved[k][j] for j in keep])
        for f, j in enumerate(keep):
            assert np.array_equal(wsets[k].parameters(j), fresh[f][0]), (k, j)
            assert res[k][j] == fresh[f][1], (k, j)
    x, s, _ = hip.lba_solve(saved[3][2])
    assert np.array_equal(wsets[3].parameters(2), x) and res[3][2] == s
    st.close()


@pytest.mark.parametrize("mode", ["pageable", "packed"])
def test_whole_set_rebuild_reads_only_the_staging_copy(hip, oracle, mode):
    """Leg 3: a refill the host accepts and k_build_layout finds too large for the slot is packed again at collect, from the staging copy:
    poisoned after every submit, each set equals a fresh batch of what its arrays held; windows of the rebuilt set against the oracle."""
    per = 40
    sets = _long_track_sets(per)
    st = hip.LBAStream(depth=1, host_threads=2, refill_headroom_percent=5)
    wsets = [hip.WindowSet(s, packed=mode == "packed") for s in sets]
    saved, res = [], []
    for ws in wsets:
        t = st.submit(ws)
        saved.append(_poison(ws))
        res.append(st.collect(t))
    ss, bs = st.stats(), st.build_stats()
    assert ss["builds"] == 2 and ss["refills"] == 2, ss                     # set 1: accepted by the host, rebuilt at collect; set 2: a refill that fits
    assert bs["device_builds"] == 2 and bs["fallback_windows"] == per, bs
    for k in range(3):
        _assert_fresh(hip, wsets[k], saved[k], res[k], (mode, k))
    for j in (0, 23):
        _assert_oracle(oracle, saved[1][j], wsets[1].parameters(j), res[1][j])
    st.close()


def test_narrowed_words_replace_the_index_arrays_on_every_path(hip):
    """Leg 4: submit_packed with window descriptors whose camera / line / constant-flag pointers name arrays of garbage from the start: the
    narrowed words replace them (include/slslam_hip.h) on the slot's first batch (host packer), in the whole-set rebuild and in a device-built
    refill - every set equals a fresh batch of the true windows."""
    from slslam_amd.capi import LBAWindow, _dp, _ip
    per = 40
    sets = _long_track_sets(per)
    st = hip.LBAStream(depth=1, host_threads=2, refill_headroom_percent=5)
    wsets = [hip.WindowSet(s, packed=True) for s in sets]
    for ws in wsets:
        ws.garbage = []
        for a in ws.arrays:
            m = len(a.cam)
            g = (np.full(m, 1 << 20, dtype=np.int32), np.full(m, -5, dtype=np.int32), np.full(2 * m, 9, dtype=np.int32))
            ws.garbage.append(g)
            a.c = LBAWindow(a.c.num_cameras, a.c.num_lines, m, _ip(g[0]), _ip(g[1]), _ip(g[2]), _dp(a.obs), _dp(a.params))
        ws.c = (LBAWindow * len(ws.arrays))(*[a.c for a in ws.arrays])
    res = [st.collect(st.submit(ws)) for ws in wsets]
    ss, bs = st.stats(), st.build_stats()
    assert ss["builds"] == 2 and ss["refills"] == 2, ss
    assert bs["device_builds"] == 2 and bs["fallback_windows"] == per, bs
    for k in range(3):
        _assert_fresh(hip, wsets[k], sets[k], res[k], k)
    st.close()


def test_rebuild_of_a_set_with_a_window_for_the_host_path(hip, host_math, oracle):
    """Leg 5: leg 3's set that does not fit, one window of it with a free camera that sees a line twice (flagged for the host path, so the
    layout leaves it out of its totals - and the rest still does not fit: asserted on the host packer's tile counts).  The slot is rebuilt
    as one batch (the host packer takes the duplicate), and the next set of that shape is a device-built refill again."""
    from test_host_side import _pack
    per, dup_at = 40, 11
    sets = _long_track_sets(per)
    sets[1][dup_at] = _with_duplicate(sets[1][dup_at])
    for g in (0, 1):
        t0 = sum(_pack(host_math, w, grouping=g)[1]["ntiles"] for w in sets[0])
        rest = sum(_pack(host_math, w, grouping=g)[1]["ntiles"] for j, w in enumerate(sets[1]) if j != dup_at)
        assert rest > t0 + t0 * 5 // 100 + 64, (g, rest, t0)                # beyond the slot's tiles without the flagged window
    st = hip.LBAStream(depth=1, host_threads=2, refill_headroom_percent=5)
    wsets = [hip.WindowSet(s) for s in sets]
    saved, res, seen = [], [], []
    for ws in wsets:
        t = st.submit(ws)
        saved.append(_poison(ws))
        res.append(st.collect(t))
        seen.append((st.stats()["builds"], st.build_stats()))
    assert seen[0][0] == 1
    assert seen[1][0] == 2 and seen[1][1]["fallback_windows"] == per and seen[1][1]["device_builds"] == 1, seen      # rebuilt as a whole
    assert seen[2][0] == 2 and seen[2][1]["fallback_windows"] == per and seen[2][1]["device_builds"] == 2, seen      # a device-built refill
    for k in range(3):
        _assert_fresh(hip, wsets[k], saved[k], res[k], k)
    for j in (dup_at, 30):
        _assert_oracle(oracle, saved[1][j], wsets[1].parameters(j), res[1][j])
    st.close()


@pytest.mark.parametrize("device_build", [0, -1])
def test_batch_refill_reads_pageable_arrays_before_it_returns(hip, device_build):
    """Leg 6: slslam_lba_batch_refill on pageable arrays, poisoned as soon as refill returns, then solve and download: each set equals a fresh
    batch of what its arrays held, on the device build (0) and the host packer (-1).  Which path served the refills: a window with a camera
    that sees a line twice is flagged by the device build (its getters report SLSLAM_ERR_UNSUPPORTED) and solved by the host packer."""
    def make(k):
        return [synth.make_window(7300 + 10 * k + i, num_lines=n) for i, n in enumerate((300, 420, 380, 350, 400, 330))]
    sets = [make(k) for k in range(3)]
    b = hip.LBABatch()
    for w in sets[0]:
        b.add(w)
    b.finalize(refill_headroom_percent=25, host_threads=2, device_build=device_build)
    keep = []
    for k in (1, 2):
        ws = hip.WindowSet(sets[k])
        keep.append(ws)
        b.refill(ws)
        saved = _poison(ws)
        b.solve(); b.download()
        fresh = _solve_fresh(hip, saved)
        for i in range(6):
            assert np.array_equal(b.parameters(i), fresh[i][0]), (device_build, k, i)
            assert b.summary(i) == fresh[i][1], (device_build, k, i)
    probe = make(1)                                         # (the arrays of sets[1] have been poisoned: WindowSet keeps them where they are)
    cam = np.asarray(probe[0]["camera_index"]).copy()
    same = np.flatnonzero(np.asarray(probe[0]["line_index"]) == probe[0]["line_index"][0])
    cam[same[1]] = cam[same[0]]
    probe[0]["camera_index"] = cam
    refused = None
    try:
        b.refill(probe)                                     # (the host packer refuses it here when the batch's sweep cannot take it)
    except hip.SlslamError as e:
        assert e.status == 4
        refused = "refill"
    if refused is None:
        b.solve(); b.download()
        try:
            b.parameters(0)
        except hip.SlslamError as e:
            assert e.status == 4
            refused = "getter"
    if device_build == 0:
        assert refused == "getter", refused                # flagged by the device build: the refills were built there
    else:
        assert refused != "getter", refused                # the host packer takes or refuses it whole
    b.close()


def test_mixed_batch_and_numerical_failure_under_poison(hip):
    """Leg 7: the oversize-window sets of test_stream_with_an_oversize_window_among_ordinary_ones (a MIXED batch: two parts) and the 1e200
    window of test_a_window_that_fails_numerically_keeps_its_parameters, pageable and poisoned after submit: every window equals a fresh
    batch of its set, and the window that fails numerically gets its initial parameters back - not the NaN its array held at collect."""
    sets = []
    for k in range(3):
        s = [synth.make_window(9100 + 10 * k + i, num_lines=180 + 20 * i) for i in range(4)]
        s.insert(2, synth.make_window(9150 + k, num_lines=50, num_kf=30, num_free=24, mean_track=10.0))
        sets.append(s)
    fails = []
    for k in range(3):
        s = [synth.make_window(9400 + 10 * k + i, num_lines=200 + 20 * i) for i in range(4)]
        s[1]["observations"] = s[1]["observations"].copy()
        s[1]["observations"].reshape(-1)[8 * 5 + 2] = 1e200
        fails.append(s)
    for group, want_dev in ((sets, 0), (fails, 1)):
        st = hip.LBAStream(depth=2, host_threads=2)
        wsets = [hip.WindowSet(s) for s in group]
        tickets, saved, res = [], [], {}
        for k in range(3):
            if k >= 2:
                res[k - 2] = st.collect(tickets[k - 2])
            tickets.append(st.submit(wsets[k]))
            saved.append(_poison(wsets[k]))
        for k in (1, 2):
            res[k] = st.collect(tickets[k])
        assert st.build_stats()["device_builds"] == want_dev, st.build_stats()
        for k in range(3):
            _assert_fresh(hip, wsets[k], saved[k], res[k], (want_dev, k))
            if group is fails:
                assert res[k][1]["termination"] == "NUMERICAL_FAILURE"
                assert np.array_equal(wsets[k].parameters(1), saved[k][1]["parameters"]), k
        st.close()

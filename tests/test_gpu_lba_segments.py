"""The 3-D segments of the lines of a resident LBA batch (include/slslam_hip.h: slslam_lba_batch_segments / _get_segments,
slslam_lba_segments; csrc/lba_segments.h) against the numpy reference tests/lba_segments_reference.py - the reference's own Pluecker
construction -, evaluated at the device's own downloaded parameters.  Needs a real MI355X.

Bounds (none taken from what the device returns):
  statuses and counts   equal.
  s = lo, hi, t_min, t_max   |ds| <= 1e-9 (1 + |s|), and the same for the coordinates of p_min / p_max.  The error of s is about
                        eps |pc| / |m^ . dc| (m^ the unit normal of the endpoint's plane): with scenes within 20 m and the condition
                        below 4e-12 (the hand-made lines of the tile cases lie up to 45 m away: 1e-11); the bound leaves more than
                        10 x for the sin / cos table and the rotation upstream.
  condition             asserted by every case on its own input, through the reference on the CPU: every used observation has
                        |m^ . dc| >= 1e-3 and no cut point within 1e-6 of the camera's plane z = 0.
Measured on MI355X: profiles/lba_segments_bench.txt."""
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_segments_reference as S  # noqa: E402
import lba_covariance_reference as R  # noqa: E402
from test_gpu_lba_report import handmade as counted  # noqa: E402
from test_lba_segments_cpu import handmade  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = 1
INT_KEYS = ("obs_status", "status", "num_observations", "num_used", "num_clamped")
REAL_KEYS = ("obs_range", "t_min", "t_max", "p_min", "p_max")
PATH_TILED, PATH_GLOBAL, PATH_MIXED = 0, 2, 3


def _small():
    return synth.make_window(3, num_lines=60, num_kf=8, num_free=4)


def _batch(hip, ws, max_range=0.0, solve=False, **opt):
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(**opt)
    if solve:
        b.solve()
    b.segments(max_range); b.download()
    return b


def _same_bytes(a, c):
    return all(a[k].tobytes() == c[k].tobytes() for k in INT_KEYS + REAL_KEYS)


def _compare(tag, w, x, got, max_range=0.0):
    """Device against the reference at the device's own point x; returns the reference."""
    ref = S.segments(w, x, max_range)
    used = np.isin(ref["obs_status"], (S.USED, S.USED_CLAMPED))
    print("%s: %d observations, %d used; smallest |m^ . dc| %.3g, smallest |depth| %.3g" % (
        tag, len(used), used.sum(), ref["cond"][used].min() if used.any() else np.inf, np.abs(ref["depth"][used]).min() if used.any() else np.inf))
    assert S.well_conditioned(ref)
    for k in INT_KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    for k in REAL_KEYS:
        assert got[k].shape == ref[k].shape
        d = np.abs(got[k] - ref[k]) / (1.0 + np.abs(ref[k]))
        print("%s: %s |d| / (1 + |.|) max %.3g (bound 1e-9)" % (tag, k, d.max() if d.size else 0.0))
        assert (d <= 1e-9).all(), k
    return ref


def _append(w, line, cam, obs):
    """w with one more observation of an existing line."""
    out = dict(w)
    out["camera_index"] = np.append(np.asarray(w["camera_index"]), cam).astype(np.int32)
    out["line_index"] = np.append(np.asarray(w["line_index"]), line).astype(np.int32)
    out["fixed_index"] = np.append(np.asarray(w["fixed_index"]).reshape(-1), (int(cam >= int(w["num_free_cameras"])), 0)).astype(np.int32)
    out["observations"] = np.append(np.asarray(w["observations"], dtype=np.float64).reshape(-1), obs)
    return out


# 1. the small window, before and after a solve
@pytest.mark.parametrize("solve", [False, True])
def test_small_window(hip, solve):
    w = _small()
    b = _batch(hip, [w], solve=solve)
    x = b.parameters(0)
    if not solve:
        assert x.tobytes() == np.asarray(w["parameters"], dtype=np.float64).tobytes()
    ref = _compare("small solve=%s" % solve, w, x, b.get_segments(0))
    assert (ref["status"] == S.OK).all()
    b.close()


# 2. the range clamp
@pytest.mark.parametrize("max_range", [5.0, 8.0])
def test_range_clamp(hip, max_range):
    w = _small()
    b = _batch(hip, [w], max_range)
    ref = _compare("max_range %g" % max_range, w, b.parameters(0), b.get_segments(0), max_range)
    b.close()
    if max_range == 5.0:            # (the comparison is not vacuous)
        assert {S.OUT_OF_RANGE, S.USED_CLAMPED, S.USED} <= set(ref["obs_status"].tolist())
        assert {S.NONE, S.OK} <= set(ref["status"].tolist())


# 3. hand-made observations
def test_handmade_observations(hip):
    w = _small()
    cases = handmade(w)
    # ... and a line whose FIRST observation puts its endpoints behind the camera, the second one in front of another
    behind = cases["behind"][0]
    far = int(w["num_cameras"]) - 1                                         # the oldest keyframe: several metres behind the newest
    R, t = synth.wt_to_rt(np.asarray(w["parameters"])[6 * far:6 * far + 6])
    ends = [R @ np.array([0.0, y, -1.0]) + t for y in (-0.5, 0.5)]
    assert min(e[2] for e in ends) > 0.3
    o = np.array([ends[0][0] / ends[0][2], ends[0][1] / ends[0][2], ends[1][0] / ends[1][2], ends[1][1] / ends[1][2], 0, 0, 0, 0])
    o[4:] = o[:4] - np.array([synth.BASELINE / ends[0][2], 0, synth.BASELINE / ends[1][2], 0])
    cases["behind_then_seen"] = (_append(behind, int(behind["num_lines"]) - 1, far, o), S.USED, S.OK)
    # a NaN in an observation never reaches the device: the packer refuses the window (the kernel's own test is for what a solve leaves)
    refused = cases.pop("nan")[0]
    b = hip.LBABatch()
    with pytest.raises(hip.SlslamError) as ei:
        b.add(refused)
    assert ei.value.status == INVALID
    b.close()
    with pytest.raises(hip.SlslamError) as ei:
        hip.lba_segments(refused)
    assert ei.value.status == INVALID
    names = list(cases)
    b = _batch(hip, [cases[k][0] for k in names])
    for i, k in enumerate(names):
        w2, want_obs, want_line = cases[k]
        got = b.get_segments(i)
        _compare(k, w2, b.parameters(i), got)
        if want_obs is not None:
            assert got["obs_status"][-1] == want_obs
        assert got["status"][-1] == want_line
    got = b.get_segments(names.index("behind_then_seen"))
    assert list(got["obs_status"][-2:]) == [S.BEHIND, S.USED] and got["num_observations"][-1] == 2 and got["num_used"][-1] == 1
    got = b.get_segments(names.index("seen_once"))
    assert got["num_observations"][-1] == 1 and abs(got["p_min"][-1, 2] - 1.0) < 1e-12 and abs(got["t_max"][-1] - got["t_min"][-1] - 1.0) < 1e-12
    b.close()


# 4. tile boundaries (csrc/lba_types.h): runs of 1, 2, 63 and 64 lanes, runs that end on and cross the 16-lane rows (a kTileMultiRow tile:
#    any line with more than 16 observations), and tiles that hold many short lines
TILE_COUNTS = [1, 2, 63, 64, 15, 16, 17, 33, 0] + [1] * 40 + [2] * 20 + [3] * 11


def test_tile_boundaries(hip):
    w = counted(TILE_COUNTS, 64)
    b = _batch(hip, [w])
    assert b.path() == PATH_TILED and b.window_chunks(0) >= 1
    got = b.get_segments(0)
    assert np.array_equal(got["num_observations"], TILE_COUNTS) and got["status"][8] == S.NO_OBSERVATIONS
    _compare("tiles", w, b.parameters(0), got)
    b.close()
    b = _batch(hip, [w], 25.0, chunks_per_window=4)                         # the same lines cut into several chunks, clamped
    assert b.path() == PATH_TILED and b.window_chunks(0) > 1
    ref = _compare("tiles, 4 chunks, max_range 25", w, b.parameters(0), b.get_segments(0), 25.0)
    assert {S.USED, S.USED_CLAMPED, S.OUT_OF_RANGE, S.COLLAPSED} <= set(ref["obs_status"].tolist())
    b.close()


# 5. the smallest windows that take the global-memory path, alone and beside an ordinary window
def test_global_memory_path(hip):
    long_line = counted([1, 2, 64, 0, 65], 65)
    many_free = synth.make_window(13, num_lines=40, num_kf=24, num_free=21)
    small = _small()
    got = {}
    # (the hand-made lines lie up to 45 m away: 25 m leaves a fifth of their observations in range, some of them clamped)
    for name, ws, path, max_range in (("line65", [long_line], PATH_GLOBAL, 25.0), ("free21", [many_free], PATH_GLOBAL, 8.0),
                                      ("mixed", [small, long_line], PATH_MIXED, 25.0)):
        b = _batch(hip, ws, max_range)
        assert b.path() == path
        for i, w in enumerate(ws):
            got[(name, i)] = b.get_segments(i)
            ref = _compare("%s window %d" % (name, i), w, b.parameters(i), got[(name, i)], max_range)
            if w is not small:      # (every line of the small window is within 25 m)
                assert {S.USED, S.USED_CLAMPED, S.OUT_OF_RANGE} <= set(ref["obs_status"].tolist())
        b.close()
    assert np.array_equal(got[("line65", 0)]["num_observations"], [1, 2, 64, 0, 65])
    assert _same_bytes(got[("line65", 0)], got[("mixed", 1)])                # the oversize window alone and in company


# 6. a window's bytes do not depend on its company
def test_bytes_do_not_depend_on_the_batch(hip):
    a = _small()
    others = [synth.make_window(30 + i, num_lines=40 + 25 * i, num_kf=6 + i, num_free=3) for i in range(4)]
    for max_range in (0.0, 5.0):
        b = _batch(hip, [a], max_range)
        alone = b.get_segments(0)
        b.close()
        b = _batch(hip, others[:2] + [a] + others[2:], max_range)
        company = b.get_segments(2)
        b.close()
        assert _same_bytes(alone, company)
        assert _same_bytes(alone, hip.lba_segments(a, max_range))


# 7. protocol
def test_protocol(hip):
    ws = [_small(), synth.make_window(31, num_lines=50, num_kf=6, num_free=3)]
    plain = hip.LBABatch()
    for w in ws:
        plain.add(w)
    plain.finalize(refill_headroom_percent=50); plain.solve(); plain.download()
    undisturbed = [(plain.parameters(i).copy(), plain.summary(i)) for i in range(2)]
    plain.report(); plain.download()
    rep_alone = [plain.get_report(i) for i in range(2)]
    plain.covariance(); plain.download()
    cov_alone = [plain.get_covariance(i) for i in range(2)]
    plain.close()

    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(refill_headroom_percent=50)
    with pytest.raises(hip.SlslamError) as ei:                  # nothing enqueued yet
        b.get_segments(0)
    assert ei.value.status == INVALID
    b.segments()
    with pytest.raises(hip.SlslamError) as ei:                  # enqueued, not downloaded
        b.get_segments(0)
    assert ei.value.status == INVALID
    b.download()
    first = [b.get_segments(i) for i in range(2)]
    for i, w in enumerate(ws):
        _compare("initial %d" % i, w, b.parameters(i), first[i])
    stats = b.segments_stats()
    assert stats["calls"] == 1 and stats["allocations"] > 0
    assert hip.lib().slslam_lba_batch_segments(b._h, None, float("nan")) == INVALID
    assert hip.lib().slslam_lba_batch_segments(b._h, None, float("inf")) == INVALID
    assert hip.lib().slslam_lba_batch_get_segments(b._h, 2, None, None, None) == INVALID
    # segments between the solve and its download leave the solve alone; report + covariance + segments before one download
    b.solve(); b.report(); b.covariance(); b.segments(8.0); b.download()
    assert b.segments_stats() == {"calls": 2, "allocations": stats["allocations"]}       # a second call allocates nothing
    both = [b.get_segments(i) for i in range(2)]
    for i, w in enumerate(ws):
        assert b.parameters(i).tobytes() == undisturbed[i][0].tobytes() and b.summary(i) == undisturbed[i][1]
        _compare("solved %d" % i, w, b.parameters(i), both[i], 8.0)
        rep = b.get_report(i)
        assert all(rep[k].tobytes() == rep_alone[i][k].tobytes() for k in ("sq_norm", "weight", "lines", "cameras"))
        cov = b.get_covariance(i)
        assert cov[0] == cov_alone[i][0] and np.array_equal(cov[1], cov_alone[i][1])
        # (the covariance adds by LDS atomics in arrival order: the yardstick of tests/test_gpu_lba_covariance.py, SAME POINT)
        assert R.rel_cameras(cov[2], cov_alone[i][2]) <= 1e-12 and R.rel_lines(cov[3], cov_alone[i][3]) <= 1e-12
    b.segments(8.0); b.download()
    assert all(_same_bytes(b.get_segments(i), both[i]) for i in range(2))      # ... and alone what they were beside the others
    b.segments()
    with pytest.raises(hip.SlslamError) as ei:                  # a newer call is still on the device
        b.get_segments(0)
    assert ei.value.status == INVALID
    b.download()
    b.refill(ws)
    with pytest.raises(hip.SlslamError) as ei:                  # the refill replaced the windows
        b.get_segments(0)
    assert ei.value.status == INVALID
    b.segments(); b.download()
    assert all(_same_bytes(b.get_segments(i), first[i]) for i in range(2))
    b.close()
    with pytest.raises(hip.SlslamError) as ei:
        hip.lba_segments(ws[0], float("nan"))
    assert ei.value.status == INVALID


def test_stream_batches_answer(hip):
    """Through slslam_lba_stream_batch: the first set is packed on the host, the third is a device-built refill of the first slot."""
    wins = [[synth.make_window(80 + 4 * k + i, num_lines=40 + 10 * i, num_kf=6, num_free=3) for i in range(2)] for k in range(3)]
    sets = [hip.WindowSet(ws, pinned=True) for ws in wins]
    st = hip.LBAStream(depth=2, host_threads=1)
    tk = [st.submit(sets[0]), st.submit(sets[1])]
    st.collect(tk[0])
    v = st.batch_of(tk[0], sets[0])
    v.segments(5.0); v.download()
    for i, w in enumerate(wins[0]):
        _compare("stream set 0 window %d" % i, w, v.parameters(i), v.get_segments(i), 5.0)
    tk.append(st.submit(sets[2]))
    st.collect(tk[1]); st.collect(tk[2])
    assert st.build_stats()["device_builds"] == 1
    v = st.batch_of(tk[2], sets[2])
    v.segments(); v.download()
    for i, w in enumerate(wins[2]):
        _compare("stream set 2 (device-built) window %d" % i, w, v.parameters(i), v.get_segments(i))
    st.close()
    for s in sets:
        s.close()

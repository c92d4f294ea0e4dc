"""GPU tests: batches on the fused motion-only path (SLAM::motion_only_ba, reference src/slam.cpp:578-675: one free camera, every line
constant, the whole LM solve in one launch) are refilled in place - slslam_lba_batch_refill and the stream object - by the device build
and by the host packer, and return what a fresh batch of the same windows returns, to the byte.  A refill whose windows are not all of
that shape is refused before the batch is touched."""
import numpy as np
import pytest

from slslam_amd import synth

pytestmark = pytest.mark.gpu

FUSED = 1          # SLSLAM_PATH_FUSED_MOTION_ONLY


def _sets():
    # the first set is the largest: the batch's room is made for it (refill_headroom_percent on top)
    sizes = [(150, 140, 150, 130, 145, 150), (60, 120, 35, 150, 90, 140), (150, 20, 75, 110, 150, 45)]
    return [[synth.make_motion_only(700 + 10 * k + i, num_lines=n) for i, n in enumerate(s)] for k, s in enumerate(sizes)]


def _fresh(hip, ws, **opt):
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(**opt)
    assert b.path() == FUSED
    b.solve(); b.download()
    out = [(b.parameters(i).copy(), b.summary(i), b.trace(i)) for i in range(len(ws))]
    b.close()
    return out


@pytest.mark.parametrize("device_build", [0, -1])
def test_motion_only_batch_refills_in_place(hip, oracle, device_build):
    """Three sets of motion-only windows of differing sizes through ONE batch (finalize once, refill three times, back to the first set),
    built on the device (device_build = 0) and by the host packer (-1): parameters, summaries and traces identical to fresh batches."""
    sets = _sets()
    b = hip.LBABatch()
    for w in sets[0]:
        b.add(w)
    b.finalize(refill_headroom_percent=25, device_build=device_build)
    assert b.path() == FUSED
    for step, k in enumerate([0, 1, 2, 0]):
        if step > 0:
            b.refill(sets[k])
        assert b.path() == FUSED
        b.solve(); b.download()
        fresh = _fresh(hip, sets[k])
        for i in range(len(sets[k])):
            assert np.array_equal(b.parameters(i), fresh[i][0]), "set %d window %d" % (k, i)
            assert b.summary(i) == fresh[i][1] and b.trace(i) == fresh[i][2], (k, i)
        b.reset(); b.solve(); b.download()                  # reset from the refilled windows' initial values
        for i in range(len(sets[k])):
            assert np.array_equal(b.parameters(i), fresh[i][0])
    for i in (1, 3):
        w = sets[1][i]
        xo, so, _ = oracle.lba_solve(w, linear_solver=1)
        b.refill(sets[1]); b.solve(); b.download()
        assert so["num_successful_steps"] == b.summary(i)["num_successful_steps"]
        assert np.abs(xo - b.parameters(i)).max() < 1e-7
        assert np.array_equal(b.parameters(i)[6:], w["parameters"][6:])        # camera 1 and the lines are constant
    b.close()


def _not_motion_only():
    """Windows a fused batch must not take: a general window, a motion-only window with one line left free, one whose constant camera
    lost its flag (two free cameras), one with no free camera."""
    out = [synth.make_window(801, num_lines=80)]
    w = synth.make_motion_only(802, num_lines=70)
    fx = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    fx[np.asarray(w["line_index"]) == 5, 1] = 0
    out.append(dict(w, fixed_index=fx.reshape(-1)))
    w = synth.make_motion_only(803, num_lines=70)
    fx = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    fx[:, 0] = 0
    out.append(dict(w, fixed_index=fx.reshape(-1)))
    w = synth.make_motion_only(804, num_lines=70)
    fx = np.asarray(w["fixed_index"]).reshape(-1, 2).copy()
    fx[:, 0] = 1
    out.append(dict(w, fixed_index=fx.reshape(-1)))
    return out


def test_motion_only_refill_refuses_other_shapes(hip):
    """A refill of a fused motion-only batch with a window of another shape is SLSLAM_ERR_UNSUPPORTED, and the batch is left as it was:
    its results and its windows solve again to the same bytes."""
    sets = _sets()
    b = hip.LBABatch()
    for w in sets[0]:
        b.add(w)
    b.finalize(refill_headroom_percent=25)
    b.solve(); b.download()
    keep = [b.parameters(i).copy() for i in range(6)]
    for bad in _not_motion_only():
        ws = list(sets[1]); ws[2] = bad
        with pytest.raises(hip.SlslamError) as e:
            b.refill(ws)
        assert e.value.status == 4
        assert [np.array_equal(b.parameters(i), keep[i]) for i in range(6)] == [True] * 6     # the results under way are kept
    b.reset(); b.solve(); b.download()
    for i in range(6):
        assert np.array_equal(b.parameters(i), keep[i])
    b.refill(sets[1]); b.solve(); b.download()                # and a motion-only set is still taken
    fresh = _fresh(hip, sets[1])
    for i in range(6):
        assert np.array_equal(b.parameters(i), fresh[i][0])
    b.close()


@pytest.mark.parametrize("pinned,packed", [(False, False), (True, True)])
def test_stream_of_motion_only_sets(hip, pinned, packed):
    """A stream of motion-only sets: the submits after the first `depth` refill the slots' fused batches on the device (build_stats), every
    window equal to the byte to a fresh batch of its set.  A set of another shape submitted to a slot whose batch is fused is served by a
    new batch of the general path."""
    sets = [[synth.make_motion_only(900 + 10 * k + i, num_lines=80 + 7 * ((i + k) % 5)) for i in range(8)] for k in range(5)]
    other = [synth.make_window(990 + i, num_lines=60) for i in range(8)]
    order = [0, 1, 2, 3, 4, "other"]
    st = hip.LBAStream(depth=2, host_threads=2)
    wsets = [hip.WindowSet(other if k == "other" else sets[k], pinned=pinned, packed=packed) for k in order]
    tickets, results = [], {}
    for j in range(len(order)):
        if j >= 2:
            results[tickets[j - 2]] = st.collect(tickets[j - 2])
        tickets.append(st.submit(wsets[j]))
    for j in range(len(order) - 2, len(order)):
        results[tickets[j]] = st.collect(tickets[j])
    bs, ss = st.build_stats(), st.stats()
    # slot 0 serves sets 0, 2, 4 and slot 1 sets 1, 3, "other": two first batches, three refills of fused batches, "other" a new batch
    assert ss["builds"] == 3 and ss["refills"] == 3, ss
    assert bs["device_builds"] == 3 and bs["fallback_windows"] == 0, bs
    for j, k in enumerate(order):
        ws = other if k == "other" else sets[k]
        b = hip.LBABatch()
        for w in ws:
            b.add(w)
        b.finalize()
        assert b.path() == (0 if k == "other" else FUSED)
        b.solve(); b.download()
        for i in range(len(ws)):
            assert np.array_equal(wsets[j].parameters(i), b.parameters(i)), (k, i)
            assert results[tickets[j]][i] == b.summary(i), (k, i)
        b.close()
    st.close()
    for ws in wsets:
        ws.close()

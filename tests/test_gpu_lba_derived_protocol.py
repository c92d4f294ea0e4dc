"""The protocol the derived results of a resident LBA batch share (include/slslam_hip.h: slslam_lba_batch_covariance, _report,
_segments and their _get_ / _stats calls): enqueue, download, read; buffers made by the first call and kept; a
refill invalidates.  One row of RESULTS per result - a new one adds a row.  What the results hold is the business of
test_gpu_lba_covariance.py, test_gpu_lba_report.py and test_gpu_lba_segments.py.  Needs a real MI355X."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_lba_report import handmade as counted  # noqa: E402

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED, STATE = 0, 1, 4, 5
PATH_MIXED = 3

# enqueue(b), get(b, i), stats(b), c_get(lib, handle, i): the C getter with every output NULL, buffers: what the first call allocates
Row = collections.namedtuple("Row", "name enqueue get stats c_get buffers")
RESULTS = [
    Row("covariance", lambda b: b.covariance(), lambda b, i: b.get_covariance(i), lambda b: b.covariance_stats(),
        lambda L, h, i: L.slslam_lba_batch_get_covariance(h, i, None, None, None, None, None), 6),       # (4, and 2 for the lines' blocks)
    Row("report", lambda b: b.report(), lambda b, i: b.get_report(i), lambda b: b.report_stats(),
        lambda L, h, i: L.slslam_lba_batch_get_report(h, i, None, None, None, None), 7),
    Row("segments", lambda b: b.segments(), lambda b, i: b.get_segments(i), lambda b: b.segments_stats(),
        lambda L, h, i: L.slslam_lba_batch_get_segments(h, i, None, None, None), 6),
]
IDS = [r.name for r in RESULTS]


def _windows():
    return [synth.make_window(3, num_lines=60, num_kf=8, num_free=4), synth.make_window(31, num_lines=50, num_kf=6, num_free=3)]


def _tiled(hip, ws):
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize(refill_headroom_percent=50)
    return b


def _blob(x):
    """Every field of a getter's result as bytes."""
    if isinstance(x, dict):
        return tuple((k, _blob(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(_blob(v) for v in x)
    return None if x is None else np.asarray(x).tobytes()


@pytest.mark.parametrize("row", RESULTS, ids=IDS)
def test_tiled_batch(hip, row):
    L = hip.lib()
    b = _tiled(hip, _windows())
    assert [row.c_get(L, b._h, i) for i in range(2)] == [INVALID, INVALID]      # nothing enqueued yet
    row.enqueue(b)
    assert [row.c_get(L, b._h, i) for i in range(2)] == [INVALID, INVALID]      # enqueued, not downloaded
    b.download_async(); b.wait()
    assert [row.c_get(L, b._h, i) for i in range(2)] == [OK, OK]
    first = [_blob(row.get(b, i)) for i in range(2)]
    b.download()                                                                # nothing new enqueued: what was read stays readable
    assert [_blob(row.get(b, i)) for i in range(2)] == first
    assert row.stats(b) == {"calls": 1, "allocations": row.buffers}
    row.enqueue(b); b.download()
    assert row.stats(b) == {"calls": 2, "allocations": row.buffers}             # a second call allocates nothing
    assert [row.c_get(L, b._h, i) for i in range(2)] == [OK, OK]
    b.close()


def test_tiled_batch_all_results_one_download(hip):
    L = hip.lib()
    ws = _windows()
    b = _tiled(hip, ws)
    for row in RESULTS:
        row.enqueue(b)
    b.solve(); b.download()
    for row in RESULTS:
        assert [row.c_get(L, b._h, i) for i in range(2)] == [OK, OK], row.name
        for i in range(2):
            row.get(b, i)
    b.refill(ws)                                                                # the refill replaced the windows
    for row in RESULTS:
        assert [row.c_get(L, b._h, i) for i in range(2)] == [INVALID, INVALID], row.name
    b.close()


def test_covariance_lines(hip):
    L = hip.lib()
    ws = _windows()
    b = _tiled(hip, ws)
    b.covariance(with_lines=False); b.download()
    assert b.covariance_stats() == {"calls": 1, "allocations": 4}
    lines = np.zeros(16 * int(ws[0]["num_lines"]))
    # (the call that was downloaded skipped the lines)
    assert L.slslam_lba_batch_get_covariance(b._h, 0, None, None, None, None, lines.ctypes.data_as(C.POINTER(C.c_double))) == STATE
    assert L.slslam_lba_batch_get_covariance(b._h, 0, None, None, None, None, None) == OK
    b.covariance(with_lines=True)
    assert b.covariance_stats() == {"calls": 2, "allocations": 6}               # the lines' blocks: made by the first call that asks
    b.covariance(with_lines=True)
    assert b.covariance_stats() == {"calls": 3, "allocations": 6}
    b.download()
    assert L.slslam_lba_batch_get_covariance(b._h, 0, None, None, None, None, lines.ctypes.data_as(C.POINTER(C.c_double))) == OK
    assert lines.any()
    b.close()


def test_mixed_batch(hip):
    """An ordinary window beside one of the global-memory path (a line with 65 observations): two batches side by side."""
    L = hip.lib()
    ws = [_windows()[0], counted([1, 2, 64, 0, 65], 65)]
    b = hip.LBABatch()
    for w in ws:
        b.add(w)
    b.finalize()
    assert b.path() == PATH_MIXED
    with pytest.raises(hip.SlslamError) as ei:
        b.covariance()
    assert ei.value.status == UNSUPPORTED and b.covariance_stats()["calls"] == 0
    rows = [r for r in RESULTS if r.name != "covariance"]
    for row in rows:
        row.enqueue(b)
    b.download()
    for row in rows:
        for i in range(2):                                                      # both windows answer, each with its own observations
            assert row.c_get(L, b._h, i) == OK
            got = row.get(b, i)
            per_line = got["lines"]["num_observations"] if row.name == "report" else got["num_observations"]
            assert len(per_line) == int(ws[i]["num_lines"]) and per_line.sum() == b.num_obs[i] > 0, (row.name, i)
        assert row.stats(b) == {"calls": 1, "allocations": 2 * row.buffers}       # (one set of buffers per part)
        row.enqueue(b)
    b.download()
    for row in rows:
        assert row.stats(b) == {"calls": 2, "allocations": 2 * row.buffers}
    assert [L.slslam_lba_batch_get_covariance(b._h, i, None, None, None, None, None) for i in range(2)] == [INVALID, INVALID]
    b.close()

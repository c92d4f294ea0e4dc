"""The line refiner and the line triangulator return what they returned before their host sides moved onto one shared plan
(csrc/line_call_plan.h): one call of each handle on three small windows - 70 running lines (two waves, a ragged tail); a flagged line, a
line without observations and a NaN camera; every line constant -, replayed from tests/golden/line_calls_parent.npz (recorded by
tools/record_line_calls.py at the commit before the move).  Integers equal, doubles bit-equal (NaN as NaN): neither kernel uses atomics
and a line's bytes do not depend on its company, so no tolerance is needed."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_line_calls", os.path.join(ROOT, "tools", "record_line_calls.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

RECORDED = rec.load(os.path.join(ROOT, "tests", "golden", "line_calls_parent.npz"))


def test_the_recording_covers_every_case_and_every_fate():
    assert sorted(RECORDED) == sorted(rec.CASES)
    rec.covers(RECORDED)
    inp = RECORDED["refine"][0]
    for name in rec.CASES:                                   # the three calls were recorded on the same windows
        assert sorted(RECORDED[name][0]) == sorted(inp)
        assert all(np.asarray(v).tobytes() == np.asarray(inp[k]).tobytes() for k, v in RECORDED[name][0].items()), name
    assert len(rec.as_windows(inp)) == 3


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_equal_to_the_recording(hip, name):
    inp, want = RECORDED[name]
    before = {k: np.array(v) for k, v in inp.items()}
    got = rec.run(*rec.CASES[name], inp)
    assert all(before[k].tobytes() == np.asarray(inp[k]).tobytes() for k in before)          # the recorded inputs are shared: left as they were
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind != "f":
            assert np.array_equal(a, b), (name, k, a, b)
        else:
            same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
            assert same.all(), "%s %s: %d of %d doubles differ, first at %s: recorded %r, now %r" % (
                name, k, int((~same).sum()), same.size, np.argwhere(~same)[0].tolist(), a[~same][0], b[~same][0])

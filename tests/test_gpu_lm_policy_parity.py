"""Every device LM loop computes what it computed before the trust-region bookkeeping moved into csrc/lm_policy.h: one tiny problem
per loop, replayed from tests/golden/lm_traces_parent.npz (recorded by tools/record_lm_traces.py at the commit before the move; every
recorded trace has accepted and rejected steps).  Integers equal; doubles bit-equal, but for the pose graphs (ATOMIC_SUMS below)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_lm_traces", os.path.join(ROOT, "tools", "record_lm_traces.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

RECORDED = rec.load(os.path.join(ROOT, "tests", "golden", "lm_traces_parent.npz"))


def test_the_recording_covers_every_loop_and_both_branches():
    assert sorted(RECORDED) == sorted(rec.CASES)
    for name, (_, out) in RECORDED.items():
        assert rec.walks_both(out), name


# The pose-graph kernels add their edge blocks into H, g and the cost with fp64 global atomics, one wave per five edges: with more
# than one wave the order of the sums, and so the last bits of everything after the first linearisation, changes from run to run (at
# the recorded commit as well).  Their doubles are held to the tolerances tests/test_gpu_po.py holds the same fields to against the
# oracle (cost 1e-8, radius 1e-5, initial cost 1e-12, final cost 1e-7, parameters 1e-6 absolute); the trace fields that test does not
# compare follow from those: cost_change is a difference of two costs (2e-8 of the cost), the others move the radius and get its 1e-5.
# Decisions, counts and termination types stay exact, and every other loop stays bit for bit.
ATOMIC_SUMS = ("po_single", "po_batch")
TRACE_RTOL = dict(zip(rec.TRACE_DBL, (1e-8, None, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5)))
SUMMARY_RTOL = dict(zip(rec.SUMMARY_DBL, (1e-12, 1e-7, 1e-12)))


def _close(name, k, a, b):
    field = k.rstrip("_01")
    if field == "parameters":
        assert np.abs(a - b).max() < 1e-6, (name, k)
    elif field == "summary_dbl":
        for j, f in enumerate(rec.SUMMARY_DBL):
            assert abs(a[j] - b[j]) <= SUMMARY_RTOL[f] * abs(a[j]), (name, k, f, a[j], b[j])
    else:
        assert field == "trace_dbl", k
        cost = a[:, rec.TRACE_DBL.index("cost")]
        for j, f in enumerate(rec.TRACE_DBL):
            tol = 2e-8 * cost if f == "cost_change" else TRACE_RTOL[f] * np.abs(a[:, j])
            print(name, k, f, "largest difference / tolerance: %.3e" % (np.abs(a[:, j] - b[:, j]) / np.maximum(tol, 1e-300)).max())
            assert (np.abs(a[:, j] - b[:, j]) <= tol).all(), (name, k, f, a[:, j], b[:, j])


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_equal_to_the_recording(hip, name):
    inp, want = RECORDED[name]
    got = rec.solve(*rec.CASES[name], inp)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape)
        if a.dtype.kind != "f":
            assert np.array_equal(a, b), (name, k, a, b)
        elif name in ATOMIC_SUMS:
            _close(name, k, a, b)
        else:
            same = a.view(np.uint64) == b.view(np.uint64)
            assert same.all(), "%s %s: %d of %d doubles differ, first at %s: recorded %r, now %r" % (
                name, k, int((~same).sum()), same.size, np.argwhere(~same)[0].tolist(), a[~same][0], b[~same][0])

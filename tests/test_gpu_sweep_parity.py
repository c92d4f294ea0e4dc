"""The LBA kernels tests/test_gpu_lm_policy_parity.py does not reach compute what they computed before the run-time experiment switch
of the kernel policy left them: the cases of SWEEP_CASES (tools/record_lm_traces.py --sweeps), replayed from
tests/golden/lm_traces_sweeps_parent.npz, which was recorded with the library of the commit before the removal.

Every case is held bit for bit: elim2, elim3, elim4, elim4_keep, elim4_mixed (the matrix-core sweeps on the 12-line window, which they
take as it is), two_chunks, many_chunks (k_slab_reduce and k_lm_update_wave: a window needs more than 8 chunks for them, so the 70-line
window in two chunks has a 240-line companion cut into one chunk per tile), batch257 (k_reduced_solve<4>; windows 0 and 256) and
big_wide (252 reduced unknowns: k_big_solve<kBsvSlots>).  The file was recorded twice at that commit, in two processes, and the two
recordings agreed in every bit of every case - the two waves of sweep 3 own disjoint accumulator tiles and their camera records are
added in a fixed order - so no case needs a tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_lm_traces", os.path.join(ROOT, "tools", "record_lm_traces.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

RECORDED = rec.load(os.path.join(ROOT, "tests", "golden", "lm_traces_sweeps_parent.npz"))


def test_the_recording_covers_every_case_and_both_branches():
    assert sorted(RECORDED) == sorted(rec.SWEEP_CASES)
    for name, (_, out) in RECORDED.items():
        assert rec.walks_both(out), name
    inp, out = RECORDED["batch257"]
    assert int(inp["copies"]) == 257 and sorted(k for k in out if k.startswith("parameters")) == ["parameters_0", "parameters_256"]
    big = rec.as_window(RECORDED["big_wide"][0])
    free = np.unique(big["camera_index"][np.asarray(big["fixed_index"]).reshape(-1, 2)[:, 0] == 0])
    assert 241 <= 6 * len(free) <= 256 and np.bincount(big["line_index"]).max() == 65


@pytest.mark.parametrize("name", sorted(rec.SWEEP_CASES))
def test_equal_to_the_recording(hip, name):
    inp, want = RECORDED[name]
    got = rec.solve(*rec.SWEEP_CASES[name], inp)      # (asserts the path, the sweep elimination() reports and the chunk count as well)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        a, b = np.asarray(want[k]), np.asarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (name, k, a.shape, b.shape)
        if a.dtype.kind != "f":
            assert np.array_equal(a, b), (name, k, a, b)
        else:
            same = a.view(np.uint64) == b.view(np.uint64)
            assert same.all(), "%s %s: %d of %d doubles differ, first at %s: recorded %r, now %r" % (
                name, k, int((~same).sum()), same.size, np.argwhere(~same)[0].tolist(), a[~same][0], b[~same][0])

"""CPU checks of the line matcher's numpy reference (tests/line_match_reference.py): its float restatement of
SLAM::reprojection_error against the oracle's ransac_score, its reductions on handmade frames, and the property of the end-to-end input
that tests/test_gpu_line_match.py relies on.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_match_reference as M  # noqa: E402

THR = 5.0 / 406.05


def oracle_pairs(oracle, frame, thr, baseline=0.12):
    """[K, L] bool: the oracle's inlier bits of the frame's K x L pairs, flattened into one hypothesis with K L common lines"""
    ob = np.asarray(frame["observations"], dtype=np.float64).reshape(-1, 8)
    ln = np.asarray(frame["lines"], dtype=np.float64).reshape(-1, 6)
    K, L = len(ob), len(ln)
    assert np.linalg.norm(np.asarray(frame["pose"])[9:]) <= 1.0          # (the scoring loop skips |t| > 1)
    _, inl = oracle.ransac_score(frame["pose"], np.repeat(ob, L, axis=0), np.tile(ln, (K, 1)), baseline=baseline, error_thr=thr)
    return inl[0].reshape(K, L)


@pytest.mark.parametrize("seed,K,L", [(501, 65, 197), (502, 150, 150), (503, 7, 300)])
def test_errors_are_the_oracles(oracle, seed, K, L):
    fr = M.make_frame(seed, K, L)
    e = M.errors(fr["pose"], fr["observations"], fr["lines"])
    assert e.dtype == np.float32 and e.shape == (K, L) and np.isfinite(e).all()
    # thresholds: the default, a few fixed ones, and the exact values of some pairs (and the next double above each): an error that is
    # off by one float ulp flips its own bit at one of them
    flat = np.sort(e.reshape(-1))
    own = [float(v) for v in flat[[0, 1, len(flat) // 100, len(flat) // 10, len(flat) // 2, -1]]]
    near = [float(v) for v in flat[np.searchsorted(flat, np.float32(THR)) + np.arange(-2, 3)]]
    thrs = [THR, 1e-3, 0.05, 0.5] + own + near + [float(np.nextafter(v, np.inf)) for v in own + near]
    for thr in thrs:
        assert np.array_equal(oracle_pairs(oracle, fr, thr), e.astype(np.float64) < thr), thr


def test_other_baseline(oracle):
    fr = M.make_frame(504, 40, 90)
    e = M.errors(fr["pose"], fr["observations"], fr["lines"], baseline=0.3)
    for thr in (THR, 0.05, float(np.median(e))):
        assert np.array_equal(oracle_pairs(oracle, fr, thr, baseline=0.3), e.astype(np.float64) < thr)


def test_reference_reductions_on_ties():
    fr = M.make_frame(505, 6, 6, rot_sigma=0.0, t_sigma=0.0)
    fr["observations"] = fr["pair"]["obs1"][:6].copy()
    lines = fr["lines"]
    twice = dict(fr, lines=np.concatenate([lines[:1], lines]))             # line 0 twice: at 0 and 1
    r = M.match(twice, ratio=1.5)
    assert r["best_line"][0] == 0 and r["second_error"][0] == r["best_error"][0] and r["match"][0] == -1
    assert M.match(twice, ratio=1.0)["match"][0] == 0
    two = dict(fr, observations=np.concatenate([fr["observations"][:1]] * 2), lines=lines[:1])
    r = M.match(two, ratio=1.0)
    assert r["best_observation"][0] == 0 and list(r["match"]) == [0, -1] and r["num_matched"] == 1


def test_reference_statuses():
    fr = M.make_frame(506, 5, 9)
    assert M.match(dict(fr, observations=np.zeros((0, 8))))["status"] == M.EMPTY
    r = M.match(dict(fr, lines=np.zeros((0, 6))))
    assert r["status"] == M.EMPTY and (r["best_line"] == -1).all() and np.isinf(r["best_error"]).all()
    bad = fr["pose"].copy()
    bad[4] = np.nan
    r = M.match(dict(fr, pose=bad))
    assert r["status"] == M.INVALID_POSE and r["num_matched"] == 0 and (r["best_observation"] == -1).all()


END_TO_END_SEED = 520


def test_end_to_end_input_is_matchable():
    """The condition of the end-to-end GPU test: the reference matches at least 90 % of the 150 shuffled observations, all correctly"""
    fr = M.make_frame(END_TO_END_SEED, 150, 150)
    r = M.match(fr)
    ok = r["match"] >= 0
    print("matched by the reference: %d of 150" % ok.sum())
    assert ok.mean() >= 0.9
    assert np.array_equal(r["match"][ok], fr["truth"][ok])

"""The place recogniser without a device (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*, slslam_place_filter_*): hand-computed
cases that pin the numpy reference (tests/place_reference.py), the host Bayes filter through the C ABI against the numpy filter, the
tree file loader, and the property of the synthetic place sequence that the GPU test relies on."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as R  # noqa: E402

# The place sequence of the end-to-end tests (here and in test_gpu_place.py): tree (10, 3, 16) of seed 1; sequence of seed 3, 60 places of
# 30 words, noise 0.03, revisit of places 10 .. 24; recent 10, 20 average words; filter sigma 1.0, threshold 0.5, seq_len 5, min_docs 10.
# Chosen on the numpy reference so that no loop closes during the first pass, one closes within +-1 of the true place during the
# revisit, and no window sum comes within 1e-4 of the threshold (the smallest distance is 0.019).
SEQ = dict(tree=(10, 3, 16), tree_seed=1, seed=3, places=60, words=30, noise=0.03, revisit=(10, 25), recent=10, navg=20,
           filt=dict(sigma=1.0, threshold=0.5, seq_len=5, min_docs=10))


def seq_inputs():
    K, L, D = SEQ["tree"]
    nodes = synth.make_voctree(SEQ["tree_seed"], K, L, D)
    s = synth.make_place_sequence(SEQ["seed"], SEQ["places"], SEQ["words"], SEQ["noise"], SEQ["revisit"], dim=D)
    return R.Tree(K, L, D, nodes), nodes, s


def test_hand_computed_scores_and_likelihoods():
    """Tree (K, L, D) = (2, 1, 2) with the children (1, 0) and (0, 1): the descriptor (1, 0) has r = (0, 1) -> word 0, (0, 1) -> word 1.
    recent = 0 (a document is visible once one more is in), 5 average words (never a virtual document with 2 words).

    Three visible documents d0 = {0: 1}, d1 = {1: 1}, d2 = {0: 1/2, 1: 1/2}, query {0: 1}: doc_size 3, df = (2, 2), i = (float)log10(3 / 2).
      d0: n = m = i, l = -((0 - i) - i) = 2 i;   d1: no common word;   d2: n = i, m = i / 2, l = -((i / 2 - i) - i / 2) = i
      (doubling and halving are exact).  Two states touched, sum 3 i, fill = 3 i / (1 + 2) = i -> scores (2 i, i, i).
      mean = 4 i / 3, sigma = sqrt(2 i^2 - 16 i^2 / 9) = 0.4714 i, mean + 2 sigma = 2.276 i > 2 i: every likelihood is 1.
    Six visible documents d0 = {0: 1}, d1 .. d5 = {1: 1}, the same query: df[0] = 1, i = (float)log10(6), d0: l = 2 i, fill = 2 i / 2 = i,
      scores (2 i, i, i, i, i, i): mean = 7 i / 6, sigma = sqrt(9 / 6 - 49 / 36) i = sqrt(5) / 6 i, mean + 2 sigma = 1.912 i < 2 i:
      likelihood[d0] = (2 - sqrt(5) / 3) / (7 / 6) = 1.0754094, the others 1.  State -1 is not scored: score 0, likelihood 1."""
    tree = R.Tree(2, 1, 2, [[[1, 0], [0, 1]]])
    a, b = np.array([[1, 0]], dtype=np.float32), np.array([[0, 1]], dtype=np.float32)
    assert tree.words(np.vstack([a, b])).tolist() == [0, 1]
    db = R.Database(tree, recent=0, num_avg_words=5)
    for d in (a, b, np.vstack([a, b]), a):
        assert db.insert(d) == R.OK
    assert (db.visible, db.doc_size, db.df.tolist()) == (3, 3, [2, 2])
    q = db.query(a, top_k=2)
    i = np.float32(math.log10(1.5))
    assert q["status"] == R.OK and not q["has_virtual"]
    assert q["score"].view(np.uint32).tolist() == np.array([0, 2 * i, i, i], dtype=np.float32).view(np.uint32).tolist()
    assert q["touched"].tolist() == [0, 1, 0, 1] and q["likelihood"].tolist() == [1, 1, 1, 1]
    assert q["top_id"].tolist() == [0, 1]                       # d1 and d2 tie at i: the lower id

    db = R.Database(tree, recent=0, num_avg_words=5)
    for d in (a, b, b, b, b, b, a):
        db.insert(d)
    q = db.query(a)
    i = np.float32(math.log10(6.0))
    assert q["score"].view(np.uint32).tolist() == np.array([0, 2 * i, i, i, i, i, i], dtype=np.float32).view(np.uint32).tolist()
    assert q["likelihood"][[0, 2, 3, 4, 5, 6]].tolist() == [1] * 6
    assert abs(q["likelihood"][1] - (2 - math.sqrt(5) / 3) / (7 / 6)) < 2e-7


def test_hand_computed_tie_goes_to_the_lowest_child():
    """(2, 2, 2): the root's two children are the same centre (1, 0), so every descriptor ties there and goes to child 0 (node 1), whose
    children (1, 0), (0, 1) then decide: (0, 1) -> node 1 * 2 + 1 + 1 = 4 -> word 4 - 3 = 1.  Child 1 of the root would give word 2 or 3."""
    tree = R.Tree(2, 2, 2, [[[1, 0], [1, 0]], [[1, 0], [0, 1]], [[1, 0], [0, 1]]])
    assert tree.words([[0, 1], [1, 0], [0.6, 0.8]]).tolist() == [1, 0, 1]


def test_visibility_and_virtual_document_on_the_reference():
    tree = R.Tree(2, 2, 2, synth.make_voctree(4, 2, 2, 2))
    rng = np.random.default_rng(5)
    R_ = 3
    db = R.Database(tree, recent=R_, num_avg_words=2)
    for k in range(R_ + 1):
        db.insert(rng.standard_normal((4, 2)))
    assert db.visible == 0 and db.doc_size == 0
    db.insert(rng.standard_normal((4, 2)))
    assert db.visible == 1 and db.df.sum() == len(db.docs[0][0])
    assert db.insert(np.zeros((0, 2))) == R.EMPTY and db.insert([[np.nan, 0]]) == R.INVALID and len(db.docs) == R_ + 2


def _abi_filter(liks, **kw):
    f = capi.PlaceFilter(**kw)
    out = [f.update(l) for l in liks]
    f.close()
    return out


def _compare(liks, **kw):
    ref = R.Filter(**kw)
    got = _abi_filter(liks, **kw)
    for l, (loop, kf, post) in zip(liks, got):
        rl, rk, rp = ref.update(l)
        assert post.shape == rp.shape and np.all(np.abs(post - rp) <= 1e-5 * np.abs(rp)), (post, rp)
        assert (loop, kf) == (rl, rk)
    assert ref.margin > 1e-4                                   # no window sum of the reference within 1e-4 of the threshold
    return got


def test_filter_against_numpy_on_a_growing_visible_set():
    rng = np.random.default_rng(21)
    liks = []
    for n in list(range(0, 30)) + [30] * 25:                   # N = 0, 1, ... : the visible set grows between updates, then stays
        l = np.ones(n + 1, dtype=np.float32)
        if n >= 6:
            l[1 + rng.integers(0, n, 3)] = rng.uniform(1.5, 6.0, 3).astype(np.float32)
        if n == 30:
            l[1 + min(len(liks) - 20, 29)] = np.float32(8.0)     # a peak that walks along the documents: the loop the filter is for
        liks.append(l)
    got = _compare(liks, sigma=0.8, threshold=0.6, seq_len=4, min_docs=8)
    assert any(loop for loop, _, _ in got) and not any(loop for loop, _, _ in got[:8])
    for _, _, post in got:
        assert abs(float(post.astype(np.float64).sum()) - 1.0) < 1e-5


def test_filter_edges():
    # N = 0 and N = 1; N < min_docs never decides, even with all mass on one document
    got = _compare([np.ones(1, np.float32), np.array([1, 50], np.float32), np.array([0, 1, 0], np.float32)],
                   sigma=1.0, threshold=0.1, seq_len=0, min_docs=5)
    assert got[0][2].tolist() == [1.0] and not any(g[0] for g in got)
    # the same with min_docs 2: the third step decides for document 0
    got = _compare([np.ones(1, np.float32), np.array([1, 50], np.float32), np.array([0, 1, 0], np.float32)],
                   sigma=1.0, threshold=0.1, seq_len=0, min_docs=2)
    assert (got[2][0], got[2][1]) == (True, 0)
    # an all-zero likelihood: uniform posterior, and the filter goes on from it
    got = _compare([np.ones(4, np.float32), np.zeros(4, np.float32), np.ones(4, np.float32)], sigma=1.0, threshold=0.99, seq_len=1, min_docs=0)
    assert got[1][2].tolist() == [0.25] * 4
    # a window needs seq_len + 1 documents: none fits, no decision
    got = _compare([np.array([0, 1, 1, 1], np.float32)], sigma=1.0, threshold=0.01, seq_len=3, min_docs=0)
    assert got[0][0] is False


def test_filter_arguments():
    L = capi.lib()
    h = C.c_void_p()
    assert L.slslam_place_filter_create(0.0, 0.5, 5, 10, C.byref(h)) == 1
    assert L.slslam_place_filter_create(1.0, float("nan"), 5, 10, C.byref(h)) == 1
    assert L.slslam_place_filter_create(1.0, 0.5, -1, 10, C.byref(h)) == 1
    assert L.slslam_place_filter_create(1.0, 0.5, 5, 10, None) == 1
    assert L.slslam_place_filter_create(1.0, 0.5, 5, 10, C.byref(h)) == 0
    assert L.slslam_place_filter_update(h, -1, None, None, None, None) == 1
    one = np.ones(1, dtype=np.float32)
    assert L.slslam_place_filter_update(h, 0, capi._fp(one), None, None, None) == 0
    assert L.slslam_place_filter_update(None, 0, capi._fp(one), None, None, None) == 1
    L.slslam_place_filter_destroy(h)
    L.slslam_place_filter_destroy(None)


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_voctree_load_takes_exactly_the_tree(tmp_path, delta):
    K, L, D = 3, 2, 5
    nodes = synth.make_voctree(9, K, L, D)
    raw = nodes.reshape(-1)
    p = tmp_path / "tree.bin"
    (np.concatenate([raw, np.ones(1, np.float32)]) if delta > 0 else raw[:len(raw) + delta]).tofile(p)
    if delta == 0:
        t = capi.VocTree(K, L, D, path=str(p))
        assert t.num_leaves == 9
        t.close()
    else:
        with pytest.raises(capi.SlslamError) as ei:
            capi.VocTree(K, L, D, path=str(p))
        assert ei.value.status == 1
    with pytest.raises(capi.SlslamError):
        capi.VocTree(K, L, D, path=str(tmp_path / "missing.bin"))


def test_place_sequence_closes_the_loop_on_the_reference():
    tree, _, s = seq_inputs()
    out, flt = R.pipeline(tree, s["frames"], SEQ["recent"], SEQ["navg"], **SEQ["filt"])
    first = s["first_pass"]
    assert len(out) == 75 and not any(loop for loop, _ in out[:first])
    hits = [(i, kf) for i, (loop, kf) in enumerate(out) if loop]
    assert hits and all(abs(kf - int(s["place"][i])) <= 1 for i, kf in hits)
    assert flt.margin > 1e-4

"""The place recogniser without a device (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*, slslam_place_filter_*): hand-computed
cases that pin the numpy reference (tests/place_reference.py), the host Bayes filter through the C ABI against the numpy filter, the
tree file loader, and the property of the synthetic place sequence that the GPU test relies on.  The inputs with which test_gpu_place.py
goes past one pass of the kernels' loops are made here, and tests here assert on the reference alone what each of them is."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


# ---- inputs of the GPU tests beyond one pass of the in-kernel loops (test_gpu_place.py imports them; what each is,
# the test_the_..._what_..._gpu_test_says tests below assert on the reference).  Seeded, made once, shared, never written to.
# The sizes are the kernels' (csrc/place_recognition.h; the test below reads them there): k_place_finish walks the states in trips of
# FINISH_THREADS from state `first` = 1 - has_virtual (the keys of top_k from state 1), its ordered fill sum takes FILL_CHUNK states at a
# time from state `first`; nearest_child takes CHILD_BLOCK children at a time; a document holds at most MAX_WORDS words.
FINISH_THREADS, FILL_CHUNK, CHILD_BLOCK, MAX_WORDS, MAX_TOP_K, MAX_K, MAX_L, MAX_D = 256, 1024, 8, 512, 32, 64, 4, 128


def unit(rng, n, D):
    d = rng.standard_normal((n, D))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def frozen(a):
    a.setflags(write=False)
    return a


# The walk: one database that grows to 1300 visible documents, queried on the way.  Document d is state d + 1.  Frame `a` is inserted as
# the documents 254 .. 257 (states 255 .. 258: about the second trip, which begins at state 256 with a virtual document and at 257
# without, and for the keys always at 257) and again as document 700; frame `b` as the documents 1022 .. 1025 (states 1023 .. 1026, about
# the second chunk at state 1024 or 1025) and before that as document 300.  Copies of one frame score alike bit for bit, so top_k has to
# order them by document number across trips.  `b` begins with two descriptors of `a`, the 12-descriptor query with one, and the
# 1-descriptor query is a's first: every query touches every copy.
WALK = dict(tree=(40, 2, 8), tree_seed=11, seed=12, inserts=1301, max_docs=1400, max_words=64, top_k=MAX_TOP_K,
            points=(255, 256, 257, 1023, 1024, 1025, 1026, 1300), navg={"virtual": 10, "plain": 2000},
            a_at=(254, 255, 256, 257, 700), b_at=(300, 1022, 1023, 1024, 1025))


@functools.lru_cache(maxsize=None)
def walk_inputs():
    K, L, D = WALK["tree"]
    rng = np.random.default_rng(WALK["seed"])
    a = unit(rng, 9, D)
    b = np.vstack([a[:2], unit(rng, 6, D)])
    frames = [unit(rng, int(rng.integers(6, 11)), D) for _ in range(WALK["inserts"])]
    for d in WALK["a_at"]:
        frames[d] = a
    for d in WALK["b_at"]:
        frames[d] = b
    queries = {"twelve": np.vstack([a[1:2], unit(rng, 11, D)]), "one": a[:1].copy(), "a": a, "b": b}
    for f in frames + list(queries.values()):
        frozen(f)
    return dict(nodes=frozen(synth.make_voctree(WALK["tree_seed"], K, L, D)), frames=frames, queries=queries)


@functools.lru_cache(maxsize=None)
def walk_reference(walk):
    """walk: "virtual" (10 average words: a virtual document from early on, first = 0) or "plain" (2000: never one, first = 1).  Returns
    {visible: {query name: the reference's result}} at the WALK's points and "virtual_from": the number of visible documents at which
    the virtual document appeared (None: never)."""
    K, L, D = WALK["tree"]
    inp = walk_inputs()
    db = R.Database(R.Tree(K, L, D, inp["nodes"]), 0, WALK["navg"][walk])
    out = {"virtual_from": None}
    for fr in inp["frames"]:
        assert db.insert(fr) == R.OK
        if out["virtual_from"] is None and len(db.virtual):
            out["virtual_from"] = db.visible
        assert out["virtual_from"] is None or len(db.virtual)          # once there, it stays
        if db.visible in WALK["points"]:
            out[db.visible] = {name: db.query(q, top_k=WALK["top_k"]) for name, q in inp["queries"].items()}
    return out


# Documents at the word limit: tree (64, 2, 16), 4096 words.  Frames of exactly 63, 64, 65 (about a wave of run starts), 511 and 512
# distinct words, one descriptor each in a shuffled order; `twice`: 512 descriptors, 256 distinct words twice each; `one`: a word of
# the 64, the 511, the 512 and `twice`.  The 511 are words of the 512.
LIMIT = dict(tree=(64, 2, 16), tree_seed=13, seed=14, max_docs=1100, max_words=MAX_WORDS, navg=100, top_k=8,
             counts={"w63": 63, "w64": 64, "w65": 65, "w511": 511, "w512": 512, "twice": 256, "one": 1},
             first=("plain0", "plain1", "w63", "plain2", "w64", "w65", "plain3"), then=("w511", "w512", "twice", "plain4"))


@functools.lru_cache(maxsize=None)
def limit_inputs():
    K, L, D = LIMIT["tree"]
    nodes = frozen(synth.make_voctree(LIMIT["tree_seed"], K, L, D))
    tree = R.Tree(K, L, D, nodes)
    rng = np.random.default_rng(LIMIT["seed"])
    drawn = unit(rng, 3000, D)
    pool, row = np.unique(tree.words(drawn), return_index=True)            # the words random descriptors reach, and one descriptor of each
    assert len(pool) >= 600
    pool = pool.tolist()
    words = {"w512": pool[:512], "w511": pool[1:512], "w65": pool[500:565], "w64": pool[0:512:8], "w63": pool[5:572:9],
             "twice": pool[256:512] * 2, "one": pool[304:305]}
    frames = {}
    for name, w in words.items():
        d = drawn[row[np.searchsorted(pool, w)]]
        frames[name] = frozen(d[rng.permutation(len(d))])
    for k in range(5):
        frames["plain%d" % k] = frozen(unit(rng, 20 + 5 * k, D))
    return dict(nodes=nodes, frames=frames, queries=("w63", "w64", "w65", "w511", "w512", "twice", "one", "plain4"))


@functools.lru_cache(maxsize=None)
def limit_reference():
    """the reference's results of every query after the `first` inserts and after the `then` inserts, and its database"""
    K, L, D = LIMIT["tree"]
    inp = limit_inputs()
    db = R.Database(R.Tree(K, L, D, inp["nodes"]), 0, LIMIT["navg"])
    out = {}
    for stage in ("first", "then"):
        for name in LIMIT[stage]:
            assert db.insert(inp["frames"][name]) == R.OK
        out[stage] = {q: db.query(inp["frames"][q], top_k=LIMIT["top_k"]) for q in inp["queries"]}
        out[stage + "_virtual"] = db.virtual.copy()
    out["db"] = db
    return out


# Trees at the child-block edges and at the limits: 8 and 16 children (no padding in the last block of CHILD_BLOCK), 9 (a block with one
# real child), L = 4, the largest root (64 x 128 floats = 32 KB of LDS) and 64 children over two levels.
EDGE_MAX_WORDS, EDGE_TREE_SEED = 96, 13          # (the seed: a (3, 4, 8) tree whose 81 words random descriptors all reach)
EDGE_TREES = [(8, 2, 8), (9, 2, 8), (16, 2, 8), (3, 4, 8), (64, 1, 128), (64, 2, 16)]


@functools.lru_cache(maxsize=None)
def edge_tree_inputs(shape):
    K, L, D = shape
    rng = np.random.default_rng(100 * K + 10 * L + D)
    nodes = frozen(synth.make_voctree(EDGE_TREE_SEED, K, L, D))
    inserts = [frozen(unit(rng, n, D)) for n in (65, 7, 33, 64, 1, 20, 65, 12, 80, 41, 8, 64)]
    drawn = unit(rng, 2000 * (MAX_D // D), D)
    _, row = np.unique(R.Tree(K, L, D, nodes).words(drawn), return_index=True)
    inserts.insert(6, frozen(drawn[row[:EDGE_MAX_WORDS]]))          # one descriptor of each word that many random ones reach, up to max_words
    return dict(nodes=nodes, inserts=inserts, queries=[frozen(unit(rng, 65, D)), inserts[0][:1], frozen(unit(rng, 40, D))])


# Two equal children: (16, 2, 8) with root child `copy` an exact copy of root child `of`: in different blocks of CHILD_BLOCK (11 of 3)
# and in one (5 of 2).  The descriptors are those, among random ones, whose nearest root child is the doubled one: the strict < sends
# them down the lower.  `control` is the same tree with the copy's centre negated instead.
TIE_TREES = {"across_blocks": (3, 11), "within_a_block": (2, 5)}


@functools.lru_cache(maxsize=None)
def tie_tree_inputs(name):
    K, L, D = 16, 2, 8
    of, copy = TIE_TREES[name]
    nodes = synth.make_voctree(16, K, L, D).copy()
    control = nodes.copy()
    nodes[0, copy] = nodes[0, of]
    control[0, copy] = -nodes[0, of]
    tree = R.Tree(K, L, D, nodes)
    rng = np.random.default_rng(17 + copy)
    tied = np.zeros((0, D), np.float32)
    while len(tied) < 20:
        d = unit(rng, 256, D)
        tied = np.vstack([tied, d[np.isin(tree.words(d) // K, (of, copy))]])
    return dict(nodes=frozen(nodes), control=frozen(control), tied=frozen(tied),
                inserts=[frozen(np.vstack([tied[i::3], unit(rng, 10 + i, D)])) for i in range(3)] + [frozen(unit(rng, 30, D)) for _ in range(4)],
                queries=[tied, frozen(np.vstack([tied[:5], unit(rng, 20, D)])), tied[:1]])


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


# ---- the inputs of the GPU tests beyond one pass of the in-kernel loops
def _clear(res):
    """no score of the reference within 1e-9 max(1, |mean|) of the bar: the GPU test may compare the likelihoods"""
    return res["status"] == R.OK and res["mean"] != 0.0 and res["margin"] > 1e-9


def test_the_sizes_are_the_kernels():
    src = open(os.path.join(ROOT, "slslam_amd", "csrc", "place_recognition.h")).read()
    assert "constexpr int kMaxK = %d, kMaxL = %d, kMaxD = %d, kMaxWords = %d, kMaxTopK = %d;" % (MAX_K, MAX_L, MAX_D, MAX_WORDS, MAX_TOP_K) in src
    for line in ("kFinishThreads = %d;" % FINISH_THREADS, "kFillChunk = %d;" % FILL_CHUNK, "kChildBlock = %d;" % CHILD_BLOCK,
                 "kDocThreads = %d;" % MAX_WORDS, "const int first = 1 - has_virtual;"):
        assert line in src, line


@pytest.mark.parametrize("walk", ["virtual", "plain"])
def test_the_walk_is_what_its_gpu_test_says(walk):
    inp, ref = walk_inputs(), walk_reference(walk)
    K, L, D = WALK["tree"]
    assert len(inp["frames"]) == WALK["inserts"] <= WALK["max_docs"] and WALK["max_docs"] >= 1400
    assert all(6 <= len(f) <= 10 for f in inp["frames"]) and max(len(q) for q in inp["queries"].values()) <= WALK["max_words"]
    assert [len(inp["queries"][q]) for q in ("twelve", "one")] == [12, 1]
    assert sorted(k for k in ref if k != "virtual_from") == list(WALK["points"])
    # a virtual document throughout the first walk, never one in the second: first = 0 and first = 1
    has_virtual = walk == "virtual"
    assert (ref["virtual_from"] is not None and ref["virtual_from"] < WALK["points"][0]) if has_virtual else ref["virtual_from"] is None
    first = 0 if has_virtual else 1
    copies = {"a": WALK["a_at"], "b": WALK["b_at"]}
    # the copies lie about both trip boundaries (of the state loops and of the key loop) and about the chunk boundary of either walk
    for lo, hi, at in ((FINISH_THREADS, FINISH_THREADS + 1, WALK["a_at"]), (FILL_CHUNK, FILL_CHUNK + 1, WALK["b_at"])):
        states = [d + 1 for d in at]
        assert {lo - 1, lo, hi, hi + 1} <= set(states)
    assert WALK["a_at"][-1] - WALK["a_at"][0] > FINISH_THREADS and WALK["b_at"][1] - WALK["b_at"][0] > FINISH_THREADS
    for visible in WALK["points"]:
        for name, res in ref[visible].items():
            assert res["has_virtual"] == has_virtual and len(res["score"]) == visible + 1
            assert _clear(res), (visible, name, res["margin"])
            t = res["touched"].astype(bool)
            assert all(t[d + 1] for at in copies.values() for d in at if d < visible), (visible, name)      # every copy is touched
            if visible > FILL_CHUNK:                             # the second chunk has touched states, the first too; the fill matters
                assert t[first:first + FILL_CHUNK].any() and t[first + FILL_CHUNK:].any()
                assert (~t[first:]).sum() >= 300, (visible, name, (~t[first:]).sum())
            assert t[first:].sum() >= 3 or visible < FINISH_THREADS + 2
        # bit-for-bit ties that the lower document number decides, from different trips of the key loop
        for name, at in copies.items():
            res, seen = ref[visible][name], [d for d in at if d < visible]
            assert res["top_id"][:len(seen)].tolist() == seen, (visible, name)
            assert len(seen) == 0 or len(set(res["top_score"][:len(seen)].view(np.uint32).tolist())) == 1
            assert len(seen) == len(at) or visible < 1026
            if seen:
                assert res["top_score"][len(seen)] < res["top_score"][0]
        assert (ref[visible]["a"]["top_id"] >= 0).all()           # 32 documents to name at every point
    last = ref[WALK["points"][-1]]
    assert last["a"]["top_id"][:5].tolist() == list(WALK["a_at"]) and last["b"]["top_id"][:5].tolist() == list(WALK["b_at"])
    assert sum(d // FINISH_THREADS for d in WALK["a_at"]) > 0 and len({d // FINISH_THREADS for d in WALK["a_at"]}) >= 3


def test_the_limit_documents_are_what_their_gpu_test_says():
    K, L, D = LIMIT["tree"]
    inp, ref = limit_inputs(), limit_reference()
    tree = R.Tree(K, L, D, inp["nodes"])
    for name, distinct in LIMIT["counts"].items():
        w = tree.words(inp["frames"][name])
        assert len(set(w.tolist())) == distinct, name
        assert len(w) == (512 if name == "twice" else distinct)
        assert not np.array_equal(w, np.sort(w)) or len(w) == 1, name                  # the sort has work to do
    assert np.array_equal(np.unique(tree.words(inp["frames"]["twice"]), return_counts=True)[1], np.full(256, 2))
    assert set(tree.words(inp["frames"]["w511"]).tolist()) < set(tree.words(inp["frames"]["w512"]).tolist())
    assert LIMIT["max_words"] == MAX_WORDS == 512 and LIMIT["max_docs"] > FILL_CHUNK       # the column stride of a stored document
    assert len(inp["queries"]) == 8 and set(LIMIT["first"] + LIMIT["then"]) >= set(LIMIT["counts"]) - {"one"}
    db = ref["db"]
    assert db.visible == len(LIMIT["first"]) + len(LIMIT["then"]) - 1 and len(ref["then_virtual"]) == LIMIT["navg"]
    assert [len(db.docs[len(LIMIT["first"]) + i][0]) for i in range(3)] == [511, 512, 256]
    for stage in ("first", "then"):
        for q, res in ref[stage].items():
            assert _clear(res), (stage, q, res.get("margin"))
    s511 = len(LIMIT["first"]) + 1                               # the states of the 511-word, the 512-word and the `twice` document
    for q in ("w512", "w511", "one", "twice", "w64"):
        assert ref["then"][q]["touched"][s511:s511 + 3].all(), q
    assert ref["first"]["one"]["touched"][LIMIT["first"].index("w64") + 1]
    assert ref["then"]["w511"]["top_id"][0] == s511 - 1 and ref["then"]["w512"]["top_id"][0] == s511 and ref["then"]["twice"]["top_id"][0] == s511 + 1


@pytest.mark.parametrize("shape", EDGE_TREES)
def test_the_edge_trees_are_what_their_gpu_test_says(shape):
    K, L, D = shape
    inp = edge_tree_inputs(shape)
    tree = R.Tree(K, L, D, inp["nodes"])
    assert K <= MAX_K and L <= MAX_L and D <= MAX_D
    words = np.concatenate([tree.words(f) for f in inp["inserts"] + inp["queries"]])
    last_block = CHILD_BLOCK * ((K - 1) // CHILD_BLOCK)
    for level in range(L):                                       # at every level: child 0, the first child of the last block, the last child
        child = (words // K ** (L - 1 - level)) % K
        assert {0, last_block, K - 1} <= set(child.tolist()), (shape, level)
    if shape == (3, 4, 8):
        assert len(set(words.tolist())) == 81
    if K == 9:
        assert last_block == 8 == K - 1                          # a block that holds one real child and seven copies of it
    if K in (8, 16):
        assert K % CHILD_BLOCK == 0
    if shape == (64, 1, 128):
        assert 4 * K * D == 32768
    db = R.Database(tree, 1, 3)
    for f in inp["inserts"]:
        assert db.insert(f) == R.OK
    assert db.visible == 11 and len(db.virtual) == 3 and max(len(f) for f in inp["inserts"]) <= EDGE_MAX_WORDS
    for q in inp["queries"]:
        assert _clear(db.query(q, top_k=3))


@pytest.mark.parametrize("name", sorted(TIE_TREES))
def test_the_tie_trees_are_what_their_gpu_test_says(name):
    K, L, D = 16, 2, 8
    of, copy = TIE_TREES[name]
    inp = tie_tree_inputs(name)
    assert (of // CHILD_BLOCK != copy // CHILD_BLOCK) == (name == "across_blocks") and of < copy
    tree, control = R.Tree(K, L, D, inp["nodes"]), R.Tree(K, L, D, inp["control"])
    assert np.array_equal(tree.nodes[0, of], tree.nodes[0, copy]) and not np.array_equal(tree.nodes[of + 1], tree.nodes[copy + 1])
    tied = inp["tied"]
    assert len(tied) >= 20
    # the distances to the two children are equal bit for bit and below every other child's: a tie and nothing else decides
    r = np.ones((len(tied), K), dtype=np.float32)
    for i in range(D):
        r = r - tree.nodes[0][None, :, i] * tied[:, i, None]
    assert (r[:, of].view(np.uint32) == r[:, copy].view(np.uint32)).all()
    others = np.delete(r, [of, copy], axis=1)
    assert (r[:, of] < others.min(axis=1)).all() and (r[:, of] < 1.0).all()
    # the reference sends every one down the lower child; with the copy taken away the same descriptors pick the same child and word
    w = tree.words(tied)
    assert (w // K == of).all()
    assert np.array_equal(control.words(tied), w)
    # the higher child's subtree would give other words
    swapped = inp["nodes"].copy()
    swapped[of + 1] = inp["nodes"][copy + 1]
    assert (R.Tree(K, L, D, swapped).words(tied) // K == of).all()
    db = R.Database(tree, 0, 5)
    for f in inp["inserts"]:
        assert db.insert(f) == R.OK
    for q in inp["queries"]:
        assert _clear(db.query(q, top_k=3))

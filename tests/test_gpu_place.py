"""The place recogniser on the device (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*) against the numpy reference
(tests/place_reference.py): words, status, touched and top_k exactly, scores bit for bit, likelihoods within 1e-6 relative (the double
reductions of mean and sigma are reordered on the device, ~1e-13, and the result is rounded once to float, 2^-24: 1e-6 is about 16 float
ulps) wherever the reference has no score within 1e-9 max(1, |mean|) of mean + 2 sigma.  The largest likelihood difference seen is
printed.  The inputs past one pass of the kernels' loops and their references are those of tests/test_place_cpu.py: made once, shared,
never written to."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

from slslam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as R  # noqa: E402
import test_place_cpu as T  # noqa: E402
from test_place_cpu import SEQ, seq_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 512]
WORST = {"likelihood": 0.0}             # the largest relative likelihood difference check() has seen


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def check(got, ref, top_k=0):
    assert got["status"] == ref["status"]
    assert np.array_equal(got["words"], ref["words"])
    assert got["has_virtual"] == ref["has_virtual"]
    assert bits(got["score"]) == bits(ref["score"])
    assert np.array_equal(got["touched"], ref["touched"])
    if top_k:
        assert np.array_equal(got["top_id"], ref["top_id"]) and bits(got["top_score"]) == bits(ref["top_score"])
    if ref["status"] == R.OK and ref["mean"] != 0.0:
        assert ref["margin"] > 1e-9
    WORST["likelihood"] = max(WORST["likelihood"], float(np.max(np.abs(got["likelihood"] - ref["likelihood"]) / np.abs(ref["likelihood"]))))
    assert np.all(np.abs(got["likelihood"] - ref["likelihood"]) <= 1e-6 * np.abs(ref["likelihood"])), (got["likelihood"], ref["likelihood"])


def same_bytes(a, b):
    return a["status"] == b["status"] and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
                                              for k in ("words", "score", "touched", "likelihood", "top_id", "top_score"))


class Pair:
    """a device database and the reference's, fed alike"""

    def __init__(self, hip, K, L, D, seed, recent, navg, max_docs=160, max_words=512, max_frames=8, nodes=None):
        nodes = synth.make_voctree(seed, K, L, D) if nodes is None else nodes
        self.ref_tree = R.Tree(K, L, D, nodes)
        self.tree = hip.VocTree(K, L, D, nodes)
        self.db = hip.PlaceDB(self.tree, max_docs=max_docs, max_words=max_words, max_frames=max_frames, recent=recent, num_avg_words=navg)
        self.ref = R.Database(self.ref_tree, recent, navg)
        self.rng = np.random.default_rng(seed + 100)
        self.D = D

    def frame(self, n):
        d = self.rng.standard_normal((n, self.D))
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)

    def for_words(self, words):
        """one descriptor per requested word (drawn until every word has one)"""
        have = {}
        while any(w not in have for w in words):
            d = self.frame(256)
            for w, row in zip(self.ref_tree.words(d).tolist(), d):
                have.setdefault(w, row)
        return np.stack([have[w] for w in words])

    def reachable(self):
        """the words random descriptors reach, ascending (a random tree may leave a leaf without any)"""
        return sorted(set(self.ref_tree.words(self.frame(2000)).tolist()))

    def insert(self, fr):
        st = self.db.insert(fr)
        assert st["status"] == self.ref.insert(fr)
        return st

    def close(self):
        self.db.close()
        self.tree.close()


def test_shapes_against_reference(hip):
    """(5, 2, 8): 25 words, so the words of a frame collide.  Frames of 1, 63, 64, 65, 512 descriptors, one whose 512 descriptors all fall
    into one word and one of distinct words, against 0, 1, 63, 64, 65 and 130 visible documents."""
    p = Pair(hip, 5, 2, 8, seed=2, recent=2, navg=10)
    one = np.repeat(p.frame(1), 512, axis=0)
    seen = p.reachable()
    distinct = p.for_words(seen)
    assert len(set(p.ref_tree.words(one).tolist())) == 1 and len(seen) >= 20
    queries = [p.frame(n) for n in SIZES] + [one, distinct]
    done = set()
    k = 0
    while p.ref.visible < 130:
        if p.ref.visible in (0, 1, 63, 64, 65) and p.ref.visible not in done and len(p.ref.docs) >= 3:
            done.add(p.ref.visible)
            for g, q in zip(p.db.run(queries, top_k=5), queries):
                check(g, p.ref.query(q, top_k=5), top_k=5)
        fr = [p.frame(SIZES[k % 5]), one, distinct][0 if k % 7 else (k // 7) % 3]
        st = p.insert(fr)
        assert np.array_equal(st["words"], p.ref_tree.words(fr))
        k += 1
    assert done == {0, 1, 63, 64, 65} and p.db.size() == {"inserted": 133, "visible": 130, "doc_size": 131}
    for g, q in zip(p.db.run(queries, top_k=32), queries):
        check(g, p.ref.query(q, top_k=32), top_k=32)
    p.close()


@pytest.mark.parametrize("shape", [(2, 1, 2), (40, 3, 72)])
def test_other_trees(hip, shape):
    K, L, D = shape
    p = Pair(hip, K, L, D, seed=3, recent=1, navg=3 if K == 40 else 1, max_docs=16, max_words=80)
    for n in (65, 7, 33, 64, 1, 20, 65, 12):
        p.insert(p.frame(n))
    assert p.db.size()["visible"] == 6 == p.ref.visible
    queries = [p.frame(65), p.frame(1), p.frame(40)]
    for g, q in zip(p.db.run(queries, top_k=3), queries):
        check(g, p.ref.query(q, top_k=3), top_k=3)
    p.close()


def worst():
    print("largest relative likelihood difference so far: %.3g" % WORST["likelihood"])


@pytest.mark.parametrize("walk", ["virtual", "plain"])
def test_walk_past_the_trips_and_chunks_of_finish(hip, walk):
    """One database grown to 1300 visible documents (test_place_cpu.WALK) and queried at 255, 256, 257 (k_place_finish's strided loops
    take a second trip from state 256 on), 1023 .. 1026 (its ordered fill sum carries from one chunk of 1024 states into the next) and
    1300, with and without a virtual document (`first` moves every boundary by a state).  Copies of two of the queries sit on either
    side of each boundary and again more than 256 documents away: bit-equal scores that top_k orders by document across trips; most
    states are untouched, so the fill decides their score.  The reference's side is test_place_cpu.walk_reference, made once."""
    K, L, D = T.WALK["tree"]
    inp, ref = T.walk_inputs(), T.walk_reference(walk)
    ref_tree = R.Tree(K, L, D, inp["nodes"])
    want_words = [ref_tree.words(fr) for fr in inp["frames"]]
    names, queries = list(inp["queries"]), list(inp["queries"].values())
    tree = hip.VocTree(K, L, D, inp["nodes"])
    db = hip.PlaceDB(tree, max_docs=T.WALK["max_docs"], max_words=T.WALK["max_words"], max_frames=len(queries), recent=0,
                     num_avg_words=T.WALK["navg"][walk])
    seen = []
    t0 = time.perf_counter()
    for k, fr in enumerate(inp["frames"]):
        st = db.insert(fr)
        assert st["status"] == "OK" and np.array_equal(st["words"], want_words[k]), k
        if k in T.WALK["points"]:                                # recent = 0: k + 1 inserted, k visible
            assert db.size() == {"inserted": k + 1, "visible": k, "doc_size": k + (walk == "virtual")}
            for name, g in zip(names, db.run(queries, top_k=T.WALK["top_k"])):
                check(g, ref[k][name], top_k=T.WALK["top_k"])
                assert g["has_virtual"] == (walk == "virtual")
            seen.append(k)
    print("walk %s: %d inserts and %d queries in %.2f s" % (walk, len(inp["frames"]), len(seen) * len(queries), time.perf_counter() - t0))
    assert seen == list(T.WALK["points"]) and db.stats()["allocations"] == 1
    db.close()
    tree.close()
    worst()


def test_documents_at_the_word_limit(hip):
    """(64, 2, 16), max_words 512 (test_place_cpu.LIMIT): documents of 63, 64 and 65 distinct words (the run starts of k_place_document
    about one wave), of 511 and of 512 (every thread starts a run), and 512 descriptors in 256 words; first as queries only, then also
    stored in a database of more than 1024 columns: 512 query words against 512 stored ones, and 1 against 512.  The stored
    documents' lengths show in df, hence in the virtual document and in every score."""
    K, L, D = T.LIMIT["tree"]
    inp, ref = T.limit_inputs(), T.limit_reference()
    p = Pair(hip, K, L, D, seed=0, recent=0, navg=T.LIMIT["navg"], max_docs=T.LIMIT["max_docs"], max_words=T.LIMIT["max_words"],
             max_frames=len(inp["queries"]), nodes=inp["nodes"])
    queries = [inp["frames"][q] for q in inp["queries"]]
    for stage in ("first", "then"):
        for name in T.LIMIT[stage]:
            st = p.insert(inp["frames"][name])
            assert np.array_equal(st["words"], p.ref_tree.words(inp["frames"][name])), name
        assert np.array_equal(p.db.virtual_words(), ref[stage + "_virtual"]) and np.array_equal(p.ref.virtual, ref[stage + "_virtual"])
        assert p.db.size()["doc_size"] == p.ref.doc_size
        for q, g in zip(inp["queries"], p.db.run(queries, top_k=T.LIMIT["top_k"])):
            check(g, ref[stage][q], top_k=T.LIMIT["top_k"])
    assert p.db.size() == {"inserted": 11, "visible": 10, "doc_size": 11}
    p.close()
    worst()


def small_database(hip, shape, inp, recent, navg):
    """a dozen inserts and the queries of `inp` against the reference fed alike, as test_other_trees does"""
    K, L, D = shape
    p = Pair(hip, K, L, D, seed=0, recent=recent, navg=navg, max_docs=16, max_words=T.EDGE_MAX_WORDS, nodes=inp["nodes"])
    for fr in inp["inserts"]:
        st = p.insert(fr)
        assert np.array_equal(st["words"], p.ref_tree.words(fr))
    got = p.db.run(inp["queries"], top_k=3)
    for g, q in zip(got, inp["queries"]):
        check(g, p.ref.query(q, top_k=3), top_k=3)
    p.close()
    return got


@pytest.mark.parametrize("shape", T.EDGE_TREES)
def test_trees_at_the_child_block_edges_and_the_limits(hip, shape):
    """8 and 16 children (whole blocks of nearest_child's 8), 9 (a block of one real child), four levels, the largest root and 64
    children over two levels; an insert of one descriptor per reachable word."""
    small_database(hip, shape, T.edge_tree_inputs(shape), recent=1, navg=3)
    worst()


@pytest.mark.parametrize("name", sorted(T.TIE_TREES))
def test_equal_children_go_to_the_lower(hip, name):
    """(16, 2, 8) with two equal root children, in one block of 8 and in two: the descriptors nearest to them go down the lower one."""
    of, _ = T.TIE_TREES[name]
    inp = T.tie_tree_inputs(name)
    got = small_database(hip, (16, 2, 8), inp, recent=0, navg=5)
    assert len(got[0]["words"]) >= 20 and (got[0]["words"] // 16 == of).all()
    worst()


def test_top_k_beyond_the_database(hip):
    """top_k = 32 against 1, 6 and 31 visible documents: the head is the documents in order, the tail -1 / +0.0f"""
    p = Pair(hip, 5, 2, 8, seed=9, recent=0, navg=10)
    queries = [p.frame(12), p.frame(1)]
    done = []
    while p.ref.visible < 31:
        p.insert(p.frame(5 + p.ref.visible % 7))
        v = p.ref.visible
        if v in (1, 6, 31):
            assert p.db.size()["visible"] == v
            for g, q in zip(p.db.run(queries, top_k=32), queries):
                ref = p.ref.query(q, top_k=32)
                check(g, ref, top_k=32)
                assert sorted(g["top_id"][:v].tolist()) == list(range(v))
                assert g["top_id"][v:].tolist() == [-1] * (32 - v) and bits(g["top_score"][v:]) == [0] * (32 - v)
            done.append(v)
    assert done == [1, 6, 31]
    p.close()


def test_virtual_document_threshold_and_df_tie(hip):
    p = Pair(hip, 5, 2, 8, seed=4, recent=0, navg=3)
    a, b, c, d, e = p.reachable()[1:10:2]
    pend = p.frame(5)
    p.insert(p.for_words([a, b, c, c]))
    p.insert(pend)                                             # recent = 0: the first document is visible now
    assert p.db.size() == {"inserted": 2, "visible": 1, "doc_size": 1}            # 3 words with df > 0 = num_avg_words: no virtual document
    assert len(p.db.virtual_words()) == 0 and len(p.ref.virtual) == 0
    q = p.for_words([a, c, d, e])
    check(p.db.run([q], top_k=2)[0], p.ref.query(q, top_k=2), top_k=2)
    p.insert(p.for_words([a, b, d]))                            # `pend` becomes visible: its words decide; then this one
    p.insert(pend)
    assert p.db.size()["visible"] == 3 and p.ref.visible == 3
    assert p.db.size()["doc_size"] == p.ref.doc_size == 4 and np.array_equal(p.db.virtual_words(), p.ref.virtual)
    g = p.db.run([q], top_k=2)[0]
    assert g["has_virtual"]
    check(g, p.ref.query(q, top_k=2), top_k=2)
    # a df tie that the lower word decides: documents over exactly {a, b, c, d}, df (2, 2, 1, 1) -> the virtual document is {a, b, c}
    p2 = Pair(hip, 5, 2, 8, seed=4, recent=0, navg=3)
    p2.insert(p2.for_words([a, b, c]))
    p2.insert(p2.for_words([a, b, d]))
    assert p2.db.size()["doc_size"] == 1 and len(p2.db.virtual_words()) == 0
    p2.insert(p2.for_words([a]))
    assert p2.db.virtual_words().tolist() == [a, b, c] == p2.ref.virtual.tolist() and p2.db.size()["doc_size"] == 3
    check(p2.db.run([q])[0], p2.ref.query(q))
    p.close()
    p2.close()


def test_visibility_rule(hip):
    Rr = 4
    p = Pair(hip, 5, 2, 8, seed=5, recent=Rr, navg=30)          # (25 words: never a virtual document)
    q = p.frame(30)
    for k in range(Rr + 1):
        p.insert(p.frame(20))
    assert p.db.size() == {"inserted": Rr + 1, "visible": 0, "doc_size": 0}
    g = p.db.run([q])[0]
    assert g["status"] == "EMPTY" and g["likelihood"].tolist() == [1.0] and np.array_equal(g["words"], p.ref_tree.words(q))
    p.insert(p.frame(20))
    assert p.db.size() == {"inserted": Rr + 2, "visible": 1, "doc_size": 1} and p.ref.visible == 1
    check(p.db.run([q])[0], p.ref.query(q))
    p.close()


def test_mixed_call_and_invalid_insert(hip):
    p = Pair(hip, 5, 2, 8, seed=6, recent=1, navg=10)
    for k in range(12):
        p.insert(p.frame(40 + k))
    nan, inf = p.frame(9), p.frame(65)
    nan[4, 3] = np.nan
    inf[64, 7] = -np.inf
    frames = [p.frame(50), np.zeros((0, 8), np.float32), nan, p.frame(64), inf, p.frame(1)]
    got = p.db.run(frames, top_k=4)
    assert [g["status"] for g in got] == ["OK", "EMPTY", "INVALID_DESCRIPTOR", "OK", "INVALID_DESCRIPTOR", "OK"]
    for g, fr in zip(got, frames):
        check(g, p.ref.query(fr, top_k=4), top_k=4)
        assert same_bytes(g, p.db.run([fr], top_k=4)[0])
    before = p.db.size()
    assert p.insert(nan)["status"] == "INVALID_DESCRIPTOR" and p.insert(frames[1])["status"] == "EMPTY"
    assert p.db.size() == before and same_bytes(got[0], p.db.run([frames[0]], top_k=4)[0])
    p.close()


def test_batch_independence(hip):
    p = Pair(hip, 5, 2, 8, seed=7, recent=0, navg=10, max_frames=64)
    for k in range(70):
        p.insert(p.frame(30 + k % 9))
    fr = p.frame(77)
    frames = [fr] + [p.frame(1 + (11 * k) % 200) for k in range(62)] + [fr]
    got = p.db.run(frames, top_k=3)
    assert same_bytes(got[0], got[63])
    check(got[63], p.ref.query(fr, top_k=3), top_k=3)
    check(got[17], p.ref.query(frames[17], top_k=3), top_k=3)
    p.close()


def test_handle_reuse_and_argument_validation(hip):
    L = hip.lib()
    p = Pair(hip, 5, 2, 8, seed=8, recent=0, navg=10, max_docs=6, max_words=64, max_frames=4)
    for k in range(6):
        p.insert(p.frame(64))
    p.db.run([p.frame(64) for _ in range(4)], top_k=32)        # a call at capacity
    first = p.db.stats()
    assert first == {"calls": 7, "allocations": 1}
    p.db.run([p.frame(3)], top_k=1)
    p.db.run([p.frame(64) for _ in range(4)])
    assert p.db.stats() == {"calls": 9, "allocations": 1}
    # the database is full
    with pytest.raises(hip.SlslamError) as ei:
        p.db.insert(p.frame(4))
    assert ei.value.status == 5
    # more frames or descriptors than declared: an error code, nothing launched, nothing counted
    for frames in ([p.frame(2)] * 5, [p.frame(65)]):
        with pytest.raises(hip.SlslamError) as ei:
            p.db.run(frames)
        assert ei.value.status == 1
    with pytest.raises(hip.SlslamError):
        p.db.run([p.frame(2)], top_k=33)
    assert p.db.stats() == {"calls": 9, "allocations": 1}
    # create: K, L, D, max_words outside the limits
    h = C.c_void_p()
    nodes = np.zeros(65 * 129, dtype=np.float32)
    for K, Lv, D in ((1, 1, 2), (65, 1, 2), (2, 0, 2), (2, 5, 2), (2, 1, 0), (2, 1, 129), (64, 5, 1)):
        assert L.slslam_voctree_create(-1, K, Lv, D, hip._fp(nodes), C.byref(h)) == 1
    assert L.slslam_voctree_create(-1, 64, 1, 128, hip._fp(nodes), C.byref(h)) == 0
    d = C.c_void_p()
    for args in ((0, 64, 4, 0, 10), (8, 0, 4, 0, 10), (8, 513, 4, 0, 10), (8, 64, 0, 0, 10), (8, 64, 4, -1, 10), (8, 64, 4, 0, 0)):
        assert L.slslam_place_db_create(h, *args, C.byref(d)) == 1
    assert L.slslam_place_db_create(None, 8, 64, 4, 0, 10, C.byref(d)) == 1
    assert L.slslam_place_db_create(h, 8, 512, 4, 0, 10, C.byref(d)) == 0
    L.slslam_place_db_destroy(d)
    L.slslam_voctree_destroy(h)
    p.close()


def test_place_sequence_end_to_end(hip):
    """the CPU test's place sequence through capi.place_candidates, keyframe by keyframe: the decisions and the reported keyframes are the
    numpy pipeline's"""
    K, L, D = SEQ["tree"]
    ref_tree, nodes, s = seq_inputs()
    want, _ = R.pipeline(ref_tree, s["frames"], SEQ["recent"], SEQ["navg"], **SEQ["filt"])
    tree = hip.VocTree(K, L, D, nodes)
    db = hip.PlaceDB(tree, max_docs=80, max_words=32, max_frames=1, recent=SEQ["recent"], num_avg_words=SEQ["navg"])
    flt = hip.PlaceFilter(**SEQ["filt"])
    got = []
    for fr in s["frames"]:
        loop, kf, post = hip.place_candidates(db, flt, fr)
        got.append((loop, kf))
    assert got == want and any(loop for loop, _ in got)
    flt.close()
    db.close()
    tree.close()

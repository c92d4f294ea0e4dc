"""The vocabulary-tree trainer without a device (include/slslam_hip.h: slslam_voctree_train and its host half): hand-computed cases that
pin the numpy reference (tests/voctree_train_reference.py), the host half (centres, keys, save) through the C ABI bit for bit against it,
the argument checks, and the property of the trained tree that the GPU end-to-end test relies on."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from slslam_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as R  # noqa: E402
import voctree_train_reference as V  # noqa: E402
from test_place_cpu import SEQ, seq_inputs  # noqa: E402

INVALID = 1
# the SEQ case: the 1800 descriptors of the first pass of test_place_cpu.SEQ's sequence, a (10, 3, 16) tree, seed 7, 10 updates
SEQ_TRAIN = dict(K=10, L=3, max_iterations=10, seed=7)


def seq_first_pass():
    _, _, s = seq_inputs()
    return np.vstack(s["frames"][:s["first_pass"]]), s


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def test_hand_computed_picks_update_and_labels():
    """(K, L, D) = (2, 1, 2), seed 0, descriptors d0 = (1, 3), d1 = (0, 2), d2 = (4, 0), d3 = (2, 1).
    The keys of m = 0 .. 3 at seed 0 are a706dd2f4d197e6f, 5e41ab087439611e, 64684c4f0fd784b4, bccdfd9c96a18897: the two smallest are
    m = 1, then m = 2, so the initial centres are d1 / |d1| = (0, 1) and d2 / |d2| = (1, 0).
    First assignment, r = 1 - <c, f>: d0 (-2, 0) -> 0; d1 (-1, 1) -> 0; d2 (1, -3) -> 1; d3 (0, -1) -> 1: all 4 labels change.
    Update: acc0 = q(d0) + q(d1) = 2^30 (1, 5), centre0 = (1, 5) / sqrt(26); acc1 = 2^30 (6, 1), centre1 = (6, 1) / sqrt(37) - the
    powers of two cancel exactly, so the centres are the floats of 1 / sqrt(26.0) ....
    Second assignment: <c0, f> = 16, 10, 4, 7 over sqrt(26) = 3.14, 1.96, 0.78, 1.37; <c1, f> = 9, 2, 24, 13 over sqrt(37) = 1.48, 0.33,
    3.95, 2.14: the labels stay (0, 0, 1, 1), changed = 0 after one update: the level stops."""
    assert [V.key(0, m) for m in range(4)] == [0xa706dd2f4d197e6f, 0x5e41ab087439611e, 0x64684c4f0fd784b4, 0xbccdfd9c96a18897]
    d = np.array([[1, 3], [0, 2], [4, 0], [2, 1]], dtype=np.float32)
    zero = V.train(d, 2, 1, max_iterations=0, seed=0)
    assert zero["nodes"].tolist() == [[[0.0, 1.0], [1.0, 0.0]]]
    assert zero["words"].tolist() == [0, 0, 1, 1] and (zero["iterations"], zero["changed"]) == ([0], [4])
    rep = V.train(d, 2, 1, max_iterations=10, seed=0)
    want = np.array([[[1 / math.sqrt(26.0), 5 / math.sqrt(26.0)], [6 / math.sqrt(37.0), 1 / math.sqrt(37.0)]]], dtype=np.float32)
    assert rep["nodes"].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert rep["words"].tolist() == [0, 0, 1, 1]
    assert (rep["iterations"], rep["changed"], rep["empty_children"]) == ([1], [0], [0])
    r = [1 - 16 / math.sqrt(26), 1 - 10 / math.sqrt(26), 1 - 24 / math.sqrt(37), 1 - 13 / math.sqrt(37)]
    assert abs(rep["distortion"][0] - sum(r) / 4) < 1e-6


def test_fewer_members_than_children_and_empty_nodes():
    """(3, 2, 2) on one descriptor (0, 2): the root's children are three copies of (0, 1), the descriptor ties and goes to child 0; at
    level 1 node 0 again gets three copies, the memberless nodes 1 and 2 get copies of the centre their parent holds for them."""
    rep = V.train(np.array([[0, 2]], dtype=np.float32), 3, 2, max_iterations=5, seed=3)
    assert rep["nodes"].tolist() == [[[0.0, 1.0]] * 3] * 4
    assert rep["words"].tolist() == [0] and rep["empty_children"] == [2, 8] and rep["iterations"] == [1, 1]


def test_q_rounds_half_to_even():
    h = 2.0 ** -31
    assert V.q(np.array([h, 3 * h, -h, -3 * h, 5 * h, 16.0, -16.0, 0.0], dtype=np.float32)).tolist() == [0, 2, 0, -2, 2, 2 ** 34, -2 ** 34, 0]


def test_host_centres_through_the_abi_bit_for_bit():
    rng = np.random.default_rng(4)
    L = capi.lib()
    for D in (1, 5, 72, 128):
        acc = rng.integers(-2 ** 40, 2 ** 40, size=(64, D), dtype=np.int64)
        acc[3] = 0                                                   # n2 == 0: the row keeps prev
        acc[4] = rng.integers(2 ** 56, 2 ** 57, size=D, dtype=np.int64) | 1            # |acc| above 2^53: (double)acc rounds
        acc[5] = -(rng.integers(2 ** 53, 2 ** 58, size=D, dtype=np.int64) | 1)
        acc[6] = 0
        acc[6, D - 1] = 1
        prev = rng.standard_normal((64, D)).astype(np.float32)
        out = np.full((64, D), 7.0, dtype=np.float32)
        assert L.slslam_voctree_centres(64, D, _lp(acc), capi._fp(prev), capi._fp(out)) == 0
        ref = V.centre(acc, prev)
        assert out.view(np.uint32).tolist() == ref.view(np.uint32).tolist()
        assert out[3].tolist() == prev[3].tolist()
        assert (acc[4].astype(np.float64).astype(np.int64) != acc[4]).any()
    assert L.slslam_voctree_centres(-1, 2, None, None, None) == INVALID
    assert L.slslam_voctree_centres(1, 0, _lp(acc), capi._fp(prev), capi._fp(out)) == INVALID
    assert L.slslam_voctree_centres(1, 2, None, capi._fp(prev), capi._fp(out)) == INVALID


def test_host_keys_through_the_abi():
    L = capi.lib()
    assert V.splitmix64(0) == 0xe220a8397b1dcdaf                      # the first output of the usual splitmix64 seeded with 0
    for seed in (0, 1, 7, 0x0123456789abcdef, 2 ** 64 - 1):
        for m in (0, 1, 2, 1799, 2 ** 24 - 1, 2 ** 63, 2 ** 64 - 1):
            assert L.slslam_voctree_key(seed, m) == V.key(seed, m)


def test_save_and_load_round_trip(tmp_path):
    K, L, D = 3, 2, 5
    nodes = np.random.default_rng(8).standard_normal((4, K, D)).astype(np.float32)
    p = tmp_path / "tree.bin"
    capi.save_voctree(str(p), nodes)
    assert p.read_bytes() == nodes.tobytes()
    t = capi.VocTree(K, L, D, path=str(p))                            # slslam_voctree_load takes exactly this file
    assert t.num_leaves == 9
    t.close()
    with pytest.raises(capi.SlslamError):
        capi.VocTree(K, L, D + 1, path=str(p))
    t = capi.VocTree(K, L, D, nodes=nodes)
    q = tmp_path / "again.bin"
    t.save(str(q))
    t.close()
    assert q.read_bytes() == nodes.tobytes()
    lib = capi.lib()
    assert lib.slslam_voctree_save(None, K, L, D, capi._fp(nodes)) == INVALID
    assert lib.slslam_voctree_save(os.fsencode(str(p)), K, L, D, None) == INVALID
    assert lib.slslam_voctree_save(os.fsencode(str(p)), 1, L, D, capi._fp(nodes)) == INVALID
    assert lib.slslam_voctree_save(os.fsencode(str(tmp_path / "no" / "dir.bin")), K, L, D, capi._fp(nodes)) == INVALID
    assert p.read_bytes() == nodes.tobytes()


def _train_status(d, K, L, D, n, max_iterations=3, nodes=True, desc=True):
    out = np.full(64 * 64 * 4, -7.5, dtype=np.float32)
    words = np.full(max(len(d), 1), -7, dtype=np.int32)
    rep = capi.VocTreeTrainReport()
    rep.levels = -7
    opt = capi.VocTreeTrainOptions(K, L, D, max_iterations, 5)
    rc = capi.lib().slslam_voctree_train(-1, C.byref(opt), n, capi._fp(d) if desc else None, capi._fp(out) if nodes else None,
                                         capi._ip(words), C.byref(rep))
    assert (out == -7.5).all() and (words == -7).all() and rep.levels == -7      # no output is written
    return rc


def test_shape_and_value_errors_write_nothing_and_need_no_device():
    d = np.random.default_rng(2).uniform(-1, 1, (8, 4)).astype(np.float32)
    assert capi.lib().slslam_voctree_train(-1, None, 8, capi._fp(d), capi._fp(d), None, None) == INVALID
    bad = [dict(K=1), dict(K=65), dict(L=0), dict(L=5), dict(D=0), dict(D=129), dict(n=0), dict(n=-1), dict(n=2 ** 24 + 1),
           dict(max_iterations=-1), dict(max_iterations=1001), dict(nodes=False), dict(desc=False),
           dict(K=64, L=4, D=16),                                    # K^L = 2^24 leaves are a tree, but K^L D = 2^28 accumulators are too many
           dict(K=64, L=4, D=9)]
    for kw in bad:
        args = dict(K=2, L=2, D=4, n=8)
        args.update(kw)
        assert _train_status(d, **args) == INVALID, kw
    for v in (np.nan, np.inf, -np.inf, 16.000002, -17.0):
        e = d.copy()
        e[5, 3] = v
        assert _train_status(e, 2, 2, 4, 8) == INVALID, v
    L = capi.lib()
    lab, acc, cnt = np.full(8, -7, np.int32), np.full(2 * 2 * 4, -7, np.int64), np.full(4, -7, np.int64)
    cen = np.zeros((2, 2, 4), np.float32)
    node = np.array([0, 1, 0, 1, 1, 1, 0, 2], np.int32)                # node 2 of 2
    good = np.zeros(8, np.int32)
    step = lambda K, D, nn, c, n, dd, nd: L.slslam_debug_voctree_step(-1, K, D, nn, c, n, dd, nd, capi._ip(lab), _lp(acc), _lp(cnt))
    assert step(2, 4, 2, capi._fp(cen), 8, capi._fp(d), capi._ip(node)) == INVALID
    assert step(1, 4, 2, capi._fp(cen), 8, capi._fp(d), capi._ip(good)) == INVALID
    assert step(2, 4, 0, capi._fp(cen), 8, capi._fp(d), capi._ip(good)) == INVALID
    assert step(2, 4, 2, None, 8, capi._fp(d), capi._ip(good)) == INVALID
    assert step(2, 4, 2, capi._fp(cen), 0, capi._fp(d), capi._ip(good)) == INVALID
    e = d.copy()
    e[0, 0] = np.nan
    assert step(2, 4, 2, capi._fp(cen), 8, capi._fp(e), capi._ip(good)) == INVALID
    assert (lab == -7).all() and (acc == -7).all() and (cnt == -7).all()
    with pytest.raises(ValueError):
        capi.train_voctree(np.zeros(4, np.float32), 2, 1)


@pytest.mark.parametrize("K,L,D,N,its", [(2, 1, 2, 4, 10), (3, 2, 5, 2, 10), (3, 3, 5, 1, 10), (4, 3, 7, 500, 4), (4, 3, 7, 500, 0)])
def test_training_words_are_find_leaf_of_the_finished_tree(K, L, D, N, its):
    d = np.random.default_rng([K, L, N]).uniform(-2, 2, (N, D)).astype(np.float32)
    rep = V.train(d, K, L, max_iterations=its, seed=11)
    assert rep["nodes"].shape == ((K ** L - 1) // (K - 1), K, D)
    assert R.Tree(K, L, D, rep["nodes"]).words(d).tolist() == rep["words"].tolist()
    assert all(i <= its for i in rep["iterations"]) and len(rep["iterations"]) == L


def test_seq_trained_tree_closes_the_loop_on_the_reference():
    """The tree trained on the first pass of SEQ's sequence closes the loop with SEQ's database and filter settings; the random tree of
    synth.make_voctree reaches 568 of the 1000 leaves with these descriptors, the trained one 997."""
    first, s = seq_first_pass()
    assert first.shape == (1800, 16)
    rep = V.train(first, **SEQ_TRAIN)
    assert rep["iterations"] == [10, 10, 3]
    tree = R.Tree(10, 3, 16, rep["nodes"])
    assert tree.words(first).tolist() == rep["words"].tolist()
    assert len(np.unique(rep["words"])) == 997
    out, flt = R.pipeline(tree, s["frames"], SEQ["recent"], SEQ["navg"], **SEQ["filt"])
    assert not any(loop for loop, _ in out[:s["first_pass"]])
    hits = [(i, kf) for i, (loop, kf) in enumerate(out) if loop]
    assert len(hits) == 13 and all(abs(kf - int(s["place"][i])) <= 1 for i, kf in hits)
    assert flt.margin > 1e-4

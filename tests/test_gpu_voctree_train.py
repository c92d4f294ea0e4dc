"""The vocabulary-tree trainer on the device (include/slslam_hip.h: slslam_voctree_train, slslam_debug_voctree_step) against the numpy
reference (tests/voctree_train_reference.py).  Labels, accumulators, counts, nodes, words and the report's counts are exact: r is
evaluated in the contract's order without contraction, and every sum that decides something is an int64 sum.  The distortion, a double
sum of N floats in another order, is within 2 N 2^-53 sum|r| / N of the reference."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_reference as R  # noqa: E402
import voctree_train_reference as V  # noqa: E402
from test_place_cpu import SEQ  # noqa: E402
from test_voctree_train_cpu import SEQ_TRAIN, seq_first_pass  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def step(hip, centres, desc, node):
    """slslam_debug_voctree_step with outputs that start as garbage"""
    num_nodes, K, D = centres.shape
    n = len(desc)
    label, acc, cnt = np.full(n, -7, np.int32), np.full((num_nodes * K, D), -7, np.int64), np.full(num_nodes * K, -7, np.int64)
    node = np.ascontiguousarray(node, dtype=np.int32)
    rc = hip.lib().slslam_debug_voctree_step(-1, K, D, num_nodes, hip._fp(centres), n, hip._fp(desc), hip._ip(node), hip._ip(label),
                                             _lp(acc), _lp(cnt))
    assert rc == 0
    return label, acc, cnt


def step_reference(centres, desc, node):
    num_nodes, K, D = centres.shape
    label, _ = V.assign(centres, np.asarray(node, dtype=np.int64), desc)
    row = np.asarray(node, dtype=np.int64) * K + label
    acc = np.zeros((num_nodes * K, D), dtype=np.int64)
    np.add.at(acc, row, V.q(desc))
    return label, acc, np.bincount(row, minlength=num_nodes * K)


def check_step(hip, centres, desc, node):
    got, ref = step(hip, centres, desc, node), step_reference(centres, desc, node)
    assert got[0].tolist() == ref[0].tolist()
    assert np.array_equal(got[1], ref[1])
    assert got[2].tolist() == ref[2].tolist() and int(got[2].sum()) == len(desc)
    return got


@pytest.mark.parametrize("num_nodes", [1, 3, 100])
@pytest.mark.parametrize("K,D", [(2, 2), (3, 5), (40, 72), (64, 128)])
def test_step_labels_sums_and_counts_are_exact(hip, K, D, num_nodes):
    rng = np.random.default_rng([K, D, num_nodes])
    centres = rng.standard_normal((num_nodes, K, D))
    centres = (centres / np.linalg.norm(centres, axis=2, keepdims=True)).astype(np.float32)
    for n in (1, 63, 64, 65, 1000):
        desc = rng.uniform(-1.5, 1.5, (n, D)).astype(np.float32)
        check_step(hip, centres, desc, np.arange(n) % num_nodes)       # interleaved: neighbours are in different nodes


def test_step_more_than_one_block_and_a_node_change_inside_a_block(hip):
    """5000 descriptors are five blocks of four rounds; sorted by node, 7 nodes of unequal size change inside rounds and blocks"""
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((7, 5, 9)).astype(np.float32)
    desc = rng.uniform(-2, 2, (5000, 9)).astype(np.float32)
    check_step(hip, centres, desc, rng.choice(7, size=5000, p=[0.4, 0.3, 0.1, 0.1, 0.05, 0.05, 0.0]))


def test_step_ties_go_to_the_lowest_child(hip):
    rng = np.random.default_rng(32)
    centres = rng.standard_normal((3, 8, 6)).astype(np.float32)
    centres[:, 1::2] = centres[:, 0::2]                                # children in identical pairs: the odd one never wins
    desc = rng.standard_normal((500, 6)).astype(np.float32)
    label, _, _ = check_step(hip, centres, desc, np.arange(500) % 3)
    assert (label % 2 == 0).all()
    same = np.repeat(centres[:, :1], 8, axis=1).copy()                 # all children equal: everything goes to child 0
    label, _, _ = check_step(hip, same, desc, np.arange(500) % 3)
    assert (label == 0).all()


def test_step_one_accumulator_takes_every_add(hip):
    rng = np.random.default_rng(33)
    centres = rng.standard_normal((1, 4, 7)).astype(np.float32)
    f = rng.uniform(-3, 3, 7).astype(np.float32)
    desc = np.repeat(f[None], 1000, axis=0).copy()
    label, acc, cnt = check_step(hip, centres, desc, np.zeros(1000, np.int32))
    assert acc[label[0]].tolist() == (1000 * V.q(f)).tolist() and cnt[label[0]] == 1000


def test_step_largest_values(hip):
    rng = np.random.default_rng(34)
    centres = rng.standard_normal((2, 3, 5)).astype(np.float32)
    desc = (16.0 * rng.choice([-1.0, 1.0], size=(4096, 5))).astype(np.float32)
    _, acc, _ = check_step(hip, centres, desc, np.arange(4096) % 2)
    assert (np.abs(acc) % 2 ** 34 == 0).all() and np.abs(acc).max() > 2 ** 34


def descriptors(K, L, D, N):
    if (K, L, D, N) == (10, 3, 16, 1800):
        return seq_first_pass()[0]
    d = np.random.default_rng([K, L, D, N]).standard_normal((N, D))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(K, L, D, N, its, seed):
    return V.train(descriptors(K, L, D, N), K, L, max_iterations=its, seed=seed)


CASES = [(2, 1, 2, 4, 10), (3, 2, 5, 2, 10), (3, 3, 5, 1, 10), (10, 3, 16, 1800, 10), (40, 2, 72, 3000, 10), (10, 3, 16, 1800, 0),
         (3, 2, 5, 2, 0), (10, 3, 16, 1800, 1)]


@pytest.mark.parametrize("K,L,D,N,its", CASES)
def test_trainer_is_the_reference_bit_for_bit(hip, K, L, D, N, its):
    seed = SEQ_TRAIN["seed"]
    d = descriptors(K, L, D, N)
    ref = reference(K, L, D, N, its, seed)
    got = hip.train_voctree(d, K, L, max_iterations=its, seed=seed)
    assert got["nodes"].shape == ref["nodes"].shape and bits(got["nodes"]) == bits(ref["nodes"])
    assert got["words"].tolist() == ref["words"].tolist()
    for k in ("iterations", "changed", "empty_children"):
        assert got[k] == ref[k], k
    for l in range(L):
        print(K, L, D, N, its, "level", l, "distortion", got["distortion"][l], ref["distortion"][l])
        bound = 2.0 * N * 2.0 ** -53 * ref["sum_abs_r"][l] / N
        assert abs(got["distortion"][l] - ref["distortion"][l]) <= bound
    again = hip.train_voctree(d, K, L, max_iterations=its, seed=seed)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got)


def test_seed_decides_the_picks(hip):
    d = descriptors(10, 3, 16, 1800)
    a, b = hip.train_voctree(d, 10, 1, max_iterations=0, seed=7), hip.train_voctree(d, 10, 1, max_iterations=0, seed=8)
    assert bits(a["nodes"]) == bits(V.train(d, 10, 1, 0, 7)["nodes"]) and bits(a["nodes"]) != bits(b["nodes"])
    big = hip.train_voctree(d, 10, 1, max_iterations=0, seed=2 ** 64 - 1)
    assert bits(big["nodes"]) == bits(V.train(d, 10, 1, 0, 2 ** 64 - 1)["nodes"])


def test_value_errors_leave_the_outputs_untouched(hip):
    d = descriptors(3, 2, 5, 200)
    for v in (np.nan, np.inf, 16.5, -16.5):
        e = d.copy()
        e[137, 4] = v
        nodes, words = np.full((4, 3, 5), -7.5, dtype=np.float32), np.full(200, -7, dtype=np.int32)
        rep = hip.VocTreeTrainReport()
        rep.levels = -7
        opt = hip.VocTreeTrainOptions(3, 2, 5, 4, 1)
        assert hip.lib().slslam_voctree_train(-1, C.byref(opt), 200, hip._fp(e), hip._fp(nodes), hip._ip(words), C.byref(rep)) == INVALID
        assert (nodes == -7.5).all() and (words == -7).all() and rep.levels == -7
    e = d.copy()
    e[0, 0], e[1, 1] = 16.0, -16.0                                     # the limits themselves are values like any other
    got, ref = hip.train_voctree(e, 3, 2, max_iterations=4, seed=1), V.train(e, 3, 2, 4, 1)
    assert bits(got["nodes"]) == bits(ref["nodes"]) and got["words"].tolist() == ref["words"].tolist()


def test_trained_tree_closes_the_loop_end_to_end(hip, tmp_path):
    """VocTree.train on the first pass of SEQ's sequence, then PlaceDB and PlaceFilter over the whole sequence: the (loop, keyframe)
    list of the reference pipeline on the reference-trained tree; the saved tree, loaded again, quantises alike."""
    first, s = seq_first_pass()
    ref = reference(10, 3, 16, 1800, SEQ_TRAIN["max_iterations"], SEQ_TRAIN["seed"])
    want, _ = R.pipeline(R.Tree(10, 3, 16, ref["nodes"]), s["frames"], SEQ["recent"], SEQ["navg"], **SEQ["filt"])
    assert any(loop for loop, _ in want)
    tree, rep = hip.VocTree.train(first, **SEQ_TRAIN)
    assert rep["words"].tolist() == ref["words"].tolist()
    db = hip.PlaceDB(tree, max_docs=160, max_words=64, max_frames=1, recent=SEQ["recent"], num_avg_words=SEQ["navg"])
    filt = hip.PlaceFilter(**SEQ["filt"])
    got = [hip.place_candidates(db, filt, fr)[:2] for fr in s["frames"]]
    assert got == [(bool(loop), int(kf)) for loop, kf in want]
    tree.save(str(tmp_path / "trained.bin"))
    loaded = hip.VocTree(10, 3, 16, path=str(tmp_path / "trained.bin"))
    db2 = hip.PlaceDB(loaded, max_docs=4, max_words=64, max_frames=1, recent=0, num_avg_words=5)
    assert db2.insert(s["frames"][0])["words"].tolist() == rep["words"][:len(s["frames"][0])].tolist()
    for h in (db2, loaded, filt, db, tree):
        h.close()

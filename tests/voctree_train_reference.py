"""numpy reference of the vocabulary-tree trainer (include/slslam_hip.h: slslam_voctree_train), written from the contract in that header:
hierarchical spherical k-means whose sums are int64 sums of fixed-point values, so that they do not depend on the order.  int64 sums,
explicit loops over i where the order of a float or double sum is part of the contract, python integers for the keys.  Checker only."""
import numpy as np

MASK = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def key(seed, m):
    return splitmix64(((int(seed) & MASK) ^ splitmix64(int(m))) & MASK)


def q(f):
    """llrint((double)f * 2^30): the product is exact, np.rint rounds to the nearest even"""
    return np.rint(np.asarray(f, dtype=np.float32).astype(np.float64) * 2.0 ** 30).astype(np.int64)


def centre(acc, prev):
    """acc [rows, D] int64, prev [rows, D] float32 -> [rows, D] float32"""
    acc = np.asarray(acc, dtype=np.int64)
    s = acc.astype(np.float64)
    n2 = np.zeros(len(s), dtype=np.float64)
    for i in range(s.shape[1]):                                     # i ascending, product and sum rounded separately
        n2 = n2 + s[:, i] * s[:, i]
    out = np.array(prev, dtype=np.float32, copy=True)
    nz = n2 != 0.0
    out[nz] = (s[nz] / np.sqrt(n2[nz])[:, None]).astype(np.float32)
    return out


def assign(centres, node, desc, chunk=16384):
    """centres [nodes, K, D], node [N]: the nearest child of every descriptor's node and its r (float32)"""
    K, D = centres.shape[1], centres.shape[2]
    label, best_r = np.zeros(len(desc), dtype=np.int64), np.zeros(len(desc), dtype=np.float32)
    for a in range(0, len(desc), chunk):
        f = desc[a:a + chunk]
        c = centres[node[a:a + chunk]]                              # [n, K, D]
        r = np.ones((len(f), K), dtype=np.float32)
        for i in range(D):
            r = r - c[:, :, i] * f[:, i, None]
        best, arg = r[:, 0].copy(), np.zeros(len(f), dtype=np.int64)
        for k in range(1, K):
            m = r[:, k] < best
            best[m] = r[m, k]
            arg[m] = k
        label[a:a + chunk], best_r[a:a + chunk] = arg, best
    return label, best_r


def initial_centres(K, D, num_nodes, node, desc, keys, parent):
    """parent: the centres of the level above as rows [num_nodes, D] (None at the root)"""
    out = np.zeros((num_nodes, K, D), dtype=np.float32)
    order = np.lexsort((np.arange(len(desc)), keys, node))          # by (node, key, m)
    start = np.searchsorted(node[order], np.arange(num_nodes + 1))
    for j in range(num_nodes):
        pick = order[start[j]:start[j + 1]][:K]
        if len(pick) == 0:
            out[j, :] = parent[j]
            continue
        out[j, :len(pick)] = centre(q(desc[pick]), np.zeros((len(pick), D), dtype=np.float32))
        out[j, len(pick):] = out[j, 0]
    return out


def train(desc, K, L, max_iterations=10, seed=0):
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    N, D = desc.shape
    assert N >= 1 and np.isfinite(desc).all() and (np.abs(desc) <= 16).all()
    keys = np.array([key(seed, m) for m in range(N)], dtype=np.uint64)
    qd = q(desc)
    node = np.zeros(N, dtype=np.int64)
    levels, parent = [], None
    rep = {"iterations": [], "changed": [], "empty_children": [], "distortion": [], "sum_abs_r": []}
    with np.errstate(all="ignore"):
        for l in range(L):
            num_nodes = K ** l
            c = initial_centres(K, D, num_nodes, node, desc, keys, parent)
            its, prev = 0, None
            while True:
                label, r = assign(c, node, desc)
                changed = N if prev is None else int((label != prev).sum())
                prev = label
                if its == max_iterations or (its >= 1 and changed == 0):
                    break
                acc = np.zeros((num_nodes * K, D), dtype=np.int64)
                np.add.at(acc, node * K + label, qd)
                c = centre(acc, c.reshape(num_nodes * K, D)).reshape(num_nodes, K, D)
                its += 1
            node = node * K + label
            rep["iterations"].append(its)
            rep["changed"].append(changed)
            rep["empty_children"].append(int(num_nodes * K - len(np.unique(node))))
            rep["distortion"].append(float(r.astype(np.float64).sum() / N))
            rep["sum_abs_r"].append(float(np.abs(r.astype(np.float64)).sum()))
            levels.append(c)
            parent = c.reshape(num_nodes * K, D)
    rep["nodes"] = np.concatenate([c.reshape(-1, K, D) for c in levels])
    rep["words"] = node.astype(np.int32)
    return rep

"""The descriptor matcher's contract (include/slslam_hip.h: slslam_descriptor_matcher_*) in numpy: what tests/test_gpu_descriptor_match.py
compares the device with, and what tests/test_descriptor_match_cpu.py pins by hand.  Every product and every difference of the distance
is a float32 operation of its own, in the contract's order; every decision is made as the contract words it."""
import numpy as np

OK, EMPTY, INVALID = "OK", "EMPTY", "INVALID_DESCRIPTOR"


def distances(q, k):
    """r [n, m] float32: r = 1; for i in 0 .. D-1: r -= q[i] * k[i], rounded to float32 after the product and after the difference."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    k = np.ascontiguousarray(k, dtype=np.float32)
    r = np.ones((len(q), len(k)), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(q.shape[1]):
            p = q[:, i:i + 1] * k[None, :, i]                    # float32 * float32 -> float32
            r = r - p
    assert r.dtype == np.float32
    return r


def _none(n, m, status):
    inf = np.full(n, np.inf, dtype=np.float32)
    return {"status": status, "num_matched": 0, "match": np.full(n, -1, np.int32), "best": np.full(n, -1, np.int32),
            "best_distance": inf, "second_distance": inf.copy(), "num_admissible": np.zeros(n, np.int32),
            "best_query": np.full(m, -1, np.int32)}


def match(q, k, ratio=1.5, max_distance=np.inf):
    """One pair: query descriptors q [n, D] against keyframe descriptors k [m, D]; k = None stands for candidate -1."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    n = len(q)
    if not np.isfinite(q).all():
        return _none(n, 0 if k is None else len(k), INVALID)
    if n == 0 or k is None:
        return _none(n, 0 if k is None else len(k), EMPTY)
    k = np.ascontiguousarray(k, dtype=np.float32)
    m = len(k)
    r = distances(q, k)
    adm = np.isfinite(r) & (r.astype(np.float64) < float(max_distance))
    out = _none(n, m, OK)
    masked = np.where(adm, r, np.float32(np.inf)).astype(np.float32)
    for a in range(n):
        js = np.nonzero(adm[a])[0]
        out["num_admissible"][a] = len(js)
        if len(js) == 0:
            continue
        b = js[np.argmin(r[a, js])]                              # (argmin: the first minimum, js ascending - the lowest j)
        out["best"][a] = b
        out["best_distance"][a] = r[a, b]
        rest = js[js != b]
        if len(rest):
            out["second_distance"][a] = r[a, rest].min()
    for j in range(m):
        as_ = np.nonzero(adm[:, j])[0]
        if len(as_):
            out["best_query"][j] = as_[np.argmin(masked[as_, j])]
    for a in range(n):
        b = out["best"][a]
        if b < 0 or out["best_query"][b] != a:
            continue
        if ratio <= 1.0 or float(out["best_distance"][a]) * float(ratio) <= float(out["second_distance"][a]):
            out["match"][a] = b
    out["num_matched"] = int((out["match"] >= 0).sum())
    return out


class Store:
    """the keyframes in the order of accepted inserts"""

    def __init__(self):
        self.keyframes = []

    def insert(self, d):
        d = np.ascontiguousarray(d, dtype=np.float32)
        if len(d) == 0:
            return EMPTY, -1
        if not np.isfinite(d).all():
            return INVALID, -1
        self.keyframes.append(d.copy())
        return OK, len(self.keyframes) - 1

    def run(self, queries, ratio=1.5, max_distance=np.inf):
        return [[dict(match(fr, self.keyframes[c] if c >= 0 else None, ratio, max_distance), candidate=int(c)) for c in cs]
                for fr, cs in queries]


def loop_matches(store, frame, candidates, ratio=1.5, max_distance=np.inf):
    best = None
    for r in store.run([(frame, candidates)], ratio, max_distance)[0]:
        if r["status"] == OK and (best is None or (r["num_matched"], -r["candidate"]) > (best["num_matched"], -best["candidate"])):
            best = r
    return (best["candidate"], best) if best is not None else (-1, None)

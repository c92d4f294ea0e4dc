"""numpy reference of the place recogniser (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*, slslam_place_filter_*), written
from the contract in that header: math.log10 for the idf, np.float32 scalars and explicit loops wherever the order of a sum or the
precision of an operation is part of the contract.  Checker only."""
import math

import numpy as np

F32 = np.float32
OK, EMPTY, INVALID = "OK", "EMPTY", "INVALID_DESCRIPTOR"


class Tree:
    def __init__(self, K, L, D, nodes):
        self.K, self.L, self.D = K, L, D
        self.num_int = (K ** L - 1) // (K - 1)
        self.num_leaves = K ** L
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float32).reshape(self.num_int, K, D)

    def words(self, desc):
        """find_leaf of every descriptor [n, D]: per level r = 1.0f, r -= c[i] * f[i] for i ascending (product and difference rounded
        separately), the first minimum under a strict < wins."""
        f = np.ascontiguousarray(desc, dtype=np.float32).reshape(-1, self.D)
        idx = np.zeros(len(f), dtype=np.int64)
        with np.errstate(all="ignore"):
            for _ in range(self.L):
                c = self.nodes[idx]                                     # [n, K, D]
                r = np.ones((len(f), self.K), dtype=np.float32)
                for i in range(self.D):
                    r = r - c[:, :, i] * f[:, i, None]
                best, arg = r[:, 0].copy(), np.zeros(len(f), dtype=np.int64)
                for k in range(1, self.K):
                    m = r[:, k] < best
                    best[m] = r[m, k]
                    arg[m] = k
                idx = idx * self.K + arg + 1
        return (idx - self.num_int).astype(np.int32)


def document(words):
    """distinct words ascending, tf = (float)count / (float)n"""
    w, cnt = np.unique(np.asarray(words, dtype=np.int32), return_counts=True)
    return w.astype(np.int32), (cnt.astype(np.float32) / F32(len(words))).astype(np.float32)


class Database:
    def __init__(self, tree, recent, num_avg_words):
        self.tree, self.recent, self.navg = tree, recent, num_avg_words
        self.docs = []                     # every inserted document (words, tf)
        self.visible = 0
        self.df = np.zeros(tree.num_leaves, dtype=np.int64)       # over the visible documents
        self.virtual = np.zeros(0, dtype=np.int32)

    def _status(self, desc):
        d = np.asarray(desc, dtype=np.float32).reshape(-1, self.tree.D)
        if not np.isfinite(d).all():
            return INVALID
        return EMPTY if len(d) == 0 else OK

    def insert(self, desc):
        st = self._status(desc)
        if st != OK:
            return st
        self.docs.append(document(self.tree.words(desc)))
        # the front is released while more than `recent` documents are pending behind it
        while len(self.docs) - self.visible - 1 > self.recent:
            self.df[self.docs[self.visible][0]] += 1
            self.visible += 1
            self._rebuild_virtual()
        return st

    def _rebuild_virtual(self):
        nonempty = np.nonzero(self.df > 0)[0]
        self.virtual = np.zeros(0, dtype=np.int32)
        if len(nonempty) > self.navg:
            order = sorted(nonempty.tolist(), key=lambda w: (-self.df[w], w))          # largest df, the lower word on ties
            self.virtual = np.array(sorted(order[:self.navg]), dtype=np.int32)

    @property
    def doc_size(self):
        return self.visible + (1 if len(self.virtual) else 0)

    def states(self):
        """the scored states in ascending order: (index into the per-state arrays, words, tf)"""
        out = []
        if len(self.virtual):
            out.append((0, self.virtual, np.full(len(self.virtual), F32(1.0) / F32(self.navg), dtype=np.float32)))
        out += [(d + 1,) + self.docs[d] for d in range(self.visible)]
        return out

    def idf(self, word):
        df = int(self.df[word]) + (1 if word in self._vset else 0)
        return F32(math.log10(float(self.doc_size) / float(df)))

    def query(self, desc, top_k=0):
        st = self._status(desc)
        S = self.visible + 1
        res = {"status": st, "has_virtual": len(self.virtual) > 0, "score": np.zeros(S, dtype=np.float32),
               "touched": np.zeros(S, dtype=np.uint8), "likelihood": np.ones(S, dtype=np.float32),
               "top_id": np.full(top_k, -1, dtype=np.int32), "top_score": np.zeros(top_k, dtype=np.float32), "margin": np.inf}
        n = len(np.asarray(desc).reshape(-1, self.tree.D))
        res["words"] = np.full(n, -1, dtype=np.int32) if st == INVALID else self.tree.words(desc)
        if st == OK and self.visible == 0:
            res["status"] = EMPTY
        if res["status"] != OK:
            return res
        self._vset = set(self.virtual.tolist())
        qw, qtf = document(res["words"])
        qpos = {int(w): i for i, w in enumerate(qw)}
        states = self.states()
        total, ntouched = 0.0, 0
        for si, dw, dtf in states:
            s, ds, hit = F32(0.0), 0.0, False
            for j, w in enumerate(dw.tolist()):                                        # ascending word order
                if w not in qpos:
                    continue
                idf = self.idf(w)
                nn = F32(qtf[qpos[w]] * idf)
                mm = F32(dtf[j] * idf)
                l = F32(-F32(F32(F32(abs(F32(nn - mm))) - nn) - mm))
                s = F32(s + l)
                ds += float(l)
                hit = True
            res["score"][si], res["touched"][si] = s, hit
            if hit:
                total += ds                                                            # states ascending
                ntouched += 1
        fill = F32(total / float(1 + ntouched))
        idxs = [si for si, _, _ in states]
        for si in idxs:
            if not res["touched"][si]:
                res["score"][si] = fill
        sc = res["score"][idxs].astype(np.float64)
        mean = float(sc.sum() / len(sc))
        var = float((sc * sc).sum() / len(sc)) - mean * mean
        sigma = math.sqrt(var) if var >= 0.0 else math.nan                 # (sqrt of a negative: NaN, and no s is above a NaN bar)
        if mean != 0.0:
            bar = mean + 2.0 * sigma
            for si, s in zip(idxs, sc):
                if s > bar:
                    res["likelihood"][si] = F32((s - 2.0 * sigma) / mean)
            res["margin"] = float(np.abs(sc - bar).min() / max(1.0, abs(mean)))
        res["mean"], res["sigma"] = mean, sigma
        docs = sorted(range(self.visible), key=lambda d: (-float(res["score"][d + 1]), d))[:top_k]
        res["top_id"][:len(docs)] = docs
        res["top_score"][:len(docs)] = res["score"][[d + 1 for d in docs]]
        return res


class Filter:
    """calc_post_prob and the loop decision, as host/place_filter.h states them"""

    def __init__(self, sigma=1.0, threshold=0.7, seq_len=10, min_docs=40):
        self.gauss = [F32(1.0 / math.sqrt(2.0 * math.pi * sigma * sigma) * math.exp(-1.0 * (float(d * d) / (2.0 * sigma * sigma))))
                      for d in range(10)]
        self.threshold, self.seq_len, self.min_docs = F32(threshold), seq_len, min_docs
        self.post = np.ones(1, dtype=np.float32)
        self.margin = np.inf               # the smallest |window sum - threshold| met so far

    def trans(self, s, j, N):
        if j == -1:
            return F32(0.9) if s == -1 else F32(0.1) / F32(N)
        if s == -1:
            return F32(0.1)
        return self.gauss[abs(s - j)] if abs(s - j) < 10 else F32(0.0)

    def update(self, likelihood):
        lik = np.asarray(likelihood, dtype=np.float32)
        N = len(lik) - 1
        prev = self.post
        post = np.zeros(N + 1, dtype=np.float32)
        eta = 0.0
        for s in range(-1, N):
            belief = F32(0.0)
            for j in range(-1, N):                                  # ascending; a prev[j] the last step did not have counts as 0
                p = prev[j + 1] if j + 1 < len(prev) else F32(0.0)
                belief = F32(belief + F32(self.trans(s, j, N) * p))
            post[s + 1] = F32(lik[s + 1] * belief)
            eta += float(post[s + 1])
        for i in range(N + 1):
            post[i] = F32(float(post[i]) / eta) if eta != 0.0 else F32(1.0) / F32(N + 1)
        self.post = post
        if N < self.min_docs:
            return False, -1, post
        for a in range(0, N - self.seq_len):
            sm, best, arg = F32(0.0), post[a + 1], a
            for d in range(a, a + self.seq_len + 1):
                sm = F32(sm + post[d + 1])
                if post[d + 1] > best:
                    best, arg = post[d + 1], d
            self.margin = min(self.margin, abs(float(sm) - float(self.threshold)))
            if sm >= self.threshold:
                return True, arg, post
        return False, -1, post


def pipeline(tree, frames, recent, num_avg_words, **filter_kw):
    """Every keyframe: insert, query, filter step.  Returns the (loop, keyframe) of every keyframe and the filter (for its margin)."""
    db, flt = Database(tree, recent, num_avg_words), Filter(**filter_kw)
    out = []
    for fr in frames:
        if db.insert(fr) != OK:
            out.append((False, -1))
            continue
        loop, kf, _ = flt.update(db.query(fr)["likelihood"])
        out.append((loop, kf))
    return out, flt

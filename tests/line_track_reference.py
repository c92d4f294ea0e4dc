"""The line tracker's contract (include/slslam_hip.h: slslam_line_tracker_*, slslam_track_lines) in numpy: what
tests/test_gpu_line_track.py compares the device with, and what tests/test_line_track_cpu.py pins by hand.  The temporal gate is fp64
from the float end points, every operation rounded on its own, in the header's order, without a division; the descriptor distance is
the float chain of descriptor_match_reference.distances; every decision is made as the contract words it.  The tracker is a plain
loop over frames: one frame at a time, which by the contract gives what any cut into runs gives."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as DM  # noqa: E402

OK, EMPTY = "OK", "EMPTY"
CONTINUED, NEW, SHORT, INVALID = "CONTINUED", "NEW", "SHORT", "INVALID"
SEGMENT_STATUS = [CONTINUED, NEW, SHORT, INVALID]
INT_MAX = 2 ** 31 - 1

DEFAULTS = dict(max_tan2=0.03, max_shift=40.0, max_offset=12.0, min_overlap=0.5, min_length=8.0, ratio=1.5, max_distance=0.25)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def options(**over):
    unknown = set(over) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown track option %s" % sorted(unknown))
    return dict(DEFAULTS, **{k: float(v) for k, v in over.items()})


def options_valid(o):
    f = np.isfinite
    return bool(f(o["max_tan2"]) and o["max_tan2"] >= 0 and f(o["max_shift"]) and o["max_shift"] >= 0 and f(o["max_offset"])
                and o["max_offset"] >= 0 and f(o["min_overlap"]) and 0 <= o["min_overlap"] <= 1 and f(o["min_length"])
                and o["min_length"] >= 0 and not np.isnan(o["ratio"]) and not np.isnan(o["max_distance"]))


def squares(o):
    """The thresholds as the gate takes them: the squares are taken once, in double."""
    return dict(max_tan2=np.float64(o["max_tan2"]), max_shift2=np.float64(o["max_shift"]) * np.float64(o["max_shift"]),
                max_offset2=np.float64(o["max_offset"]) * np.float64(o["max_offset"]), min_overlap=np.float64(o["min_overlap"]),
                min_length2=np.float64(o["min_length"]) * np.float64(o["min_length"]))


def warp(seg, predict=None):
    """[n, 4] float64: the end points of float segments under predict (None: the identity), x' = (a11 x + a12 y) + tx."""
    s = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    a11, a12, tx, a21, a22, ty = (np.float64(v) for v in (IDENTITY if predict is None else predict))
    with np.errstate(all="ignore"):
        cols = []
        for x, y in ((s[:, 0], s[:, 1]), (s[:, 2], s[:, 3])):
            cols += [(a11 * x + a12 * y) + tx, (a21 * x + a22 * y) + ty]
    return np.stack(cols, axis=1) if len(s) else np.zeros((0, 4))


def segments(ends):
    """What the contract derives per segment from its end points [n, 4] float64: dict of [n] arrays."""
    e = np.asarray(ends, dtype=np.float64).reshape(-1, 4)
    x0, y0, x1, y1 = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    with np.errstate(all="ignore"):
        dx, dy = x1 - x0, y1 - y0
        len2 = dx * dx + dy * dy
        mx, my = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, dx=dx, dy=dy, len2=len2, mx=mx, my=my)


def segment_ok(seg, desc):
    """[n] bool: every end point and every descriptor value is finite."""
    seg = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4)
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    desc = desc.reshape(len(seg), -1) if len(seg) else np.zeros((0, 0), np.float32)
    return np.isfinite(seg).all(axis=1) & np.isfinite(desc).all(axis=1)


def is_short(seg, o):
    """[n] bool: len2 < min_length^2, of the segment as it lies in its own frame."""
    with np.errstate(all="ignore"):
        return segments(warp(seg))["len2"] < squares(o)["min_length2"]


def gate(rows, cols, o, predict=None, margins=False):
    """The geometric part of admissibility of float row segments against float column segments under predict, [n, m] bool;
    margins=True returns instead the list of (value, threshold, reached) of every comparison, for the tests' "no decision near its
    threshold" check."""
    A = {k: v[:, None] for k, v in segments(warp(rows)).items()}
    B = {k: v[None, :] for k, v in segments(warp(cols, predict)).items()}
    g = squares(o)
    with np.errstate(all="ignore"):
        dot = A["dx"] * B["dx"] + A["dy"] * B["dy"]
        cross = A["dx"] * B["dy"] - A["dy"] * B["dx"]
        c2, d2 = cross * cross, dot * dot
        lim = g["max_tan2"] * d2
        direction = (c2 <= lim) & (dot != 0)
        ex, ey = A["mx"] - B["mx"], A["my"] - B["my"]
        s2 = ex * ex + ey * ey
        shift = s2 <= g["max_shift2"]
        eab = (A["mx"] - B["x0"]) * B["dy"] - (A["my"] - B["y0"]) * B["dx"]
        eba = (B["mx"] - A["x0"]) * A["dy"] - (B["my"] - A["y0"]) * A["dx"]
        eab2, eba2 = eab * eab, eba * eba
        lab, lba = g["max_offset2"] * B["len2"], g["max_offset2"] * A["len2"]
        offset = (eab2 <= lab) & (eba2 <= lba)
        s0 = (B["x0"] - A["x0"]) * A["dx"] + (B["y0"] - A["y0"]) * A["dy"]
        s1 = (B["x1"] - A["x0"]) * A["dx"] + (B["y1"] - A["y0"]) * A["dy"]
        lo, hi = np.where(s1 < s0, s1, s0), np.where(s1 < s0, s0, s1)
        la = np.broadcast_to(A["len2"], hi.shape)
        top, bot = np.where(hi < la, hi, la), np.where(lo > 0, lo, 0.0)
        ov, span = top - bot, hi - lo
        need = g["min_overlap"] * np.where(span < la, span, la)
        overlap = (ov >= need) & (ov > 0)
    if margins:
        return [(c2, lim, np.ones(c2.shape, bool)), (s2, g["max_shift2"], direction), (eab2, lab, direction & shift),
                (eba2, lba, direction & shift), (ov, need, direction & shift & offset), (ov, 0.0, direction & shift & offset)]
    return direction & shift & offset & overlap


def _empty_frame(D=0):
    return dict(seg=np.zeros((0, 4), np.float32), desc=np.zeros((0, D), np.float32), ok=np.zeros(0, bool), id=np.zeros(0, np.int32),
                age=np.zeros(0, np.int32))


class Tracker:
    """The handle's state (the carried frame, next_id) and the run."""

    def __init__(self, next_id=0):
        self.reset(next_id)

    def reset(self, next_id=0):
        self.next_id, self.prev = int(next_id), _empty_frame()

    def state(self):
        return {"next_id": self.next_id, "carried_segments": len(self.prev["seg"])}

    def run(self, frames, **over):
        """frames: (segments, descriptors[, predict]) each.  None (and nothing changed) for a run the library refuses."""
        o = options(**over)
        assert options_valid(o)
        if self.next_id + sum(len(np.asarray(f[0]).reshape(-1, 4)) for f in frames) > INT_MAX:
            return None
        return [self._frame(f[0], f[1], f[2] if len(f) > 2 else None, o) for f in frames]

    def _frame(self, seg, desc, predict, o):
        seg = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4)
        n = len(seg)
        desc = np.ascontiguousarray(desc, dtype=np.float32)
        desc = desc.reshape(n, -1) if n else np.zeros((0, 0), np.float32)
        prev = self.prev
        m = len(prev["seg"])
        out = DM._none(n, m, EMPTY if n == 0 or m == 0 else OK)
        out["best_row"] = out.pop("best_query")
        ok, short = segment_ok(seg, desc), is_short(seg, o)
        if n and m:
            geo = gate(seg, prev["seg"], o, predict)
            r = DM.distances(desc, prev["desc"])
            adm = (geo & (ok & ~short)[:, None] & (prev["ok"] & ~is_short(prev["seg"], o))[None, :] & np.isfinite(r)
                   & (r.astype(np.float64) < o["max_distance"]))
        else:
            r, adm = np.zeros((n, m), np.float32), np.zeros((n, m), bool)
        masked = np.where(adm, r, np.float32(np.inf)).astype(np.float32)
        for a in range(n):
            js = np.nonzero(adm[a])[0]
            out["num_admissible"][a] = len(js)
            if len(js) == 0:
                continue
            b = js[np.argmin(r[a, js])]
            out["best"][a] = b
            out["best_distance"][a] = r[a, b]
            rest = js[js != b]
            if len(rest):
                out["second_distance"][a] = r[a, rest].min()
        for j in range(m):
            as_ = np.nonzero(adm[:, j])[0]
            if len(as_):
                out["best_row"][j] = as_[np.argmin(masked[as_, j])]
        for a in range(n):
            b = out["best"][a]
            if b < 0 or out["best_row"][b] != a:
                continue
            if o["ratio"] <= 1.0 or float(out["best_distance"][a]) * o["ratio"] <= float(out["second_distance"][a]):
                out["match"][a] = b
        status = [INVALID if not ok[a] else SHORT if short[a] else CONTINUED if out["match"][a] >= 0 else NEW for a in range(n)]
        ids, age = np.full(n, -1, np.int32), np.zeros(n, np.int32)
        for a in range(n):
            if status[a] == CONTINUED:
                ids[a], age[a] = prev["id"][out["match"][a]], prev["age"][out["match"][a]] + 1
            elif status[a] == NEW:
                ids[a], age[a] = self.next_id, 1
                self.next_id += 1
        out["num_continued"] = out.pop("num_matched")
        out["num_continued"] = status.count(CONTINUED)
        out.update(num_new=status.count(NEW), segment_status=status, id=ids, age=age, admissible=adm)
        # a segment without an id is carried as not valid: it is nobody's partner, whatever the next run's options
        self.prev = dict(seg=seg, desc=desc, ok=ok & (ids >= 0), id=ids, age=age)
        return out


def track(frames, **over):
    """slslam_track_lines: a sequence from an empty tracker."""
    return Tracker().run(frames, **over)

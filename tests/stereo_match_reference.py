"""The stereo line matcher's contract (include/slslam_hip.h: slslam_stereo_matcher_*, slslam_match_stereo) in numpy: what
tests/test_gpu_stereo_match.py compares the device with, and what tests/test_stereo_match_cpu.py pins by hand.  The geometric gate is
fp64 from the float end points, every operation rounded on its own, in the header's order; the descriptor distance is the float chain
of descriptor_match_reference.distances; every decision is made as the contract words it.  `real=np.longdouble` evaluates the same
formulas in extended precision: the measure of the fp64 rounding the tests' tolerance for the doubles is made from."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import descriptor_match_reference as DM  # noqa: E402

OK, EMPTY = "OK", "EMPTY"
MATCHED, UNMATCHED, FLAT, INVALID = "MATCHED", "UNMATCHED", "FLAT", "INVALID"
SEGMENT_STATUS = [MATCHED, UNMATCHED, FLAT, INVALID]

DEFAULTS = dict(min_disparity=0.0, max_disparity=128.0, max_tan2=0.03, min_rows=3.0, min_overlap=0.5, ratio=1.5, max_distance=0.25,
                fx=1.0, fy=1.0, cx=0.0, cy=0.0)


def options(**over):
    unknown = set(over) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown stereo option %s" % sorted(unknown))
    return dict(DEFAULTS, **{k: float(v) for k, v in over.items()})


def options_valid(o):
    f = np.isfinite
    return bool(f(o["min_disparity"]) and f(o["max_disparity"]) and o["min_disparity"] <= o["max_disparity"]
                and f(o["max_tan2"]) and o["max_tan2"] >= 0 and f(o["min_rows"]) and o["min_rows"] >= 0
                and f(o["min_overlap"]) and 0 <= o["min_overlap"] <= 1 and not np.isnan(o["ratio"]) and not np.isnan(o["max_distance"])
                and f(o["fx"]) and f(o["fy"]) and o["fx"] != 0 and o["fy"] != 0 and f(o["cx"]) and f(o["cy"]))


def segments(seg, real=np.float64):
    """What the contract derives per segment, from its float end points: dict of [n] arrays x0, y0, x1, y1, lo, hi, ext, dx, dy, slope
    (slope = dx / dy where ext > 0, else 0: it is only read where ext > 0)."""
    s = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4).astype(real)
    x0, y0, x1, y1 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    with np.errstate(all="ignore"):
        lo, hi = np.where(y1 < y0, y1, y0), np.where(y1 < y0, y0, y1)
        ext, dx, dy = hi - lo, x1 - x0, y1 - y0
        slope = np.where(ext > 0, dx / np.where(ext > 0, dy, real(1)), real(0))
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, lo=lo, hi=hi, ext=ext, dx=dx, dy=dy, slope=slope)


def segment_ok(seg, desc):
    """[n] bool: every end point and every descriptor value is finite."""
    seg = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4)
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    desc = desc.reshape(len(seg), -1) if len(seg) else np.zeros((0, 0), np.float32)
    return np.isfinite(seg).all(axis=1) & np.isfinite(desc).all(axis=1)


def gate(left, right, o, real=np.float64, margins=False):
    """The geometric part of admissibility, [n, m] bool, with the signed dot product [n, m]; margins=True returns instead the list of
    (value, threshold) array pairs of every comparison that was reached, for the tests' "no decision near its threshold" check."""
    A = {k: v[:, None] for k, v in segments(left, real).items()}
    B = {k: v[None, :] for k, v in segments(right, real).items()}
    R = real
    with np.errstate(all="ignore"):
        rows = (A["ext"] >= R(o["min_rows"])) & (B["ext"] >= R(o["min_rows"]))
        top, bot = np.where(A["lo"] > B["lo"], A["lo"], B["lo"]), np.where(A["hi"] < B["hi"], A["hi"], B["hi"])
        ov, mn = bot - top, np.where(A["ext"] < B["ext"], A["ext"], B["ext"])
        need = R(o["min_overlap"]) * mn
        overlap = (ov >= need) & (ov > 0)
        p1, p2 = A["dx"] * B["dx"], A["dy"] * B["dy"]
        dot = p1 + p2
        q1, q2 = A["dx"] * B["dy"], A["dy"] * B["dx"]
        cross = q1 - q2
        c2, d2 = cross * cross, dot * dot
        lim = R(o["max_tan2"]) * d2
        direction = (c2 <= lim) & (dot != 0)
        yc = R(0.5) * (top + bot)
        xa = A["x0"] + (yc - A["y0"]) * A["slope"]
        xb = B["x0"] + (yc - B["y0"]) * B["slope"]
        d = xa - xb
        disparity = (R(o["min_disparity"]) <= d) & (d <= R(o["max_disparity"]))
    if margins:
        full = np.broadcast_to
        shape = rows.shape
        out = [(full(A["ext"], shape), o["min_rows"], np.ones(shape, bool)), (full(B["ext"], shape), o["min_rows"], np.ones(shape, bool)),
               (ov, need, rows), (ov, 0.0, rows), (c2, lim, rows & overlap), (d, o["min_disparity"], rows & overlap & direction),
               (d, o["max_disparity"], rows & overlap & direction)]
        return out
    return rows & overlap & direction & disparity, dot


def emit(a, b, o, real=np.float64):
    """observations [8] and disparity [2] of left segment a [4] matched to right segment b [4]."""
    A = {k: v[0] for k, v in segments(a, real).items()}
    B = {k: v[0] for k, v in segments(b, real).items()}
    dot = A["dx"] * B["dx"] + A["dy"] * B["dy"]
    r = (B["x1"], B["y1"], B["x0"], B["y0"]) if dot < 0 else (B["x0"], B["y0"], B["x1"], B["y1"])
    v = (A["x0"], A["y0"], A["x1"], A["y1"]) + r
    fx, fy, cx, cy = (real(o[k]) for k in ("fx", "fy", "cx", "cy"))
    obs = np.array([v[q] / fx - cx / fx if q % 2 == 0 else v[q] / fy - cy / fy for q in range(8)], dtype=real)
    disp = np.array([A["x0"] - (B["x0"] + (A["y0"] - B["y0"]) * B["slope"]), A["x1"] - (B["x0"] + (A["y1"] - B["y0"]) * B["slope"])],
                    dtype=real)
    return obs, disp


def match(left, left_desc, right, right_desc, real=np.float64, **over):
    """One stereo frame.  Returns dict(status, num_matched, match, best, best_distance, second_distance, num_admissible [n],
    best_left [m], segment_status [n] (names), observations [n, 8] and disparity [n, 2] float64 - NaN in rows that are not MATCHED,
    which the library leaves untouched)."""
    o = options(**over)
    assert options_valid(o)
    left = np.ascontiguousarray(left, dtype=np.float32).reshape(-1, 4)
    right = np.ascontiguousarray(right, dtype=np.float32).reshape(-1, 4)
    n, m = len(left), len(right)
    ld, rd = (np.ascontiguousarray(d, dtype=np.float32) for d in (left_desc, right_desc))
    ld = ld.reshape(n, -1) if n else np.zeros((0, 0), np.float32)
    rd = rd.reshape(m, -1) if m else np.zeros((0, 0), np.float32)
    out = DM._none(n, m, EMPTY if n == 0 or m == 0 else OK)
    out["best_left"] = out.pop("best_query")
    okl, okr = segment_ok(left, ld), segment_ok(right, rd)
    geo, _ = gate(left, right, o)
    r = DM.distances(ld, rd) if n and m else np.zeros((n, m), np.float32)
    adm = geo & okl[:, None] & okr[None, :] & np.isfinite(r) & (r.astype(np.float64) < o["max_distance"])
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
            out["best_left"][j] = as_[np.argmin(masked[as_, j])]
    for a in range(n):
        b = out["best"][a]
        if b < 0 or out["best_left"][b] != a:
            continue
        if o["ratio"] <= 1.0 or float(out["best_distance"][a]) * o["ratio"] <= float(out["second_distance"][a]):
            out["match"][a] = b
    out["num_matched"] = int((out["match"] >= 0).sum())
    ext = segments(left)["ext"]
    with np.errstate(invalid="ignore"):
        flat = ~(ext >= o["min_rows"])
    out["segment_status"] = [INVALID if not okl[a] else FLAT if flat[a] else MATCHED if out["match"][a] >= 0 else UNMATCHED
                             for a in range(n)]
    out["observations"] = np.full((n, 8), np.nan, dtype=real)
    out["disparity"] = np.full((n, 2), np.nan, dtype=real)
    for a in np.nonzero(out["match"] >= 0)[0]:
        out["observations"][a], out["disparity"][a] = emit(left[a], right[out["match"][a]], o, real)
    out["admissible"] = adm
    return out


def observations(result):
    """([k, 8], left indices [k]) of the MATCHED rows."""
    idx = np.nonzero(np.asarray(result["match"]) >= 0)[0]
    return np.asarray(result["observations"])[idx], idx

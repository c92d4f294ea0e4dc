"""Records what one call of the line refiner and of the line triangulator returns on three small windows: tests/golden/line_calls_parent.npz.

    python tools/record_line_calls.py [--out tests/golden/line_calls_parent.npz]

Run on the GPU at the commit whose behaviour is to be kept; tests/test_gpu_line_calls_parity.py replays the recorded inputs and demands
equal integers and bit-equal doubles (NaN as NaN): neither kernel uses atomics and a line's bytes do not depend on its company.

The windows (synth.make_window, fixed seeds) are what the host side of the two calls can meet in one run:
  0  70 lines that all run, 8 keyframes: two waves, the second with a ragged tail; lines started from their first stereo observation,
     so that the refiner has steps to take;
  1  10 lines: line 2 has every observation flagged, line 5 has none, camera 2 is NaN (lines 0, 3 and 4 see it and are invalid);
  2  every line constant.
The file holds, per case of CASES, the windows' input arrays and, per window, the returned parameter vector, the per-line records as an
integer and a double array, lines_av (the triangulator) and the totals (the refiner).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from slslam_amd import capi, synth  # noqa: E402

WINDOW_KEYS = ("camera_index", "line_index", "fixed_index", "observations", "parameters")
SUMMARY_INT = ("num_successful_steps", "num_unsuccessful_steps", "termination_type", "num_free_parameters", "num_residual_blocks")
SUMMARY_DBL = ("initial_cost", "final_cost", "fixed_cost")
LINE_INT = ("status", "termination_type", "num_successful_steps", "num_unsuccessful_steps", "num_observations")
LINE_DBL = ("initial_cost", "final_cost")
TRI_INT = ("status", "num_observations", "num_planes", "first_camera", "clamped")

# case -> (kind, keyword arguments of run)
CASES = {
    "refine": ("refine", {}),
    "triangulate_0": ("triangulate", {"method": 0}),
    "triangulate_1": ("triangulate", {"method": 1}),
}


def windows():
    a = synth.make_window(21, num_lines=70, num_kf=8, num_free=4, line_init="triangulate")
    b = synth.make_window(22, num_lines=10, num_kf=4, num_free=2, mean_track=3.0)
    keep = np.asarray(b["line_index"]) != 5
    b = dict(b, camera_index=np.asarray(b["camera_index"])[keep], line_index=np.asarray(b["line_index"])[keep],
             fixed_index=np.array(b["fixed_index"]).reshape(-1, 2)[keep].copy(), observations=np.asarray(b["observations"])[keep],
             parameters=np.array(b["parameters"]))
    b["fixed_index"][b["line_index"] == 2, 1] = 1
    b["fixed_index"] = b["fixed_index"].reshape(-1)
    b["parameters"][6 * 2 + 4] = np.nan
    c = synth.make_window(23, num_lines=12, num_kf=3, num_free=2, mean_track=3.0)
    f = np.array(c["fixed_index"]).reshape(-1, 2).copy()
    f[:, 1] = 1
    c = dict(c, fixed_index=f.reshape(-1))
    return [a, b, c]


def inputs(ws):
    d = {}
    for i, w in enumerate(ws):
        for k in WINDOW_KEYS:
            d["%s_%d" % (k, i)] = np.array(w[k])
        d["sizes_%d" % i] = np.array([w["num_cameras"], w["num_lines"]], dtype=np.int64)
    d["num_windows"] = np.array(len(ws), dtype=np.int64)
    return d


def as_windows(d):
    ws = []
    for i in range(int(d["num_windows"])):
        w = {k: d["%s_%d" % (k, i)] for k in WINDOW_KEYS}
        w["num_cameras"], w["num_lines"] = (int(v) for v in d["sizes_%d" % i])
        ws.append(w)
    return ws


def _fields(res, names, dtype):
    return np.array([[r[k] for k in names] for r in res], dtype=dtype).reshape(len(res), len(names))


def run(kind, kw, inp):
    """One case: the recorded outputs as a dict of arrays."""
    ws = as_windows(inp)
    out = {}
    if kind == "refine":
        h = capi.LineRefiner(0, 0)
        try:
            xs, rs, ts = h.run(ws, **kw)
        finally:
            h.close()
        for i in range(len(ws)):
            out["line_int_%d" % i], out["line_dbl_%d" % i] = _fields(rs[i], LINE_INT, np.int64), _fields(rs[i], LINE_DBL, np.float64)
            out["summary_int_%d" % i] = np.array([ts[i][k] for k in SUMMARY_INT], dtype=np.int64)
            out["summary_dbl_%d" % i] = np.array([ts[i][k] for k in SUMMARY_DBL], dtype=np.float64)
    else:
        h = capi.LineTriangulator(0, 0)
        try:
            xs, rs, avs = h.run(ws, **kw)
        finally:
            h.close()
        for i in range(len(ws)):
            out["line_int_%d" % i] = _fields(rs[i], TRI_INT, np.int64)
            out["line_dbl_%d" % i] = np.array(rs[i]["eigenvalues"], dtype=np.float64).reshape(len(rs[i]), 4)
            out["lines_av_%d" % i] = np.array(avs[i])
    for i in range(len(ws)):
        out["parameters_%d" % i] = np.array(xs[i])
    return out


def covers(done):
    """The recording meets what its windows were made for; says what is missing."""
    st = [done["refine"][1]["line_int_%d" % i][:, 0] for i in range(3)]
    assert (st[0] == capi.LINE_REFINED).all() and len(st[0]) == 70, st[0]
    assert st[1][2] == capi.LINE_CONSTANT and st[1][5] == capi.LINE_NO_OBSERVATIONS, st[1]
    assert (st[1] == capi.LINE_INVALID).any() and (st[1] == capi.LINE_REFINED).any(), st[1]
    assert (st[2] == capi.LINE_CONSTANT).all(), st[2]
    steps = done["refine"][1]["line_int_0"]
    assert (steps[:, 2] > 0).any(), "no line of window 0 took a step"
    for name in ("triangulate_0", "triangulate_1"):
        tt = [done[name][1]["line_int_%d" % i][:, 0] for i in range(3)]
        assert (tt[0] <= capi.TRI_STEREO).all(), tt[0]
        assert tt[1][2] == capi.TRI_CONSTANT and tt[1][5] == capi.TRI_NO_OBSERVATIONS and (tt[1] == capi.TRI_INVALID).any(), tt[1]
        assert (tt[2] == capi.TRI_CONSTANT).all(), tt[2]
    assert (done["triangulate_1"][1]["line_int_0"][:, 0] == capi.TRI_MULTIVIEW).any()


def load(path):
    """{case: (inputs, outputs)} of a recorded file."""
    cases = {}
    with np.load(path) as z:
        for key in z.files:
            name, side, k = key.split("/")
            cases.setdefault(name, ({}, {}))[0 if side == "in" else 1][k] = z[key]
    return cases


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "line_calls_parent.npz"))
    a = ap.parse_args()
    inp = inputs(windows())
    done = {name: (inp, run(kind, kw, inp)) for name, (kind, kw) in CASES.items()}
    covers(done)
    flat = {}
    for name, (i, o) in done.items():
        flat.update({"%s/in/%s" % (name, k): v for k, v in i.items()})
        flat.update({"%s/out/%s" % (name, k): v for k, v in o.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **flat)
    print("wrote %s: %d arrays, %d bytes" % (a.out, len(flat), os.path.getsize(a.out)))

"""Time of slslam_line_detector_run beside the numpy / scipy reference (tests/line_detect_reference.py) on one host thread.

    python tools/line_detect_bench.py [--width 752] [--height 480] [--segments 300] [--repeats 5] [--out profiles/line_detect_bench.txt]

Shapes: a stereo pair (2 frames per call) and 64 frames per call of width x height from synth.make_line_image with `segments` drawn
segments each, at the default options.  Warm (three untimed calls first), median and spread of `repeats` calls.  Per shape: the wall
time of the call - synchronous: packing the images into the page-locked block, upload, eleven launches, download, scatter - and the
launches alone between two events on the handle's stream (slslam_line_detector_timing), also per launch.  Before anything is timed the
first stereo pair's results are compared with the reference's (verify); a difference ends the tool with a non-zero status and no timing
line.  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LAUNCHES = 11


def verify(capi, R, views, max_pixels):
    """The device against the reference on `views`, untimed: the integer results equal, the fp64 ones within R.DEVICE_TOLERANCE (the float
    segments within that and half a float's spacing).  Ends the tool on the first difference."""
    import numpy as np
    d = capi.LineDetector(max_frames=len(views), max_pixels=max_pixels)          # (a handle of its own: the timed one keeps its buffers)
    got = d.run(views, labels=True)
    d.close()
    for f, (g, view) in enumerate(zip(got, views)):
        r = R.detect(view, max_segments=d.opt.max_segments)
        bad = [k for k in ("num_components", "num_ok", "num_written") if g[k] != r[k]]
        bad += [k for k in ("labels", "pixels", "label") if not np.array_equal(g[k], r[k])]
        if [g["status_counts"][s] for s in R.STATUS] != r["status_counts"]:
            bad.append("status_counts")
        for k in ("segments", "length", "thickness", "strength"):
            slack = 0.5 * np.spacing(np.abs(r[k]).astype(np.float32)).astype(np.float64) if k == "segments" else 0.0
            if g[k].shape != r[k].shape or not (np.abs(g[k].astype(np.float64) - r[k]) <= R.DEVICE_TOLERANCE + slack).all():
                bad.append(k)
        if bad:
            raise SystemExit("line_detect_bench: frame %d differs from the reference in %s: nothing is timed" % (f, ", ".join(bad)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--segments", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_detect_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")                # (the host row: one thread; set before numpy loads its BLAS)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    os.environ.setdefault("MKL_NUM_THREADS", "1")
    from slslam_amd import capi, synth
    import line_detect_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    W, H, S = a.width, a.height, a.segments
    views = [synth.make_line_image(9800 + i, H, W, S)["image"] for i in range(4)]
    lines = ["line_detect_bench: %d x %d, %d drawn segments per frame, default options, max_segments 512" % (W, H, S)]
    verify(capi, R, views[:2], W * H)                           # what is timed below is what the reference computes

    d = capi.LineDetector(max_frames=64, max_pixels=W * H)
    d.set_timing(True)
    for F in (2, 64):
        # the raw entry point on prepared arrays, so that the binding's conversions are not in the time; no label plane
        frs, outs, keep = (capi.LineDetectFrame * F)(), (capi.LineDetectResult * F)(), []
        for f in range(F):
            frs[f], outs[f], k = capi._detect_frame(views[f % 4], 512, False)
            keep.append(k)

        def call():
            rc = capi.lib().slslam_line_detector_run(d._h, F, frs, outs)
            assert rc == 0, rc

        for _ in range(3):
            call()
        wall, kern = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(d.kernel_ms())
        comps = sum(int(k[1]["counts"][0]) for k in keep)
        ok = sum(int(k[1]["counts"][1]) for k in keep)
        up, down = F * (W * H + 32), F * (48 + 512 * 48)
        for name, ms in (("wall", wall), ("kernels alone, events", kern)):
            md = statistics.median(ms)
            lines.append("%d frames per call, %s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ms per frame, %.3f ns per pixel"
                         % (F, name, md, min(ms), max(ms), len(ms), md / F, 1e6 * md / (F * W * H)))
        lines.append("  %.1f us per launch (%d launches); %d components and %d segments in all; %.2f MB up, %.2f MB down"
                     % (1e3 * statistics.median(kern) / LAUNCHES, LAUNCHES, comps, ok, 1e-6 * up, 1e-6 * down))
        lines.append("  wall - kernels = %.3f ms: packing, upload, download, scatter; the upload alone at 50 GB/s would take %.3f ms"
                     % (statistics.median(wall) - statistics.median(kern), 1e3 * up / 50e9))
    lines.append("handle buffers: %s" % d.stats())
    d.close()

    # the host, one thread, the stereo pair
    t_ref = []
    for _ in range(3):
        t0 = time.perf_counter()
        for v in views[:2]:
            R.detect(v)
        t_ref.append(1e3 * (time.perf_counter() - t0))
    md = statistics.median(t_ref)
    lines.append("numpy / scipy reference, 2 frames, one thread, wall: median %.1f ms (min %.1f, max %.1f, %d calls); x 32 = %.0f ms"
                 % (md, min(t_ref), max(t_ref), len(t_ref), 32 * md))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the register counts kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Resources of the kernels")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

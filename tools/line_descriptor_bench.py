"""Time of slslam_line_descriptor_run beside the numpy reference (tests/line_descriptor_reference.py, fp64) on one host thread.

    python tools/line_descriptor_bench.py [--width 752] [--height 480] [--segments 300] [--repeats 5] [--out profiles/line_descriptor_bench.txt]

Shapes: a stereo pair (2 frames per call) and 64 frames per call of width x height with `segments` segments each, from
synth.make_line_image, at the default options (M = 9, w = 5, D = 72).  Warm (three untimed calls first), median and spread of `repeats`
calls.  Two figures per shape: the wall time of the call - synchronous: packing the images into the page-locked block, upload, launch,
download, scatter - and the launch alone between two events on the handle's stream (slslam_line_descriptor_timing).  The bytes each way
and the interpolated gradient samples are counted from the shapes.  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--segments", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_descriptor_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")                # (the host row: one thread; set before numpy loads its BLAS)
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    os.environ.setdefault("MKL_NUM_THREADS", "1")
    from slslam_amd import capi, synth
    import line_descriptor_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    W, H, S = a.width, a.height, a.segments
    views = [synth.make_line_image(9800 + i, H, W, S) for i in range(4)]
    rows, D = 45, 72
    lines = ["line_descriptor_bench: %d x %d, %d segments per frame, M = 9, w = 5, D = %d" % (W, H, S, D)]

    d = capi.LineDescriptor(max_frames=64, max_pixels=W * H, max_segments=S)
    d.set_timing(True)
    for F in (2, 64):
        # the raw entry point on prepared arrays, so that the binding's conversions are not in the time
        frs, outs, keep = (capi.MsldFrame * F)(), (capi.MsldResult * F)(), []
        for f in range(F):
            frs[f], outs[f], k = capi._msld_frame(views[f % 4]["image"], views[f % 4]["segments"], D)
            keep.append(k)

        def call():
            rc = capi.lib().slslam_line_descriptor_run(d._h, F, frs, outs)
            assert rc == 0, rc

        for _ in range(3):
            call()
        wall, kern = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            call()
            wall.append(1e3 * (time.perf_counter() - t0))
            kern.append(d.kernel_ms())
        samples = sum(int(k[2]["num_samples"].sum()) for k in keep) * rows
        up, down = F * (W * H + 40 * S + 16) + 16 * rows, F * S * (4 * D + 12)
        ok = sum(int((k[2]["status"] == 0).sum()) for k in keep)
        for name, ms in (("wall", wall), ("kernel alone, events", kern)):
            md = statistics.median(ms)
            lines.append("%d frames per call, %s: median %.3f ms (min %.3f, max %.3f, %d calls) = %.3f ms per frame, %.2f us per segment, "
                         "%.3f ns per gradient sample" % (F, name, md, min(ms), max(ms), len(ms), md / F, 1e3 * md / (F * S), 1e6 * md / samples))
        lines.append("  %d of %d segments OK, %.2f M gradient samples; %.2f MB up, %.2f MB down" % (ok, F * S, 1e-6 * samples, 1e-6 * up, 1e-6 * down))
        lines.append("  wall - kernel = %.3f ms: packing, upload, download, scatter; the upload alone at 50 GB/s would take %.3f ms"
                     % (statistics.median(wall) - statistics.median(kern), 1e3 * up / 50e9))
    lines.append("handle buffers: %s" % d.stats())
    d.close()

    # the host, one thread, the stereo pair
    t_ref = []
    for _ in range(3):
        t0 = time.perf_counter()
        for v in views[:2]:
            R.describe(v["image"], v["segments"])
        t_ref.append(1e3 * (time.perf_counter() - t0))
    md = statistics.median(t_ref)
    lines.append("numpy reference (fp64), 2 frames, one thread, wall: median %.1f ms (min %.1f, max %.1f, %d calls); x 32 = %.0f ms"
                 % (md, min(t_ref), max(t_ref), len(t_ref), 32 * md))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    keep = ""                                            # (the register counts kept below the timings)
    if os.path.exists(a.out):
        old = open(a.out).read()
        i = old.find("Resources of the kernel")
        keep = "\n" + old[i:] if i >= 0 else ""
    with open(a.out, "w") as f:
        f.write(text + keep)


if __name__ == "__main__":
    main()

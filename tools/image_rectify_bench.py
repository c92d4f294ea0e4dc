"""Time of slslam_image_rectifier_run beside the numpy reference (tests/image_rectify_reference.py) on one host thread.

    python tools/image_rectify_bench.py [--width 752] [--height 480] [--repeats 5] [--out profiles/image_rectify_bench.txt]

Shapes: one raw stereo pair (2 frames per call) and 64 pairs (128 frames per call) of width x height through the two cameras that
slslam_stereo_rectify makes of a rig with a turned, distorted right camera, with smoothing off and at sigma = 0.6.  Warm (three untimed
calls first), median and spread of `repeats` calls.  Per shape: the wall time of the call - synchronous: packing, upload, one launch,
download, scatter -, the launch alone between two events on the handle's stream (slslam_image_rectifier_timing), the upload and the
download alone as copies of the same bytes between page-locked and device memory, and the launch against the bytes it moves: per
output pixel 8 map bytes, 1 valid byte, 1 byte written and the source bytes read, as a fraction of the HBM peak of 8 TB/s.  Before
anything is timed the first pair is compared with the reference (maps, valid bytes and output bytes equal, both settings); a
difference ends the tool with a non-zero status and no timing line.  The kernels' register, LDS and scratch counts are appended
from tools/kernel_resources.py.  A measurement, not a gate: needs a GPU and fails without one."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12
SIGMA = 0.6


def rig_cameras(capi, W, H):
    """The rig of synth.make_raw_stereo_pair at this size, rectified by the library."""
    from slslam_amd import synth
    f = 0.9 * W
    left = dict(fx=f + 0.7, fy=f - 0.4, cx=0.5 * (W - 1) + 2.3, cy=0.5 * (H - 1) - 1.9, k1=-0.28, k2=0.09, p1=0.0012, p2=-0.0009, k3=-0.01,
                width=W, height=H)
    right = dict(fx=1.01 * f + 0.7, fy=1.01 * f - 0.4, cx=0.5 * (W - 1) - 1.7, cy=0.5 * (H - 1) + 1.2, k1=-0.24, k2=0.07, p1=-0.001, p2=0.0014,
                 width=W, height=H)
    R = synth.rodrigues([0.012, -0.02, 0.016])
    k = capi.stereo_rectify(left, right, R, -(R @ [0.12, 0.004, -0.003]))
    return [k["left"], k["right"]]


def verify(capi, R, cams, pair):
    import numpy as np
    for sigma in (0.0, SIGMA):
        radius, taps = capi.smooth_taps(sigma)
        r = capi.ImageRectifier(cams, max_frames=2, max_pixels=pair[0].size, border="replicate", smooth_sigma=sigma)
        got = r.run([(0, pair[0]), (1, pair[1])], valid=True)
        for k in range(2):
            cam = cams[k].as_dict()
            m, dev = R.make_map(cam), r.get_map(k)
            ref = R.rectify(pair[k], cam, R.REPLICATE, 0, radius, taps, m=m)
            bad = [n for n in ("qx", "qy", "valid") if not np.array_equal(dev[n], m[n])]
            bad += [n for n in ("image", "valid") if not np.array_equal(got[k][n], ref[n])]
            if got[k]["num_valid"] != ref["num_valid"]:
                bad.append("num_valid")
            if bad:
                raise SystemExit("image_rectify_bench: camera %d at sigma %.1f differs from the reference in %s: nothing is timed"
                                 % (k, sigma, ", ".join(bad)))
        r.close()


def copy_ms(nbytes, to_device, repeats):
    """A synchronous hipMemcpy of nbytes between page-locked and device memory alone (the runtime the library runs on), median ms."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    host, dev = C.c_void_p(), C.c_void_p()
    assert hip.hipHostMalloc(C.byref(host), C.c_size_t(nbytes), 0) == 0 and hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) == 0
    C.memset(host, 1, nbytes)
    ms = []
    for i in range(repeats + 2):
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        rc = hip.hipMemcpy(dev, host, C.c_size_t(nbytes), 1) if to_device else hip.hipMemcpy(host, dev, C.c_size_t(nbytes), 2)
        assert rc == 0 and hip.hipDeviceSynchronize() == 0
        if i >= 2:
            ms.append(1e3 * (time.perf_counter() - t0))
    hip.hipFree(dev)
    hip.hipHostFree(host)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_rectify_bench.txt"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
    os.environ.setdefault("MKL_NUM_THREADS", "1")
    import numpy as np
    from slslam_amd import capi, synth
    import image_rectify_reference as R
    if capi.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    W, H = a.width, a.height
    cams = rig_cameras(capi, W, H)
    views = [synth.make_line_image(9900 + i, H, W, 300)["image"] for i in range(4)]
    lines = ["image_rectify_bench: %d x %d raw to %d x %d rectified, two cameras, border replicate" % (W, H, W, H)]
    verify(capi, R, cams, views[:2])                            # what is timed below is what the reference computes
    n = W * H
    for sigma in (0.0, SIGMA):
        r = capi.ImageRectifier(cams, max_frames=128, max_pixels=n, border="replicate", smooth_sigma=sigma)
        r.set_timing(True)
        radius = capi.smooth_taps(sigma)[0]
        for pairs in (1, 64):
            F = 2 * pairs
            frs, outs, keep = (capi.RectifyFrame * F)(), (capi.RectifyResult * F)(), []
            for f in range(F):
                frs[f], outs[f], k = capi._rectify_frame(cams, f % 2, views[f % 4], False)
                keep.append(k)

            def call():
                rc = capi.lib().slslam_image_rectifier_run(r._h, F, frs, outs)
                assert rc == 0, rc

            for _ in range(3):
                call()
            wall, kern = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                call()
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(r.kernel_ms())
            up, down = F * (n + 24), F * n
            t_up, t_down = copy_ms(up, True, a.repeats), copy_ms(down, False, a.repeats)
            halo = ((64 + 2 * radius) * (16 + 2 * radius)) / 1024.0 if radius else 1.0
            moved = F * n * (halo * (8 + 1 + 4) + 1)           # map and valid bytes and four source bytes per remapped pixel, one byte out
            mk, mw = statistics.median(kern), statistics.median(wall)
            lines.append("sigma %.1f (radius %d), %d pair%s per call: wall median %.3f ms (min %.3f, max %.3f, %d calls); launch alone, events "
                         "%.3f ms (min %.3f, max %.3f)" % (sigma, radius, pairs, "" if pairs == 1 else "s", mw, min(wall), max(wall), len(wall),
                                                          mk, min(kern), max(kern)))
            lines.append("  upload %.2f MB alone %.3f ms, download %.2f MB alone %.3f ms; wall - launch - copies = %.3f ms: packing and scatter"
                         % (1e-6 * up, t_up, 1e-6 * down, t_down, mw - mk - t_up - t_down))
            lines.append("  launch: %.2f MB requested (9 map + 4 source bytes x %.2f remaps + 1 written, per output pixel) = %.1f GB/s = %.2f %% of "
                         "the 8 TB/s HBM peak" % (1e-6 * moved, halo, 1e-9 * moved / (1e-3 * mk), 100.0 * moved / (1e-3 * mk) / HBM_PEAK))
            if pairs == 64:
                t_again = copy_ms(down, True, a.repeats)
                lines.append("  the host round trip a device hand-over to the detector would remove: download %.3f ms + the detector's upload of "
                             "the same bytes %.3f ms = %.3f ms per 64 pairs" % (t_down, t_again, t_down + t_again))
        lines.append("  handle buffers: %s" % r.stats())
        r.close()
        radius, taps = capi.smooth_taps(sigma)
        t_ref = []
        maps = [R.make_map(c.as_dict()) for c in cams]
        for _ in range(3):
            t0 = time.perf_counter()
            for k in range(2):
                R.rectify(views[k], cams[k].as_dict(), R.REPLICATE, 0, radius, taps, m=maps[k])
            t_ref.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        R.make_map(cams[0].as_dict())
        t_map = 1e3 * (time.perf_counter() - t0)
        lines.append("  numpy reference, one pair, one thread, maps given: median %.1f ms (min %.1f, max %.1f); one map %.1f ms"
                     % (statistics.median(t_ref), min(t_ref), max(t_ref), t_map))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "rectify_api.hip"], capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit("image_rectify_bench: tools/kernel_resources.py failed:\n" + res.stdout + res.stderr)
    text += "\nResources of the kernels (tools/kernel_resources.py rectify_api.hip, gfx950):\n" + res.stdout
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

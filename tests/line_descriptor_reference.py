"""The MSLD line descriptor's contract (include/slslam_hip.h: slslam_line_descriptor_*) in numpy: what tests/test_gpu_line_descriptor.py
compares the device with, and what tests/test_line_descriptor_cpu.py pins by hand.  Every step is the contract's, in its order; all real
arithmetic runs in `dtype` - float64 is the reference, float32 is the same evaluation at the precision the device's interpolation has,
and is what the device tolerance below is measured with.  L and N are evaluated in double under either dtype, as the contract words it,
and the weight table holds floats under either.  Mean and standard deviation are taken two-pass about the first sample's value: the
same numbers in real arithmetic, and a band that is constant along the line has a standard deviation of exactly 0."""
import numpy as np

OK, FLAT, TOO_SHORT, OUTSIDE, INVALID = "OK", "FLAT", "TOO_SHORT", "OUTSIDE", "INVALID"

# The largest difference of a descriptor component between describe(dtype=float32) and describe(dtype=float64) over every input of
# tests/test_gpu_line_descriptor.py (test_line_descriptor_cpu.gpu_inputs()): measured 8.8e-7, rounded up to one digit
# (test_float32_figure prints the five largest: the long segments of `along` lead, 8.2e-7 on the 320 x 240 pair follows; the issue's
# prototype saw 6e-7 to 2.4e-6).  test_line_descriptor_cpu.py asserts that the float32 evaluation stays within it.
F32_FIGURE = 1.0e-6
# What the device may differ by from describe(dtype=float64): 8 x the figure.  The margin covers another summation order and fused
# multiply-adds on the device; the device's sample positions and moments are fp64, so it has less to cover than the float32 evaluation.
DEVICE_TOLERANCE = 8 * F32_FIGURE


def weight_table(bands, band_width):
    """(wa, wb, f, band) [M w]: row r adds wa[r] x its components to band[r] and wb[r] x them to band[r] + 1; f[r] is its global weight.
    Computed in double, rounded to float."""
    rows = bands * band_width
    r = np.arange(rows, dtype=np.float64)
    rho = r - 0.5 * (rows - 1)
    sigma = 0.5 * (rows - 1) if rows > 1 else 1.0
    f = np.exp(-rho * rho / (2.0 * sigma * sigma))
    t = (r + 0.5) / band_width - 0.5
    i0 = np.floor(t)
    a = t - i0
    return (f * (1.0 - a)).astype(np.float32), (f * a).astype(np.float32), f.astype(np.float32), i0.astype(np.int64)


def segment_status(width, height, seg):
    """(status, L, N): INVALID before OUTSIDE before TOO_SHORT; N = floor(L) for a segment that runs, else 0."""
    s = np.asarray(seg, dtype=np.float32)
    if not np.isfinite(s).all():
        return INVALID, 0.0, 0
    if s[0] < 0 or s[0] > width - 1 or s[2] < 0 or s[2] > width - 1 or s[1] < 0 or s[1] > height - 1 or s[3] < 0 or s[3] > height - 1:
        return OUTSIDE, 0.0, 0
    dx, dy = np.float64(s[2]) - np.float64(s[0]), np.float64(s[3]) - np.float64(s[1])
    length = float(np.sqrt(dx * dx + dy * dy))
    if length < 2.0:
        return TOO_SHORT, length, 0
    return OK, length, int(np.floor(length))


def pixel_gradients(image, dtype):
    """gx, gy [H, W] at the integer pixels: central differences over the replicated border."""
    img = np.asarray(image).astype(dtype)
    h, w = img.shape
    xs, ys = np.arange(w), np.arange(h)
    gx = (img[:, np.minimum(xs + 1, w - 1)] - img[:, np.maximum(xs - 1, 0)]) / dtype(2)
    gy = (img[np.minimum(ys + 1, h - 1), :] - img[np.maximum(ys - 1, 0), :]) / dtype(2)
    return gx, gy


def _bilinear(g, x, y):
    h, w = g.shape
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    cx0, cx1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    cy0, cy1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    one = g.dtype.type(1)
    return (one - ay) * ((one - ax) * g[cy0, cx0] + ax * g[cy0, cx1]) + ay * ((one - ax) * g[cy1, cx0] + ax * g[cy1, cx1])


def describe_segment(gx, gy, seg, length, n, table, bands, orient, dtype):
    """(descriptor [8 M], polarity, flat) of a segment that runs."""
    wa, wb, f, band = table
    rows = len(f)
    s = np.asarray(seg, dtype=np.float32).astype(dtype)
    L = dtype(length)
    dlx, dly = (s[2] - s[0]) / L, (s[3] - s[1]) / L
    j = np.arange(n).astype(dtype)
    sj = L / dtype(2) + j - dtype(n - 1) / dtype(2)
    rho = np.arange(rows).astype(dtype) - dtype(rows - 1) / dtype(2)
    x = s[0] + sj[:, None] * dlx + rho[None, :] * (-dly)
    y = s[1] + sj[:, None] * dly + rho[None, :] * dlx
    assert x.dtype == dtype
    qx, qy = _bilinear(gx, x, y), _bilinear(gy, x, y)
    gl = qx * dlx + qy * dly
    gp = qx * (-dly) + qy * dlx
    fw = f.astype(dtype)
    polarity = (fw[None, :] * gp).sum()
    if orient and polarity < 0:
        gp, gl, polarity = -gp[:, ::-1], -gl[:, ::-1], -polarity
    zero = dtype(0)
    comp = np.stack([np.maximum(gp, zero), np.maximum(-gp, zero), np.maximum(gl, zero), np.maximum(-gl, zero)], axis=2)    # [N, R, 4]
    v = np.zeros((n, bands, 4), dtype=dtype)
    for r in range(rows):
        i0 = int(band[r])
        if 0 <= i0 < bands:
            v[:, i0] += dtype(wa[r]) * comp[:, r]
        if 0 <= i0 + 1 < bands:
            v[:, i0 + 1] += dtype(wb[r]) * comp[:, r]
    d = v - v[0]
    md = d.sum(axis=0) / dtype(n)
    mu = v[0] + md
    sd = np.sqrt(((d - md) ** 2).sum(axis=0) / dtype(n))
    nm, ns = np.sqrt((mu * mu).sum()), np.sqrt((sd * sd).sum())
    half = dtype(1) / np.sqrt(dtype(2))
    out = np.zeros(8 * bands, dtype=dtype)
    if nm > 0:
        out[:4 * bands] = (mu * (half / nm)).reshape(-1)
    if ns > 0:
        out[4 * bands:] = (sd * (half / ns)).reshape(-1)
    assert out.dtype == dtype
    return out, polarity, not (nm > 0 or ns > 0)


def describe(image, segments, bands=9, band_width=5, orient=True, dtype=np.float64):
    """One frame.  Returns dict(descriptors [n, 8 M] of `dtype`, status [n] (names), num_samples [n] int32, polarity [n] of `dtype`)."""
    assert 1 <= bands <= 16 and 1 <= band_width <= 9 and bands * band_width <= 144
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    h, w = image.shape
    seg = np.asarray(segments, dtype=np.float32).reshape(-1, 4)
    table = weight_table(bands, band_width)
    gx, gy = pixel_gradients(image, dtype)
    out = {"descriptors": np.zeros((len(seg), 8 * bands), dtype=dtype), "status": [], "num_samples": np.zeros(len(seg), np.int32),
           "polarity": np.zeros(len(seg), dtype=dtype)}
    for i, s in enumerate(seg):
        st, length, n = segment_status(w, h, s)
        if st == OK:
            d, pol, flat = describe_segment(gx, gy, s, length, n, table, bands, bool(orient), dtype)
            out["num_samples"][i], out["polarity"][i] = n, pol
            if flat:
                st = FLAT
            else:
                out["descriptors"][i] = d
        out["status"].append(st)
    return out

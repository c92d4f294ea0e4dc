"""The line segment detector's contract (include/slslam_hip.h: slslam_line_detector_*) in numpy: what tests/test_gpu_line_detect.py compares
the device with, and what tests/test_line_detect_cpu.py pins by hand.  Every step is the contract's, in its order: the gradient, the
links, the components and the sums are integers (int64) and must be met bit for bit; the fit runs in `dtype` - float64 is the reference,
np.longdouble is the same evaluation at a higher precision and is what the device tolerance below is measured with."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

OK, SMALL, ISOTROPIC, SHORT, THICK = "OK", "SMALL", "ISOTROPIC", "SHORT", "THICK"
STATUS = [OK, SMALL, ISOTROPIC, SHORT, THICK]              # the values of SLSLAM_LSD_*, the index of status_counts
DEFAULTS = dict(grad_threshold=24, tol_num=11, tol_den=64, min_pixels=12, min_length=10.0, max_thickness=3.0)
# the forward links of a pixel, in the order of their bits (bit 0 is `strong`): E, SW, S, SE as (dx, dy)
FORWARD = ((1, 0), (-1, 1), (0, 1), (1, 1))

# The largest difference of an end-point coordinate, a length or a thickness (pixels; the strength moves by less) between
# detect(dtype=float64) and detect(dtype=np.longdouble) over every input of tests/test_gpu_line_detect.py
# (test_line_detect_cpu.gpu_inputs()): measured 1.0e-12 on the 200 x 200 diagonal - whose smallest eigenvalue is a difference of
# moments near 3000 - and 5e-14 or less on every other input; rounded up to one digit.  test_line_detect_cpu.py asserts that the two evaluations stay within it.
F64_FIGURE = 2.0e-12
# What the device may differ by from detect(dtype=float64): 8 x the figure, the factor of the MSLD descriptor's tolerance.  The device
# evaluates the same operations in the same order in fp64 without contraction; the margin is for a sqrt or a division that rounds otherwise.
DEVICE_TOLERANCE = 8 * F64_FIGURE


def isqrt(m2):
    """The largest integer whose square is at most m2, exactly (int64 array)."""
    m2 = np.asarray(m2, dtype=np.int64)
    w = np.floor(np.sqrt(m2.astype(np.float64))).astype(np.int64)
    w -= (w * w > m2)
    w += ((w + 1) * (w + 1) <= m2)
    return w


def gradients(image):
    """gx, gy [H, W] int64: differences over the replicated border, not halved."""
    img = np.asarray(image).astype(np.int64)
    h, w = img.shape
    xs, ys = np.arange(w), np.arange(h)
    gx = img[:, np.minimum(xs + 1, w - 1)] - img[:, np.maximum(xs - 1, 0)]
    gy = img[np.minimum(ys + 1, h - 1), :] - img[np.maximum(ys - 1, 0), :]
    return gx, gy


def linked(gax, gay, gbx, gby, tol_num, tol_den):
    """Step 2 for two strong pixels of gradients ga and gb (int64 arrays or scalars)."""
    gax, gay, gbx, gby = (np.asarray(v, dtype=np.int64) for v in (gax, gay, gbx, gby))
    dot = gax * gbx + gay * gby
    cross = gax * gby - gay * gbx
    return (dot > 0) & (np.int64(tol_den) * cross * cross <= np.int64(tol_num) * dot * dot)


def link_planes(image, grad_threshold=24, tol_num=11, tol_den=64):
    """(gx, gy, strong [H, W] bool, links [4, H, W] bool): links[k][y, x] joins (x, y) to (x + dx, y + dy) of FORWARD[k]."""
    gx, gy = gradients(image)
    h, w = gx.shape
    strong = gx * gx + gy * gy >= int(grad_threshold) ** 2
    links = np.zeros((4, h, w), dtype=bool)
    ys, xs = np.mgrid[0:h, 0:w]
    for k, (dx, dy) in enumerate(FORWARD):
        inside = (xs + dx >= 0) & (xs + dx < w) & (ys + dy < h)
        ya, xa = ys[inside], xs[inside]
        yb, xb = ya + dy, xa + dx
        links[k][ya, xa] = strong[ya, xa] & strong[yb, xb] & linked(gx[ya, xa], gy[ya, xa], gx[yb, xb], gy[yb, xb], tol_num, tol_den)
    return gx, gy, strong, links


def label_plane(strong, links):
    """labels [H, W] int32: the smallest pixel index y W + x of the pixel's component, -1 where the pixel is not strong."""
    h, w = strong.shape
    idx = np.arange(h * w).reshape(h, w)
    rows, cols = [], []
    for k, (dx, dy) in enumerate(FORWARD):
        ya, xa = np.nonzero(links[k])
        rows.append(idx[ya, xa])
        cols.append(idx[ya + dy, xa + dx])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(h * w, h * w)), directed=False)
    smallest = np.full(comp.max() + 1, h * w, dtype=np.int64)
    np.minimum.at(smallest, comp, idx.reshape(-1))
    labels = smallest[comp].reshape(h, w)
    return np.where(strong, labels, -1).astype(np.int32)


def fit(sums, dtype=np.float64):
    """Step 5 for the sums (sw, swu, swv, swuu, swuv, swvv) of one component, each operation rounded on its own in `dtype`.
    Returns (cx, cy, ex, ey, thickness); ex = ey = 0 for an isotropic component."""
    sw, swu, swv, swuu, swuv, swvv = (dtype(int(v)) for v in sums)
    cx, cy = swu / sw, swv / sw
    sxx, syy, sxy = swuu / sw - cx * cx, swvv / sw - cy * cy, swuv / sw - cx * cy
    two = dtype(2)
    h = (sxx - syy) / two
    rt = np.sqrt(h * h + sxy * sxy)
    lmin = (sxx + syy) / two - rt
    ex, ey = (h + rt, sxy) if h >= 0 else (sxy, rt - h)
    norm = np.sqrt(ex * ex + ey * ey)
    if norm == 0:
        return cx, cy, dtype(0), dtype(0), dtype(0)
    return cx, cy, ex / norm, ey / norm, np.sqrt(max(lmin, dtype(0)))


def detect(image, max_segments=None, dtype=np.float64, **options):
    """One frame.  Returns dict(labels [H, W] int32, num_components, num_ok, num_written, status_counts [5] (the order of STATUS),
    segments [num_written, 4] of `dtype` (x0, y0, x1, y1), length, thickness, strength [num_written] of `dtype`, pixels, label
    [num_written] int32) - the arrays of the OK components in label order, the first max_segments of them - and, for the tests, `all`:
    one dict per component in label order with its label, status, pixel count, integer sums and, where a fit was made, length and
    thickness."""
    opt = dict(DEFAULTS)
    opt.update(options)
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 2
    gx, gy, strong, links = link_planes(image, opt["grad_threshold"], opt["tol_num"], opt["tol_den"])
    labels = label_plane(strong, links)
    h, w = image.shape
    weight = isqrt(gx * gx + gy * gy)
    flat = labels.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] >= 0]
    roots, first = np.unique(flat[order], return_index=True)
    bounds = list(first) + [len(order)]
    comps, counts = [], [0] * 5
    seg, length, thickness, strength, pixels, label = [], [], [], [], [], []
    for c, root in enumerate(roots):
        p = order[bounds[c]:bounds[c + 1]]
        y, x = p // w, p % w
        xr, yr = int(root) % w, int(root) // w
        u, v, wt = x - xr, y - yr, weight[y, x]
        sums = dict(n=len(p), sw=int(wt.sum()), swu=int((wt * u).sum()), swv=int((wt * v).sum()), swuu=int((wt * u * u).sum()),
                    swuv=int((wt * u * v).sum()), swvv=int((wt * v * v).sum()), sgx=int(gx[y, x].sum()), sgy=int(gy[y, x].sum()))
        rec = dict(label=int(root), sums=sums)
        if sums["n"] < opt["min_pixels"]:
            rec["status"] = SMALL
        else:
            cx, cy, ex, ey, thick = fit([sums[k] for k in ("sw", "swu", "swv", "swuu", "swuv", "swvv")], dtype)
            if ex == 0 and ey == 0:
                rec["status"] = ISOTROPIC
            else:
                t = (u.astype(dtype) - cx) * ex + (v.astype(dtype) - cy) * ey
                tmin, tmax = t.min(), t.max()
                rec["length"], rec["thickness"] = tmax - tmin, thick
                if rec["length"] < dtype(opt["min_length"]):
                    rec["status"] = SHORT
                elif thick > dtype(opt["max_thickness"]):
                    rec["status"] = THICK
                else:
                    rec["status"] = OK
                    bx, by = dtype(xr) + cx, dtype(yr) + cy
                    a, b = (bx + tmin * ex, by + tmin * ey), (bx + tmax * ex, by + tmax * ey)
                    if not ex * dtype(sums["sgy"]) - ey * dtype(sums["sgx"]) >= 0:
                        a, b = b, a
                    seg.append(a + b)
                    length.append(rec["length"])
                    thickness.append(thick)
                    strength.append(dtype(sums["sw"]) / dtype(sums["n"]))
                    pixels.append(sums["n"])
                    label.append(int(root))
        counts[STATUS.index(rec["status"])] += 1
        comps.append(rec)
    num_ok = len(seg)
    k = num_ok if max_segments is None else min(num_ok, int(max_segments))
    return {"labels": labels, "num_components": len(roots), "num_ok": num_ok, "num_written": k, "status_counts": counts,
            "segments": np.array(seg[:k], dtype=dtype).reshape(k, 4), "length": np.array(length[:k], dtype=dtype),
            "thickness": np.array(thickness[:k], dtype=dtype), "strength": np.array(strength[:k], dtype=dtype),
            "pixels": np.array(pixels[:k], dtype=np.int32), "label": np.array(label[:k], dtype=np.int32), "all": comps}

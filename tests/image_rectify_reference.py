"""The image rectifier's contract (include/slslam_hip.h: slslam_image_rectifier_*, slslam_stereo_rectify) restated in numpy: the map of a
camera, its quantisation, the integer remap with both border modes, the integer separable smoothing, and the rig construction.  The
reference project has no counterpart of any of it, so this file and the header are the definition; the device is compared with it bit
for bit (tests/test_gpu_image_rectify.py).  The smoothing taps are an input: the tests take them from the library.  numpy only."""
import numpy as np

SUBPIXEL_BITS = 8
SUB = 1 << SUBPIXEL_BITS
NO_COORD = -2 ** 31
CONSTANT, REPLICATE = 0, 1
MAX_RADIUS = 7
# The largest |float64 - longdouble| of sx, sy over the cameras of the GPU tests (tests/test_image_rectify_cpu.py measures and asserts
# it); the device may differ from the float64 reference by 8 x that.
F64_FIGURE = 2.5e-9
DEVICE_TOLERANCE = 8 * F64_FIGURE
# ... and of |float64 - longdouble| / max(1, |s|): the absolute figure is set by the few pixels of a turned camera that lie 1e5 source
# pixels out; relative to the magnitude the device is held to this one as well.
F64_RELATIVE = 6e-14
DEVICE_RELATIVE = 8 * F64_RELATIVE

CAMERA_KEYS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "fx2", "fy2", "cx2", "cy2")


def camera(src_width, src_height, dst_width=None, dst_height=None, fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
           R=None, fx2=None, fy2=None, cx2=None, cy2=None):
    """A camera as a dict, with the defaults of capi.RectifyCamera.make."""
    return dict(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), k1=float(k1), k2=float(k2), p1=float(p1), p2=float(p2), k3=float(k3),
                R=np.array(np.eye(3) if R is None else R, dtype=np.float64).reshape(3, 3),
                fx2=float(fx if fx2 is None else fx2), fy2=float(fy if fy2 is None else fy2),
                cx2=float(cx if cx2 is None else cx2), cy2=float(cy if cy2 is None else cy2),
                src_width=int(src_width), src_height=int(src_height),
                dst_width=int(src_width if dst_width is None else dst_width), dst_height=int(src_height if dst_height is None else dst_height))


def source_coordinates(cam, dtype=np.float64):
    """(sx, sy, coords) [dst_height, dst_width]: the map before quantisation, every operation rounded on its own in `dtype`, in the
    order of the header; coords: the pixel has coordinates (Z > 0 and sx, sy finite) - sx = sy = NaN where it has none."""
    f = {k: dtype(cam[k]) for k in CAMERA_KEYS}
    R = np.asarray(cam["R"], dtype=np.float64).reshape(9).astype(dtype)
    v, u = np.mgrid[0:cam["dst_height"], 0:cam["dst_width"]]
    u, v = u.astype(dtype), v.astype(dtype)
    one, two = dtype(1.0), dtype(2.0)
    with np.errstate(all="ignore"):
        xr, yr = (u - f["cx2"]) / f["fx2"], (v - f["cy2"]) / f["fy2"]
        X = (R[0] * xr + R[3] * yr) + R[6]
        Y = (R[1] * xr + R[4] * yr) + R[7]
        Z = (R[2] * xr + R[5] * yr) + R[8]
        pos = Z > 0
        Zs = np.where(pos, Z, one)
        x, y = X / Zs, Y / Zs
        r2 = x * x + y * y
        rad = one + r2 * (f["k1"] + r2 * (f["k2"] + r2 * f["k3"]))
        xd = x * rad + ((two * f["p1"]) * x * y + f["p2"] * (r2 + two * (x * x)))
        yd = y * rad + (f["p1"] * (r2 + two * (y * y)) + (two * f["p2"]) * x * y)
        sx, sy = f["fx"] * xd + f["cx"], f["fy"] * yd + f["cy"]
    coords = pos & np.isfinite(sx) & np.isfinite(sy)
    return np.where(coords, sx, dtype(np.nan)), np.where(coords, sy, dtype(np.nan)), coords


def make_map(cam):
    """dict(qx, qy int32, valid uint8, sx, sy float64, coords bool) [dst_height, dst_width]."""
    sx, sy, coords = source_coordinates(cam)
    w, h = cam["src_width"], cam["src_height"]
    out = {"sx": sx, "sy": sy, "coords": coords}
    with np.errstate(all="ignore"):
        for name, s, side in (("qx", sx, w), ("qy", sy, h)):
            q = np.floor(np.where(coords, s, 0.0) * float(SUB) + 0.5)
            q = np.clip(q, -float(SUB), float(SUB) * side).astype(np.int64)
            out[name] = np.where(coords, q, NO_COORD).astype(np.int32)
        valid = coords & (sx >= -0.5) & (sx < w - 0.5) & (sy >= -0.5) & (sy < h - 0.5)
    out["valid"] = valid.astype(np.uint8)
    return out


def remap(image, m, border_mode=CONSTANT, border_value=0):
    """The remapped uint8 image [dst_height, dst_width] of the source `image` under the map m: integers only."""
    img = np.asarray(image, dtype=np.uint8).astype(np.int64)
    h, w = img.shape
    qx, qy = m["qx"].astype(np.int64), m["qy"].astype(np.int64)
    ix, ax, iy, ay = qx >> SUBPIXEL_BITS, qx & (SUB - 1), qy >> SUBPIXEL_BITS, qy & (SUB - 1)
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    p = ((SUB - ax) * (SUB - ay) * img[y0, x0] + ax * (SUB - ay) * img[y0, x1] + (SUB - ax) * ay * img[y1, x0] + ax * ay * img[y1, x1]
         + 32768) >> 16
    assert p.max(initial=0) <= 255 and p.min(initial=0) >= 0
    valid = m["valid"] != 0
    if border_mode == CONSTANT:
        fill = ~valid
    else:
        fill = ~valid & (m["qx"] == NO_COORD)
    return np.where(fill, int(border_value), p).astype(np.uint8)


def smooth(image, radius, taps):
    """The separable integer Gaussian of the header over a uint8 image, both passes replicating at the image's border."""
    p = np.asarray(image, dtype=np.uint8).astype(np.int64)
    if radius == 0:
        return p.astype(np.uint8)
    t = [int(x) for x in taps]
    h, w = p.shape
    xs, ys = np.arange(w), np.arange(h)
    acc = t[0] * p
    for k in range(1, radius + 1):
        acc = acc + t[k] * (p[:, np.clip(xs - k, 0, w - 1)] + p[:, np.clip(xs + k, 0, w - 1)])
    hor = (acc + 32) >> 6
    assert hor.max(initial=0) < 65536 and acc.max(initial=0) < 2 ** 31
    acc = t[0] * hor
    for k in range(1, radius + 1):
        acc = acc + t[k] * (hor[np.clip(ys - k, 0, h - 1), :] + hor[np.clip(ys + k, 0, h - 1), :])
    assert acc.max(initial=0) + (1 << 21) < 2 ** 31
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def rectify(image, cam, border_mode=CONSTANT, border_value=0, radius=0, taps=(16384,), m=None):
    """dict(image, valid, num_valid) of one frame: remap, then the smoothing when radius > 0."""
    m = make_map(cam) if m is None else m
    out = smooth(remap(image, m, border_mode, border_value), radius, taps)
    return {"image": out, "valid": m["valid"], "num_valid": int(m["valid"].sum())}


def taps_restated(sigma):
    """(radius, taps [8]) as the header words them, with numpy's exp: the library's may differ by one unit where w 16384 / sum lies at
    a half."""
    t = np.zeros(8, dtype=np.int64)
    if sigma == 0:
        t[0] = 16384
        return 0, t
    r = int(min(MAX_RADIUS, max(1, np.ceil(3.0 * sigma))))
    w = np.exp(-np.arange(r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    total = w[0] + 2.0 * w[1:].sum()
    t[1:r + 1] = np.floor(w[1:] / total * 16384.0 + 0.5).astype(np.int64)
    t[0] = 16384 - 2 * t[1:].sum()
    return r, t


def stereo_rectify(left, right, R, t, dst_size=None, principal=None):
    """slslam_stereo_rectify restated.  left, right: dict(fx, fy, cx, cy, width, height[, k1 ..]); x_right = R x_left + t.  Returns
    dict(left, right: camera dicts; baseline; fx, fy, cx, cy)."""
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    c = -(R.T @ t)
    b = np.sqrt(c @ c)
    e1 = c / b
    e2 = np.array([-e1[1], e1[0], 0.0])
    e2 = e2 / np.sqrt(e2 @ e2)
    e3 = np.cross(e1, e2)
    Rl = np.stack([e1, e2, e3])
    Rr = Rl @ R.T
    f = ((left["fx"] + left["fy"]) + (right["fx"] + right["fy"])) / 4.0
    cx2, cy2 = (left["cx"], left["cy"]) if principal is None else principal
    dw, dh = (left["width"], left["height"]) if dst_size is None else dst_size
    cams = []
    for side, rot in ((left, Rl), (right, Rr)):
        cams.append(camera(side["width"], side["height"], dw, dh, fx=side["fx"], fy=side["fy"], cx=side["cx"], cy=side["cy"],
                           R=rot, fx2=f, fy2=f, cx2=cx2, cy2=cy2, **{k: side.get(k, 0.0) for k in ("k1", "k2", "p1", "p2", "k3")}))
    return dict(left=cams[0], right=cams[1], baseline=float(b), fx=float(f), fy=float(f), cx=float(cx2), cy=float(cy2))


def to_capi(cam):
    """The camera dict as a capi.RectifyCamera."""
    from slslam_amd import capi
    return capi.RectifyCamera.make(cam["src_width"], cam["src_height"], cam["dst_width"], cam["dst_height"], R=cam["R"],
                                   **{k: cam[k] for k in CAMERA_KEYS})

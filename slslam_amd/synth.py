"""Deterministic synthetic inputs for the hot path.

The reference's datasets are not shipped (reference README:18-26), so tests and benches feed the
solver the same five arrays `SLAM::bundle_adjustment` builds (reference src/slam.cpp:899-920)
from a synthetic stereo line scene:

* camera model / constants: reference src/parameter.h:43-52 (640x480, f=406.05, cx=327.783,
  cy=237.172, baseline 0.12 along +x), pixel -> normalised as src/slam.cpp:121-128
* window shape: 2W keyframes, the W newest free, the rest fixed (src/slam.cpp:813-814, 855-870),
  newest keyframe exactly identity (metric_embedding, src/slam.cpp:1322)
* landmark initialisation: stereo triangulation of the first observation
  (SLAM::initialize_lm, src/slam.cpp:190-219) then gc_av_to_orth (src/gc.cpp:361-379)
* observations grouped by line in keyframe order, as the packer emits them (src/slam.cpp:848-882)

Pure numpy; no oracle, no GPU.
"""
import numpy as np

FOCAL = 406.05
CX = 327.783
CY = 237.172
WIDTH = 640
HEIGHT = 480
BASELINE = 0.12
HUBER_DELTA = 1.0 / FOCAL
INVERSE_DEPTH = 0.1


# ----------------------------------------------------------------------------- rotations
def rodrigues(w):
    """angle-axis -> rotation matrix (ceres::AngleAxisToRotationMatrix semantics, gc.cpp:24-36)."""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K)


def log_so3(R):
    """rotation matrix -> angle-axis (gc_Rodriguez(Matrix3d), gc.cpp:38-49)."""
    q = np.empty(4)
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q[:] = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    sn = np.linalg.norm(q[1:])
    if sn < 1e-15:
        return 2.0 * q[1:]
    ang = 2.0 * (np.arctan2(-sn, -q[0]) if q[0] < 0 else np.arctan2(sn, q[0]))
    return q[1:] * (ang / sn)


def rt_to_wt(R, t):
    return np.concatenate([log_so3(R), t])


def wt_to_rt(wt):
    return rodrigues(wt[:3]), np.asarray(wt[3:6], dtype=np.float64)


def av_to_orth(av):
    """gc_av_to_orth, reference src/gc.cpp:361-379 (batched over leading dims)."""
    av = np.asarray(av, dtype=np.float64)
    a, v = av[..., :3], av[..., 3:]
    n = np.cross(a, v)
    nn = np.linalg.norm(n, axis=-1, keepdims=True)
    vn = np.linalg.norm(v, axis=-1, keepdims=True)
    x, y = n / nn, v / vn
    z = np.cross(x, y)
    o = np.empty(av.shape[:-1] + (4,))
    o[..., 0] = np.arctan2(y[..., 2], z[..., 2])
    o[..., 1] = np.arcsin(-x[..., 2])
    o[..., 2] = np.arctan2(x[..., 1], x[..., 0])
    o[..., 3] = np.arcsin(vn[..., 0] / np.sqrt(nn[..., 0] ** 2 + vn[..., 0] ** 2))
    return o


def orth_to_av(orth):
    """gc_orth_to_av, reference src/gc.cpp:419-442 (batched)."""
    orth = np.asarray(orth, dtype=np.float64)
    a, b, g, t = orth[..., 0], orth[..., 1], orth[..., 2], orth[..., 3]
    s1, c1, s2, c2, s3, c3 = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(g), np.cos(g)
    d = np.cos(t) / np.sin(t)
    av = np.empty(orth.shape[:-1] + (6,))
    av[..., 0] = -(c1 * s2 * c3 + s1 * s3) * d
    av[..., 1] = -(c1 * s2 * s3 - s1 * c3) * d
    av[..., 2] = -(c1 * c2) * d
    av[..., 3] = s1 * s2 * c3 - c1 * s3
    av[..., 4] = s1 * s2 * s3 + c1 * c3
    av[..., 5] = s1 * c2
    return av


# ----------------------------------------------------------------------------- scene
def _trajectory(rng, num_kf):
    """Gently curving planar path with sinusoidal heave; returns camera-to-world (Rwc, c) per KF,
    oldest first.  Spacing ~0.75 m / <=15 deg per keyframe (reference src/parameter.h:59-60)."""
    yaw_rate = np.deg2rad(rng.uniform(-4.0, 4.0))
    phase = rng.uniform(0, 2 * np.pi)
    Rwc, c = [], []
    pos = np.zeros(3)
    yaw = 0.0
    for k in range(num_kf):
        Ry = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        pitch = np.deg2rad(1.0) * np.sin(0.7 * k + phase)
        Rx = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
        R = Ry @ Rx
        p = pos.copy()
        p[1] += 0.05 * np.sin(0.9 * k + phase)
        Rwc.append(R)
        c.append(p)
        step = rng.uniform(0.6, 0.8)
        pos = pos + R[:, 2] * step
        yaw += yaw_rate + np.deg2rad(rng.normal(0, 0.5))
    return np.array(Rwc), np.array(c)


def _project(R, t, P):
    """world points P[...,3] -> (left px, right px, depth) for pose (R,t) world->camera."""
    Pc = P @ R.T + t
    z = Pc[..., 2]
    zl = np.where(np.abs(z) < 1e-9, 1e-9, z)
    ul = FOCAL * Pc[..., 0] / zl + CX
    vl = FOCAL * Pc[..., 1] / zl + CY
    ur = FOCAL * (Pc[..., 0] - BASELINE) / zl + CX
    return ul, vl, ur, z


def _initialize_lm(obs):
    """SLAM::initialize_lm (reference src/slam.cpp:190-219), batched over rows of obs[...,8]."""
    one = np.ones(obs.shape[:-1])
    p1 = np.stack([obs[..., 0], obs[..., 1], one], -1)
    p2 = np.stack([obs[..., 2], obs[..., 3], one], -1)
    p3 = np.stack([obs[..., 4] + BASELINE, obs[..., 5], one], -1)
    p4 = np.stack([obs[..., 6] + BASELINE, obs[..., 7], one], -1)
    o1 = np.zeros_like(p1)
    o2 = np.zeros_like(p1)
    o2[..., 0] = BASELINE

    def ppp(x1, x2, x3):  # gc_ppp_pi, gc.cpp:100-105
        n = np.cross(x1 - x3, x2 - x3)
        d = -np.sum(x3 * np.cross(x1, x2), -1)
        return np.concatenate([n, d[..., None]], -1)

    pi1, pi2 = ppp(p1, p2, o1), ppp(p3, p4, o2)
    dp = pi1[..., :, None] * pi2[..., None, :] - pi2[..., :, None] * pi1[..., None, :]
    n = np.stack([dp[..., 0, 3], dp[..., 1, 3], dp[..., 2, 3]], -1)            # gc_pipi_plk, gc.cpp:107-113
    v = np.stack([-dp[..., 1, 2], dp[..., 0, 2], -dp[..., 0, 1]], -1)
    cp = np.cross(v, n) / np.sum(v * v, -1, keepdims=True)                    # gc_plucker_origin
    cpn = np.linalg.norm(cp, axis=-1, keepdims=True)
    bad = (cpn < 0.1) | (cpn > 10.0)
    cp = np.where(bad, cp / cpn / INVERSE_DEPTH, cp)
    cp = np.where(cp[..., 2:3] < 0, -cp, cp)
    return np.concatenate([cp, v], -1)


def _camera_planes(ob):
    """The back-projected planes of the left and right segments of one observation, in its camera (gc_ppp_pi, gc.cpp:100-105)."""
    p1, p2 = np.array([ob[0], ob[1], 1.0]), np.array([ob[2], ob[3], 1.0])
    p3, p4 = np.array([ob[4] + BASELINE, ob[5], 1.0]), np.array([ob[6] + BASELINE, ob[7], 1.0])
    c = np.array([BASELINE, 0.0, 0.0])
    return (np.concatenate([np.cross(p1, p2), [0.0]]),
            np.concatenate([np.cross(p3 - c, p4 - c), [-np.dot(c, np.cross(p3, p4))]]))


def _multiview_lm(obs, Rs, ts, cp0, v0):
    """The linear multi-view start of one line (the algorithm of tests/lba_triangulate_reference.py with
    min_parallax = 0): the best-fitting pencil of the back-projected planes of all its observations obs[n, 8] under their cameras
    (Rs[n], ts[n]) - the two leading eigenvectors of the Gram matrix of the unit-normal world planes -, direction signed like the
    stereo-first line (cp0, v0), which a line with one observation or a non-finite fit keeps."""
    G = np.zeros((4, 4))
    for ob, R, t in zip(obs, Rs, ts):
        for pi in _camera_planes(ob):
            nw = R.T @ pi[:3]
            nn = np.sqrt(np.dot(nw, nw))
            if nn > 0.0:
                pw = np.concatenate([nw, [np.dot(pi[:3], t) + pi[3]]]) / nn
                G += np.outer(pw, pw)
    lam, vec = np.linalg.eigh(G)
    dp = np.outer(vec[:, 3], vec[:, 2]) - np.outer(vec[:, 2], vec[:, 3])     # gc_pipi_plk, gc.cpp:107-113
    n = np.array([dp[0, 3], dp[1, 3], dp[2, 3]])
    v = np.array([-dp[1, 2], dp[0, 2], -dp[0, 1]])
    with np.errstate(all="ignore"):
        cp = np.cross(v, n) / np.dot(v, v)                                    # gc_plucker_origin
    if np.dot(v, v0) < 0:
        v = -v
    if len(obs) < 2 or not (np.isfinite(cp).all() and np.isfinite(v).all() and np.isfinite(lam).all()):
        return cp0, v0
    return cp, v


def make_window(seed, num_lines=2000, num_kf=20, num_free=10, noise_px=0.5,
                pose_sigma_t=0.01, pose_sigma_r_deg=0.3, all_free=False,
                line_init="perturb", line_sigma_rel=0.01, line_sigma_dir_deg=0.5, mean_track=9.0):
    """One sliding-window LBA problem in the reference array contract.

    Returns a dict with the five arrays of src/slam.cpp:899-920 (`camera_index`, `line_index`,
    `fixed_index` [2M], `observations` [M,8], `parameters` [6C+4L]), sizes, and ground truth
    (`true_parameters`) for trajectory-error reporting.  Cameras 0..num_free-1 are the free
    keyframes (oldest..newest; the newest is exactly identity), the rest are the fixed ones.

    A line is tracked over a contiguous run of keyframes (mean length `mean_track`) inside its
    geometric visibility, which gives the M ~ 6 L of a real window.  `line_init`:
    "perturb" = landmarks already refined by earlier windows (truth + small error; the
    reference's windows start within a few % of their optimum cost);
    "triangulate" = every landmark freshly initialised from its first stereo observation
    (SLAM::initialize_lm) - the hard, far-from-optimum case;
    "multiview" = every landmark from all its observations under the window's (perturbed) cameras: the linear start the line
    triangulator makes (slslam_line_triangulator_run, method 1, min_parallax 0).
    """
    if (num_kf if all_free else min(num_free, num_kf)) < 2:
        raise ValueError("a window line must be seen by >= 2 free keyframes (slam.cpp:839-840): num_free >= 2; "
                         "the 1-free-camera shape is make_motion_only()")
    rng = np.random.default_rng(np.random.SeedSequence([4, int(seed)]))   # rseed=4: main.cpp:26
    Rwc, cw = _trajectory(rng, num_kf)
    # re-root on the newest keyframe: world := newest camera frame
    Rn, cn = Rwc[-1], cw[-1]
    R_wc = np.einsum("ij,kjl->kil", Rn.T, Rwc)          # cam k -> new world
    c_w = (cw - cn) @ Rn
    R_cw = np.transpose(R_wc, (0, 2, 1))                # world -> camera (the reference's T.R)
    t_cw = -np.einsum("kij,kj->ki", R_cw, c_w)
    R_cw[-1] = np.eye(3)
    t_cw[-1] = 0.0
    if all_free:
        num_free = num_kf
    order = list(range(num_kf - num_free, num_kf)) + list(range(0, num_kf - num_free))  # cam idx -> kf
    kf_to_cam = np.empty(num_kf, dtype=np.int64)
    kf_to_cam[order] = np.arange(num_kf)

    # ---- lines: segments placed in the frustum union, kept if seen by >= 2 free keyframes
    ends_a, ends_b, vis_all = [], [], []
    have = 0
    while have < num_lines:
        n = max(256, 2 * (num_lines - have))
        kf = rng.integers(0, num_kf, n)
        u = rng.uniform(0, WIDTH, n)
        v = rng.uniform(0, HEIGHT, n)
        z = rng.uniform(2.0, 10.0, n)
        mid_c = np.stack([(u - CX) / FOCAL * z, (v - CY) / FOCAL * z, z], -1)
        mid_w = np.einsum("nij,nj->ni", R_wc[kf], mid_c) + c_w[kf]
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        half = 0.5 * rng.uniform(0.5, 3.0, n)[:, None]
        A, B = mid_w - d * half, mid_w + d * half
        vis = np.zeros((n, num_kf), dtype=bool)
        for k in range(num_kf):
            ok = np.ones(n, dtype=bool)
            for P in (A, B):
                ul, vl, ur, zz = _project(R_cw[k], t_cw[k], P)
                ok &= (zz > 0.5) & (ul >= 0) & (ul < WIDTH) & (ur >= 0) & (ur < WIDTH) & (vl >= 0) & (vl < HEIGHT)
            vis[:, k] = ok
        # tracker model: a contiguous run of keyframes around the seeding keyframe
        length = 2 + rng.poisson(max(mean_track - 2.0, 0.0), n)
        start = kf - rng.integers(0, length)
        kk = np.arange(num_kf)[None, :]
        vis &= (kk >= start[:, None]) & (kk < (start + length)[:, None])
        keep = vis[:, num_kf - num_free:].sum(1) >= 2                      # slam.cpp:839-840
        ends_a.append(A[keep]); ends_b.append(B[keep]); vis_all.append(vis[keep])
        have += int(keep.sum())
    A = np.concatenate(ends_a)[:num_lines]
    B = np.concatenate(ends_b)[:num_lines]
    vis = np.concatenate(vis_all)[:num_lines]

    # ---- noisy observations, grouped by line, keyframes in time order
    li, ki = np.nonzero(vis)                                               # row-major: by line, then kf
    M = len(li)
    obs = np.empty((M, 8))
    for k in range(num_kf):
        sel = ki == k
        if not sel.any():
            continue
        for e, P in enumerate((A, B)):
            ul, vl, ur, _ = _project(R_cw[k], t_cw[k], P[li[sel]])
            obs[sel, 2 * e] = ul
            obs[sel, 2 * e + 1] = vl
            obs[sel, 4 + 2 * e] = ur
            obs[sel, 4 + 2 * e + 1] = vl
    obs += rng.normal(0, noise_px, obs.shape) if noise_px > 0 else 0.0
    obs[:, 0::2] = (obs[:, 0::2] - CX) / FOCAL                             # slam.cpp:121-128
    obs[:, 1::2] = (obs[:, 1::2] - CY) / FOCAL

    # ---- parameters: true and perturbed poses
    true_cams = np.array([rt_to_wt(R_cw[k], t_cw[k]) for k in order])
    init_R, init_t = R_cw.copy(), t_cw.copy()
    for k in range(num_kf - num_free, num_kf - 1):                        # newest stays identity
        dw = rng.normal(0, np.deg2rad(pose_sigma_r_deg), 3)
        init_R[k] = rodrigues(dw) @ R_cw[k]
        init_t[k] = t_cw[k] + rng.normal(0, pose_sigma_t, 3)
    init_cams = np.array([rt_to_wt(init_R[k], init_t[k]) for k in order])

    # true lines: closest point + direction in the world frame
    dvec = (B - A) / np.linalg.norm(B - A, axis=1, keepdims=True)
    cp = A - np.sum(A * dvec, 1, keepdims=True) * dvec
    true_lines = av_to_orth(np.concatenate([cp, dvec], 1))
    # initial lines: triangulate the first observation in its keyframe, move to the world with
    # that keyframe's CURRENT (perturbed) pose: gc_line_from_pose(lm->line, init_kf->T), slam.cpp:884-886
    first = np.r_[True, li[1:] != li[:-1]]
    lm_c = _initialize_lm(obs[first])
    kf0 = ki[first]
    Rinv = np.transpose(init_R[kf0], (0, 2, 1))
    cp_w = np.einsum("nij,nj->ni", Rinv, lm_c[:, :3] - init_t[kf0])
    dv_w = np.einsum("nij,nj->ni", Rinv, lm_c[:, 3:])
    init_lines = av_to_orth(np.concatenate([cp_w, dv_w], 1))
    if line_init == "perturb":
        depth = np.linalg.norm(cp, axis=1, keepdims=True) + 1.0
        cp_p = cp + rng.normal(size=cp.shape) * line_sigma_rel * depth
        dw = rng.normal(0, np.deg2rad(line_sigma_dir_deg), cp.shape)
        dv_p = dvec + np.cross(dw, dvec)
        dv_p /= np.linalg.norm(dv_p, axis=1, keepdims=True)
        cp_p = cp_p - np.sum(cp_p * dv_p, 1, keepdims=True) * dv_p
        init_lines = av_to_orth(np.concatenate([cp_p, dv_p], 1))
    elif line_init == "multiview":
        starts = np.nonzero(first)[0].tolist() + [M]
        mv = [_multiview_lm(obs[a:b], init_R[ki[a:b]], init_t[ki[a:b]], cp_w[l], dv_w[l])
              for l, (a, b) in enumerate(zip(starts[:-1], starts[1:]))]
        init_lines = av_to_orth(np.array([np.concatenate(m) for m in mv]))
    elif line_init != "triangulate":
        raise ValueError(line_init)

    cam_idx = kf_to_cam[ki].astype(np.int32)
    fixed = np.zeros((M, 2), dtype=np.int32)
    fixed[:, 0] = cam_idx >= num_free                                      # slam.cpp:855-870
    return {
        "num_cameras": num_kf, "num_lines": num_lines, "num_free_cameras": num_free,
        "camera_index": cam_idx, "line_index": li.astype(np.int32),
        "fixed_index": fixed.reshape(-1), "observations": obs,
        "parameters": np.concatenate([init_cams.reshape(-1), init_lines.reshape(-1)]),
        "true_parameters": np.concatenate([true_cams.reshape(-1), true_lines.reshape(-1)]),
        "baseline": BASELINE, "seed": int(seed),
    }


def make_motion_only(seed, num_lines=100, noise_px=0.5):
    """The motion_only_ba shape (reference src/slam.cpp:578-675): camera 0 = current estimate
    (free), camera 1 = identity (fixed), every line fixed, two observations per line."""
    w = make_window(seed, num_lines=num_lines, num_kf=2, num_free=2, noise_px=noise_px)
    M = len(w["camera_index"])
    # make_window orders cams oldest..newest with the newest = identity -> cam 1 is identity
    fixed = np.empty((M, 2), dtype=np.int32)
    fixed[:, 0] = w["camera_index"] == 1
    fixed[:, 1] = 1
    w["fixed_index"] = fixed.reshape(-1)
    w["num_free_cameras"] = 1
    return w


def make_pose_graph(seed, num_poses=260, num_loops=8, sigma_t=0.01, sigma_r_deg=0.2):
    """Closed-loop pose graph in the POProblem array contract (reference src/slam.cpp:1248-1280):
    sorted edge set (edge 0 = (0,1) fixes pose 0), constraints C = T_{n2<-n1}, parameters from
    dead-reckoned odometry (drift), loop-closure edges near the start/end of the loop."""
    rng = np.random.default_rng(np.random.SeedSequence([5, int(seed)]))
    N = num_poses
    radius = 0.75 * N / (2 * np.pi)
    Rs, ts = [], []
    for k in range(N):
        ang = 2 * np.pi * k / N
        c = np.array([radius * np.sin(ang), 0.05 * np.sin(5 * ang), radius * (1 - np.cos(ang))])
        yaw = ang
        Rwc = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        Rs.append(Rwc.T)
        ts.append(-Rwc.T @ c)
    # re-root on the last pose like metric_embedding (slam.cpp:1239-1240)? keep pose 0 = identity
    # frame: the reference re-roots on the newest kf; either way pose 0 is the gauge.
    edges = {}
    est_R, est_t = [Rs[0]], [ts[0]]
    for k in range(N - 1):
        Rrel = Rs[k + 1] @ Rs[k].T
        trel = ts[k + 1] - Rrel @ ts[k]
        Rn = rodrigues(rng.normal(0, np.deg2rad(sigma_r_deg), 3)) @ Rrel
        tn = trel + rng.normal(0, sigma_t, 3)
        edges[(k, k + 1)] = (Rn, tn)
        est_R.append(Rn @ est_R[k])
        est_t.append(Rn @ est_t[k] + tn)
    loops = 0
    cand = [(i, N - 1 - j) for i in range(0, 12) for j in range(0, 12)]
    rng.shuffle(cand)
    for (a, b) in cand:
        if loops >= num_loops:
            break
        if (a, b) in edges or a >= b:
            continue
        Rrel = Rs[b] @ Rs[a].T
        trel = ts[b] - Rrel @ ts[a]
        edges[(a, b)] = (rodrigues(rng.normal(0, np.deg2rad(0.05), 3)) @ Rrel, trel + rng.normal(0, 0.002, 3))
        loops += 1
    keys = sorted(edges.keys())                                            # std::set<pii> order
    p1 = np.array([k[0] for k in keys], dtype=np.int32)
    p2 = np.array([k[1] for k in keys], dtype=np.int32)
    cons = np.array([rt_to_wt(*edges[k]) for k in keys])
    params = np.array([rt_to_wt(est_R[k], est_t[k]) for k in range(N)])
    truth = np.array([rt_to_wt(Rs[k], ts[k]) for k in range(N)])
    return {"num_poses": N, "pose_index_1": p1, "pose_index_2": p2, "constraints": cons,
            "parameters": params.reshape(-1), "true_parameters": truth.reshape(-1), "seed": int(seed)}


def make_edge_information(seed, g, s_min=0.5, s_max=2.0, off_diagonal=0.3):
    """Square-root information matrices for the edges of a pose graph (g["sqrt_information"]; an extension the reference does not
    have): [E, 6, 6], W_e = R_e diag(s_e) T_e with R_e a random orthogonal 6 x 6, s_e in [s_min, s_max] and T_e unit lower triangular
    with off-diagonals in [-off_diagonal, off_diagonal].  Full, NOT symmetric and O(1): a transposed or column-major read is a
    different problem, and the conditioning of the graph stays what it was."""
    rng = np.random.default_rng(np.random.SeedSequence([11, int(seed)]))
    E = len(g["pose_index_1"])
    W = np.zeros((E, 6, 6))
    for e in range(E):
        q, r = np.linalg.qr(rng.normal(size=(6, 6)))
        q = q * np.sign(np.diag(r))                                        # (the factorisation's sign convention taken out)
        t = np.eye(6) + np.tril(rng.uniform(-off_diagonal, off_diagonal, (6, 6)), -1)
        W[e] = q @ np.diag(rng.uniform(s_min, s_max, 6)) @ t
    return W


def camera_centers(cams):
    """camera centres c = -R^T t of a [C,6] pose array (for trajectory-error reporting,
    reference matlab_script/calc_traj_err.m:28-40)."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 6)
    return np.array([-(rodrigues(c[:3]).T @ c[3:]) for c in cams])


def make_ransac_frame(seed, num_lines=150, num_hypotheses=256, noise_px=0.5):
    """Inputs of the RANSAC scoring loop (reference src/slam.cpp:396-413): the lines common to two
    frames in the previous keyframe's frame (world), their observations in the CURRENT frame, and a
    set of motion hypotheses around the true motion (some exact, some perturbed, some with |t| > 1
    which the reference skips).  Returns (poses [H,12] = R row-major | t, observations [K,8], lines [K,6],
    true_pose [12])."""
    rng = np.random.default_rng(np.random.SeedSequence([6, int(seed)]))
    w = make_window(seed, num_lines=num_lines, num_kf=2, num_free=2, noise_px=noise_px, mean_track=50.0)
    prm = w["true_parameters"]
    lines = orth_to_av(prm[12:].reshape(-1, 4))
    sel = w["camera_index"] == 0                      # camera 0 = the moving (current) frame, camera 1 = identity
    obs = np.zeros((num_lines, 8))
    has = np.zeros(num_lines, dtype=bool)
    obs[w["line_index"][sel]] = w["observations"][sel]
    has[w["line_index"][sel]] = True
    R, t = wt_to_rt(prm[:6])
    poses = []
    for h in range(num_hypotheses):
        s = [0.0, 1e-3, 1e-2, 0.1, 2.0][h % 5] * (1.0 if h < 5 else rng.uniform(0.2, 1.5))
        Rh = rodrigues(rng.normal(size=3) * 0.3 * s) @ R
        th = t + rng.normal(size=3) * s
        poses.append(np.concatenate([Rh.reshape(-1), th]))
    return np.array(poses), obs[has], lines[has], np.concatenate([R.reshape(-1), t])


def make_ransac_pair(seed, num_lines=150, noise_px=0.5, outlier_frac=0.2, num_trials=64, sample_size=5,
                     rot_deg=1.0, step_m=0.15):
    """Inputs of SLAM::ransac_motion (reference src/slam.cpp:322-427): the lines common to the previous
    and the current frame (world = previous frame), their stereo observations in both frames (a
    fraction of the current ones corrupted: wrong matches), and a pre-drawn sample sequence
    (rand.rand_sample draws sample_size distinct indices per trial).  Frame-to-frame motion is small
    (the generator linearises the rotation).  Returns dict(obs0, obs1, lines, samples, true_pose)."""
    rng = np.random.default_rng(np.random.SeedSequence([7, int(seed)]))
    # a dedicated small-motion pair: previous frame = identity, current frame = small motion
    wv = rng.normal(size=3) * np.deg2rad(rot_deg)
    tv = rng.normal(size=3) * step_m * np.array([0.3, 0.1, 1.0])
    R = rodrigues(wv)
    f, cx, cy, B = 406.05, 327.783, 237.172, 0.12
    obs0, obs1, lines = [], [], []
    while len(lines) < num_lines:
        c = np.array([rng.uniform(-4, 4), rng.uniform(-2, 2), rng.uniform(2.5, 10)])
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        h = rng.uniform(0.25, 1.5)
        P = np.stack([c - h * d, c + h * d])
        ok, rec = True, []
        for (Rc, tc) in ((np.eye(3), np.zeros(3)), (R, tv)):
            o = []
            for k in range(2):
                Q = (Rc @ P.T).T + tc - np.array([k * B, 0, 0])
                if np.any(Q[:, 2] < 0.5):
                    ok = False
                px = np.stack([f * Q[:, 0] / Q[:, 2] + cx, f * Q[:, 1] / Q[:, 2] + cy], axis=1)
                if np.any(px[:, 0] < 0) or np.any(px[:, 0] > 640) or np.any(px[:, 1] < 0) or np.any(px[:, 1] > 480):
                    ok = False
                px = px + rng.normal(size=(2, 2)) * noise_px
                o.append(((px - [cx, cy]) / f).reshape(-1))
            rec.append(np.concatenate(o))
        if not ok:
            continue
        dv = (P[1] - P[0]) / np.linalg.norm(P[1] - P[0])
        cp = P[0] - dv * (P[0] @ dv)
        obs0.append(rec[0]); obs1.append(rec[1]); lines.append(np.concatenate([cp, dv]))
    obs0, obs1, lines = np.array(obs0), np.array(obs1), np.array(lines)
    bad = rng.random(num_lines) < outlier_frac
    obs1[bad] += rng.normal(size=(int(bad.sum()), 8)) * 0.05
    samples = np.stack([rng.choice(num_lines, size=sample_size, replace=False) for _ in range(num_trials)]).astype(np.int32)
    return dict(obs0=obs0, obs1=obs1, lines=lines, samples=samples, true_pose=np.concatenate([R.reshape(-1), tv]),
                outliers=bad)


def make_voctree(seed, K, L, D):
    """A seeded random vocabulary tree: the interior nodes [(K^L - 1) / (K - 1), K, D] float32 (breadth-first, as slslam_voctree_create
    takes them), every centre of unit norm.  Stands in for the tree file the reference does not ship."""
    rng = np.random.default_rng(np.random.SeedSequence([12, int(seed)]))
    c = rng.standard_normal(((K ** L - 1) // (K - 1), K, D))
    return (c / np.linalg.norm(c, axis=2, keepdims=True)).astype(np.float32)


def make_place_sequence(seed, places=60, words_per_place=40, noise=0.05, revisit=(10, 25), dim=16):
    """Descriptors of a walk that passes `places` distinct places, one keyframe each, and then revisits places revisit[0] ..
    revisit[1] - 1 in the same order.  A place is words_per_place random unit vectors of `dim` floats; a visit sees each of them with
    Gaussian noise of that standard deviation per component, renormalised.  Returns dict(frames: list of [words_per_place, dim] float32,
    place: the place of every keyframe, first_pass: places)."""
    rng = np.random.default_rng(np.random.SeedSequence([13, int(seed)]))
    base = rng.standard_normal((places, words_per_place, dim))
    base /= np.linalg.norm(base, axis=2, keepdims=True)
    order = list(range(places)) + list(range(int(revisit[0]), int(revisit[1])))
    frames = []
    for p in order:
        d = base[p] + noise * rng.standard_normal((words_per_place, dim))
        frames.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return {"frames": frames, "place": np.array(order, dtype=np.int32), "first_pass": places}


def make_descriptor_pair(seed, n=150, dim=72, noise=0.03, outliers=0):
    """Two views of the same n random unit descriptors of `dim` floats - a keyframe and a later frame that sees the same features -,
    each with Gaussian noise of that standard deviation per component, renormalised, each with `outliers` further descriptors the other
    view does not hold, each in a shuffled order of its own.  Returns dict(query [n + outliers, dim] float32, keyframe likewise,
    query_id / keyframe_id: the feature (0 .. n-1) a row shows, -1 for an outlier, truth [n + outliers]: the keyframe row that shows
    the feature of query row a, -1 for an outlier)."""
    rng = np.random.default_rng(np.random.SeedSequence([14, int(seed)]))
    n, o = int(n), int(outliers)
    base = rng.standard_normal((n, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    views, ids = [], []
    for _ in range(2):
        d = np.concatenate([base + noise * rng.standard_normal((n, dim)), rng.standard_normal((o, dim))])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        perm = rng.permutation(n + o)
        views.append(d[perm].astype(np.float32))
        ids.append(np.where(perm < n, perm, -1).astype(np.int32))
    row_of = np.full(n + 1, -1, dtype=np.int32)                 # feature -> keyframe row (the last entry: an outlier's -1)
    kf_rows = np.nonzero(ids[1] >= 0)[0]
    row_of[ids[1][kf_rows]] = kf_rows
    return {"query": views[0], "keyframe": views[1], "query_id": ids[0], "keyframe_id": ids[1],
            "truth": row_of[ids[0]]}


def _line_scene(seed, height, width, num_segments, min_length, max_length, margin):
    """A grey scene as a function of the plane: sinusoidal texture plus one soft edge per segment, each edge a smoothed step across its
    segment that fades out beyond the segment's ends and away from its line."""
    rng = np.random.default_rng(np.random.SeedSequence([16, int(seed)]))
    n = int(num_segments)
    lo_x, hi_x, lo_y, hi_y = margin, width - 1 - margin, margin, height - 1 - margin
    if hi_x <= lo_x or hi_y <= lo_y:
        raise ValueError("the margin leaves no room in the image")
    seg = np.zeros((n, 4))
    for i in range(n):
        while True:
            length = rng.uniform(min_length, max_length)
            th = rng.uniform(0.0, 2.0 * np.pi)
            c = np.array([rng.uniform(lo_x, hi_x), rng.uniform(lo_y, hi_y)])
            h = 0.5 * length * np.array([np.cos(th), np.sin(th)])
            p = np.concatenate([c - h, c + h])
            if lo_x <= p[[0, 2]].min() and p[[0, 2]].max() <= hi_x and lo_y <= p[[1, 3]].min() and p[[1, 3]].max() <= hi_y:
                seg[i] = p
                break
    return {"segments": seg,
            "amplitude": rng.uniform(25.0, 60.0, n) * rng.choice([-1.0, 1.0], n), "softness": rng.uniform(0.8, 2.5, n),
            "reach": rng.uniform(4.0, 10.0, n),
            "waves": np.stack([rng.uniform(0.05, 0.45, 6), rng.uniform(0.0, 2.0 * np.pi, 6), rng.uniform(0.0, 2.0 * np.pi, 6),
                               rng.uniform(5.0, 11.0, 6)], axis=1)}                     # frequency (rad / px), direction, phase, amplitude


def _render_scene(scene, height, width, shift=(0.0, 0.0), gain=1.0, offset=0.0):
    """uint8 [height, width]: gain * scene(x - shift.x, y - shift.y) + offset at the pixel centres, rounded and clipped."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = xx - shift[0], yy - shift[1]
    val = np.full((height, width), 118.0)
    for k, th, ph, a in scene["waves"]:
        val += a * np.sin(k * (np.cos(th) * u + np.sin(th) * v) + ph)
    for (x0, y0, x1, y1), amp, soft, reach in zip(scene["segments"], scene["amplitude"], scene["softness"], scene["reach"]):
        pad = 4.0 * reach + 8.0                                                        # beyond it the edge has faded to nothing
        c0 = max(int(np.floor(min(x0, x1) + shift[0] - pad)), 0), max(int(np.floor(min(y0, y1) + shift[1] - pad)), 0)
        c1 = min(int(np.ceil(max(x0, x1) + shift[0] + pad)) + 1, width), min(int(np.ceil(max(y0, y1) + shift[1] + pad)) + 1, height)
        if c1[0] <= c0[0] or c1[1] <= c0[1]:
            continue
        du, dv = u[c0[1]:c1[1], c0[0]:c1[0]] - 0.5 * (x0 + x1), v[c0[1]:c1[1], c0[0]:c1[0]] - 0.5 * (y0 + y1)
        length = np.hypot(x1 - x0, y1 - y0)
        ex, ey = (x1 - x0) / length, (y1 - y0) / length
        along, across = du * ex + dv * ey, dv * ex - du * ey
        fade = 0.5 * (1.0 + np.tanh((0.5 * length + 2.0 - np.abs(along)) / 2.0)) * np.exp(-0.5 * (across / reach) ** 2)
        val[c0[1]:c1[1], c0[0]:c1[0]] += amp * np.tanh(across / soft) * fade
    return np.clip(np.rint(gain * val + offset), 0, 255).astype(np.uint8)


def make_line_image(seed, height, width, num_segments, min_length=12.0, max_length=80.0, margin=26.0):
    """A seeded grey image of soft edges over sinusoidal texture, and the line segments that follow the edges: every segment lies on the
    edge that was drawn for it, at least `margin` pixels inside the image, between min_length and max_length pixels long, at sub-pixel
    end points.  Stands in for a camera image and a line detector.  Returns dict(image uint8 [height, width], segments [n, 4] float32
    (x0, y0, x1, y1))."""
    scene = _line_scene(seed, height, width, num_segments, min_length, max_length, margin)
    return {"image": _render_scene(scene, height, width), "segments": scene["segments"].astype(np.float32)}


def make_line_image_pair(seed, height, width, num_segments, shift=(2.3, -1.6), gain=0.8, offset=15.0, **kw):
    """make_line_image and a second view of the same scene: moved by a sub-pixel `shift` (x, y), its grey values gain * I + offset, its
    segments moved along and listed in a shuffled order.  Returns dict(image, segments: the first view; image2, segments2: the second;
    truth [n]: the row of segments2 that shows segment a of the first view)."""
    kw.setdefault("margin", 26.0)
    scene = _line_scene(seed, height, width, num_segments, kw.get("min_length", 12.0), kw.get("max_length", 80.0),
                        kw["margin"] + max(abs(shift[0]), abs(shift[1])))
    rng = np.random.default_rng(np.random.SeedSequence([17, int(seed)]))
    perm = rng.permutation(int(num_segments))                                          # row b of the second view shows segment perm[b]
    moved = scene["segments"] + np.array([shift[0], shift[1], shift[0], shift[1]])
    truth = np.empty(int(num_segments), dtype=np.int32)
    truth[perm] = np.arange(int(num_segments), dtype=np.int32)
    return {"image": _render_scene(scene, height, width), "segments": scene["segments"].astype(np.float32),
            "image2": _render_scene(scene, height, width, shift, gain, offset), "segments2": moved[perm].astype(np.float32),
            "truth": truth}


def make_edge_image(height, width, segments, amplitude=60.0, softness=1.5, reach=6.0):
    """A grey image of clean edges on a flat background, with no texture: per segment (x0, y0, x1, y1) a smoothed step of +-amplitude
    grey levels across its line, amplitude tanh(across / softness), that runs between exactly the end points given and fades out within
    about a pixel beyond them and, across the line, with a Gaussian of `reach` pixels.  The profile is antisymmetric about the line, so
    the gradient's weight is centred on it: analytic ground truth for a detector.  amplitude and softness are scalars or one value per
    segment; the peak gradient is amplitude / softness grey levels per pixel.  Returns uint8 [height, width]."""
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    amp = np.broadcast_to(np.asarray(amplitude, dtype=np.float64), (len(seg),))
    soft = np.broadcast_to(np.asarray(softness, dtype=np.float64), (len(seg),))
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    val = np.full((height, width), 118.0)
    for (x0, y0, x1, y1), a, s in zip(seg, amp, soft):
        length = np.hypot(x1 - x0, y1 - y0)
        ex, ey = (x1 - x0) / length, (y1 - y0) / length
        du, dv = u - 0.5 * (x0 + x1), v - 0.5 * (y0 + y1)
        along, across = du * ex + dv * ey, dv * ex - du * ey
        fade = 0.5 * (1.0 + np.tanh(0.5 * length - np.abs(along))) * np.exp(-0.5 * (across / reach) ** 2)
        val += a * np.tanh(across / s) * fade
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def make_stereo_line_pair(seed, height, width, num_segments, disparity=(4.0, 24.0), slant=0.05, gain=0.8, offset=15.0,
                          min_length=12.0, max_length=80.0, margin=26.0):
    """A rectified stereo pair of one make_line_image scene.  Every segment gets a disparity per end point - d0, d1 inside
    `disparity` = (lo, hi), their difference at most `slant` pixels per pixel of the segment's length -: the right segment has the
    same rows and x_right = x_left - d.  The texture of the right view is shifted by the mean disparity, its grey values are
    gain * I + offset, and its segments are listed in a shuffled order.  Left segments keep `margin` + hi pixels from the border, so
    the right ones keep `margin`.  Returns dict(left, right: uint8 [height, width]; left_segments, right_segments [n, 4] float32;
    disparity [n, 2]: d0, d1 of left segment a; truth [n]: the row of right_segments that shows left segment a)."""
    lo, hi = float(disparity[0]), float(disparity[1])
    if not 0.0 <= lo <= hi:
        raise ValueError("disparity = (lo, hi) with 0 <= lo <= hi")
    n = int(num_segments)
    scene = _line_scene(seed, height, width, n, min_length, max_length, margin + hi)
    rng = np.random.default_rng(np.random.SeedSequence([18, int(seed)]))
    seg = scene["segments"]
    length = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1])
    base = rng.uniform(lo, hi, n)
    half = 0.5 * rng.uniform(-slant, slant, n) * length
    d = np.clip(np.stack([base - half, base + half], axis=1), lo, hi)
    perm = rng.permutation(n)                                                          # row b of the right view shows segment perm[b]
    mean = float(d.mean()) if n else 0.0
    right = seg - np.stack([d[:, 0], np.zeros(n), d[:, 1], np.zeros(n)], axis=1)
    # the right scene in scene coordinates: rendered with shift (-mean, 0), which moves its texture and puts its segments at `right`
    scene2 = dict(scene, segments=right + np.array([mean, 0.0, mean, 0.0]))
    truth = np.empty(n, dtype=np.int32)
    truth[perm] = np.arange(n, dtype=np.int32)
    return {"left": _render_scene(scene, height, width), "right": _render_scene(scene2, height, width, (-mean, 0.0), gain, offset),
            "left_segments": seg.astype(np.float32), "right_segments": right[perm].astype(np.float32), "disparity": d, "truth": truth}


def make_line_sequence(seed, height, width, num_segments, num_frames, shifts, drop=0.15, disparity=None, gain=0.8, offset=15.0,
                       min_length=12.0, max_length=80.0, margin=26.0):
    """A sequence of views of one make_line_image scene for a tracker.  Frame t shows the scene moved by the sub-pixel shifts[t] =
    (x, y) - shifts: [num_frames, 2] -; every segment is absent from (not drawn in) a frame with probability `drop`, never from
    frame 0; the rows of every frame are listed in a shuffled order.  disparity = d > 0 adds a rectified right view per frame: the
    same frame's scene moved a further d pixels to the left, its grey values gain * I + offset, its rows shuffled on their own.
    Segments keep `margin` pixels from the border in every view.  Returns dict(images: uint8 [height, width] per frame; segments:
    [n_t, 4] float32 per frame; labels: [n_t] int32 per frame, the scene's segment - the true track - of every row; with a disparity
    also right_images, right_segments, right_labels)."""
    shifts = np.asarray(shifts, dtype=np.float64).reshape(int(num_frames), 2)
    d = 0.0 if disparity is None else float(disparity)
    if d < 0.0:
        raise ValueError("disparity >= 0")
    reach = float(np.abs(shifts).max()) if len(shifts) else 0.0
    scene = _line_scene(seed, height, width, num_segments, min_length, max_length, margin + reach + d)
    rng = np.random.default_rng(np.random.SeedSequence([19, int(seed)]))
    n = int(num_segments)
    out = {"images": [], "segments": [], "labels": []}
    if disparity is not None:
        out.update(right_images=[], right_segments=[], right_labels=[])
    for t in range(int(num_frames)):
        here = np.nonzero((rng.uniform(size=n) >= drop) | (t == 0))[0]
        part = dict(scene, **{k: scene[k][here] for k in ("segments", "amplitude", "softness", "reach")})
        sx, sy = shifts[t]
        rows = rng.permutation(len(here))
        out["images"].append(_render_scene(part, height, width, (sx, sy)))
        out["segments"].append((part["segments"][rows] + np.array([sx, sy, sx, sy])).astype(np.float32))
        out["labels"].append(here[rows].astype(np.int32))
        if disparity is not None:
            rows = rng.permutation(len(here))
            out["right_images"].append(_render_scene(part, height, width, (sx - d, sy), gain, offset))
            out["right_segments"].append((part["segments"][rows] + np.array([sx - d, sy, sx - d, sy])).astype(np.float32))
            out["right_labels"].append(here[rows].astype(np.int32))
    return out


def _undistort(xd, yd, k1, k2, p1, p2, k3, iterations=30):
    """The inverse of the Brown-Conrady model by fixed-point iteration: the undistorted normalised point of a distorted one."""
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x, y


def _rectifying_rotations(R, t):
    """Fusiello's construction (include/slslam_hip.h: slslam_stereo_rectify) for x_right = R x_left + t: (the left camera's rotation
    into the rectified frame, the right camera's, the baseline)."""
    c = -(R.T @ t)
    b = np.sqrt(c @ c)
    e1 = c / b
    e2 = np.array([-e1[1], e1[0], 0.0])
    e2 /= np.sqrt(e2 @ e2)
    Rl = np.stack([e1, e2, np.cross(e1, e2)])
    return Rl, Rl @ R.T, float(b)


def make_raw_stereo_pair(seed, height=160, width=224, num_segments=8, disparity=(4.0, 14.0), background_disparity=2.5,
                         focal=None, distortion=((-0.28, 0.09, 0.0012, -0.0009, -0.01), (-0.24, 0.07, -0.0010, 0.0014, 0.0)),
                         rotation=(0.012, -0.02, 0.016), baseline=(0.12, 0.004, -0.003), right_gain=1.0, right_offset=0.0,
                         min_length=24.0, max_length=70.0, margin=30.0, texture=0.35, segments=None):
    """The raw images of a stereo rig whose right camera is rotated (`rotation`: the angle-axis of R in x_right = R x_left + t) and
    displaced (`baseline`: its centre in the left camera), both lenses distorted (k1, k2, p1, p2, k3 each), looking at straight 3-D
    edges - `segments` [n, 4] in rectified left pixel coordinates, each with the profile of make_edge_image, or num_segments seeded
    ones -: every edge lies in a plane of constant depth of the RECTIFIED frame, in front of a textured background plane.  Both raw
    images are rendered by inverse mapping through the distortion model: a raw pixel is undistorted to its ray, the ray is rotated into
    the rectified frame and cut with each edge's plane.  The right image's grey values are right_gain * I + right_offset; the default
    is no photometric difference, so that the two views differ by geometry alone: an edge fades out beyond its end points, and a gain
    moves the place along the edge where a detector's gradient threshold cuts it - with 0.8 the two detections of one edge end up to
    0.8 px of rows apart, which says nothing about the rectification.  Returns dict(left, right: raw uint8 [height, width]; rig: dict(left, right:
    dict(fx, fy, cx, cy, k1, k2, p1, p2, k3, width, height), R, t); Rl, Rr: the rectifying rotations; baseline, focal, cx, cy: the
    rectified geometry (focal = the mean of the four focal lengths, the left principal point);  left_segments, right_segments
    [n, 4] float64: the drawn edges in rectified pixel coordinates, row i of both the same edge; disparity [n])."""
    rng = np.random.default_rng(np.random.SeedSequence([20, int(seed)]))
    f0 = float(focal) if focal is not None else 0.9 * width
    cams = []
    for side in range(2):
        k = dict(zip(("k1", "k2", "p1", "p2", "k3"), [float(v) for v in distortion[side]]))
        k.update(fx=f0 * (1.0 + 0.01 * side) + 0.7, fy=f0 * (1.0 + 0.01 * side) - 0.4, cx=0.5 * (width - 1) + (2.3 if side == 0 else -1.7),
                 cy=0.5 * (height - 1) + (-1.9 if side == 0 else 1.2), width=int(width), height=int(height))
        cams.append(k)
    R = rodrigues(np.asarray(rotation, dtype=np.float64))
    c = np.asarray(baseline, dtype=np.float64)
    t = -(R @ c)
    Rl, Rr, b = _rectifying_rotations(R, t)
    f = ((cams[0]["fx"] + cams[0]["fy"]) + (cams[1]["fx"] + cams[1]["fy"])) / 4.0
    cx2, cy2 = cams[0]["cx"], cams[0]["cy"]
    lo, hi = float(disparity[0]), float(disparity[1])
    n = int(num_segments) if segments is None else len(segments)
    scene = _line_scene(seed, height, width, n, min_length, max_length, margin + hi)
    d = rng.uniform(lo, hi, n)
    # edges a detector with default options takes: a peak gradient of 25 to 70 grey levels a pixel
    scene["amplitude"] = rng.uniform(45.0, 70.0, n) * rng.choice([-1.0, 1.0], n)
    scene["softness"] = rng.uniform(1.0, 1.8, n)
    if segments is not None:
        scene["segments"] = np.asarray(segments, dtype=np.float64).reshape(n, 4)
        scene["softness"], scene["reach"] = np.full(n, 1.5), np.full(n, 6.0)
    seg = scene["segments"]
    images = []
    for side, (cam, rot) in enumerate(zip(cams, (Rl, Rr))):
        vv, uu = np.mgrid[0:height, 0:width].astype(np.float64)
        x, y = _undistort((uu - cam["cx"]) / cam["fx"], (vv - cam["cy"]) / cam["fy"], *[cam[k] for k in ("k1", "k2", "p1", "p2", "k3")])
        ray = np.stack([x, y, np.ones_like(x)], axis=-1) @ rot.T                       # in the rectified frame
        # where the ray meets the plane of a disparity dd, in rectified LEFT pixel coordinates: the camera's centre is (side b, 0, 0)
        def at(dd):
            return f * ray[..., 0] / ray[..., 2] + cx2 + side * dd, f * ray[..., 1] / ray[..., 2] + cy2
        val = np.full((height, width), 118.0)
        xb, yb = at(background_disparity)
        for kk, th, ph, a in scene["waves"]:
            val += texture * a * np.sin(kk * (np.cos(th) * xb + np.sin(th) * yb) + ph)
        for (x0, y0, x1, y1), amp, soft, reach, dd in zip(seg, scene["amplitude"], scene["softness"], scene["reach"], d):
            xp, yp = at(dd)
            length = np.hypot(x1 - x0, y1 - y0)
            ex, ey = (x1 - x0) / length, (y1 - y0) / length
            du, dv = xp - 0.5 * (x0 + x1), yp - 0.5 * (y0 + y1)
            along, across = du * ex + dv * ey, dv * ex - du * ey
            fade = 0.5 * (1.0 + np.tanh(0.5 * length - np.abs(along))) * np.exp(-0.5 * (across / reach) ** 2)
            val += amp * np.tanh(across / soft) * fade
        gain, off = (1.0, 0.0) if side == 0 else (right_gain, right_offset)
        images.append(np.clip(np.rint(gain * val + off), 0, 255).astype(np.uint8))
    right = seg - np.stack([d, np.zeros(n), d, np.zeros(n)], axis=1)
    return {"left": images[0], "right": images[1], "rig": dict(left=cams[0], right=cams[1], R=R, t=t), "Rl": Rl, "Rr": Rr, "baseline": b,
            "focal": f, "cx": cx2, "cy": cy2, "left_segments": seg.copy(), "right_segments": right, "disparity": d}

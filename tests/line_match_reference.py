"""numpy reference for the line matcher (include/slslam_hip.h: slslam_line_matcher_run): the contract restated, with np.float32 casts at
the places where SLAM::reprojection_error (reference src/slam.cpp:691-726) holds a float - `float sql`, the `float error` accumulator and
the float return value.  Every product and sum is written out in the reference's order (no dot(), no matmul: numpy may evaluate those in
another order or fused), so errors() is meant to be the reference's float bit for bit; tests/test_line_match_cpu.py pins it to the
oracle's ransac_score at several thresholds.

The overlap test takes the closed form of the segment contract from tests/lba_segments_reference.py (observation_closed_form with no
range clamp) under the frame's pose."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_segments_reference as S  # noqa: E402

OK, EMPTY, INVALID_POSE = "OK", "EMPTY", "INVALID_POSE"
TILE = 64          # the pair kernel's LDS line tile (csrc/line_match.h: kTile)


def errors(pose, observations, lines, baseline=0.12):
    """e [K, L] float32: reprojection_error(obs_k, pose, line_l)"""
    T = np.asarray(pose, dtype=np.float64).reshape(12)
    ob = np.asarray(observations, dtype=np.float64).reshape(-1, 8)
    ln = np.asarray(lines, dtype=np.float64).reshape(-1, 6)
    cp, dv = ln[:, :3], ln[:, 3:]
    with np.errstate(all="ignore"):
        d = [T[3 * r] * dv[:, 0] + T[3 * r + 1] * dv[:, 1] + T[3 * r + 2] * dv[:, 2] for r in range(3)]
        error = np.zeros((len(ob), len(ln)), dtype=np.float32)
        tt0 = T[9]
        for i in range(2):
            if i == 1:
                tt0 = tt0 - baseline
            c0 = T[0] * cp[:, 0] + T[1] * cp[:, 1] + T[2] * cp[:, 2] + tt0
            c1 = T[3] * cp[:, 0] + T[4] * cp[:, 1] + T[5] * cp[:, 2] + T[10]
            c2 = T[6] * cp[:, 0] + T[7] * cp[:, 1] + T[8] * cp[:, 2] + T[11]
            n0, n1, n2 = c1 * d[2] - c2 * d[1], c2 * d[0] - c0 * d[2], c0 * d[1] - c1 * d[0]
            sql = np.sqrt(n0 * n0 + n1 * n1).astype(np.float32).astype(np.float64)
            n0, n1, n2 = n0 / sql, n1 / sql, n2 / sql
            for j in range(2):
                x, y = ob[:, 4 * i + 2 * j, None], ob[:, 4 * i + 2 * j + 1, None]
                e = np.abs(n0[None, :] * x + n1[None, :] * y + n2[None, :])
                error = (error.astype(np.float64) + e).astype(np.float32)
        return (error.astype(np.float64) / 4.0).astype(np.float32)


def interval(pose, observation, line):
    """(status, lo, hi) of the observation's left segment on the line under the pose: the segment contract, no range clamp"""
    T = np.asarray(pose, dtype=np.float64).reshape(12)
    return S.observation_closed_form(T[:9].reshape(3, 3), T[9:], np.asarray(line[:3], dtype=np.float64), np.asarray(line[3:], dtype=np.float64),
                                     np.asarray(observation, dtype=np.float64), 0.0)


def admissible(frame, baseline=0.12, error_thr=5.0 / 406.05, margin=0.0):
    """(e [K, L] float32, admissible [K, L] bool, gap [K, L]: for pairs that reached the interval test the distance of the decision from
    its boundary, inf elsewhere)"""
    ob = np.asarray(frame["observations"], dtype=np.float64).reshape(-1, 8)
    ln = np.asarray(frame["lines"], dtype=np.float64).reshape(-1, 6)
    e = errors(frame["pose"], ob, ln, baseline)
    with np.errstate(invalid="ignore"):
        adm = np.isfinite(e) & (e.astype(np.float64) < error_thr)
    gap = np.full(e.shape, np.inf)
    ext = frame.get("extents")
    if ext is not None:
        ext = np.asarray(ext, dtype=np.float64).reshape(-1, 2)
        for k, l in zip(*np.nonzero(adm)):
            st, lo, hi = interval(frame["pose"], ob[k, :4], ln[l])
            a, b = ext[l, 0] - margin, ext[l, 1] + margin
            adm[k, l] = st == S.USED and hi >= a and lo <= b
            if st == S.USED:
                # inside: how far both conditions hold; outside: how far the violated one is from holding
                gap[k, l] = min(hi - a, b - lo) if adm[k, l] else max(a - hi, lo - b)
    return e, adm, gap


def match(frame, baseline=0.12, error_thr=5.0 / 406.05, ratio=1.5, margin=0.0):
    """The dict LineMatcher.run returns for the frame (plus admissible [K, L], errors [K, L] and gap [K, L])"""
    ob = np.asarray(frame["observations"], dtype=np.float64).reshape(-1, 8)
    ln = np.asarray(frame["lines"], dtype=np.float64).reshape(-1, 6)
    K, L = len(ob), len(ln)
    inf = np.float32(np.inf)
    out = dict(status=OK, num_matched=0, match=np.full(K, -1, np.int32), best_line=np.full(K, -1, np.int32),
               best_error=np.full(K, inf, np.float32), second_error=np.full(K, inf, np.float32), num_admissible=np.zeros(K, np.int32),
               best_observation=np.full(L, -1, np.int32), admissible=np.zeros((K, L), bool), errors=np.full((K, L), np.nan, np.float32),
               gap=np.full((K, L), np.inf))
    if K == 0 or L == 0:
        out["status"] = EMPTY
        return out
    if not np.isfinite(np.asarray(frame["pose"], dtype=np.float64)).all():
        out["status"] = INVALID_POSE
        return out
    e, adm, gap = admissible(frame, baseline, error_thr, margin)
    out.update(admissible=adm, errors=e, gap=gap)
    em = np.where(adm, e, inf)
    for k in range(K):
        if not adm[k].any():
            continue
        bl = int(np.argmin(em[k]))                    # (the first of equal minima)
        out["best_line"][k], out["best_error"][k] = bl, em[k, bl]
        rest = np.delete(em[k], bl)
        out["second_error"][k] = rest.min() if rest.size else inf
        out["num_admissible"][k] = int(adm[k].sum())
    for l in range(L):
        if adm[:, l].any():
            out["best_observation"][l] = int(np.argmin(em[:, l]))
    for k in range(K):
        bl = out["best_line"][k]
        if bl < 0 or out["best_observation"][bl] != k:
            continue
        if ratio <= 1.0 or float(out["best_error"][k]) * ratio <= float(out["second_error"][k]):
            out["match"][k] = bl
    out["num_matched"] = int((out["match"] >= 0).sum())
    return out


# ----------------------------------------------------------------------------- inputs for the tests
def make_frame(seed, K, L, rot_sigma=1e-3, t_sigma=3e-3, extents=False):
    """A frame of K observations against a map of L lines from one synthetic stereo pair (synth.make_ransac_pair, no wrong matches): the
    observations are those of the current frame in shuffled order (observation k shows line truth[k]; -1: a line the map does not hold),
    the pose is the true motion perturbed by (rot_sigma rad, t_sigma m) per axis.  extents: per line the interval that its own observation
    cuts out of it under the TRUE pose (what one keyframe's slslam_lba_batch_segments would hold); (inf, -inf) when it cuts none.
    Also returns obs0 [L, 8], every map line's observation in the previous frame, and pair, the synthetic pair itself."""
    from slslam_amd import synth
    n = max(K, L, 5)                                            # (the pair draws samples of five)
    pair = synth.make_ransac_pair(seed, num_lines=n, outlier_frac=0.0, num_trials=1)
    rng = np.random.default_rng(np.random.SeedSequence([13, int(seed)]))
    perm = rng.permutation(n)[:K]
    T = pair["true_pose"]
    R = synth.rodrigues(rng.normal(size=3) * rot_sigma) @ T[:9].reshape(3, 3)
    t = T[9:] + rng.normal(size=3) * t_sigma
    fr = dict(pose=np.concatenate([R.reshape(-1), t]), observations=pair["obs1"][perm].copy(), lines=pair["lines"][:L].copy(),
              truth=np.where(perm < L, perm, -1).astype(np.int32), perm=perm, obs0=pair["obs0"][:L].copy(), pair=pair)
    if extents:
        ext = np.zeros((L, 2))
        for l in range(L):
            st, lo, hi = interval(T, pair["obs1"][l, :4], pair["lines"][l])
            ext[l] = (lo, hi) if st == S.USED else (np.inf, -np.inf)
        fr["extents"] = ext
    return fr

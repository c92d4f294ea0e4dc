// slslam_amd/csrc/segment_eval.h — one left-image segment against one 3-D line: the interval [lo, hi] of the line's parameter s that the
// segment's two endpoints cut out (steps 1-5 of the contract in lba_segments.h, the reference's SLAM::extend_end_points per observation).
// Shared by the segments of an LBA batch (lba_segments.h) and the overlap test of the line matcher (line_match.h), which has the line in
// the camera's frame already and enters at segment_cut.
#ifndef SLSLAM_SEGMENT_EVAL_H_
#define SLSLAM_SEGMENT_EVAL_H_

#include <hip/hip_runtime.h>

namespace slslam {

enum { kSegObsUsed = 0, kSegObsUsedClamped = 1, kSegObsDegenerate = 2, kSegObsBehind = 3, kSegObsOutOfRange = 4, kSegObsCollapsed = 5 };   // = SLSLAM_SEGMENT_OBS_*

// The line in the camera's frame (pc = R cp + t, dc = R dv); e = x0 y0 x1 y1 of the left image.  lo, hi: zeros unless USED / USED_CLAMPED.
__device__ __forceinline__ int segment_cut(const double (&pc)[3], const double (&dc)[3], const double (&e)[4], double max_range, double& lo,
                                           double& hi) {
  lo = 0.0; hi = 0.0;
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) fin = fin && isfinite(pc[i]) && isfinite(dc[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) fin = fin && isfinite(e[i]);
  double lx = e[1] - e[3], ly = e[2] - e[0];                 // (p1 x p2)[0:2]
  const double nrm = sqrt(lx * lx + ly * ly);
  if (!fin || !(nrm > 0.0)) return kSegObsDegenerate;
  lx /= nrm; ly /= nrm;
  double s[2];
  bool degenerate = false;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double m2 = e[2 * k] * ly - e[2 * k + 1] * lx;     // m = p x (ln, 0) = (-ly, lx, px ly - py lx)
    const double mn = sqrt(ly * ly + lx * lx + m2 * m2);
    const double den = -ly * dc[0] + lx * dc[1] + m2 * dc[2];
    const double num = -ly * pc[0] + lx * pc[1] + m2 * pc[2];
    degenerate = degenerate || !(fabs(den) > 1e-6 * mn);
    s[k] = -num / den;
  }
  if (degenerate) return kSegObsDegenerate;
  if (pc[2] + s[0] * dc[2] < 0.0 || pc[2] + s[1] * dc[2] < 0.0) return kSegObsBehind;
  bool clamped = false;
  if (max_range > 0.0) {
    const double q = pc[0] * dc[0] + pc[1] * dc[1] + pc[2] * dc[2];
    const double p0[3] = { pc[0] - q * dc[0], pc[1] - q * dc[1], pc[2] - q * dc[2] };
    const double d2 = p0[0] * p0[0] + p0[1] * p0[1] + p0[2] * p0[2];
    if (sqrt(d2) > max_range) return kSegObsOutOfRange;
    const double ext = sqrt(fmax(max_range * max_range - d2, 0.0));
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double tau = s[k] + q;
      if (fabs(tau) > ext) { s[k] = copysign(ext, tau) - q; clamped = true; }
    }
  }
  const double a = fmin(s[0], s[1]), b = fmax(s[0], s[1]);
  if (a == b) return kSegObsCollapsed;
  lo = a; hi = b;
  return clamped ? kSegObsUsedClamped : kSegObsUsed;
}

// Steps 1-5 of the contract for one observation of line (cp, dv) from camera (R, t) world to camera
__device__ __forceinline__ int segment_eval(const double (&R)[9], const double (&t)[3], const double (&cp)[3], const double (&dv)[3],
                                            const double (&e)[4], double max_range, double& lo, double& hi) {
  double pc[3], dc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pc[i] = R[3 * i] * cp[0] + R[3 * i + 1] * cp[1] + R[3 * i + 2] * cp[2] + t[i];
    dc[i] = R[3 * i] * dv[0] + R[3 * i + 1] * dv[1] + R[3 * i + 2] * dv[2];
  }
  return segment_cut(pc, dc, e, max_range, lo, hi);
}

}  // namespace slslam
#endif  // SLSLAM_SEGMENT_EVAL_H_

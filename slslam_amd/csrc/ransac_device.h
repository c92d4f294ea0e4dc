// slslam_amd/csrc/ransac_device.h — the bodies of RANSAC hypothesis scoring and generation: called by the one kernel pair of
// ransac_api.hip (every frame of a call in one launch), for the final inlier set by frame_api.hip's k_frame_finish, and - the error in
// its two parts - by the line matcher (line_match.h).
//
// Scoring: SLAM::reprojection_error (reference src/slam.cpp:691-726) of one line under one pose.  The reference mixes float
// and double (float `sql = nc.head(2).norm()`, `float error`); the same conversions are applied in the same places so that
// scores and inlier sets are bit-identical.
// Generation: SLAM::vo_angle_axis_approx (reference src/slam.cpp:433-574) for one trial.
#ifndef SLSLAM_RANSAC_DEVICE_H_
#define SLSLAM_RANSAC_DEVICE_H_

#include <hip/hip_runtime.h>

// no FMA contraction: the reference evaluates these expressions with separate multiplies and adds,
// and the inlier test sits on a threshold
#pragma clang fp contract(off)

namespace slslam_ransac {

// `if ( motion[j].t.norm() > 1 ) continue;` (slam.cpp:398-399)
__device__ __forceinline__ bool pose_skipped(const double* T) {
  const double t0 = T[9], t1 = T[10], t2 = T[11];
  return sqrt(t0 * t0 + t1 * t1 + t2 * t2) > 1.0;
}

// reprojection_error in two parts, so that a caller with many observations per line (line_match.h) evaluates the first once per line;
// the operations and their order are the reference's, so splitting them changes no rounding.
// Part 1, pose and line ln = (closest point, direction) [6]: per stereo camera i the image line's normal n[i] = nc / (float)sql; pc, dc =
// the line's point and direction in the left camera (gc_point_to_pose, T.R * dv)
__device__ __forceinline__ void line_normals(const double* T, const double* __restrict__ ln, double baseline, double (&n)[2][3],
                                             double (&pc)[3], double (&dc)[3]) {
  const double t0 = T[9], t1 = T[10], t2 = T[11];
  const double cp[3] = { ln[0], ln[1], ln[2] }, dv[3] = { ln[3], ln[4], ln[5] };
  double tt0 = t0;
  // dvc = T.R * dv is the same for both cameras
  const double d0 = T[0] * dv[0] + T[1] * dv[1] + T[2] * dv[2];
  const double d1 = T[3] * dv[0] + T[4] * dv[1] + T[5] * dv[2];
  const double d2 = T[6] * dv[0] + T[7] * dv[1] + T[8] * dv[2];
  dc[0] = d0; dc[1] = d1; dc[2] = d2;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (i == 1) tt0 -= baseline;                                   // T.t(0) -= baseline
    const double c0 = T[0] * cp[0] + T[1] * cp[1] + T[2] * cp[2] + tt0;   // gc_point_to_pose
    const double c1 = T[3] * cp[0] + T[4] * cp[1] + T[5] * cp[2] + t1;
    const double c2 = T[6] * cp[0] + T[7] * cp[1] + T[8] * cp[2] + t2;
    if (i == 0) { pc[0] = c0; pc[1] = c1; pc[2] = c2; }
    double n0 = c1 * d2 - c2 * d1, n1 = c2 * d0 - c0 * d2, n2 = c0 * d1 - c1 * d0;   // cpc.cross(dvc)
    const float sql = (float)sqrt(n0 * n0 + n1 * n1);              // float sql = nc.head(2).norm()
    n0 /= (double)sql; n1 /= (double)sql; n2 /= (double)sql;       // nc /= sql
    n[i][0] = n0; n[i][1] = n1; n[i][2] = n2;
  }
}

// Part 2, the normals and one observation ft [8]: the float reprojection_error returns
__device__ __forceinline__ float normals_error(const double (&n)[2][3], const double* __restrict__ ft) {
  float error = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double e1 = fabs(n[i][0] * ft[4 * i] + n[i][1] * ft[4 * i + 1] + n[i][2]);          // nc.dot(p1), p1 = (x, y, 1)
    const double e2 = fabs(n[i][0] * ft[4 * i + 2] + n[i][1] * ft[4 * i + 3] + n[i][2]);
    error = (float)((double)error + e1);                           // float error += double
    error = (float)((double)error + e2);
  }
  return (float)((double)error / 4.0);                             // return error / 4.0  (float function)
}

// reprojection_error(ft, T, line) of one common line: ft = its observation [8], ln = (closest point, direction) [6]
__device__ __forceinline__ float line_error(const double* T, const double* __restrict__ ft, const double* __restrict__ ln, double baseline) {
  double n[2][3], pc[3], dc[3];
  line_normals(T, ln, baseline, n, pc, dc);
  return normals_error(n, ft);
}

// reprojection_error(ft, T, line) < thr
__device__ __forceinline__ bool line_inlier(const double* T, const double* __restrict__ ft, const double* __restrict__ ln, double baseline,
                                            double thr) {
  return (double)line_error(T, ft, ln, baseline) < thr;            // error < error_thr (double)
}

// ---------------------------------------------------------------------------------------------
// Hypothesis generation, lane <-> trial.  Each lane walks its s sampled correspondences twice (rotation rows K, then translation
// rows M), accumulating the 3x3 normal matrices in registers; (A^T A)^-1 by partially pivoted LU as Eigen's dynamic inverse()
// does.  Same operation order as the oracle.
__device__ inline void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double norm3(const double a[3]) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
__device__ inline void image_line(const double* ob, double l[3]) {
  const double p1[3] = { ob[0], ob[1], 1 }, p2[3] = { ob[2], ob[3], 1 };
  cross3(p1, p2, l);
}
__device__ inline void solve_normal3(const double N[9], const double v[3], double x[3]) {
  double a[3][6];
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { a[i][j] = N[3 * i + j]; a[i][3 + j] = i == j ? 1.0 : 0.0; }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int piv = c;
#pragma unroll
    for (int r = c + 1; r < 3; ++r) if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
#pragma unroll
    for (int r = c + 1; r < 3; ++r)
      if (piv == r)
        for (int j = 0; j < 6; ++j) { const double t = a[c][j]; a[c][j] = a[r][j]; a[r][j] = t; }
#pragma unroll
    for (int r = c + 1; r < 3; ++r) {
      const double f = a[r][c] / a[c][c];
#pragma unroll
      for (int j = c; j < 6; ++j) a[r][j] -= f * a[c][j];
    }
  }
  double inv[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 2; i >= 0; --i) {
      double s = a[i][3 + j];
#pragma unroll
      for (int k = i + 1; k < 3; ++k) s -= a[i][k] * inv[k][j];
      inv[i][j] = s / a[i][i];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = inv[i][0] * v[0] + inv[i][1] * v[1] + inv[i][2] * v[2];
}
__device__ inline void aa_to_matrix(const double w[3], double R[9]) {   // ceres::AngleAxisToRotationMatrix, row-major
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (th2 > 2.220446049250313e-16) {
    const double th = sqrt(th2), wx = w[0] / th, wy = w[1] / th, wz = w[2] / th;
    const double c = cos(th), s = sin(th);
    R[0] = c + wx * wx * (1 - c);       R[1] = wx * wy * (1 - c) - wz * s;  R[2] = wy * s + wx * wz * (1 - c);
    R[3] = wz * s + wx * wy * (1 - c);  R[4] = c + wy * wy * (1 - c);       R[5] = -wx * s + wy * wz * (1 - c);
    R[6] = -wy * s + wx * wz * (1 - c); R[7] = wx * s + wy * wz * (1 - c);  R[8] = c + wz * wz * (1 - c);
  } else {
    R[0] = 1; R[1] = -w[2]; R[2] = w[1];
    R[3] = w[2]; R[4] = 1; R[5] = -w[0];
    R[6] = -w[1]; R[7] = w[0]; R[8] = 1;
  }
}

// One trial: smp = its s sample indices; writes the pose P[12] (R row-major | t) and returns num_sol (0: a degenerate sample)
__device__ __forceinline__ int generate_trial(int s, const int* __restrict__ smp, const double* __restrict__ obs0,
                                              const double* __restrict__ obs1, double baseline, double* P) {
  double N[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, v[3] = { 0, 0, 0 };
  bool ok = true;
  for (int i = 0; i < s; ++i) {                                          // slam.cpp:437-482
    const double* o0 = obs0 + 8 * (long long)smp[i];
    const double* o1 = obs1 + 8 * (long long)smp[i];
    double l1[3], l2[3], l3[3], l4[3], lx[3];
    image_line(o0, l1); image_line(o0 + 4, l2); image_line(o1, l3); image_line(o1 + 4, l4);
    cross3(l1, l2, lx);
    const double lxn = norm3(lx);
    if (lxn == 0) ok = false;
    lx[0] /= lxn; lx[1] /= lxn; lx[2] /= lxn;
    for (int j = 0; j < 2; ++j) {
      const double* tl = j == 0 ? l3 : l4;
      const double tln = norm3(tl);
      if (tln == 0) ok = false;
      const double ly[3] = { tl[0] / tln, tl[1] / tln, tl[2] / tln };
      const double row[4] = { lx[2] * ly[1] - lx[1] * ly[2], lx[0] * ly[2] - lx[2] * ly[0], lx[1] * ly[0] - lx[0] * ly[1],
                              lx[0] * ly[0] + lx[1] * ly[1] + lx[2] * ly[2] };
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) N[3 * a + b] += row[a] * row[b];
        v[a] += row[a] * (-row[3]);
      }
    }
  }
  double w[3], R[9];
  solve_normal3(N, v, w);                                                // :484-488
  w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2];
  aa_to_matrix(w, R);
  for (int a = 0; a < 9; ++a) N[a] = 0;
  v[0] = v[1] = v[2] = 0;
  for (int i = 0; i < s; ++i) {                                          // :495-559
    const double* o0 = obs0 + 8 * (long long)smp[i];
    const double* o1 = obs1 + 8 * (long long)smp[i];
    double l1[3], l2[3], lx[3];
    image_line(o0, l1);
    const double l1n = norm3(l1);
    if (l1n == 0) ok = false;
    l1[0] /= l1n; l1[1] /= l1n; l1[2] /= l1n;
    image_line(o0 + 4, l2);
    const double l2n = norm3(l2);
    if (l2n == 0) ok = false;
    l2[0] /= l2n; l2[1] /= l2n; l2[2] /= l2n;
    cross3(l1, l2, lx);
    if (norm3(lx) == 0) ok = false;
    for (int j = 0; j < 2; ++j) {
      double l3[3];
      image_line(o1 + 4 * j, l3);
      const double l3n = norm3(l3);
      if (l3n == 0) ok = false;
      l3[0] /= l3n; l3[1] /= l3n; l3[2] /= l3n;
      double c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double rc[3] = { R[k], R[3 + k], R[6 + k] };
        double u[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) u[q] = -l2[0] * (baseline * rc[q]) + -l2[1] * (0.0 * rc[q]) + -l2[2] * (0.0 * rc[q]);
        c[k] = u[0] * l3[0] + u[1] * l3[1] + u[2] * l3[2];
        if (j == 1) c[k] += l2[k] * baseline * l3[0];
      }
      const double rows[3][4] = {
        { l1[1] * l2[2] * l3[0] - l1[2] * l2[1] * l3[0], l1[1] * l2[2] * l3[1] - l1[2] * l2[1] * l3[1],
          l1[1] * l2[2] * l3[2] - l1[2] * l2[1] * l3[2], l1[1] * c[2] - l1[2] * c[1] },
        { l1[2] * l2[0] * l3[0] - l1[0] * l2[2] * l3[0], l1[2] * l2[0] * l3[1] - l1[0] * l2[2] * l3[1],
          l1[2] * l2[0] * l3[2] - l1[0] * l2[2] * l3[2], l1[2] * c[0] - l1[0] * c[2] },
        { l1[0] * l2[1] * l3[0] - l1[1] * l2[0] * l3[0], l1[0] * l2[1] * l3[1] - l1[1] * l2[0] * l3[1],
          l1[0] * l2[1] * l3[2] - l1[1] * l2[0] * l3[2], l1[0] * c[1] - l1[1] * c[0] } };
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
          for (int b = 0; b < 3; ++b) N[3 * a + b] += rows[r][a] * rows[r][b];
          v[a] += rows[r][a] * (-rows[r][3]);
        }
    }
  }
  double t[3];
  solve_normal3(N, v, t);                                                // :561-565
  for (int q = 0; q < 9; ++q) P[q] = R[q];
  P[9] = t[0]; P[10] = t[1]; P[11] = t[2];
  return ok ? 1 : 0;
}

}  // namespace slslam_ransac

#endif  // SLSLAM_RANSAC_DEVICE_H_

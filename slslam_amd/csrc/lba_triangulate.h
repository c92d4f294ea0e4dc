// slslam_amd/csrc/lba_triangulate.h — making a line landmark from all its observations: every line of every window of a
// call in ONE launch, lane <-> line.
//
// A workgroup is one wave = 64 lines of one window (sorted by observation count, observations lane-interleaved: lba_refine_layout.h,
// the refiner's layout); it copies the window's camera table (R, t per camera, made by slslam_gc::wt_to_Rt) to LDS once; then every lane
//   1. makes the stereo-first line of its line's first observation - SLAM::initialize_lm (reference src/slam.cpp:190-219) in its
//      operation order - and moves it to the world with gc_line_from_pose under that observation's camera;
//   2. (method 1) walks its observations: the two back-projected planes of each, moved to the world and scaled to a unit normal, summed
//      into the symmetric 4 x 4 Gram matrix G in the caller's order; G's eigen-decomposition by kTriSweeps cyclic Jacobi sweeps in
//      registers (the pair order is fixed, no pivot search); the line of the two leading eigenvectors, direction signed like step 1's;
//   3. chooses: the multi-view line when the line has >= 2 observations, every number of it is finite and lambda2 >= min_parallax
//      lambda1, else the stereo-first line;
//   4. writes av_to_orth of the chosen line, the line itself and the record from its own lane.
// The row loop is wave-uniform (a group's rows), the lanes predicated.  fp64 throughout, no atomics, nothing shared between lanes but
// the read-only camera table: a line's bytes cannot depend on its company.  The line maths is __host__ __device__ and uses +, -, *, /
// and sqrt only up to the chosen (cp, v) - the host evaluates the same functions to the same bits (slslam_debug_stereo_first_line).
#ifndef SLSLAM_LBA_TRIANGULATE_H_
#define SLSLAM_LBA_TRIANGULATE_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "gc_convert.h"
#include "lba_triangulate_host.h"

#pragma clang fp contract(off)

namespace slslam {

enum { kTriSweeps = 6 };   // cyclic Jacobi sweeps over the 6 pairs of a 4 x 4 matrix (DESIGN.md 4.6 has what they leave off the diagonal)

// gc_ppp_pi (reference src/gc.cpp:100-105): the plane through x1, x2, x3
__host__ __device__ inline void tri_ppp_pi(const double x1[3], const double x2[3], const double x3[3], double pi[4]) {
  const double a[3] = { x1[0] - x3[0], x1[1] - x3[1], x1[2] - x3[2] }, b[3] = { x2[0] - x3[0], x2[1] - x3[1], x2[2] - x3[2] };
  double c[3];
  slslam_gc::cross3(a, b, pi);
  slslam_gc::cross3(x1, x2, c);
  pi[3] = -(x3[0] * c[0] + x3[1] * c[1] + x3[2] * c[2]);
}

// gc_pipi_plk (src/gc.cpp:107-113) then gc_plucker_origin (:115-117): direction v and closest point cp of the line two planes meet in
__host__ __device__ inline void tri_pipi_line(const double p[4], const double q[4], double cp[3], double v[3]) {
  const double n[3] = { p[0] * q[3] - q[0] * p[3], p[1] * q[3] - q[1] * p[3], p[2] * q[3] - q[2] * p[3] };
  v[0] = -(p[1] * q[2] - q[1] * p[2]);
  v[1] = p[0] * q[2] - q[0] * p[2];
  v[2] = -(p[0] * q[1] - q[0] * p[1]);
  double c[3];
  slslam_gc::cross3(v, n, c);
  const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  cp[0] = c[0] / vv; cp[1] = c[1] / vv; cp[2] = c[2] / vv;
}

// The back-projected planes of the left and the right segment of an observation, in its camera (the first lines of initialize_lm)
__host__ __device__ inline void tri_camera_planes(const double ob[8], double baseline, double pl[4], double pr[4]) {
  const double p1[3] = { ob[0], ob[1], 1.0 }, p2[3] = { ob[2], ob[3], 1.0 };
  const double p3[3] = { ob[4] + baseline, ob[5], 1.0 }, p4[3] = { ob[6] + baseline, ob[7], 1.0 };
  const double o[3] = { 0.0, 0.0, 0.0 }, c[3] = { baseline, 0.0, 0.0 };
  tri_ppp_pi(p1, p2, o, pl);
  tri_ppp_pi(p3, p4, c, pr);
}

__host__ __device__ inline bool tri_finite3(const double a[3]) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// Step 1.  T = R row-major | t of the observation's camera.  false: v = 0 (the two planes are parallel or one is none) or a number
// is not finite - no line.
__host__ __device__ inline bool tri_stereo_first(const double ob[8], const double T[12], double baseline, double inverse_depth, double cp_w[3],
                                                 double v_w[3], int* clamped) {
  double pl[4], pr[4], cp[3], v[3];
  tri_camera_planes(ob, baseline, pl, pr);
  tri_pipi_line(pl, pr, cp, v);
  *clamped = 0;
  if ((v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0) || !tri_finite3(v) || !tri_finite3(cp)) return false;
  const double cpn = sqrt(cp[0] * cp[0] + cp[1] * cp[1] + cp[2] * cp[2]);
  if (cpn < 0.1 || cpn > 10.0) {
    cp[0] = cp[0] / cpn / inverse_depth; cp[1] = cp[1] / cpn / inverse_depth; cp[2] = cp[2] / cpn / inverse_depth;
    *clamped = 1;
  }
  if (cp[2] < 0.0) { cp[0] = -cp[0]; cp[1] = -cp[1]; cp[2] = -cp[2]; }
  // gc_line_from_pose: cp_w = R^T (cp - t), v_w = R^T v
  const double d[3] = { cp[0] - T[9], cp[1] - T[10], cp[2] - T[11] };
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cp_w[a] = T[a] * d[0] + T[3 + a] * d[1] + T[6 + a] * d[2];
    v_w[a] = T[a] * v[0] + T[3 + a] * v[1] + T[6 + a] * v[2];
  }
  return tri_finite3(cp_w) && tri_finite3(v_w);
}

// Step 2, per plane: pi (camera) -> the world, unit normal, G += pi pi^T (lower triangle, G[tri(a, b)] with tri(a, b) = a (a + 1) / 2 + b).
// false: the normal has no length (a segment of zero length) - nothing is added.
__host__ __device__ inline bool tri_gram_add(const double pi[4], const double T[12], double G[10]) {
  double w[4];
#pragma unroll
  for (int a = 0; a < 3; ++a) w[a] = T[a] * pi[0] + T[3 + a] * pi[1] + T[6 + a] * pi[2];
  w[3] = pi[0] * T[9] + pi[1] * T[10] + pi[2] * T[11] + pi[3];
  const double nn = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  if (!(nn > 0.0)) return false;
#pragma unroll
  for (int a = 0; a < 4; ++a) w[a] = w[a] / nn;
  int q = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b, ++q) G[q] += w[a] * w[b];
  }
  return true;
}

// One Jacobi rotation of the pair (P, Q), P < Q, of the symmetric A[4][4] (both triangles kept) and of the eigenvector columns V.
// The smaller root t of t^2 + 2 t theta - 1 = 0, theta = (a_qq - a_pp) / (2 a_pq), written without the division by a_pq:
// t = 2 a_pq sgn(d) / (|d| + sqrt(d^2 + 4 a_pq^2)), d = a_qq - a_pp; a pair that is already diagonal (the denominator 0) is not turned.
template <int P, int Q>
__host__ __device__ inline void tri_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q], d = A[Q][Q] - A[P][P];
  const double den = fabs(d) + sqrt(d * d + 4.0 * apq * apq);
  const double t = den > 0.0 ? (d < 0.0 ? -2.0 * apq : 2.0 * apq) / den : 0.0;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = A[r][P], arq = A[r][Q];
      A[r][P] = c * arp - s * arq; A[P][r] = A[r][P];
      A[r][Q] = s * arp + c * arq; A[Q][r] = A[r][Q];
    }
    const double vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = c * vrp - s * vrq;
    V[r][Q] = s * vrp + c * vrq;
  }
}

// compare-exchange of the eigenpairs I < J: the larger eigenvalue to I
template <int I, int J>
__host__ __device__ inline void tri_order(double* lam, double (&V)[4][4]) {
  const bool sw = lam[J] > lam[I];
  const double a = lam[I], b = lam[J];
  lam[I] = sw ? b : a; lam[J] = sw ? a : b;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double x = V[r][I], y = V[r][J];
    V[r][I] = sw ? y : x; V[r][J] = sw ? x : y;
  }
}

// Eigenvalues (descending) of the Gram matrix G (packed lower triangle) and the line of the two leading eigenvectors.
// *offdiag: the off-diagonal Frobenius norm the sweeps leave (of the upper triangle), for the record of DESIGN.md 4.6.
__host__ __device__ inline void tri_multiview_line(const double G[10], double lam[4], double cp[3], double v[3], double* offdiag) {
  double A[4][4], V[4][4];
  int q = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b <= a; ++b, ++q) { A[a][b] = G[q]; A[b][a] = G[q]; }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kTriSweeps; ++sweep) {
    tri_jacobi_rotate<0, 1>(A, V); tri_jacobi_rotate<0, 2>(A, V); tri_jacobi_rotate<0, 3>(A, V);
    tri_jacobi_rotate<1, 2>(A, V); tri_jacobi_rotate<1, 3>(A, V); tri_jacobi_rotate<2, 3>(A, V);
  }
  if (offdiag)
    *offdiag = sqrt(A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3]);
#pragma unroll
  for (int a = 0; a < 4; ++a) lam[a] = A[a][a];
  tri_order<0, 1>(lam, V); tri_order<2, 3>(lam, V); tri_order<0, 2>(lam, V); tri_order<1, 3>(lam, V); tri_order<1, 2>(lam, V);
  const double e1[4] = { V[0][0], V[1][0], V[2][0], V[3][0] }, e2[4] = { V[0][1], V[1][1], V[2][1], V[3][1] };
  tri_pipi_line(e1, e2, cp, v);
}

// Step 3: is the multi-view line taken?  (n_obs: observations of the line)
__host__ __device__ inline bool tri_take_multiview(int n_obs, const double lam[4], const double cp[3], const double v[3], double min_parallax) {
  return n_obs >= 2 && tri_finite3(cp) && tri_finite3(v) && isfinite(lam[0]) && isfinite(lam[1]) && isfinite(lam[2]) && isfinite(lam[3]) &&
         lam[1] >= min_parallax * lam[0];
}

#if defined(__HIPCC__)

struct TriPtrs {
  const TriGroup* groups;
  const double* cam;       // [ncam][12] R row-major | t
  const int* cnt;          // [nslot] observations of the slot's line; 0: an unused slot
  const int* ob_cam;       // [nrow * 64] window-local camera of observation (row, lane)
  const double* ob;        // [4][ob_stride] double2: the four observed endpoints, as RefinePtrs.ob
  long long ob_stride;     // = nrow * 64
  TriOut* out;             // [nslot]
};

__host__ __device__ inline int lds_doubles_triangulate(int C) { return C * kTriCamTab; }

__global__ __launch_bounds__(64) void k_triangulate_lines(TriPtrs p, double baseline, double inverse_depth, double min_parallax, int method) {
  extern __shared__ __attribute__((aligned(16))) double tri_smem[];
  const int lane = threadIdx.x;
  const TriGroup gr = p.groups[blockIdx.x];
  for (int i = lane; i < gr.C * kTriCamRec; i += 64) {
    const int c = i / kTriCamRec;
    tri_smem[c * kTriCamTab + (i - c * kTriCamRec)] = p.cam[(long long)gr.cam_off * kTriCamRec + i];
  }
  __syncthreads();

  const long long slot = (long long)blockIdx.x * 64 + lane;
  const int cnt = p.cnt[slot];
  const long long e0 = gr.row_base * 64 + lane;            // the lane's observation j is element e0 + 64 j

  // observation j of this lane and its camera's table entry
  auto load_obs = [&](int j, double (&ob)[8], double (&T)[12]) {
    const long long e = e0 + (long long)j * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double2 v = reinterpret_cast<const double2*>(p.ob)[(long long)q * p.ob_stride + e];
      ob[2 * q] = v.x; ob[2 * q + 1] = v.y;
    }
    const double* ct = tri_smem + p.ob_cam[e] * kTriCamTab;
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = ct[q];
  };

  TriOut o;
#pragma unroll
  for (int a = 0; a < 4; ++a) { o.u[a] = 0.0; o.eig[a] = 0.0; }
#pragma unroll
  for (int a = 0; a < 6; ++a) o.av[a] = 0.0;
  o.status = SLSLAM_TRI_INVALID; o.num_planes = 0; o.clamped = 0; o.pad = 0;

  // ---- 1. the stereo-first line
  double cp[3] = { 0.0, 0.0, 0.0 }, v[3] = { 0.0, 0.0, 0.0 };
  int clamped = 0;
  bool have = false;
  if (cnt > 0) {
    double ob[8], T[12];
    load_obs(0, ob, T);
    have = tri_stereo_first(ob, T, baseline, inverse_depth, cp, v, &clamped);
  }
  int status = SLSLAM_TRI_STEREO;

  // ---- 2. the multi-view line, 3. the choice
  if (method == 1) {
    double G[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) G[q] = 0.0;
    int planes = 0;
    for (int j = 0; j < gr.depth; ++j) {
      if (have && j < cnt) {
        double ob[8], T[12], pl[4], pr[4];
        load_obs(j, ob, T);
        tri_camera_planes(ob, baseline, pl, pr);
        planes += tri_gram_add(pl, T, G) ? 1 : 0;
        planes += tri_gram_add(pr, T, G) ? 1 : 0;
      }
    }
    double lam[4], cpm[3], vm[3];
    tri_multiview_line(G, lam, cpm, vm, nullptr);
    if (vm[0] * v[0] + vm[1] * v[1] + vm[2] * v[2] < 0.0) { vm[0] = -vm[0]; vm[1] = -vm[1]; vm[2] = -vm[2]; }
    o.num_planes = planes;
    if (have && tri_take_multiview(cnt, lam, cpm, vm, min_parallax)) {
      status = SLSLAM_TRI_MULTIVIEW;
#pragma unroll
      for (int a = 0; a < 3; ++a) { cp[a] = cpm[a]; v[a] = vm[a]; }
#pragma unroll
      for (int a = 0; a < 4; ++a) o.eig[a] = lam[a];
    }
  }

  // ---- 4. write-out
  if (have) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { o.av[a] = cp[a]; o.av[3 + a] = v[a]; }
    slslam_gc::av_to_orth(o.av, o.u);
    o.status = status;
    o.clamped = (status == SLSLAM_TRI_STEREO) ? clamped : 0;
  } else {
    o.num_planes = 0;
  }
  p.out[slot] = o;
}

#endif  // __HIPCC__

}  // namespace slslam
#endif

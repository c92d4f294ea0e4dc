// slslam_amd/csrc/lba_covariance.h — posterior covariances of the windows of a resident LBA batch.
//
// What it replaces: nothing in the reference, whose odometry edges are identity-weighted; the Ceres counterpart is
// ceres::Covariance.  For every window, at the parameters the batch holds on the device (the accepted buffer: the solved
// point after a solve, the initial one after finalize / reset / refill - what slslam_lba_batch_linearise evaluates):
//   J    = Jacobian of all residual blocks w.r.t. the free blocks, after the Huber corrector, WITHOUT Jacobi scaling or damping
//   H    = J^T J, split into cameras (c) and lines (l);  S = H_cc - sum_lines H_cl H_ll^-1 H_lc
//   Σ_cc = S^-1 (6F x 6F, cross blocks included);  Σ_ll = H_ll^-1 + K Σ_cc K^T with K = H_ll^-1 H_lc, per free line (its 4 x 4 marginal)
// fp64 throughout.  One workgroup of four waves per window, three passes:
//   1. wave <-> line, lane <-> observation (lane_linearise, the routine of every sweep): H_ll by a wave sum, factored after symmetric
//      scaling to unit diagonal with the pivot test below; the observation's H_cc block and the line's Schur blocks
//      (H_cl H_ll^-1) H_lc go into the LDS image of S (lower triangle) by fp64 LDS atomics;
//   2. Cholesky of S scaled to unit diagonal in LDS, L^-1 by one forward substitution per column (kept in the upper triangle),
//      Σ_cc = D L^-T L^-1 D into memory and into the lower triangle, which pass 3 reads;
//   3. (lines requested) wave <-> line again: the blocks are formed a second time (2000 x (4 x 6F) of K do not fit LDS) and Σ_ll
//      written at the caller's line index.
// MEASURED (MI355X, bench batch of 1024 windows x 2000 lines, profiles/lba_covariance_bench.txt): 14.4 ms without, 33.5 ms with the lines,
// beside 1.72 ms for one LM iteration: passes 1 and 3 give a wave to ONE line (~10 of 64 lanes busy) - packing several lines into a
// wave pass as the sweeps' tiles do, and L^-1 by row blocks over all 256 threads, are the next steps.
// SINGULAR: a pivot <= 1e-10 of a unit-diagonal factorisation (any free line's block, or S - a window without a constant camera has
// a 6-dimensional gauge null space) makes the window SLSLAM_COV_SINGULAR with zero outputs; the other windows are not affected.
// LDS: 8 (1 + 21 C + 2 max(6F, 6) + 6F (6F + 1)) + C bytes: 127 KB at 64 cameras of which 20 free (one workgroup per CU), 35 KB for the
// bench shape's 20 cameras of which 10 free; 256 registers hold it to two workgroups per CU.  The launch is sized for the largest window the batch was made for.
// Tiled and fused motion-only batches only: the 240 x 240 system of a W = 40 window (global-memory path) does not fit LDS - the
// call returns SLSLAM_ERR_UNSUPPORTED for such a batch and for a mixed one.
#ifndef SLSLAM_LBA_COVARIANCE_H_
#define SLSLAM_LBA_COVARIANCE_H_

#include "lba_kernels.h"

namespace slslam {

enum { kCovThreads = 256, kCovWaves = 4 };
enum { kCovHdr = 24 };                   // ints per window: status | free cameras F | free_camera[20] | pad
enum { kCovOk = 0, kCovSingular = 1 };   // = SLSLAM_COV_OK / SLSLAM_COV_SINGULAR (include/slslam_hip.h)
constexpr double kCovPivotMin = 1e-10;

__host__ __device__ inline int cov_ld(int n) { return n + 1; }       // odd row stride (doubles): a column walks all banks
__host__ __device__ inline size_t lds_bytes_covariance(int C, int n) {
  const int nv = n > 6 ? n : 6;
  return sizeof(double) * (size_t)(1 + C * kCamTab + 2 * nv + n * cov_ld(n)) + (size_t)((C + 7) & ~7);
}

__host__ __device__ constexpr int cov_tri(int i, int j) { return i * (i + 1) / 2 + j; }     // i >= j

// Inverse of a symmetric positive definite 4 x 4 (lower triangle, packed by rows) through the Cholesky factor of the matrix scaled
// to unit diagonal.  false: a diagonal entry is not positive or a pivot is <= kCovPivotMin.
__device__ __forceinline__ bool cov_inv4(const double (&h)[10], double (&inv)[10]) {
  double d[4], A[4][4], Lm[4][4], X[4][4], r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!(h[cov_tri(i, i)] > 0.0)) return false;
    d[i] = 1.0 / sqrt(h[cov_tri(i, i)]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i][j] = h[cov_tri(i, j)] * d[i] * d[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double pv = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) pv -= Lm[j][k] * Lm[j][k];
    if (!(pv > kCovPivotMin)) return false;
    r[j] = 1.0 / sqrt(pv);
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = s * r[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {                         // X = L^-1
    X[j][j] = r[j];
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) s += Lm[i][k] * X[k][j];
      X[i][j] = -s * r[i];
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = a; k < 4; ++k) s += X[k][a] * X[k][b];
      inv[cov_tri(a, b)] = s * d[a] * d[b];
    }
  return true;
}

// The blocks of one line, lane <-> observation: H_ll^-1 (every lane), E = J_c^T J_l (6 x 4, the lane's block of H_cl) and
// G = E H_ll^-1 for the lanes whose camera is free (`act`).  false: the line's block failed the pivot test.
__device__ __forceinline__ bool cov_line_blocks(const LaneLin& L, bool act, double (&hinv)[10], double (&E)[24], double (&G)[24]) {
  double h[10];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) v += L.Jl[4 * q + a] * L.Jl[4 * q + b];
      h[cov_tri(a, b)] = wave_sum(L.valid ? v : 0.0);
    }
  if (!cov_inv4(h, hinv)) return false;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) v += L.Jc[6 * q + a] * L.Jl[4 * q + b];
      E[4 * a + b] = act ? v : 0.0;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      double v = 0.0;
#pragma unroll
      for (int c = 0; c < 4; ++c) v += E[4 * a + c] * hinv[c >= b ? cov_tri(c, b) : cov_tri(b, c)];
      G[4 * a + b] = v;
    }
  return true;
}

// hdr [nwin][kCovHdr]; cov_cam [nwin][cam_stride]: row-major (6F)^2 at the front of the window's slot; cov_line [nline][16] or nullptr:
// the block of a line at (the window's first line record + its caller index).  Ccap / ncap: what the launch's LDS was sized for.
__global__ __launch_bounds__(kCovThreads, 2) void k_lba_covariance(BatchPtrs p, Policy pol, const int* line_orig, int* hdr, double* cov_cam,
                                                                long long cam_stride, double* cov_line, int Ccap, int ncap) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (w >= p.nwin) return;
  const WinDesc wd = p.wins[w];
  const int n = wd.n, ld = cov_ld(n), nv = n > 6 ? n : 6;
  int* my_hdr = hdr + (long long)w * kCovHdr;
  double* out = cov_cam + (long long)w * cam_stride;
  if (wd.C > Ccap || n > ncap || n != 6 * wd.Cf || wd.Cf > kMaxFreeCams) {            // (not a window this launch was sized for)
    if (tid == 0) { my_hdr[0] = kCovSingular; my_hdr[1] = 0; }
    return;
  }
  const int cur = p.state[w].cur;
  int* flag = reinterpret_cast<int*>(smem);
  double* camtab = smem + 1;
  double* dvec = camtab + wd.C * kCamTab;        // the cameras' (unit) scale while the table is built, then S's diagonal scaling
  double* rvec = dvec + nv;                      // 1 / L_kk
  double* S = rvec + nv;
  signed char* camcf = reinterpret_cast<signed char*>(S + n * ld);
  if (tid == 0) *flag = 0;
  if (wave == 0) load_cam_table<true>(p, wd, cur, lane, camtab, dvec, camcf, true);
  for (int q = tid; q < n * ld; q += kCovThreads) S[q] = 0.0;
  __syncthreads();
  if (tid == 0) { my_hdr[0] = kCovOk; my_hdr[1] = wd.Cf; }
  for (int c = tid; c < wd.C; c += kCovThreads) { const int cf = camcf[c]; if (cf >= 0 && cf < kMaxFreeCams) my_hdr[2 + cf] = c; }

  // ---- pass 1: S (lower triangle) = H_cc - sum over free lines of (H_cl H_ll^-1) H_lc
  for (int l = wave; l < wd.L; l += kCovWaves) {
    const int ls = wd.line_off + l;
    const int o0 = p.line_ptr[ls], k = p.line_ptr[ls + 1] - o0;
    if (k <= 0) continue;
    const int lflags = p.line_flags[ls];
    LaneLin L;
    double ob[8];
    lane_linearise<false>(p, pol, camtab, dvec, camcf, ls, lane, k, o0, true, lflags, cur, wd.obs_off, L, ob);
    const bool act = L.valid && L.cf >= 0;
    if (act) {
      double* blk = S + (6 * L.cf) * ld + 6 * L.cf;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          double v = 0.0;
#pragma unroll
          for (int q = 0; q < 4; ++q) v += L.Jc[6 * q + a] * L.Jc[6 * q + b];
          lds_add(&blk[a * ld + b], v);
        }
    }
    if (lflags & 1) continue;                              // a constant line: H_cc only
    double hinv[10], E[24], G[24];
    if (!cov_line_blocks(L, act, hinv, E, G)) { if (lane == 0) *flag = 1; continue; }
    for (unsigned long long m = __ballot(act); m; m &= m - 1) {
      const int j = __ffsll((unsigned long long)m) - 1;
      const int cfj = __shfl(L.cf, j);
      double Ej[24];
#pragma unroll
      for (int q = 0; q < 24; ++q) Ej[q] = __shfl(E[q], j);
      if (act && cfj <= L.cf) {
        double* blk = S + (6 * L.cf) * ld + 6 * cfj;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            double v = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) v += G[4 * a + c] * Ej[4 * b + c];
            if (cfj < L.cf || b <= a) lds_add(&blk[a * ld + b], -v);
          }
      }
    }
  }
  __syncthreads();
  bool singular = *flag != 0;

  // ---- pass 2: Σ_cc = S^-1 through the Cholesky factor of S scaled to unit diagonal
  const int ti = tid >> 4, tj = tid & 15;
  if (!singular) {
    for (int a = tid; a < n; a += kCovThreads) {
      const double v = S[a * ld + a];
      if (!(v > 0.0)) *flag = 1;
      dvec[a] = v > 0.0 ? 1.0 / sqrt(v) : 0.0;
    }
    __syncthreads();
    singular = *flag != 0;
  }
  if (!singular) {
    for (int i = ti; i < n; i += 16)
      for (int j = tj; j <= i; j += 16) S[i * ld + j] *= dvec[i] * dvec[j];
    for (int k = 0; k < n; ++k) {                          // right-looking; column k stays unscaled until the end
      __syncthreads();
      const double pv = S[k * ld + k];
      if (!(pv > kCovPivotMin)) { singular = true; break; }     // (every thread reads the same pivot)
      const double rr = 1.0 / pv;
      if (tid == 0) rvec[k] = 1.0 / sqrt(pv);
      for (int i = k + 1 + ti; i < n; i += 16) {
        const double lik = S[i * ld + k] * rr;
        for (int j = k + 1 + tj; j <= i; j += 16) S[i * ld + j] -= lik * S[j * ld + k];
      }
    }
  }
  __syncthreads();
  if (!singular) {
    for (int i = ti; i < n; i += 16)
      for (int j = tj; j < i; j += 16) S[i * ld + j] *= rvec[j];
    __syncthreads();
    // X = L^-1, column j by thread j, X[i][j] (i > j) kept at S[j][i]; X[j][j] = rvec[j]
    for (int j = tid; j < n; j += kCovThreads) {
      const double* xr = S + j * ld;
      for (int i = j + 1; i < n; ++i) {
        const double* li = S + i * ld;
        double s = li[j] * rvec[j];
        for (int k = j + 1; k < i; ++k) s += li[k] * xr[k];
        S[j * ld + i] = -s * rvec[i];
      }
    }
    __syncthreads();
    // Σ[a][b] = d_a d_b sum_{k >= a} X[k][a] X[k][b] (a >= b): to memory (both halves) and to the lower triangle (L is not needed any more)
    for (int a = ti; a < n; a += 16)
      for (int b = tj; b <= a; b += 16) {
        const double* xa = S + a * ld;
        const double* xb = S + b * ld;
        double s = rvec[a] * (a == b ? rvec[a] : xb[a]);
        for (int k = a + 1; k < n; ++k) s += xa[k] * xb[k];
        const double v = s * dvec[a] * dvec[b];
        S[a * ld + b] = v;
        out[(long long)a * n + b] = v;
        out[(long long)b * n + a] = v;
      }
    __syncthreads();
  }
  if (singular) {
    if (tid == 0) my_hdr[0] = kCovSingular;
    for (int q = tid; q < n * n; q += kCovThreads) out[q] = 0.0;
  }
  if (!cov_line) return;

  // ---- pass 3: Σ_ll = H_ll^-1 + K Σ_cc K^T of every free line, zeros for the others
  for (int l = wave; l < wd.L; l += kCovWaves) {
    const int ls = wd.line_off + l;
    const int o0 = p.line_ptr[ls], k = p.line_ptr[ls + 1] - o0;
    const int lflags = p.line_flags[ls];
    double* ol = cov_line + 16 * ((long long)wd.line_off + line_orig[ls]);
    if (singular || k <= 0 || (lflags & 1)) {
      if (lane < 16) ol[lane] = 0.0;
      continue;
    }
    LaneLin L;
    double ob[8];
    lane_linearise<false>(p, pol, camtab, dvec, camcf, ls, lane, k, o0, true, lflags, cur, wd.obs_off, L, ob);
    const bool act = L.valid && L.cf >= 0;
    double hinv[10], E[24], G[24];
    if (!cov_line_blocks(L, act, hinv, E, G)) {            // (cannot happen: pass 1 passed the same block)
      if (lane < 16) ol[lane] = 0.0;
      continue;
    }
    double T[24];                                          // sum_j Σ[cf, cf_j] G_j  (6 x 4)
#pragma unroll
    for (int q = 0; q < 24; ++q) T[q] = 0.0;
    for (unsigned long long m = __ballot(act); m; m &= m - 1) {
      const int j = __ffsll((unsigned long long)m) - 1;
      const int cfj = __shfl(L.cf, j);
      double Gj[24];
#pragma unroll
      for (int q = 0; q < 24; ++q) Gj[q] = __shfl(G[q], j);
      if (act) {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            const int row = 6 * L.cf + a, col = 6 * cfj + b;
            const double sg = row >= col ? S[row * ld + col] : S[col * ld + row];
#pragma unroll
            for (int c = 0; c < 4; ++c) T[4 * a + c] += sg * Gj[4 * b + c];
          }
      }
    }
    double res[10];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int d = 0; d <= c; ++d) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) v += G[4 * a + c] * T[4 * a + d];
        res[cov_tri(c, d)] = hinv[cov_tri(c, d)] + wave_sum(act ? v : 0.0);
      }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int d = 0; d < 4; ++d) ol[4 * c + d] = res[c >= d ? cov_tri(c, d) : cov_tri(d, c)];
    }
  }
}

}  // namespace slslam
#endif  // SLSLAM_LBA_COVARIANCE_H_

// slslam_amd/csrc/lba_report.h — which observations the Huber loss down-weighted and which line is depth-degenerate, for every
// window of a resident LBA batch.  The LBA counterpart of slslam_po_edge_report; Ceres: ceres::Problem::Evaluate with
// per-block residuals.
//
// Evaluated at the parameters the batch holds on the device (the accepted buffer: what slslam_lba_batch_linearise and
// slslam_lba_batch_covariance evaluate), with a = Policy.huber_delta (a <= 0: no loss):
//   per observation i (ALL of them, the constant-camera / constant-line ones the reduced program drops included), caller's order:
//     sq_norm[i] = s_i = |r_i|^2 of the four raw residuals;  weight[i] = rho'(s_i) = 1 if s_i <= a^2 or a <= 0, else a / sqrt(s_i)
//   per line, caller's index (slslam_lba_line_report): status, observations, observations with weight < 1, sum s_i, cost = sum rho(s_i) / 2,
//     min_pivot (free lines): H_ll = sum J_l^T J_l over the line's observations (J_l after the corrector: the covariance's H_ll),
//     scaled to unit diagonal and Cholesky-factored - the smallest value under the square roots up to and including the first
//     non-positive one; a non-positive diagonal entry gives that entry.  The number k_lba_covariance tests against 1e-10.
//   per camera, caller's index (slslam_lba_camera_report): status, observations, down-weighted ones, sum s_i, cost.
// fp64 throughout.  Reads the batch, writes only its own buffers: nothing the solve or the covariance reads is touched, the sin / cos
// table of the lines included - the accepted buffer's table is current whenever a batch can be asked (k_reset writes it with the
// initial point, the back-substitution writes the candidate's before a step is accepted).
//
// Two launches for all windows:
//   k_lba_report_tiles  one wave per chunk, the sweeps' tile layout (lba_types.h): lane <-> observation, several lines per 64-lane pass,
//                       lane_linearise; the 14 per-line sums (H_ll's 10, s, cost, two counts) close inside the tile by seg_sum_n - row-local
//                       DPP scans, cross-row sums for kTileMultiRow tiles - and the first lane of every run factors its line's 4 x 4 once.
//                       Per-camera sums: fp64 LDS atomics into the chunk's table (one wave: a fixed order), written as the chunk's partial.
//   k_lba_report_cameras one wave per window: the chunks' partials added in chunk order (bitwise reproducible), the cameras' records.
// Windows of the global-memory path (lba_big.h: more than 64 observations on a line, more than 64 cameras or 20 free ones) have no tiles:
//   k_lba_report_lines   one workgroup of four waves per window, wave <-> line over line_ptr, lane <-> observation 64 at a time; every wave
//                       keeps a camera table of its own in LDS, added in wave order at the end - one launch, no partials.
#ifndef SLSLAM_LBA_REPORT_H_
#define SLSLAM_LBA_REPORT_H_

#include "lba_kernels.h"

namespace slslam {

enum { kRepLineFree = 0, kRepLineConstant = 1, kRepLineNoObs = 2 };   // = SLSLAM_LBA_LINE_* / SLSLAM_LBA_CAMERA_* (include/slslam_hip.h)
enum { kRepCamAcc = 4 };                 // doubles per camera of a partial: sum s | cost | observations | down-weighted ones
enum { kRepLinesThreads = 256, kRepLinesWaves = 4 };

struct RepLine { int status, num_observations, num_downweighted, pad; double sq_norm_sum, cost, min_pivot; };   // = slslam_lba_line_report
struct RepCam { int status, num_observations, num_downweighted, pad; double sq_norm_sum, cost; };              // = slslam_lba_camera_report

struct ReportPtrs {
  const int* ob_orig;        // [nobs] sorted observation -> its place in the caller's order (window-local)
  const int* line_orig;      // [nline] sorted line -> caller's line index (window-local)
  double* sq_norm;           // [nobs] at WinDesc.obs_off + caller's index
  double* weight;
  RepLine* lines;            // [nline] at WinDesc.line_off + caller's index
  RepCam* cams;              // [ncam] at WinDesc.cam_off + camera
  double* cam_part;          // [nchunk][cam_stride] per-chunk camera sums (tiled batches)
  long long cam_stride;      // kRepCamAcc x the largest camera count the batch was made for
};

__host__ __device__ inline size_t lds_bytes_report_tiles(int C, int n) {
  return sizeof(double) * (size_t)(C * kCamTab + (n > 0 ? n : 6) + C * kRepCamAcc) + (size_t)((C + 7) & ~7);
}
__host__ __device__ inline size_t lds_bytes_report_lines(int C, int n) {
  return sizeof(double) * (size_t)(C * kCamTab + (n > 0 ? n : 6) + kRepLinesWaves * C * kRepCamAcc) + (size_t)((C + 7) & ~7);
}

// rho'(s) of the Huber loss (the semantics of slslam_po_edge_report)
__device__ __forceinline__ double report_weight(double s, double a) { return (a > 0.0 && s > a * a) ? a / sqrt(s) : 1.0; }

// The smallest value under the square roots of the Cholesky factorisation of h (lower triangle, packed by rows) scaled to unit
// diagonal, up to and including the first non-positive one; a non-positive diagonal entry: the smallest diagonal entry.
__device__ __forceinline__ double report_min_pivot(const double (&h)[10]) {
  double d[4], A[4][4], Lm[4][4];
  double dmin = h[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) dmin = fmin(dmin, h[tri_index(i, i)]);
  if (!(dmin > 0.0)) return dmin;
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = 1.0 / sqrt(h[tri_index(i, i)]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i][j] = h[tri_index(i, j)] * d[i] * d[j];
  double pmin = __builtin_huge_val();
  bool live = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double pv = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) pv -= Lm[j][k] * Lm[j][k];
    if (live) pmin = fmin(pmin, pv);
    live = live && pv > 0.0;
    const double r = live ? 1.0 / sqrt(pv) : 0.0;
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= Lm[i][k] * Lm[j][k];
      Lm[i][j] = s * r;
    }
  }
  return pmin;
}

// What an observation adds to its line's sums: H_ll's lower triangle | s | cost | 1 | down-weighted; zeros for a lane without one.
__device__ __forceinline__ void report_terms(const LaneLin& L, double s, double wgt, double (&v)[14]) {
  int q = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b <= a; ++b) {
      double h = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) h += L.Jl[4 * r + a] * L.Jl[4 * r + b];
      v[q++] = L.valid ? h : 0.0;
    }
  v[10] = L.valid ? s : 0.0;
  v[11] = L.valid ? L.cost : 0.0;
  v[12] = L.valid ? 1.0 : 0.0;
  v[13] = (L.valid && wgt < 1.0) ? 1.0 : 0.0;
}

// The record of one line from its sums (one lane per line)
__device__ __forceinline__ void report_store_line(const ReportPtrs& rp, const WinDesc& wd, int ls, int lflags, const double (&v)[14]) {
  RepLine out;
  const int k = (int)v[12];
  out.status = (lflags & 1) ? kRepLineConstant : k > 0 ? kRepLineFree : kRepLineNoObs;
  out.num_observations = k; out.num_downweighted = (int)v[13]; out.pad = 0;
  out.sq_norm_sum = v[10]; out.cost = v[11];
  double h[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) h[q] = v[q];
  out.min_pivot = out.status == kRepLineFree ? report_min_pivot(h) : 0.0;
  rp.lines[(long long)wd.line_off + rp.line_orig[ls]] = out;
}

__device__ __forceinline__ void report_store_obs(const ReportPtrs& rp, const WinDesc& wd, int o, double s, double wgt) {
  const long long at = (long long)wd.obs_off + rp.ob_orig[o];
  rp.sq_norm[at] = s; rp.weight[at] = wgt;
}

__device__ __forceinline__ void report_cam_add(double* acc, int cam, double s, double cost, double wgt) {
  double* a = acc + cam * kRepCamAcc;
  lds_add(a, s); lds_add(a + 1, cost); lds_add(a + 2, 1.0);
  if (wgt < 1.0) lds_add(a + 3, 1.0);
}

__device__ __forceinline__ void report_store_cam(const ReportPtrs& rp, const WinDesc& wd, int c, int cf, const double (&a)[kRepCamAcc]) {
  RepCam out;
  const int k = (int)a[2];
  out.status = k <= 0 ? kRepLineNoObs : cf >= 0 ? kRepLineFree : kRepLineConstant;
  out.num_observations = k; out.num_downweighted = (int)a[3]; out.pad = 0;
  out.sq_norm_sum = a[0]; out.cost = a[1];
  rp.cams[(long long)wd.cam_off + c] = out;
}

// ------------------------------------------------------------------------------------------
// Tiled and fused motion-only batches: one wave per chunk.  Ccap / ncap: what the launch's LDS was sized for.
__global__ __launch_bounds__(64) void k_lba_report_tiles(BatchPtrs p, Policy pol, ReportPtrs rp, int Ccap, int ncap) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= p.nchunk) return;
  const Chunk ck = p.chunks[blockIdx.x];
  if (ck.win < 0) return;                              // an unused entry of a refillable batch's chunk array (lba_types.h)
  const WinDesc wd = p.wins[ck.win];
  if (wd.C > Ccap || wd.n > ncap || kRepCamAcc * (long long)wd.C > rp.cam_stride) return;     // (not a window this launch was sized for)
  const int cur = p.state[ck.win].cur;
  double* camtab = smem;
  double* camscale = camtab + wd.C * kCamTab;
  double* camacc = camscale + (wd.n > 0 ? wd.n : 6);
  signed char* camcf = reinterpret_cast<signed char*>(camacc + wd.C * kRepCamAcc);
  load_cam_table<true>(p, wd, cur, lane, camtab, camscale, camcf, true);
  for (int q = lane; q < wd.C * kRepCamAcc; q += 64) camacc[q] = 0.0;
  __syncthreads();
  for (int t = ck.tile_begin; t < ck.tile_end; ++t) {
    const TileCtx tc = fetch_tile(p, t, ck.tile_end, lane);
    const SegCtx sg = make_seg(tc, lane);
    LaneLin L;
    double ob[8], s = 0.0;
    lane_linearise<false>(p, pol, camtab, camscale, camcf, tc.ls, tc.j, tc.k, tc.o0, tc.line_ok, tc.lflags, cur, wd.obs_off, L, ob, nullptr, false, &s);
    const double wgt = report_weight(s, pol.huber_delta);
    if (L.valid) {
      report_store_obs(rp, wd, tc.o0 + tc.j, s, wgt);
      report_cam_add(camacc, L.cam, s, L.cost, wgt);
    }
    double v[14];
    report_terms(L, s, wgt, v);
    seg_sum_n<14>(v, sg);
    if (tc.line_ok && tc.j == 0) report_store_line(rp, wd, tc.ls, tc.lflags, v);
  }
  __syncthreads();
  double* part = rp.cam_part + (long long)ck.id * rp.cam_stride;
  for (int q = lane; q < wd.C * kRepCamAcc; q += 64) part[q] = camacc[q];
}

// ... and the cameras' records: the partials of a window's chunks added in chunk order; lane <-> camera
__global__ __launch_bounds__(64) void k_lba_report_cameras(BatchPtrs p, ReportPtrs rp) {
  const int w = blockIdx.x, lane = threadIdx.x;
  if (w >= p.nwin) return;
  const WinDesc wd = p.wins[w];
  if (kRepCamAcc * (long long)wd.C > rp.cam_stride) return;
  for (int c = lane; c < wd.C; c += 64) {
    double a[kRepCamAcc] = { 0.0, 0.0, 0.0, 0.0 };
    for (int k = 0; k < wd.nchunks; ++k) {
      const double* part = rp.cam_part + (long long)(wd.chunk_off + k) * rp.cam_stride + c * kRepCamAcc;
#pragma unroll
      for (int q = 0; q < kRepCamAcc; ++q) a[q] += part[q];
    }
    report_store_cam(rp, wd, c, p.cam_cf[wd.cam_off + c], a);
  }
}

// ------------------------------------------------------------------------------------------
// Windows of the global-memory path: one workgroup per window, wave <-> line, lane <-> observation (64 at a time, in order).
__global__ __launch_bounds__(kRepLinesThreads) void k_lba_report_lines(BatchPtrs p, Policy pol, ReportPtrs rp, int Ccap, int ncap) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (w >= p.nwin) return;
  const WinDesc wd = p.wins[w];
  if (wd.C > Ccap || wd.n > ncap) return;              // (not a window this launch was sized for)
  const int cur = p.state[w].cur;
  double* camtab = smem;
  double* camscale = camtab + wd.C * kCamTab;
  double* camacc = camscale + (wd.n > 0 ? wd.n : 6);
  signed char* camcf = reinterpret_cast<signed char*>(camacc + kRepLinesWaves * wd.C * kRepCamAcc);
  if (wave == 0) load_cam_table<true>(p, wd, cur, lane, camtab, camscale, camcf, true);
  for (int q = tid; q < kRepLinesWaves * wd.C * kRepCamAcc; q += kRepLinesThreads) camacc[q] = 0.0;
  __syncthreads();
  double* myacc = camacc + wave * wd.C * kRepCamAcc;
  for (int l = wave; l < wd.L; l += kRepLinesWaves) {
    const int ls = wd.line_off + l;
    const int o0 = p.line_ptr[ls], k = p.line_ptr[ls + 1] - o0;
    const int lflags = p.line_flags[ls];
    double tot[14];
#pragma unroll
    for (int q = 0; q < 14; ++q) tot[q] = 0.0;
    for (int j0 = 0; j0 < k; j0 += 64) {
      LaneLin L;
      double ob[8], s = 0.0, v[14];
      lane_linearise<false>(p, pol, camtab, camscale, camcf, ls, j0 + lane, k, o0, true, lflags, cur, wd.obs_off, L, ob, nullptr, false, &s);
      const double wgt = report_weight(s, pol.huber_delta);
      if (L.valid) {
        report_store_obs(rp, wd, o0 + j0 + lane, s, wgt);
        report_cam_add(myacc, L.cam, s, L.cost, wgt);
      }
      report_terms(L, s, wgt, v);
#pragma unroll
      for (int q = 0; q < 14; ++q) tot[q] += wave_sum(v[q]);
    }
    if (lane == 0) report_store_line(rp, wd, ls, lflags, tot);
  }
  __syncthreads();
  for (int c = tid; c < wd.C; c += kRepLinesThreads) {
    double a[kRepCamAcc];
#pragma unroll
    for (int q = 0; q < kRepCamAcc; ++q) {
      double x = 0.0;
      for (int wv = 0; wv < kRepLinesWaves; ++wv) x += camacc[(wv * wd.C + c) * kRepCamAcc + q];
      a[q] = x;
    }
    report_store_cam(rp, wd, c, camcf[c], a);
  }
}

}  // namespace slslam
#endif  // SLSLAM_LBA_REPORT_H_

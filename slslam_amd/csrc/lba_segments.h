// slslam_amd/csrc/lba_segments.h — the 3-D segment of every line landmark of every window of a resident LBA batch:
// the extent of a solved infinite line along its direction, from the image segments that observed it.  The reference's
// SLAM::extend_end_points (src/slam.cpp:979-1084, extension_length = 5.0 in src/parameter.h:62), per observation.
//
// Evaluated at the parameters the batch holds on the device (the accepted buffer: what slslam_lba_batch_report and _covariance
// evaluate), for EVERY line of the window, constant ones included.  A line u = (a, b, g, t) is cp + s dv with cp its point closest to
// the origin and dv its unit direction (line_points in lba_math.h: the residual's); a segment is an interval [t_min, t_max] of s.
//   per observation of line l from camera c (R, t_c world to camera), LEFT image only (obs[0..3] = x0 y0 x1 y1), caller's order:
//     pc = R cp + t_c, dc = R dv;  ln = (p1 x p2)[0:2] / |.| with p = (x, y, 1), |ln| = sqrt(lx^2 + ly^2) = 0 or a non-finite input: DEGENERATE
//     per endpoint p: the plane through the camera centre, p and p + (ln, 0) has the normal m = p x (ln, 0) and cuts the line at
//       s = -(m . pc) / (m . dc) (the reference's Lc * pi);  |m . dc| <= 1e-6 |m| for either endpoint: DEGENERATE
//     (pc + s dc).z < 0 for either endpoint: BEHIND (slam.cpp:1037)
//     max_range > 0: q = pc . dc, p0 = pc - q dc (the line's point closest to the camera centre); |p0| > max_range: OUT_OF_RANGE; else
//       e = sqrt(max_range^2 - |p0|^2) and an endpoint with |s + q| > e moves to s = sign(s + q) e - q: USED_CLAMPED (slam.cpp:1029-1056)
//     lo = min(s1, s2), hi = max(s1, s2); lo == hi: COLLAPSED (slam.cpp:1057); else USED / USED_CLAMPED
//     obs_status[i], obs_range[2 i] = lo, hi - zeros unless USED / USED_CLAMPED
//   per line, caller's index (slslam_lba_line_segment): status, observations, used ones, clamped ones, t_min = min lo and t_max = max hi over
//     the used observations, p_min = cp + t_min dv, p_max = cp + t_max dv in the window's world frame; all doubles 0 unless OK.
// The union over a line's observations is what the reference's keyframe-by-keyframe update (slam.cpp:1065-1074) arrives at for a line that
// does not move; its reset of tt when the direction pvn turns is map bookkeeping and stays with the caller.
// fp64, no atomics.  Reads the batch, writes only its own buffers.  min and max do not depend on the order of the observations and the
// counts are exact: a window's bytes do not depend on its batch.
//
// One launch for all windows:
//   k_lba_segments_tiles  one wave per chunk, the sweeps' tile layout (lba_types.h): lane <-> observation, several lines per 64-lane pass,
//                         residual-only geometry (cam_rotation, line_points: no Jacobians); the line's min lo / max hi close inside the tile by
//                         seg_min_n - seg_sum_n's twin: row-local DPP scans, cross-row for kTileMultiRow tiles -, its three counts by
//                         seg_sum_n, and the first lane of every run writes its line's record.  A line's run lies inside one tile and a
//                         chunk is a range of tiles: no line spans chunks, nothing is combined afterwards.
// Windows of the global-memory path (lba_big.h) have no tiles:
//   k_lba_segments_lines  one workgroup of four waves per window, wave <-> line over line_ptr, lane <-> observation 64 at a time.
#ifndef SLSLAM_LBA_SEGMENTS_H_
#define SLSLAM_LBA_SEGMENTS_H_

#include "lba_kernels.h"
#include "segment_eval.h"      // segment_eval: steps 1-5 of the contract for one observation

namespace slslam {

enum { kSegOk = 0, kSegNoObs = 1, kSegNone = 2 };                                                                                     // = SLSLAM_SEGMENT_*
enum { kSegLinesThreads = 256, kSegLinesWaves = 4 };

struct SegLine { int status, num_observations, num_used, num_clamped; double t_min, t_max, p_min[3], p_max[3]; };   // = slslam_lba_line_segment

struct SegmentPtrs {
  const int* ob_orig;        // [nobs] sorted observation -> its place in the caller's order (window-local)
  const int* line_orig;      // [nline] sorted line -> caller's line index (window-local)
  int* obs_status;           // [nobs] at WinDesc.obs_off + caller's index
  double* obs_range;         // [2 nobs] lo, hi
  SegLine* lines;            // [nline] at WinDesc.line_off + caller's index
  double max_range;          // <= 0: no clamp, nothing out of range
};

__host__ __device__ inline size_t lds_bytes_segments(int C, int n) { return sizeof(double) * (size_t)lds_doubles_cost(C, n); }

// Min over the lanes of a line's run, result in every lane of the run: seg_sum_n's twin.  Inclusive prefix along the 16-lane row
// restricted to the lane's own run (row_shr by 1, 2, 4, 8; the source is in the same run AND the same row iff the lane's position in
// the row's part of the run is >= d - a lane whose source lies outside the row reads 0, which a sum may add and a minimum may not),
// then every lane fetches the row's value from the run's last lane in the row.  Runs that span rows (they start on a row boundary) take
// the minimum of their rows' values.  A maximum is the minimum of the negated values, exactly.
template <int CTRL>
__device__ __forceinline__ double seg_min_step(double v, bool m) {
  const double x = dpp_shift0<CTRL>(v);
  return fmin(v, m ? x : v);
}
template <int N>
__device__ __forceinline__ void seg_min_n(double (&v)[N], const SegCtx& s, int lane) {
  const int jr = s.j < (lane & 15) ? s.j : (lane & 15);
  if (s.max_run > 1) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = seg_min_step<0x111>(v[q], jr >= 1);
  }
  if (s.max_run > 2) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = seg_min_step<0x112>(v[q], jr >= 2);
  }
  if (s.max_run > 4) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = seg_min_step<0x114>(v[q], jr >= 4);
  }
  if (s.max_run > 8) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = seg_min_step<0x118>(v[q], jr >= 8);
  }
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = bperm64(v[q], s.rl4);
  if (s.multirow) {
    const bool spans = s.r1 > s.r0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double tot = __builtin_huge_val();
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = bperm64(v[q], 64 * r);      // lane 16 r belongs to the run whenever the run covers row r
        if (r >= s.r0 && r <= s.r1) tot = fmin(tot, x);
      }
      if (spans) v[q] = tot;
    }
  }
}
__device__ __forceinline__ double wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// The record of one line (one lane per line): vmin = min lo, -max hi over its used observations
__device__ __forceinline__ void segments_store_line(const SegmentPtrs& sp, const WinDesc& wd, int ls, int nobs, int nused, int nclamped,
                                                    double vlo, double vnhi, const double (&cp)[3], const double (&dv)[3]) {
  SegLine out;
  out.status = nobs <= 0 ? kSegNoObs : nused > 0 ? kSegOk : kSegNone;
  out.num_observations = nobs; out.num_used = nused; out.num_clamped = nclamped;
  const bool ok = out.status == kSegOk;
  out.t_min = ok ? vlo : 0.0; out.t_max = ok ? -vnhi : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out.p_min[i] = ok ? cp[i] + out.t_min * dv[i] : 0.0;
    out.p_max[i] = ok ? cp[i] + out.t_max * dv[i] : 0.0;
  }
  sp.lines[(long long)wd.line_off + sp.line_orig[ls]] = out;
}

// One lane's observation: loads, geometry, the per-observation outputs.  Returns the status, or -1 for a lane without an observation.
__device__ __forceinline__ int segments_lane(const BatchPtrs& p, const SegmentPtrs& sp, const WinDesc& wd, const double* camtab, int cur,
                                             int ls, bool line_ok, int o, bool valid, double (&cp)[3], double (&dv)[3], double& lo, double& hi) {
  lo = 0.0; hi = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { cp[i] = 0.0; dv[i] = 0.0; }
  if (!line_ok) return -1;
  const double* lrec = p.line_x + line_rec(p, ls, cur);
  double trig[7];
#pragma unroll
  for (int q = 0; q < 7; ++q) trig[q] = lrec[4 + q];
  line_points<double>(trig, cp, dv);
  if (!valid) return -1;
  const double2 e0 = reinterpret_cast<const double2*>(p.ob)[o];                        // left image: planes 0 and 1 of the four
  const double2 e1 = reinterpret_cast<const double2*>(p.ob)[p.ob_stride + o];
  const double e[4] = { e0.x, e0.y, e1.x, e1.y };
  const double* ct = camtab + p.ob_cam[o] * kCamTab;
  double R[9], t[3];
#pragma unroll
  for (int q = 0; q < 9; ++q) R[q] = ct[q];
  t[0] = ct[18]; t[1] = ct[19]; t[2] = ct[20];
  const int status = segment_eval(R, t, cp, dv, e, sp.max_range, lo, hi);
  const long long at = (long long)wd.obs_off + sp.ob_orig[o];
  sp.obs_status[at] = status;
  reinterpret_cast<double2*>(sp.obs_range)[at] = make_double2(lo, hi);
  return status;
}

// ------------------------------------------------------------------------------------------
// Tiled and fused motion-only batches: one wave per chunk.  Ccap / ncap: what the launch's LDS was sized for.
__global__ __launch_bounds__(64) void k_lba_segments_tiles(BatchPtrs p, SegmentPtrs sp, int Ccap, int ncap) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= p.nchunk) return;
  const Chunk ck = p.chunks[blockIdx.x];
  if (ck.win < 0) return;                              // an unused entry of a refillable batch's chunk array (lba_types.h)
  const WinDesc wd = p.wins[ck.win];
  if (wd.C > Ccap || wd.n > ncap) return;              // (not a window this launch was sized for)
  const int cur = p.state[ck.win].cur;
  double* camtab = smem;
  double* camscale = camtab + wd.C * kCamTab;
  signed char* camcf = reinterpret_cast<signed char*>(camscale + (wd.n > 0 ? wd.n : 6));
  load_cam_table<false>(p, wd, cur, lane, camtab, camscale, camcf, true);
  __syncthreads();
  for (int t = ck.tile_begin; t < ck.tile_end; ++t) {
    const TileCtx tc = fetch_tile(p, t, ck.tile_end, lane);
    const SegCtx sg = make_seg(tc, lane);
    const bool valid = tc.line_ok && tc.j < tc.k;
    double cp[3], dv[3], lo, hi;
    const int status = segments_lane(p, sp, wd, camtab, cur, tc.ls, tc.line_ok, tc.o0 + tc.j, valid, cp, dv, lo, hi);
    const bool used = status == kSegObsUsed || status == kSegObsUsedClamped;
    double v[2] = { used ? lo : __builtin_huge_val(), used ? -hi : __builtin_huge_val() };
    double n[3] = { valid ? 1.0 : 0.0, used ? 1.0 : 0.0, status == kSegObsUsedClamped ? 1.0 : 0.0 };
    seg_min_n<2>(v, sg, lane);
    seg_sum_n<3>(n, sg);
    if (tc.line_ok && tc.j == 0) segments_store_line(sp, wd, tc.ls, (int)n[0], (int)n[1], (int)n[2], v[0], v[1], cp, dv);
  }
}

// ------------------------------------------------------------------------------------------
// Windows of the global-memory path: one workgroup per window, wave <-> line, lane <-> observation (64 at a time).
__global__ __launch_bounds__(kSegLinesThreads) void k_lba_segments_lines(BatchPtrs p, SegmentPtrs sp, int Ccap, int ncap) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (w >= p.nwin) return;
  const WinDesc wd = p.wins[w];
  if (wd.C > Ccap || wd.n > ncap) return;              // (not a window this launch was sized for)
  const int cur = p.state[w].cur;
  double* camtab = smem;
  double* camscale = camtab + wd.C * kCamTab;
  signed char* camcf = reinterpret_cast<signed char*>(camscale + (wd.n > 0 ? wd.n : 6));
  if (wave == 0) load_cam_table<false>(p, wd, cur, lane, camtab, camscale, camcf, true);
  __syncthreads();
  for (int l = wave; l < wd.L; l += kSegLinesWaves) {
    const int ls = wd.line_off + l;
    const int o0 = p.line_ptr[ls], k = p.line_ptr[ls + 1] - o0;
    double vlo = __builtin_huge_val(), vnhi = __builtin_huge_val(), cp[3], dv[3];
    int nused = 0, nclamped = 0;
    for (int j0 = 0; j0 < (k > 0 ? k : 1); j0 += 64) {       // (a line without observations: one pass for cp and dv)
      double lo, hi;
      const int status = segments_lane(p, sp, wd, camtab, cur, ls, true, o0 + j0 + lane, j0 + lane < k, cp, dv, lo, hi);
      const bool used = status == kSegObsUsed || status == kSegObsUsedClamped;
      vlo = fmin(vlo, wave_min(used ? lo : __builtin_huge_val()));
      vnhi = fmin(vnhi, wave_min(used ? -hi : __builtin_huge_val()));
      nused += __popcll(__ballot(used));
      nclamped += __popcll(__ballot(status == kSegObsUsedClamped));
    }
    if (lane == 0) segments_store_line(sp, wd, ls, k, nused, nclamped, vlo, vnhi, cp, dv);
  }
}

}  // namespace slslam
#endif  // SLSLAM_LBA_SEGMENTS_H_

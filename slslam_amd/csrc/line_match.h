// slslam_amd/csrc/line_match.h — the kernels of the line matcher (include/slslam_hip.h: slslam_line_matcher_*): every
// observation of a frame against every map line under the frame's predicted pose, many frames per launch, reduced to matches.
//
//   k_match_lines   lane <-> line.  The part of SLAM::reprojection_error that does not look at the observation (ransac_device.h:
//                   line_normals) once per line instead of once per pair: the two image-line normals nc / (float)sql, 6 doubles; for a
//                   frame with extents also the line in the left camera (pc, dc) and its interval widened by the margin, 14 doubles.
//                   Written as a structure of arrays (value c of line l at soa[c Ltot + l]): the pair kernel's tile loads are coalesced.
//   k_match_pairs   one wave per (frame, 64 observations): lane <-> observation, its 8 doubles in registers.  The frame's lines stream
//                   through LDS in tiles of kTile = 64 (a lane fetches the next tile's line while the wave works on this one) and are
//                   read by broadcast: every lane reads line j of the tile at the same address.  Per pair the four dot products and the
//                   float accumulation (normals_error), the compare, for a frame with extents and only for pairs that passed it
//                   segment_cut and the interval test, then the lane's running (best, second, count).  Lines go by in ascending order and
//                   the lowest line wins a tie (mutual_match.h: take_pair).  The key of line l's best observation (offer_key) carries
//                   the float bits of e: e >= 0, so its bits order as e does.
// The mutual and ratio tests are mutual_match.h's k_mutual_finish: observations are its rows, lines its columns.
#ifndef SLSLAM_LINE_MATCH_H_
#define SLSLAM_LINE_MATCH_H_

#include <hip/hip_runtime.h>

#include "mutual_match.h"
#include "ransac_device.h"
#include "segment_eval.h"

// (as ransac_device.h: the reference's separate multiplies and adds, the admissibility test sits on a threshold)
#pragma clang fp contract(off)

namespace slslam_match {

enum { kTile = 64, kLineValues = 6, kLineValuesExt = 14 };

// Per frame, where its inputs lie in the upload and its results in the output arrays
struct FrameDesc {
  long long pose, obs, lines, ext;      // doubles: [12], [8 K], [6 L], [2 L] (ext < 0: the frame has no extents)
  slslam::Span span;                    // observations (a0, n) and lines (j0, m)
  int run, pad;                         // run = 0: EMPTY or INVALID_POSE - no pair is evaluated, the outputs say "nothing admissible"
};

using Out = slslam::MatchOut;         // best = best_line, best_value / second_value = the errors, best_row = best_observation

// blockIdx = (64 lines, frame)
__global__ __launch_bounds__(64) void k_match_lines(const FrameDesc* __restrict__ fr, const double* __restrict__ dd, double baseline, double margin,
                                                    long long Ltot, double* __restrict__ soa) {
  const FrameDesc fd = fr[blockIdx.y];
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (!fd.run || l >= fd.span.m) return;
  double n[2][3], pc[3], dc[3];
  slslam_ransac::line_normals(dd + fd.pose, dd + fd.lines + 6 * (long long)l, baseline, n, pc, dc);
  double* o = soa + fd.span.j0 + l;
#pragma unroll
  for (int c = 0; c < 6; ++c) o[c * Ltot] = n[c / 3][c % 3];
  if (fd.ext < 0) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) { o[(6 + c) * Ltot] = pc[c]; o[(9 + c) * Ltot] = dc[c]; }
  o[12 * Ltot] = dd[fd.ext + 2 * (long long)l] - margin;
  o[13 * Ltot] = dd[fd.ext + 2 * (long long)l + 1] + margin;
}

// One lane's observation ob against every line of the frame.  tile: kTile * NV doubles of LDS, line j of the tile at tile[NV j].
template <bool EXT>
__device__ __forceinline__ void match_sweep(const FrameDesc& fd, const double* __restrict__ soa, long long Ltot, const double (&ob)[8], int k,
                                            bool kvalid, double thr, double* tile, unsigned long long* __restrict__ lbest, float& best,
                                            float& second, int& best_line, int& count) {
  constexpr int NV = EXT ? kLineValuesExt : kLineValues;
  const int lane = threadIdx.x;
  const double* src = soa + fd.span.j0;
  const double el[4] = { ob[0], ob[1], ob[2], ob[3] };
  double nxt[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) nxt[c] = lane < fd.span.m ? src[c * Ltot + lane] : 0.0;
  for (int l0 = 0; l0 < fd.span.m; l0 += kTile) {
    __syncthreads();                                             // (the wave is done with the tile before)
#pragma unroll
    for (int c = 0; c < NV; ++c) tile[NV * lane + c] = nxt[c];
    __syncthreads();
    const int ln = l0 + kTile + lane;
#pragma unroll
    for (int c = 0; c < NV; ++c) nxt[c] = ln < fd.span.m ? src[c * Ltot + ln] : 0.0;
    const int nl = fd.span.m - l0 < kTile ? fd.span.m - l0 : kTile;
    for (int j = 0; j < nl; ++j) {
      const double* t = tile + NV * j;
      const double n[2][3] = { { t[0], t[1], t[2] }, { t[3], t[4], t[5] } };
      const float e = slslam_ransac::normals_error(n, ob);
      bool adm = kvalid && isfinite(e) && (double)e < thr;
      if (EXT) {
        if (adm) {
          const double pc[3] = { t[6], t[7], t[8] }, dc[3] = { t[9], t[10], t[11] };
          double lo, hi;
          const int st = slslam::segment_cut(pc, dc, el, 0.0, lo, hi);
          adm = st == slslam::kSegObsUsed && hi >= t[12] && lo <= t[13];
        }
      }
      slslam::offer_key(adm, __float_as_uint(e), k, lbest, fd.span.j0 + l0 + j);
      slslam::take_pair(adm, e, l0 + j, best, second, best_line, count);
    }
  }
}

// blockIdx = (64 observations, frame)
__global__ __launch_bounds__(64) void k_match_pairs(const FrameDesc* __restrict__ fr, const double* __restrict__ dd, const double* __restrict__ soa,
                                                    long long Ltot, double thr, unsigned long long* __restrict__ lbest, Out out) {
  __shared__ __attribute__((aligned(16))) double tile[kTile * kLineValuesExt];
  const FrameDesc fd = fr[blockIdx.y];
  const int k = blockIdx.x * 64 + threadIdx.x;
  if ((int)blockIdx.x * 64 >= fd.span.n) return;                      // (the whole wave)
  const bool kvalid = k < fd.span.n;
  double ob[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ob[q] = kvalid ? dd[fd.obs + 8 * (long long)k + q] : 0.0;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_line = -1, count = 0;
  if (fd.run) {
    if (fd.ext >= 0) match_sweep<true>(fd, soa, Ltot, ob, k, kvalid, thr, tile, lbest, best, second, best_line, count);
    else match_sweep<false>(fd, soa, Ltot, ob, k, kvalid, thr, tile, lbest, best, second, best_line, count);
  }
  if (!kvalid) return;
  const long long at = fd.span.a0 + k;
  out.best[at] = best_line; out.best_value[at] = best; out.second_value[at] = second; out.num_admissible[at] = count;
}

}  // namespace slslam_match

#endif  // SLSLAM_LINE_MATCH_H_

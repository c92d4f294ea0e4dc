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
//                   only a strictly smaller error replaces the best: the lowest line wins a tie whatever the launch geometry.  The best
//                   observation of line l is a 64-bit minimum over (float bits of e << 32 | k) - e >= 0, so its bits order as e does, and
//                   the low word breaks ties towards the lowest k -, taken across the wave by shuffles and once per wave by atomicMin on
//                   global memory: a minimum does not depend on the order it is taken in.
//   k_match_finish  lane <-> observation and lane <-> line: the mutual and ratio tests, best_observation out of its key, num_matched by a
//                   ballot and one integer atomicAdd per wave.
// No fp atomics, no sums of floating-point values across lanes: a frame's bytes do not depend on its place in the call.
#ifndef SLSLAM_LINE_MATCH_H_
#define SLSLAM_LINE_MATCH_H_

#include <hip/hip_runtime.h>

#include "ransac_device.h"
#include "segment_eval.h"

// (as ransac_device.h: the reference's separate multiplies and adds, the admissibility test sits on a threshold)
#pragma clang fp contract(off)

namespace slslam_match {

enum { kTile = 64, kLineValues = 6, kLineValuesExt = 14 };
constexpr unsigned long long kNoObservation = ~0ull;

// Per frame, where its inputs lie in the upload and its results in the output arrays
struct FrameDesc {
  long long pose, obs, lines, ext;      // doubles: [12], [8 K], [6 L], [2 L] (ext < 0: the frame has no extents)
  long long k0, l0;                     // the frame's first observation / line among those of all frames
  int K, L;
  int run, pad;                         // run = 0: EMPTY or INVALID_POSE - no pair is evaluated, the outputs say "nothing admissible"
};

// Where the results of all frames go: [F], then [Ktot] each, then [Ltot]
struct Out {
  int* num_matched;
  int *match, *best_line, *num_admissible;
  float *best_error, *second_error;
  int* best_observation;
};

// blockIdx = (64 lines, frame)
__global__ __launch_bounds__(64) void k_match_lines(const FrameDesc* __restrict__ fr, const double* __restrict__ dd, double baseline, double margin,
                                                    long long Ltot, double* __restrict__ soa) {
  const FrameDesc fd = fr[blockIdx.y];
  const int l = blockIdx.x * 64 + threadIdx.x;
  if (!fd.run || l >= fd.L) return;
  double n[2][3], pc[3], dc[3];
  slslam_ransac::line_normals(dd + fd.pose, dd + fd.lines + 6 * (long long)l, baseline, n, pc, dc);
  double* o = soa + fd.l0 + l;
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
  const double* src = soa + fd.l0;
  const double el[4] = { ob[0], ob[1], ob[2], ob[3] };
  double nxt[NV];
#pragma unroll
  for (int c = 0; c < NV; ++c) nxt[c] = lane < fd.L ? src[c * Ltot + lane] : 0.0;
  for (int l0 = 0; l0 < fd.L; l0 += kTile) {
    __syncthreads();                                             // (the wave is done with the tile before)
#pragma unroll
    for (int c = 0; c < NV; ++c) tile[NV * lane + c] = nxt[c];
    __syncthreads();
    const int ln = l0 + kTile + lane;
#pragma unroll
    for (int c = 0; c < NV; ++c) nxt[c] = ln < fd.L ? src[c * Ltot + ln] : 0.0;
    const int nl = fd.L - l0 < kTile ? fd.L - l0 : kTile;
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
      if (__ballot(adm) != 0ull) {                                // (wave-uniform)
        unsigned long long key = adm ? ((unsigned long long)__float_as_uint(e) << 32) | (unsigned)k : kNoObservation;
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long other = __shfl_xor(key, o);
          key = other < key ? other : key;
        }
        if (lane == 0) atomicMin(&lbest[fd.l0 + l0 + j], key);
      }
      if (adm) {
        ++count;
        if (e < best) { second = best; best = e; best_line = l0 + j; }
        else if (e < second) second = e;
      }
    }
  }
}

// blockIdx = (64 observations, frame)
__global__ __launch_bounds__(64) void k_match_pairs(const FrameDesc* __restrict__ fr, const double* __restrict__ dd, const double* __restrict__ soa,
                                                    long long Ltot, double thr, unsigned long long* __restrict__ lbest, Out out) {
  __shared__ __attribute__((aligned(16))) double tile[kTile * kLineValuesExt];
  const FrameDesc fd = fr[blockIdx.y];
  const int k = blockIdx.x * 64 + threadIdx.x;
  if ((int)blockIdx.x * 64 >= fd.K) return;                      // (the whole wave)
  const bool kvalid = k < fd.K;
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
  const long long at = fd.k0 + k;
  out.best_line[at] = best_line; out.best_error[at] = best; out.second_error[at] = second; out.num_admissible[at] = count;
}

// blockIdx = (64 observations and 64 lines, frame)
__global__ __launch_bounds__(64) void k_match_finish(const FrameDesc* __restrict__ fr, const unsigned long long* __restrict__ lbest, double ratio,
                                                     Out out) {
  const FrameDesc fd = fr[blockIdx.y];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if ((int)blockIdx.x * 64 >= fd.K && (int)blockIdx.x * 64 >= fd.L) return;      // (the whole wave)
  if (i < fd.L) {
    const unsigned long long key = lbest[fd.l0 + i];
    out.best_observation[fd.l0 + i] = key == kNoObservation ? -1 : (int)(unsigned)(key & 0xffffffffull);
  }
  bool matched = false;
  if (i < fd.K) {
    const long long at = fd.k0 + i;
    const int bl = out.best_line[at];
    if (bl >= 0) {
      const unsigned long long key = lbest[fd.l0 + bl];
      const bool mutual = key != kNoObservation && (int)(unsigned)(key & 0xffffffffull) == i;
      const bool unambiguous = ratio <= 1.0 || (double)out.best_error[at] * ratio <= (double)out.second_error[at];
      matched = mutual && unambiguous;
    }
    out.match[at] = matched ? bl : -1;
  }
  const int n = __popcll(__ballot(matched));
  if (threadIdx.x == 0 && n > 0) atomicAdd(&out.num_matched[blockIdx.y], n);
}

}  // namespace slslam_match

#endif  // SLSLAM_LINE_MATCH_H_

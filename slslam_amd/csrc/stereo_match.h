// slslam_amd/csrc/stereo_match.h — the kernels of the stereo line matcher (include/slslam_hip.h: slslam_stereo_matcher_*):
// every left segment of a rectified stereo frame against every right segment, first by the epipolar gate (stereo_match_layout.h:
// gate_admits), then by the place recogniser's descriptor distance, many frames per launch, reduced to mutual, unambiguous matches and
// written out as stereo line observations.
//
//   k_stereo_pairs  one wave per (frame, 64 left segments): lane <-> left segment, its geometry in registers.  The frame's right segments
//                   are staged in LDS once (end points, the slope dx / dy - so that no pair divides -, the valid flag); the wave's 64
//                   left descriptors are staged transposed as k_desc_pairs stages its queries (stride 65).
//                   Pass 1, the gate: right segments go by in ascending order in groups of kGroup = 8; a lane reads a right segment
//                   from one LDS address for the whole wave (a broadcast) and keeps the group's eight verdicts as a byte at
//                   s_mask[group][lane] (neighbouring lanes, neighbouring bytes); a ballot per group says whether any lane admits any
//                   of its eight: bit g of the wave-uniform word `active`.
//                   Pass 2, the chains: only the groups whose bit is set, in ascending order.  The right descriptors are row-major in
//                   the upload; a group is 8 D contiguous floats.  Lane l fetches value i = l / 8 + 8 c of segment j = l % 8 and
//                   writes tile[i][j] = tile[l + 64 c]: 64 neighbouring banks, no conflict; the fetch touches eight 32-byte pieces.
//                   The next active group is fetched into registers while the wave works on this one.  Then the eight chains
//                   r_j = 1.0f; r_j -= q[i] * k_j[i] side by side from two 16-byte broadcast reads per i, as in k_desc_pairs, and per
//                   right segment offer_key / take_pair (mutual_match.h) under (verdict, r finite, r < max_distance).
//                   A skipped group would have offered and taken nothing: its verdicts are all false.  The result's bytes are those
//                   of the loop over every group.
//   k_mutual_finish (mutual_match.h), unchanged: left segments are its rows, right segments its columns.
//   k_stereo_emit   lane <-> left segment: segment_status, and for a MATCHED segment the eight normalised doubles and the two
//                   disparities (stereo_match_layout.h: emit_row).
// No fp atomics, no sums of floating-point values across lanes: a frame's bytes do not depend on its place in the call.
#ifndef SLSLAM_STEREO_MATCH_H_
#define SLSLAM_STEREO_MATCH_H_

#include <hip/hip_runtime.h>

#include "mutual_match.h"
#include "stereo_match_layout.h"

// every product and difference of the chain and of the gate is rounded on its own
#pragma STDC FP_CONTRACT OFF

namespace slslam_stereo {

using slslam::ordered;

constexpr int kQueryStride = 65;        // floats between value i and value i + 1 of the staged left descriptors (descriptor_match.h)
constexpr int kTileLoads = kMaxD / 8;   // floats a lane fetches for a group of the largest D

using Out = slslam::MatchOut;         // best_value / second_value = the distances, best_row = best_left

// The upload's regions on the device (stereo_match_layout.h: CallLayout)
struct In {
  const FrameDesc* frames;
  const float4 *lseg, *rseg;
  const int *lok, *rok;
  const float *ldesc, *rdesc;
};

struct EmitOut {
  int* status;                          // [A]
  double* observations;                 // [A 8]
  double* disparity;                    // [A 2]
};

// dynamic LDS of k_stereo_pairs: the group's tile [D][8] and the left descriptors [D][kQueryStride]
inline size_t pairs_lds_bytes(int D) { return 4 * ((size_t)D * kGroup + (size_t)D * kQueryStride); }

// blockIdx = (64 left segments, frame); dynamic LDS pairs_lds_bytes(D)
__global__ __launch_bounds__(64) void k_stereo_pairs(In in, int D, Gate gate, unsigned long long* __restrict__ keys, Out out) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  __shared__ float4 s_rseg[kMaxSegments];
  __shared__ double s_rslope[kMaxSegments];
  __shared__ unsigned char s_rok[kMaxSegments];
  __shared__ unsigned char s_mask[kMaxGroups * 64];
  float* tile = s_mem;                                           // [D][8]: the group the wave works on
  const float4* tile4 = reinterpret_cast<const float4*>(s_mem);
  float* sq = s_mem + (size_t)D * kGroup;                        // [D][kQueryStride]
  const slslam::Span sp = in.frames[blockIdx.y].span;
  const int lane = threadIdx.x;
  const int a_base = blockIdx.x * 64;
  if (a_base >= sp.n) return;                                    // (the whole wave)
  const int a = a_base + lane;
  const bool avalid = a < sp.n;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_j = -1, count = 0;
  const int m = sp.m;
  if (m > 0) {
    // ---- the lane's left segment; the frame's right segments
    const float4 ls = avalid ? in.lseg[sp.a0 + a] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool aok = avalid && in.lok[sp.a0 + a] != 0;
    const Segment A = segment_of(ls.x, ls.y, ls.z, ls.w);
    for (int b = lane; b < m; b += 64) {
      const float4 rs = in.rseg[sp.j0 + b];
      s_rseg[b] = rs;
      s_rslope[b] = slope_of(rs.x, rs.y, rs.z, rs.w);
      s_rok[b] = in.rok[sp.j0 + b] != 0 ? 1 : 0;
    }
    // the wave's left descriptors, transposed: rows are contiguous in the upload, read coalesced; rows past n are zeros
    {
      const int rows = sp.n - a_base < 64 ? sp.n - a_base : 64;
      const float* src = in.ldesc + ((size_t)sp.a0 + (size_t)a_base) * D;
      int row = 0, i = lane;
      for (int e = lane; e < 64 * D; e += 64) {
        while (i >= D) { i -= D; ++row; }
        sq[i * kQueryStride + row] = row < rows ? src[e] : 0.0f;
        i += 64;
      }
    }
    __syncthreads();

    // ---- pass 1: the gate
    const int ng = (m + kGroup - 1) / kGroup;
    unsigned long long active = 0ull;
    for (int g = 0; g < ng; ++g) {
      unsigned mask = 0u;
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        if (j < m) {                                             // (wave-uniform)
          const float4 rs = s_rseg[j];
          const Segment B = segment_with(rs.x, rs.y, rs.z, rs.w, s_rslope[j]);
          const bool adm = aok && s_rok[j] != 0 && gate_admits(A, B, gate);
          mask |= adm ? 1u << jj : 0u;
        }
      }
      s_mask[g * 64 + lane] = (unsigned char)mask;               // (read back by this lane alone)
      if (__ballot(mask != 0u) != 0ull) active |= 1ull << g;
    }

    // ---- pass 2: the chains of the groups somebody admits
    const int nc = D / 8;                                        // floats a lane fetches per group
    const int tj = lane & 7, ti = lane >> 3;
    const float* rd = in.rdesc + (size_t)sp.j0 * D;
    float nxt[kTileLoads];
    int g = active != 0ull ? __ffsll((long long)active) - 1 : -1;
    if (g >= 0) {
      const int j = g * kGroup + tj;
#pragma unroll
      for (int c = 0; c < kTileLoads; ++c) nxt[c] = (c < nc && j < m) ? rd[(size_t)j * D + ti + 8 * c] : 0.0f;
    }
    while (g >= 0) {
      __syncthreads();                                           // (the wave is done with the group before)
#pragma unroll
      for (int c = 0; c < kTileLoads; ++c)
        if (c < nc) tile[lane + 64 * c] = nxt[c];
      __syncthreads();
      const unsigned long long rest = g + 1 < 64 ? active >> (g + 1) : 0ull;
      const int gn = rest != 0ull ? g + 1 + (__ffsll((long long)rest) - 1) : -1;
      if (gn >= 0) {
        const int j = gn * kGroup + tj;
#pragma unroll
        for (int c = 0; c < kTileLoads; ++c) nxt[c] = (c < nc && j < m) ? rd[(size_t)j * D + ti + 8 * c] : 0.0f;
      }
      float r[kGroup];
#pragma unroll
      for (int j = 0; j < kGroup; ++j) r[j] = 1.0f;
      for (int d = 0; d < D; ++d) {
        const float qi = sq[d * kQueryStride + lane];
        const float4 k0 = tile4[2 * d], k1 = tile4[2 * d + 1];
        const float kv[kGroup] = { k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w };
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const float p = qi * kv[j];
          r[j] = r[j] - p;
        }
      }
      const unsigned mask = s_mask[g * 64 + lane];
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        const float rj = r[jj];
        const bool adm = ((mask >> jj) & 1u) != 0u && isfinite(rj) && (double)rj < gate.max_distance;
        slslam::offer_key(adm, ordered(rj), a, keys, sp.j0 + j);
        slslam::take_pair(adm, rj, j, best, second, best_j, count);
      }
      g = gn;
    }
  }
  if (!avalid) return;
  const long long at = sp.a0 + a;
  out.best[at] = best_j; out.best_value[at] = best; out.second_value[at] = second; out.num_admissible[at] = count;
}

// blockIdx = (64 left segments, frame); after k_mutual_finish
__global__ __launch_bounds__(64) void k_stereo_emit(In in, Gate gate, Camera cam, const int* __restrict__ match, EmitOut eo) {
  const slslam::Span sp = in.frames[blockIdx.y].span;
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= sp.n) return;
  const long long at = sp.a0 + a;
  const float4 ls = in.lseg[at];
  const Segment A = segment_of(ls.x, ls.y, ls.z, ls.w);
  const int b = match[at];
  const int st = status_of(in.lok[at], A, gate, b);
  eo.status[at] = st;
  if (st != kMatched) return;
  const float4 rs = in.rseg[sp.j0 + b];
  const Segment B = segment_of(rs.x, rs.y, rs.z, rs.w);
  double obs[8], disp[2];
  emit_row(A, B, cam, obs, disp);
#pragma unroll
  for (int q = 0; q < 8; ++q) eo.observations[8 * at + q] = obs[q];
  eo.disparity[2 * at] = disp[0];
  eo.disparity[2 * at + 1] = disp[1];
}

}  // namespace slslam_stereo

#endif  // SLSLAM_STEREO_MATCH_H_

// slslam_amd/csrc/descriptor_match.h — the kernels of the descriptor matcher (include/slslam_hip.h: slslam_descriptor_matcher_*, DESIGN.md
// 6.6): every descriptor of a query frame against every descriptor of a stored keyframe by the place recogniser's distance, many
// (frame, candidate keyframe) pairs per launch, reduced to mutual, unambiguous matches.
//
//   k_desc_pairs    one wave per (pair, 64 query descriptors): lane <-> query descriptor.  The wave's 64 query descriptors are staged
//                   transposed in LDS (gated_pairs.h: stage_rows).  The keyframe's descriptors stream through LDS in groups of
//                   kGroup = 8 (a lane fetches the next group while the wave works on this one); the store holds a group as [D][8],
//                   so value i of its eight descriptors is two 16-byte reads at one address for the whole wave: a broadcast.  Each
//                   lane carries the eight chains r_j = 1.0f; r_j -= q[i] * k_j[i] side by side (gated_pairs.h: group_chains), as
//                   slslam_place::nearest_child does with kChildBlock: one chain alone would wait D times for its own last subtraction.
//                   Then per keyframe descriptor the compare and the lane's running (best, second, count).  Descriptors go by in
//                   ascending j: the lowest j wins a tie (mutual_match.h: take_pair).  The key of keyframe descriptor j's best query
//                   descriptor (offer_key) carries ordered(r), which maps the float's bits to an unsigned that orders as the float
//                   does: r may be below zero.
// The mutual and ratio tests are mutual_match.h's k_mutual_finish: query descriptors are its rows, keyframe descriptors its columns.
// The chain's order is the contract's: a pair's bytes do not depend on its place in the call.
#ifndef SLSLAM_DESCRIPTOR_MATCH_H_
#define SLSLAM_DESCRIPTOR_MATCH_H_

#include <hip/hip_runtime.h>

#include "gated_pairs.h"
#include "mutual_match.h"

namespace slslam_desc {

constexpr int kMaxD = 128, kMaxDescriptors = 512, kMaxCandidates = 8;
using slslam::gated::kGroup;            // keyframe descriptors whose chains a lane carries at a time
using slslam::gated::pairs_lds_bytes;   // dynamic LDS of k_desc_pairs
constexpr int kGroupLoads = 2 * kMaxD / 64;       // 16-byte loads a lane makes for a group of the largest D

// floats of a group in the store and in LDS: [D][kGroup]
__host__ __device__ inline size_t group_floats(int D) { return (size_t)D * kGroup; }

// Per (query frame, candidate keyframe), where its inputs lie and where its results go
struct PairDesc {
  long long q;                          // float offset of the frame's [n][D] descriptors in the upload
  long long k;                          // float offset of the keyframe in the store: ceil(m / 8) groups of [D][8], zeros past m
  slslam::Span span;                    // query descriptors (a0, n) and keyframe descriptors (j0, m)
  int run, pad;                         // run = 0: EMPTY or INVALID_DESCRIPTOR - no pair is evaluated, the outputs say "none"
};

using Out = slslam::MatchOut;         // best_value / second_value = the distances, best_row = best_query

using slslam::ordered;                 // (mutual_match.h: the stereo matcher's keys carry the same word)

// blockIdx = (64 query descriptors, pair); dynamic LDS pairs_lds_bytes(D)
__global__ __launch_bounds__(64) void k_desc_pairs(const PairDesc* __restrict__ pairs, const float* __restrict__ qd,
                                                   const float* __restrict__ store, int D, double max_distance,
                                                   unsigned long long* __restrict__ keys, Out out) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  float4* tile4 = reinterpret_cast<float4*>(s_mem);              // [D][8]: the group the wave works on
  float* sq = s_mem + group_floats(D);                           // [D][kQueryStride]
  const PairDesc pd = pairs[blockIdx.y];
  const int lane = threadIdx.x;
  const int a_base = blockIdx.x * 64;
  if (a_base >= pd.span.n) return;                                    // (the whole wave)
  const int a = a_base + lane;
  const bool avalid = a < pd.span.n;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_j = -1, count = 0;
  if (pd.run) {
    // the wave's rows are contiguous in the upload: element e = row D + i, read coalesced; rows past n are zeros (never admissible)
    slslam::gated::stage_rows(sq, qd + pd.q + (size_t)a_base * D, pd.span.n - a_base < 64 ? pd.span.n - a_base : 64, D, lane);
    const int ng = (pd.span.m + kGroup - 1) / kGroup;
    const int n4 = 2 * D;                                        // 16-byte words of a group
    const float4* kp = reinterpret_cast<const float4*>(store + pd.k);
    float4 nxt[kGroupLoads];
#pragma unroll
    for (int c = 0; c < kGroupLoads; ++c) {
      const int w = lane + 64 * c;
      nxt[c] = w < n4 ? kp[w] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    for (int g = 0; g < ng; ++g) {
      __syncthreads();                                           // (the wave is done with the group before; the first time: sq is written)
#pragma unroll
      for (int c = 0; c < kGroupLoads; ++c) {
        const int w = lane + 64 * c;
        if (w < n4) tile4[w] = nxt[c];
      }
      __syncthreads();
      if (g + 1 < ng) {
        const float4* np = kp + (size_t)(g + 1) * n4;
#pragma unroll
        for (int c = 0; c < kGroupLoads; ++c) {
          const int w = lane + 64 * c;
          if (w < n4) nxt[c] = np[w];
        }
      }
      float r[kGroup];
      slslam::gated::group_chains(sq, tile4, D, lane, r);
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        const float rj = r[jj];
        const bool adm = avalid && j < pd.span.m && isfinite(rj) && (double)rj < max_distance;
        slslam::offer_key(adm, ordered(rj), a, keys, pd.span.j0 + j);
        slslam::take_pair(adm, rj, j, best, second, best_j, count);
      }
    }
  }
  if (!avalid) return;
  const long long at = pd.span.a0 + a;
  out.best[at] = best_j; out.best_value[at] = best; out.second_value[at] = second; out.num_admissible[at] = count;
}

}  // namespace slslam_desc

#endif  // SLSLAM_DESCRIPTOR_MATCH_H_

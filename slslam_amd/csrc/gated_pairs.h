// slslam_amd/csrc/gated_pairs.h — the pair kernel of the matchers that compare descriptors by the place recogniser's distance (DESIGN.md
// 6.6, 6.9): lane <-> row, the wave's 64 row descriptors staged transposed in LDS, the columns going by in ascending order in groups of
// kGroup = 8 whose chains r_j = 1.0f; r_j -= q[i] * k_j[i] a lane carries side by side.
//
//   stage_rows     the transposed staging of the wave's row descriptors: k_desc_pairs (descriptor_match.h) and k_gated_pairs
//   group_chains   the eight chains of one group from the tile [D][8] in LDS: the same two
//   k_gated_pairs  the whole pair kernel of a gated problem - the stereo matcher's (stereo_match.h) and the tracker's (line_track.h):
//                  a geometric gate first, the chains only for the groups somebody admits.  What differs between the two is a Problem:
//                    In, Gate, FrameDesc (its Span in .span, as k_mutual_finish asks), Segment
//                    Columns          what a wave keeps of the problem's columns in LDS (trivially default-constructible)
//                    row(...)         this lane's row as a Segment, and whether it may match at all
//                    stage(...)       column b into Columns
//                    admits(...)      does the row admit column j: the column's flag and the gate
//                    row_descriptors, column_descriptors   where the [.][D] floats lie; both are indexed by a0 / j0 of the span
// No fp atomics, no sums of floating-point values across lanes: a problem's bytes do not depend on its place in the call.
#ifndef SLSLAM_GATED_PAIRS_H_
#define SLSLAM_GATED_PAIRS_H_

#include <hip/hip_runtime.h>

#include <type_traits>

#include "call_layout.h"
#include "mutual_match.h"

// every product and difference of the chain is rounded on its own
#pragma STDC FP_CONTRACT OFF

namespace slslam {
namespace gated {

constexpr int kQueryStride = 65;        // floats between value i and value i + 1 of the staged row descriptors: the lanes read
                                        // neighbouring banks, and the staging writes - neighbouring lanes, neighbouring i - miss a common one
constexpr int kTileLoads = kMaxD / 8;   // floats a lane fetches for a group of the largest D

// dynamic LDS of a pair kernel: the group's tile [D][kGroup] and the row descriptors [D][kQueryStride]
inline size_t pairs_lds_bytes(int D) { return 4 * ((size_t)D * kGroup + (size_t)D * kQueryStride); }

// The wave's `rows` row descriptors, contiguous at src, to sq[i * kQueryStride + row]: element e = row D + i, read coalesced; rows past
// `rows` are zeros
__device__ __forceinline__ void stage_rows(float* sq, const float* __restrict__ src, int rows, int D, int lane) {
  int row = 0, i = lane;
  for (int e = lane; e < 64 * D; e += 64) {
    while (i >= D) { i -= D; ++row; }
    sq[i * kQueryStride + row] = row < rows ? src[e] : 0.0f;
    i += 64;
  }
}

// The lane's eight chains against the group in tile4 ([D][8]: two 16-byte reads at one address for the whole wave per value)
__device__ __forceinline__ void group_chains(const float* sq, const float4* tile4, int D, int lane, float (&r)[kGroup]) {
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
}

// blockIdx = (64 rows, problem); dynamic LDS pairs_lds_bytes(D)
template <typename Problem>
__global__ __launch_bounds__(64) void k_gated_pairs(typename Problem::In in, int D, typename Problem::Gate gate,
                                                    unsigned long long* __restrict__ keys, MatchOut out) {
  static_assert(std::is_trivially_default_constructible<typename Problem::Columns>::value, "Columns lies in LDS: nothing constructs it");
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  __shared__ typename Problem::Columns s_cols;
  __shared__ unsigned char s_mask[kMaxGroups * 64];
  float* tile = s_mem;                                           // [D][8]: the group the wave works on
  const float4* tile4 = reinterpret_cast<const float4*>(s_mem);
  float* sq = s_mem + (size_t)D * kGroup;                        // [D][kQueryStride]
  const typename Problem::FrameDesc fd = in.frames[blockIdx.y];
  const Span sp = fd.span;
  const int lane = threadIdx.x;
  const int a_base = blockIdx.x * 64;
  if (a_base >= sp.n) return;                                    // (the whole wave)
  const int a = a_base + lane;
  const bool avalid = a < sp.n;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_j = -1, count = 0;
  const int m = sp.m;
  if (m > 0) {
    // ---- the lane's row; the problem's columns; the wave's row descriptors
    bool aok;
    const typename Problem::Segment A = Problem::row(in, sp.a0 + a, avalid, gate, aok);
    for (int b = lane; b < m; b += 64) Problem::stage(s_cols, in, fd, gate, b);
    stage_rows(sq, Problem::row_descriptors(in) + ((size_t)sp.a0 + (size_t)a_base) * D, sp.n - a_base < 64 ? sp.n - a_base : 64, D, lane);
    __syncthreads();

    // ---- pass 1: the gate.  A lane reads a column from one LDS address for the whole wave (a broadcast) and keeps the group's eight
    // verdicts as a byte; a ballot per group says whether any lane admits any of its eight: bit g of the wave-uniform word `active`
    const int ng = (m + kGroup - 1) / kGroup;
    unsigned long long active = 0ull;
    for (int g = 0; g < ng; ++g) {
      unsigned mask = 0u;
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        if (j < m) {                                             // (wave-uniform)
          const bool adm = aok && Problem::admits(s_cols, A, j, gate);
          mask |= adm ? 1u << jj : 0u;
        }
      }
      s_mask[g * 64 + lane] = (unsigned char)mask;               // (read back by this lane alone)
      if (__ballot(mask != 0u) != 0ull) active |= 1ull << g;
    }

    // ---- pass 2: the chains of the groups somebody admits.  The column descriptors are row-major: a group is 8 D contiguous floats.
    // Lane l fetches value i = l / 8 + 8 c of column j = l % 8 and writes tile[i][j] = tile[l + 64 c]: 64 neighbouring banks.  The
    // next active group is fetched into registers while the wave works on this one.  A skipped group would have offered and taken
    // nothing: its verdicts are all false
    const int nc = D / 8;                                        // floats a lane fetches per group
    const int tj = lane & 7, ti = lane >> 3;
    const float* cd = Problem::column_descriptors(in) + (size_t)sp.j0 * D;
    float nxt[kTileLoads];
    int g = active != 0ull ? __ffsll((long long)active) - 1 : -1;
    if (g >= 0) {
      const int j = g * kGroup + tj;
#pragma unroll
      for (int c = 0; c < kTileLoads; ++c) nxt[c] = (c < nc && j < m) ? cd[(size_t)j * D + ti + 8 * c] : 0.0f;
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
        for (int c = 0; c < kTileLoads; ++c) nxt[c] = (c < nc && j < m) ? cd[(size_t)j * D + ti + 8 * c] : 0.0f;
      }
      float r[kGroup];
      group_chains(sq, tile4, D, lane, r);
      const unsigned mask = s_mask[g * 64 + lane];
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        const float rj = r[jj];
        const bool adm = ((mask >> jj) & 1u) != 0u && isfinite(rj) && (double)rj < gate.max_distance;
        offer_key(adm, ordered(rj), a, keys, sp.j0 + j);
        take_pair(adm, rj, j, best, second, best_j, count);
      }
      g = gn;
    }
  }
  if (!avalid) return;
  const long long at = sp.a0 + a;
  out.best[at] = best_j; out.best_value[at] = best; out.second_value[at] = second; out.num_admissible[at] = count;
}

}  // namespace gated
}  // namespace slslam

#endif  // SLSLAM_GATED_PAIRS_H_

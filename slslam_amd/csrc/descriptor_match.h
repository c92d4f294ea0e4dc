// slslam_amd/csrc/descriptor_match.h — the kernels of the descriptor matcher (include/slslam_hip.h: slslam_descriptor_matcher_*, DESIGN.md
// 6.6): every descriptor of a query frame against every descriptor of a stored keyframe by the place recogniser's distance, many
// (frame, candidate keyframe) pairs per launch, reduced to mutual, unambiguous matches.
//
//   k_desc_pairs    one wave per (pair, 64 query descriptors): lane <-> query descriptor.  The wave's 64 query descriptors are staged
//                   transposed in LDS (value i of lane a at sq[i kQueryStride + a]: the lanes read neighbouring banks, and the stride of
//                   65 keeps the staging writes - neighbouring lanes, neighbouring i - off a common bank as well).  The keyframe's
//                   descriptors stream through LDS in groups of kGroup = 8 (a lane fetches the next group while the wave works on this
//                   one); the store holds a group as [D][8], so value i of its eight descriptors is two 16-byte reads at one address for
//                   the whole wave: a broadcast.  Each lane carries the eight chains r_j = 1.0f; r_j -= q[i] * k_j[i] side by side, as
//                   slslam_place::nearest_child does with kChildBlock: one chain alone would wait D times for its own last subtraction.
//                   Then per keyframe descriptor the compare and the lane's running (best, second, count).  Descriptors go by in
//                   ascending j and only a strictly smaller r replaces the best: the lowest j wins a tie whatever the launch geometry.
//                   The best query descriptor of keyframe descriptor j is a 64-bit minimum over (ordered(r) << 32 | a) - ordered() maps
//                   the float's bits to an unsigned that orders as the float does, r may be below zero -, taken across the wave by
//                   shuffles and once per wave by atomicMin on global memory: a minimum does not depend on the order it is taken in.
//   k_desc_finish   lane <-> query descriptor and lane <-> keyframe descriptor: the mutual and ratio tests, best_query out of its key,
//                   num_matched by a ballot and one integer atomicAdd per wave.
// No fp atomics, no sums across lanes, and the chain's order is the contract's: a pair's bytes do not depend on its place in the call.
#ifndef SLSLAM_DESCRIPTOR_MATCH_H_
#define SLSLAM_DESCRIPTOR_MATCH_H_

#include <hip/hip_runtime.h>

// every product and difference of the chain is rounded on its own
#pragma STDC FP_CONTRACT OFF

namespace slslam_desc {

constexpr int kMaxD = 128, kMaxDescriptors = 512, kMaxCandidates = 8;
constexpr int kGroup = 8;               // keyframe descriptors whose chains a lane carries at a time
constexpr int kQueryStride = 65;        // floats between value i and value i + 1 of the staged query descriptors
constexpr int kGroupLoads = 2 * kMaxD / 64;       // 16-byte loads a lane makes for a group of the largest D
constexpr unsigned long long kNoQuery = ~0ull;

// floats of a group in the store and in LDS: [D][kGroup]
__host__ __device__ inline size_t group_floats(int D) { return (size_t)D * kGroup; }
// dynamic LDS of k_desc_pairs
inline size_t pairs_lds_bytes(int D) { return 4 * (group_floats(D) + (size_t)D * kQueryStride); }

// Per (query frame, candidate keyframe), where its inputs lie and where its results go
struct PairDesc {
  long long q;                          // float offset of the frame's [n][D] descriptors in the upload
  long long k;                          // float offset of the keyframe in the store: ceil(m / 8) groups of [D][8], zeros past m
  long long a0, j0;                     // the pair's first query / keyframe descriptor among those of all pairs
  int n, m;
  int run, pad;                         // run = 0: EMPTY or INVALID_DESCRIPTOR - no pair is evaluated, the outputs say "none"
};

// Where the results of all pairs go: [P], then [sum n] each, then [sum m]
struct Out {
  int* num_matched;
  int *match, *best, *num_admissible;
  float *best_distance, *second_distance;
  int* best_query;
};

// float bits -> an unsigned that orders as the float does (finite r; -0 counts as +0, as it does under <)
__device__ __forceinline__ unsigned ordered(float r) {
  const unsigned u = __float_as_uint(r + 0.0f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

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
  if (a_base >= pd.n) return;                                    // (the whole wave)
  const int a = a_base + lane;
  const bool avalid = a < pd.n;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_j = -1, count = 0;
  if (pd.run) {
    // the wave's rows are contiguous in the upload: element e = row D + i, read coalesced; rows past n are zeros (never admissible)
    const int rows = pd.n - a_base < 64 ? pd.n - a_base : 64;
    const float* src = qd + pd.q + (size_t)a_base * D;
    int row = 0, i = lane;
    for (int e = lane; e < 64 * D; e += 64) {
      while (i >= D) { i -= D; ++row; }
      sq[i * kQueryStride + row] = row < rows ? src[e] : 0.0f;
      i += 64;
    }
    const int ng = (pd.m + kGroup - 1) / kGroup;
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
#pragma unroll
      for (int jj = 0; jj < kGroup; ++jj) {
        const int j = g * kGroup + jj;
        const float rj = r[jj];
        const bool adm = avalid && j < pd.m && isfinite(rj) && (double)rj < max_distance;
        if (__ballot(adm) != 0ull) {                              // (wave-uniform)
          unsigned long long key = adm ? ((unsigned long long)ordered(rj) << 32) | (unsigned)a : kNoQuery;
          for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other < key ? other : key;
          }
          if (lane == 0) atomicMin(&keys[pd.j0 + j], key);
        }
        if (adm) {
          ++count;
          if (rj < best) { second = best; best = rj; best_j = j; }
          else if (rj < second) second = rj;
        }
      }
    }
  }
  if (!avalid) return;
  const long long at = pd.a0 + a;
  out.best[at] = best_j; out.best_distance[at] = best; out.second_distance[at] = second; out.num_admissible[at] = count;
}

// blockIdx = (64 query descriptors and 64 keyframe descriptors, pair)
__global__ __launch_bounds__(64) void k_desc_finish(const PairDesc* __restrict__ pairs, const unsigned long long* __restrict__ keys,
                                                    double ratio, Out out) {
  const PairDesc pd = pairs[blockIdx.y];
  const int i = blockIdx.x * 64 + threadIdx.x;
  if ((int)blockIdx.x * 64 >= pd.n && (int)blockIdx.x * 64 >= pd.m) return;        // (the whole wave)
  if (i < pd.m) {
    const unsigned long long key = keys[pd.j0 + i];
    out.best_query[pd.j0 + i] = key == kNoQuery ? -1 : (int)(unsigned)(key & 0xffffffffull);
  }
  bool matched = false;
  if (i < pd.n) {
    const long long at = pd.a0 + i;
    const int bj = out.best[at];
    if (bj >= 0) {
      const unsigned long long key = keys[pd.j0 + bj];
      const bool mutual = key != kNoQuery && (int)(unsigned)(key & 0xffffffffull) == i;
      const bool unambiguous = ratio <= 1.0 || (double)out.best_distance[at] * ratio <= (double)out.second_distance[at];
      matched = mutual && unambiguous;
    }
    out.match[at] = matched ? bj : -1;
  }
  const int n = __popcll(__ballot(matched));
  if (threadIdx.x == 0 && n > 0) atomicAdd(&out.num_matched[blockIdx.y], n);
}

}  // namespace slslam_desc

#endif  // SLSLAM_DESCRIPTOR_MATCH_H_

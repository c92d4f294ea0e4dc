// slslam_amd/csrc/mutual_match.h — what the line matcher (line_match.h) and the descriptor matcher (descriptor_match.h) share on the
// device: rows against columns (observations against map lines, query descriptors against keyframe descriptors), many problems per
// launch, reduced to mutual, unambiguous matches.  A pairs kernel of its own kind per matcher - lane <-> row, the columns going by in
// ascending order - calls for every pair
//   offer_key     the best row of a column is a 64-bit minimum over (ordered word of the value << 32 | row): the word orders as the value
//                 does and the low word breaks ties towards the lowest row.  Taken across the wave by shuffles and once per wave by
//                 atomicMin on global memory: a minimum does not depend on the order it is taken in.
//   take_pair     the lane's running (best, second, best column, count).  Only a strictly smaller value replaces the best: the lowest
//                 column wins a tie whatever the launch geometry.
// and both end with
//   k_mutual_finish  lane <-> row and lane <-> column: the mutual and ratio tests, best_row out of its key, num_matched by a ballot and
//                    one integer atomicAdd per wave.
// No fp atomics, no sums of floating-point values across lanes: a problem's bytes do not depend on its place in the call.
#ifndef SLSLAM_MUTUAL_MATCH_H_
#define SLSLAM_MUTUAL_MATCH_H_

#include <hip/hip_runtime.h>

#include "call_layout.h"

namespace slslam {

constexpr unsigned long long kNone = ~0ull;       // the key of a column no row was admissible for

// Where the results of all problems go (call_layout.h: MatchBlock): [P], then over all rows, then over all columns
struct MatchOut {
  int* num_matched;
  int *match, *best, *num_admissible;
  float *best_value, *second_value;
  int* best_row;
};

// float bits -> an unsigned that orders as the float does (finite r; -0 counts as +0, as it does under <): the word of a key whose
// value may be below zero (descriptor_match.h, stereo_match.h)
__device__ __forceinline__ unsigned ordered(float r) {
  const unsigned u = __float_as_uint(r + 0.0f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// One wave of 64 lanes; wave-uniform keys and slot
__device__ __forceinline__ void offer_key(bool adm, unsigned word, int row, unsigned long long* __restrict__ keys, long long slot) {
  if (__ballot(adm) != 0ull) {
    unsigned long long key = adm ? ((unsigned long long)word << 32) | (unsigned)row : kNone;
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o);
      key = other < key ? other : key;
    }
    if (threadIdx.x == 0) atomicMin(&keys[slot], key);
  }
}

__device__ __forceinline__ void take_pair(bool adm, float v, int col, float& best, float& second, int& best_col, int& count) {
  if (adm) {
    ++count;
    if (v < best) { second = best; best = v; best_col = col; }
    else if (v < second) second = v;
  }
}

// blockIdx = (64 rows and 64 columns, problem); Desc: the matcher's per-problem descriptor, its Span in .span
template <typename Desc>
__global__ __launch_bounds__(64) void k_mutual_finish(const Desc* __restrict__ descs, const unsigned long long* __restrict__ keys, double ratio,
                                                      MatchOut out) {
  const Span sp = descs[blockIdx.y].span;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if ((int)blockIdx.x * 64 >= sp.n && (int)blockIdx.x * 64 >= sp.m) return;        // (the whole wave)
  if (i < sp.m) {
    const unsigned long long key = keys[sp.j0 + i];
    out.best_row[sp.j0 + i] = key == kNone ? -1 : (int)(unsigned)(key & 0xffffffffull);
  }
  bool matched = false;
  if (i < sp.n) {
    const long long at = sp.a0 + i;
    const int bj = out.best[at];
    if (bj >= 0) {
      const unsigned long long key = keys[sp.j0 + bj];
      const bool mutual = key != kNone && (int)(unsigned)(key & 0xffffffffull) == i;
      const bool unambiguous = ratio <= 1.0 || (double)out.best_value[at] * ratio <= (double)out.second_value[at];
      matched = mutual && unambiguous;
    }
    out.match[at] = matched ? bj : -1;
  }
  const int n = __popcll(__ballot(matched));
  if (threadIdx.x == 0 && n > 0) atomicAdd(&out.num_matched[blockIdx.y], n);
}

}  // namespace slslam

#endif  // SLSLAM_MUTUAL_MATCH_H_

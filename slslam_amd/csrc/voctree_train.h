// slslam_amd/csrc/voctree_train.h — the device half of the vocabulary-tree trainer (include/slslam_hip.h: slslam_voctree_train; DESIGN.md
// 6.5): one Lloyd step of every node of a level.  The host (host/voctree_host.h) partitions the descriptors by node once per level and
// hands over a permutation, so that the descriptors of a node sit together without being moved.
//   k_voctree_step   block <-> kStepRounds rounds of kStepThreads consecutive positions of the permutation.
//                    assign: thread <-> descriptor, slslam_place::nearest_child against the K centres of its node - the centres of the
//                    round's first node are staged in LDS (at the root that is every centre there is), a descriptor of another node
//                    reads its own from global memory; the winner's r, the label, whether it changed, the child's member count.
//                    accumulate: wave <-> its 64 descriptors one after the other, lane <-> dimension: acc[node][child][i] += q(f[i]) as
//                    an int64 LDS atomic for the staged node (consecutive addresses over the lanes: no conflict inside a wave), as a
//                    global vector atomic for any other.  The LDS accumulators go out, non-zero ones only, as global vector atomics
//                    when the staged node changes and at the block's end.
// The sums are int64 sums of fixed-point values: any order gives the same bits.  The only float sum, the distortion, is a fixed tree per
// block; the host adds the blocks in order.  Contraction is off, as in place_recognition.h: r is the recogniser's.
#ifndef SLSLAM_VOCTREE_TRAIN_H_
#define SLSLAM_VOCTREE_TRAIN_H_

#include <hip/hip_runtime.h>

#include "place_recognition.h"

#pragma STDC FP_CONTRACT OFF

namespace slslam_vtrain {

constexpr int kStepThreads = 256, kStepRounds = 4;
constexpr long long kStepBlockItems = (long long)kStepThreads * kStepRounds;

struct Step {
  int K, D;
  long long n;
  const float* centres;                 // [num_nodes][K][D] of the level
  const float* desc;                    // [n][D]
  const int* perm;                      // [n] descriptors ordered by node
  const int* node;                      // [n] by descriptor
  int* label;                           // [n] by descriptor: the previous label in, the new one out
  unsigned long long* acc;              // [num_nodes K][D] int64 sums of q, zero before the launch
  unsigned long long* count;            // [num_nodes K] members, zero before the launch
  unsigned* changed;                    // labels that differ from the previous ones, zero before the launch
  double* partial;                      // [blocks] the block's sum of the winning r
  int accumulate;                       // 0: the last assignment of a level whose updates are used up - labels and counts only
};

inline size_t step_lds_bytes(int K, int D) { return (size_t)K * (size_t)D * (sizeof(unsigned long long) + sizeof(float)); }
inline unsigned step_blocks(long long n) { return (unsigned)((n + kStepBlockItems - 1) / kStepBlockItems); }

__device__ inline unsigned long long quantise(float f) {
  return (unsigned long long)__double2ll_rn((double)f * 1073741824.0);      // (two's complement: the unsigned sum is the signed one)
}

// grid step_blocks(n), block kStepThreads, dynamic LDS step_lds_bytes(K, D)
static __global__ __launch_bounds__(kStepThreads) void k_voctree_step(Step a) {
  extern __shared__ unsigned long long s_dyn[];
  __shared__ int s_m[kStepThreads], s_nd[kStepThreads], s_lb[kStepThreads];
  __shared__ unsigned s_cnt[slslam_place::kMaxK];
  __shared__ double s_red[kStepThreads];
  __shared__ unsigned s_changed;
  const int t = threadIdx.x, K = a.K, D = a.D, KD = K * D;
  unsigned long long* s_acc = s_dyn;                                  // [K][D] of the staged node
  float* s_c = reinterpret_cast<float*>(s_dyn + KD);                  // [K][D] its centres
  for (int i = t; i < KD; i += kStepThreads) s_acc[i] = 0ull;
  if (t < K) s_cnt[t] = 0u;
  if (t == 0) s_changed = 0u;

  int cur = -1;                                                       // the staged node: uniform over the block
  double rsum = 0.0;
  unsigned nchanged = 0u;
  const long long base = (long long)blockIdx.x * kStepBlockItems;
  for (int round = 0; round < kStepRounds; ++round) {
    const long long p0 = base + (long long)round * kStepThreads;
    if (p0 >= a.n) break;                                             // (uniform)
    const int first = a.node[a.perm[p0]];
    if (first != cur) {
      if (cur >= 0) {                                                 // (every wave is past the last round's accumulation: the barrier below)
        for (int i = t; i < KD; i += kStepThreads) {
          const unsigned long long v = s_acc[i];
          if (v) { atomicAdd(a.acc + (size_t)cur * KD + i, v); s_acc[i] = 0ull; }
        }
        if (t < K && s_cnt[t]) { atomicAdd(a.count + (size_t)cur * K + t, (unsigned long long)s_cnt[t]); s_cnt[t] = 0u; }
      }
      cur = first;
      for (int i = t; i < KD; i += kStepThreads) s_c[i] = a.centres[(size_t)cur * KD + i];
    }
    __syncthreads();

    // ---- assign: thread <-> descriptor
    const long long p = p0 + t;
    int m = -1, nd = 0, lb = 0;
    if (p < a.n) {
      m = a.perm[p];
      nd = a.node[m];
      const float* f = a.desc + (size_t)m * D;
      const float* c;
      if (nd == cur) { c = s_c; lb = slslam_place::nearest_child(s_c, f, K, D); }
      else { c = a.centres + (size_t)nd * KD; lb = slslam_place::nearest_child(c, f, K, D); }
      c += (size_t)lb * D;
      float r = 1.0f;
      for (int i = 0; i < D; ++i) {
        const float pr = c[i] * f[i];
        r = r - pr;
      }
      rsum = rsum + (double)r;
      nchanged += a.label[m] != lb ? 1u : 0u;
      a.label[m] = lb;
      if (nd == cur) atomicAdd(&s_cnt[lb], 1u);
      else atomicAdd(a.count + (size_t)nd * K + lb, 1ull);
    }
    s_m[t] = m; s_nd[t] = nd; s_lb[t] = lb;
    __syncthreads();

    // ---- accumulate: wave <-> its 64 descriptors in turn, lane <-> dimension
    if (a.accumulate) {
      const int lane = t & 63, w0 = t & ~63;
      for (int j = 0; j < 64; ++j) {
        const int mj = s_m[w0 + j];
        if (mj < 0) break;                                            // (uniform over the wave: only the tail of the positions is empty)
        const int ndj = s_nd[w0 + j], lbj = s_lb[w0 + j];
        const float* f = a.desc + (size_t)mj * D;
        if (ndj == cur) {
          unsigned long long* s = s_acc + lbj * D;
          for (int i = lane; i < D; i += 64) atomicAdd(s + i, quantise(f[i]));
        } else {
          unsigned long long* g = a.acc + ((size_t)ndj * K + lbj) * D;
          for (int i = lane; i < D; i += 64) atomicAdd(g + i, quantise(f[i]));
        }
      }
    }
    __syncthreads();
  }

  if (cur >= 0) {
    for (int i = t; i < KD; i += kStepThreads) {
      const unsigned long long v = s_acc[i];
      if (v) atomicAdd(a.acc + (size_t)cur * KD + i, v);
    }
    if (t < K && s_cnt[t]) atomicAdd(a.count + (size_t)cur * K + t, (unsigned long long)s_cnt[t]);
  }
  if (nchanged) atomicAdd(&s_changed, nchanged);
  s_red[t] = rsum;
  __syncthreads();
  for (int w = kStepThreads / 2; w > 0; w >>= 1) {
    if (t < w) s_red[t] = s_red[t] + s_red[t + w];
    __syncthreads();
  }
  if (t == 0) {
    a.partial[blockIdx.x] = s_red[0];
    if (s_changed) atomicAdd(a.changed, s_changed);
  }
}

}  // namespace slslam_vtrain

#endif  // SLSLAM_VOCTREE_TRAIN_H_

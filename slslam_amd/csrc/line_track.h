// slslam_amd/csrc/line_track.h — the kernels of the line tracker (include/slslam_hip.h: slslam_line_tracker_*): every
// segment of a frame against every segment of the frame before it, first by the temporal gate (line_track_layout.h: gate_admits),
// then by the place recogniser's descriptor distance, many frames per launch, reduced to mutual, unambiguous matches and turned into
// persistent feature ids.  Everything per segment lies in regions over [carried | frame 0 | ... | frame T-1]: a frame is uploaded
// once and read as the rows of its own problem and as the columns of the next.
//
//   k_track_copy    the carried frame (segments, flags, descriptors, ids, ages) from the handle's carried block to the front of the
//                   regions before the other launches, and the run's last frame to the carried block after them.  A segment without
//                   an id is carried as not valid: it is nobody's partner.
//   k_track_pairs   one wave per (frame, 64 rows): lane <-> row, its geometry in registers.  The problem's columns are staged in LDS
//                   once, after the warp, as four doubles each, with one flag (valid and not short).
//                   Pass 1, the gate: columns go by in ascending order in groups of kGroup = 8; a lane reads a column from one LDS
//                   address for the whole wave (a broadcast) and keeps the group's eight verdicts as a byte at s_mask[group][lane];
//                   a ballot per group says whether any lane admits any of its eight: bit g of the wave-uniform word `active`.
//                   Pass 2, the chains: only the groups whose bit is set, in ascending order, exactly as k_stereo_pairs
//                   (stereo_match.h) runs them - the tile [D][8], the next active group's fetch in flight, the eight chains
//                   r_j = 1.0f; r_j -= q[i] * k_j[i] side by side - and per column offer_key / take_pair (mutual_match.h) under
//                   (verdict, r finite, r < max_distance).  A skipped group would have offered and taken nothing.
//   k_mutual_finish (mutual_match.h), unchanged.
//   k_track_status  one wave per frame: segment_status, and by ballots the rank of every NEW segment among those of its frame and
//                   the frame's count of them.
//   k_track_prefix  one wave: new_before[t] = the NEW segments of frames 0 .. t-1, kScanWidth frames per pass, the total carried
//                   from pass to pass.
//   k_track_ids     lane <-> (frame, segment): follows match back frame by frame until a NEW segment or the carried frame
//                   (line_track_layout.h: id_of); reads what the launches before it wrote, waits for nobody; writes id and age.
// No fp atomics, no sums of floating-point values across lanes: the bytes do not depend on how frames are cut into runs.
#ifndef SLSLAM_LINE_TRACK_H_
#define SLSLAM_LINE_TRACK_H_

#include <hip/hip_runtime.h>

#include "line_track_layout.h"
#include "mutual_match.h"

// every product and difference of the chain and of the gate is rounded on its own
#pragma STDC FP_CONTRACT OFF

namespace slslam_track {

using slslam::ordered;

constexpr int kQueryStride = 65;        // floats between value i and value i + 1 of the staged row descriptors (descriptor_match.h)
constexpr int kTileLoads = kMaxD / 8;   // floats a lane fetches for a group of the largest D

using Out = slslam::MatchOut;           // best_value / second_value = the distances

// The upload's regions on the device (line_track_layout.h: CallLayout)
struct In {
  const FrameDesc* frames;
  const float4* seg;
  const int* ok;
  const float* desc;
};

// What the id launches write and read, over the regions' positions and over the frames
struct Ids {
  int *status, *id, *age, *rank;        // [S]
  int *num_new, *new_before;            // [F], [F + 1]
};

// One frame's worth of every region: the carried block, the front of the regions, the run's last frame
struct FrameRef {
  float4* seg;
  int* ok;
  float* desc;
  int *id, *age;
};

// dynamic LDS of k_track_pairs: the group's tile [D][8] and the row descriptors [D][kQueryStride]
inline size_t pairs_lds_bytes(int D) { return 4 * ((size_t)D * kGroup + (size_t)D * kQueryStride); }

// any grid of 64-lane blocks; n <= kMaxSegments
__global__ __launch_bounds__(64) void k_track_copy(FrameRef dst, FrameRef src, int n, int D) {
  const int i0 = blockIdx.x * 64 + threadIdx.x, step = gridDim.x * 64;
  for (int i = i0; i < n; i += step) {
    const int id = src.id[i];
    dst.seg[i] = src.seg[i];
    dst.ok[i] = src.ok[i] != 0 && id >= 0 ? 1 : 0;
    dst.id[i] = id;
    dst.age[i] = src.age[i];
  }
  for (int e = i0; e < n * D; e += step) dst.desc[e] = src.desc[e];
}

// blockIdx = (64 rows, frame); dynamic LDS pairs_lds_bytes(D)
__global__ __launch_bounds__(64) void k_track_pairs(In in, int D, Gate gate, unsigned long long* __restrict__ keys, Out out) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  __shared__ Ends s_col[kMaxSegments];
  __shared__ unsigned char s_cok[kMaxSegments];
  __shared__ unsigned char s_mask[kMaxGroups * 64];
  float* tile = s_mem;                                           // [D][8]: the group the wave works on
  const float4* tile4 = reinterpret_cast<const float4*>(s_mem);
  float* sq = s_mem + (size_t)D * kGroup;                        // [D][kQueryStride]
  const FrameDesc fd = in.frames[blockIdx.y];
  const slslam::Span sp = fd.span;
  const int lane = threadIdx.x;
  const int a_base = blockIdx.x * 64;
  if (a_base >= sp.n) return;                                    // (the whole wave)
  const int a = a_base + lane;
  const bool avalid = a < sp.n;
  float best = __builtin_huge_valf(), second = __builtin_huge_valf();
  int best_j = -1, count = 0;
  const int m = sp.m;
  if (m > 0) {
    // ---- the lane's row; the problem's columns, warped
    const float4 rs = avalid ? in.seg[sp.a0 + a] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const Segment A = segment_of(ends_of(rs.x, rs.y, rs.z, rs.w));
    const bool aok = avalid && in.ok[sp.a0 + a] != 0 && !is_short(A, gate);
    for (int b = lane; b < m; b += 64) {
      const float4 cs = in.seg[sp.j0 + b];
      const Ends e = ends_of(cs.x, cs.y, cs.z, cs.w);
      s_col[b] = warped(e, fd.warp);
      s_cok[b] = in.ok[sp.j0 + b] != 0 && !is_short(segment_of(e), gate) ? 1 : 0;
    }
    // the wave's row descriptors, transposed: rows are contiguous in the upload, read coalesced; rows past n are zeros
    {
      const int rows = sp.n - a_base < 64 ? sp.n - a_base : 64;
      const float* src = in.desc + ((size_t)sp.a0 + (size_t)a_base) * D;
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
          const Segment B = segment_of(s_col[j]);
          const bool adm = aok && s_cok[j] != 0 && gate_admits(A, B, gate);
          mask |= adm ? 1u << jj : 0u;
        }
      }
      s_mask[g * 64 + lane] = (unsigned char)mask;               // (read back by this lane alone)
      if (__ballot(mask != 0u) != 0ull) active |= 1ull << g;
    }

    // ---- pass 2: the chains of the groups somebody admits
    const int nc = D / 8;                                        // floats a lane fetches per group
    const int tj = lane & 7, ti = lane >> 3;
    const float* cd = in.desc + (size_t)sp.j0 * D;
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

// blockIdx.x = frame; after k_mutual_finish
__global__ __launch_bounds__(64) void k_track_status(In in, Gate gate, const int* __restrict__ match, Ids ids) {
  const slslam::Span sp = in.frames[blockIdx.x].span;
  const int lane = threadIdx.x;
  int running = 0;
  for (int base = 0; base < sp.n; base += 64) {                  // (wave-uniform)
    const int a = base + lane;
    const bool valid = a < sp.n;
    const long long at = sp.a0 + (valid ? a : 0);
    int st = -1;
    if (valid) {
      const float4 rs = in.seg[at];
      st = status_of(in.ok[at], is_short(segment_of(ends_of(rs.x, rs.y, rs.z, rs.w)), gate), match[at]);
    }
    const unsigned long long fresh = __ballot(st == kNew);
    if (valid) {
      ids.status[at] = st;
      ids.rank[at] = running + __popcll(fresh & ((1ull << lane) - 1ull));
    }
    running += __popcll(fresh);
  }
  if (lane == 0) ids.num_new[blockIdx.x] = running;
}

// one block of kScanWidth lanes
__global__ __launch_bounds__(kScanWidth) void k_track_prefix(int F, Ids ids) {
  static_assert(kScanWidth == 64, "one wave: the scan is by shuffles");
  const int lane = threadIdx.x;
  int total = 0;
  for (int base = 0; base < F; base += kScanWidth) {             // (wave-uniform)
    const int f = base + lane;
    const int v = f < F ? ids.num_new[f] : 0;
    int incl = v;
    for (int o = 1; o < kScanWidth; o <<= 1) {
      const int other = __shfl_up(incl, o);
      if (lane >= o) incl += other;
    }
    if (f < F) ids.new_before[f] = total + (incl - v);
    total += __shfl(incl, kScanWidth - 1);
  }
  if (lane == 0) ids.new_before[F] = total;
}

// blockIdx = (64 segments, frame - f0); frames: those of the whole run
__global__ __launch_bounds__(64) void k_track_ids(const FrameDesc* __restrict__ frames, int f0, const int* __restrict__ match, Ids ids,
                                                  int next_id) {
  const int t = f0 + (int)blockIdx.y;
  const int a = blockIdx.x * 64 + threadIdx.x;
  const slslam::Span sp = frames[t].span;
  if (a >= sp.n) return;
  const IdAge r = id_of(frames, t, a, ids.status, match, ids.rank, ids.new_before, ids.id, ids.age, next_id);
  ids.id[sp.a0 + a] = r.id;
  ids.age[sp.a0 + a] = r.age;
}

}  // namespace slslam_track

#endif  // SLSLAM_LINE_TRACK_H_

// slslam_amd/csrc/line_track.h — the kernels of the line tracker (include/slslam_hip.h: slslam_line_tracker_*): every
// segment of a frame against every segment of the frame before it, first by the temporal gate (line_track_layout.h: gate_admits),
// then by the place recogniser's descriptor distance, many frames per launch, reduced to mutual, unambiguous matches and turned into
// persistent feature ids.  Everything per segment lies in regions over [carried | frame 0 | ... | frame T-1]: a frame is uploaded
// once and read as the rows of its own problem and as the columns of the next.
//
//   k_track_copy    the carried frame (segments, flags, descriptors, ids, ages) from the handle's carried block to the front of the
//                   regions before the other launches, and the run's last frame to the carried block after them.  A segment without
//                   an id is carried as not valid: it is nobody's partner.
//   k_gated_pairs<Pairs>  (gated_pairs.h) one wave per (frame, 64 rows): lane <-> row, its geometry in registers.  Pairs below is
//                   what that kernel asks of the tracker: the problem's columns staged in LDS once, after the warp, as four doubles
//                   each, with one flag (valid and not short), and the temporal gate on a row and a staged column.  The gate pass,
//                   the chains of the groups somebody admits and offer_key / take_pair are the shared kernel's, as the stereo
//                   matcher runs them (stereo_match.h).
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

#include "gated_pairs.h"
#include "line_track_layout.h"

// every product and difference of the gate is rounded on its own, as those of the chain are (gated_pairs.h)
#pragma STDC FP_CONTRACT OFF

namespace slslam_track {

using slslam::gated::pairs_lds_bytes;

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

// What k_gated_pairs (gated_pairs.h) asks of the tracker: rows = a frame's segments, columns = those of the frame before it, which lie
// in the same regions (for frame 0 the carried frame, in front)
struct Pairs {
  using In = slslam_track::In;
  using Gate = slslam_track::Gate;
  using FrameDesc = slslam_track::FrameDesc;
  using Segment = slslam_track::Segment;
  struct Columns {                      // after the warp, four doubles each, with one flag: valid and not short
    Ends col[kMaxSegments];
    unsigned char ok[kMaxSegments];
  };
  static __device__ __forceinline__ Segment row(const In& in, long long at, bool valid, const Gate& gate, bool& ok) {
    const float4 rs = valid ? in.seg[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const Segment A = segment_of(ends_of(rs.x, rs.y, rs.z, rs.w));
    ok = valid && in.ok[at] != 0 && !is_short(A, gate);
    return A;
  }
  static __device__ __forceinline__ void stage(Columns& c, const In& in, const FrameDesc& fd, const Gate& gate, int b) {
    const float4 cs = in.seg[fd.span.j0 + b];
    const Ends e = ends_of(cs.x, cs.y, cs.z, cs.w);
    c.col[b] = warped(e, fd.warp);
    c.ok[b] = in.ok[fd.span.j0 + b] != 0 && !is_short(segment_of(e), gate) ? 1 : 0;
  }
  static __device__ __forceinline__ bool admits(const Columns& c, const Segment& A, int j, const Gate& gate) {
    return c.ok[j] != 0 && gate_admits(A, segment_of(c.col[j]), gate);
  }
  static __device__ __forceinline__ const float* row_descriptors(const In& in) { return in.desc; }
  static __device__ __forceinline__ const float* column_descriptors(const In& in) { return in.desc; }
};

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

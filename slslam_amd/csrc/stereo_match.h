// slslam_amd/csrc/stereo_match.h — the kernels of the stereo line matcher (include/slslam_hip.h: slslam_stereo_matcher_*):
// every left segment of a rectified stereo frame against every right segment, first by the epipolar gate (stereo_match_layout.h:
// gate_admits), then by the place recogniser's descriptor distance, many frames per launch, reduced to mutual, unambiguous matches and
// written out as stereo line observations.
//
//   k_gated_pairs<Pairs>  (gated_pairs.h) one wave per (frame, 64 left segments): lane <-> left segment, its geometry in registers.
//                   Pairs below is what that kernel asks of this matcher: the frame's right segments staged in LDS once (end points,
//                   the slope dx / dy - so that no pair divides -, the valid flag) and the epipolar gate on a left segment and a
//                   staged right one.  The gate pass, the chains of the groups somebody admits and offer_key / take_pair under
//                   (verdict, r finite, r < max_distance) are the shared kernel's.
//   k_mutual_finish (mutual_match.h), unchanged: left segments are its rows, right segments its columns.
//   k_stereo_emit   lane <-> left segment: segment_status, and for a MATCHED segment the eight normalised doubles and the two
//                   disparities (stereo_match_layout.h: emit_row).
// No fp atomics, no sums of floating-point values across lanes: a frame's bytes do not depend on its place in the call.
#ifndef SLSLAM_STEREO_MATCH_H_
#define SLSLAM_STEREO_MATCH_H_

#include <hip/hip_runtime.h>

#include "gated_pairs.h"
#include "stereo_match_layout.h"

// every product and difference of the gate is rounded on its own, as those of the chain are (gated_pairs.h)
#pragma STDC FP_CONTRACT OFF

namespace slslam_stereo {

using slslam::gated::pairs_lds_bytes;

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

// What k_gated_pairs (gated_pairs.h) asks of the stereo matcher: rows = left segments, columns = right segments
struct Pairs {
  using In = slslam_stereo::In;
  using Gate = slslam_stereo::Gate;
  using FrameDesc = slslam_stereo::FrameDesc;
  using Segment = slslam_stereo::Segment;
  struct Columns {                      // end points, the slope dx / dy - so that no pair divides -, the valid flag
    float4 seg[kMaxSegments];
    double slope[kMaxSegments];
    unsigned char ok[kMaxSegments];
  };
  static __device__ __forceinline__ Segment row(const In& in, long long at, bool valid, const Gate&, bool& ok) {
    const float4 ls = valid ? in.lseg[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ok = valid && in.lok[at] != 0;
    return segment_of(ls.x, ls.y, ls.z, ls.w);
  }
  static __device__ __forceinline__ void stage(Columns& c, const In& in, const FrameDesc& fd, const Gate&, int b) {
    const float4 rs = in.rseg[fd.span.j0 + b];
    c.seg[b] = rs;
    c.slope[b] = slope_of(rs.x, rs.y, rs.z, rs.w);
    c.ok[b] = in.rok[fd.span.j0 + b] != 0 ? 1 : 0;
  }
  static __device__ __forceinline__ bool admits(const Columns& c, const Segment& A, int j, const Gate& gate) {
    const float4 rs = c.seg[j];
    const Segment B = segment_with(rs.x, rs.y, rs.z, rs.w, c.slope[j]);
    return c.ok[j] != 0 && gate_admits(A, B, gate);
  }
  static __device__ __forceinline__ const float* row_descriptors(const In& in) { return in.ldesc; }
  static __device__ __forceinline__ const float* column_descriptors(const In& in) { return in.rdesc; }
};

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

// slslam_amd/csrc/stereo_api.hip — the stereo line matcher (include/slslam_hip.h: slslam_stereo_matcher_*, slslam_match_stereo): the link
// between the detector and MSLD, which give two unrelated lists of segments per stereo frame, and everything that takes a stereo line
// observation.  Per run, whatever the number of frames:
//   upload   one block [FrameDesc F | left segments | right segments | left flags | right flags | left descriptors | right descriptors]
//   pairs    k_gated_pairs<Pairs> (gated_pairs.h): the epipolar gate, then the descriptor chains of the groups somebody admits -> per left segment (best,
//            second, count), per right segment the key of its best left segment
//   finish   k_mutual_finish (mutual_match.h): mutual and ratio tests, matches, num_matched
//   emit     k_stereo_emit: segment_status, the eight normalised doubles and the two disparities of every matched left segment
//   download one block [the matchers' result block | segment_status | observations | disparity]
// The frame index lies in the grid.  The kernels are in stereo_match.h, the layout and the validation in stereo_match_layout.h, the
// scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "stereo_match.h"

using namespace slslam_stereo;
using slslam::device_present;
using slslam::kMaxGridY;

static_assert(kMaxD == SLSLAM_STEREO_MAX_D && kMaxSegments == SLSLAM_STEREO_MAX_SEGMENTS, "the header's limits are the kernels'");
static_assert(kMatched == SLSLAM_STEREO_MATCHED && kUnmatched == SLSLAM_STEREO_UNMATCHED && kFlat == SLSLAM_STEREO_FLAT &&
              kInvalid == SLSLAM_STEREO_INVALID, "the header's statuses are the kernels'");

struct slslam_stereo_matcher : slslam::TimedHandle {
  int D = 0, max_frames = 0, max_segments = 0;
  slslam::BlockPair block;
};

extern "C" void slslam_stereo_match_default_options(slslam_stereo_match_options* opt) {
  if (!opt) return;
  opt->min_disparity = 0.0;
  opt->max_disparity = 128.0;
  opt->max_tan2 = 0.03;
  opt->min_rows = 3.0;
  opt->min_overlap = 0.5;
  opt->ratio = 1.5;
  opt->max_distance = 0.25;
  opt->fx = opt->fy = 1.0;
  opt->cx = opt->cy = 0.0;
}

extern "C" int slslam_stereo_matcher_create(int device, int D, int max_frames, int max_segments, slslam_stereo_matcher** out) {
  if (!out || !shape_valid(D, max_frames, max_segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_stereo_matcher* h = new (std::nothrow) slslam_stereo_matcher();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->device = device;
  h->D = D; h->max_frames = max_frames; h->max_segments = max_segments;
  *out = h;
  return SLSLAM_OK;
}

extern "C" void slslam_stereo_matcher_destroy(slslam_stereo_matcher* h) { delete h; }

extern "C" int slslam_stereo_matcher_stats(const slslam_stereo_matcher* h, long long* calls, long long* allocations) {
  return slslam::handle_stats(h, calls, allocations);
}

extern "C" int slslam_stereo_matcher_timing(slslam_stereo_matcher* h, int enable, double* kernel_ms) {
  return slslam::handle_timing(h, enable, kernel_ms);
}

extern "C" int slslam_stereo_matcher_run(slslam_stereo_matcher* h, const slslam_stereo_match_options* opt, int num_frames,
                                         const slslam_stereo_frame* frames, slslam_stereo_result* out) {
  // ---- every argument before anything is written or the device is asked
  if (!h || !options_valid(opt) || num_frames < 0 || (num_frames > 0 && (!frames || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  for (int f = 0; f < F; ++f)
    if (!frame_valid(frames[f], h->max_segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = h->stream;
  ++h->calls;
  if (F == 0) return SLSLAM_OK;

  // ---- layout.  The blocks: made for the matcher's capacity at the first run, larger only when a call exceeds them
  const int D = h->D;
  std::vector<slslam::Span> span((size_t)F);
  size_t Atot = 0, Jtot = 0;
  int maxN = 0, maxM = 0;
  for (int f = 0; f < F; ++f) {
    span[(size_t)f] = slslam::Span{(long long)Atot, (long long)Jtot, frames[f].num_left, frames[f].num_right};
    Atot += (size_t)frames[f].num_left; Jtot += (size_t)frames[f].num_right;
    maxN = std::max(maxN, frames[f].num_left); maxM = std::max(maxM, frames[f].num_right);
  }
  const CallLayout y = call_layout((size_t)F, Atot, Jtot, (size_t)D);
  const size_t capF = (size_t)std::max(F, h->max_frames), capS = capF * (size_t)h->max_segments;
  if ((rc = h->block.fit(call_layout(capF, capS, capS, (size_t)D).bytes, y.bytes, &h->allocations)) != SLSLAM_OK) return rc;

  // ---- one upload
  char* hb = h->block.host.p;
  char* dv = h->block.dev.p;
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(hb);
  float* lseg = reinterpret_cast<float*>(hb + y.off_lseg);
  float* rseg = reinterpret_cast<float*>(hb + y.off_rseg);
  int* lok = reinterpret_cast<int*>(hb + y.off_lok);
  int* rok = reinterpret_cast<int*>(hb + y.off_rok);
  float* ldesc = reinterpret_cast<float*>(hb + y.off_ldesc);
  float* rdesc = reinterpret_cast<float*>(hb + y.off_rdesc);
  for (int f = 0; f < F; ++f) {
    const slslam_stereo_frame& fr = frames[f];
    const slslam::Span& sp = span[(size_t)f];
    fd[f].span = sp;
    slslam::gated::fill_side(lseg, ldesc, lok, (size_t)sp.a0, fr.left_segments, fr.left_descriptors, (size_t)sp.n, D);
    slslam::gated::fill_side(rseg, rdesc, rok, (size_t)sp.j0, fr.right_segments, fr.right_descriptors, (size_t)sp.m, D);
  }
  HIP_TRY(hipMemcpyAsync(dv, hb, y.in_bytes, hipMemcpyHostToDevice, s));
  In in;
  in.frames = reinterpret_cast<const FrameDesc*>(dv);
  in.lseg = reinterpret_cast<const float4*>(dv + y.off_lseg);
  in.rseg = reinterpret_cast<const float4*>(dv + y.off_rseg);
  in.lok = reinterpret_cast<const int*>(dv + y.off_lok);
  in.rok = reinterpret_cast<const int*>(dv + y.off_rok);
  in.ldesc = reinterpret_cast<const float*>(dv + y.off_ldesc);
  in.rdesc = reinterpret_cast<const float*>(dv + y.off_rdesc);
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(dv + y.off_keys);
  char* d_out = dv + y.off_out;
  const Out o = slslam::match_bind(d_out, y.out);
  EmitOut eo;
  eo.status = reinterpret_cast<int*>(d_out + y.o_status);
  eo.observations = reinterpret_cast<double*>(d_out + y.o_obs);
  eo.disparity = reinterpret_cast<double*>(d_out + y.o_disp);
  if ((rc = slslam::match_clear(o, (size_t)F, d_keys, Jtot, s)) != SLSLAM_OK) return rc;

  // ---- three launches for all frames
  const Gate gate = gate_of(*opt);
  const Camera cam = camera_of(*opt);
  if ((rc = h->timer_start()) != SLSLAM_OK) return rc;
  const unsigned tn = (unsigned)((maxN + 63) / 64), tm = (unsigned)((maxM + 63) / 64);
  for (int f0 = 0; f0 < F; f0 += kMaxGridY) {
    const unsigned nf = (unsigned)std::min(F - f0, kMaxGridY);
    Out of = o;
    of.num_matched += f0;
    In inf = in;
    inf.frames += f0;
    if (tn > 0) hipLaunchKernelGGL(slslam::gated::k_gated_pairs<Pairs>, dim3(tn, nf), dim3(64), pairs_lds_bytes(D), s, inf, D, gate, d_keys, of);
    if (std::max(tn, tm) > 0)
      hipLaunchKernelGGL(slslam::k_mutual_finish<FrameDesc>, dim3(std::max(tn, tm), nf), dim3(64), 0, s, inf.frames,
                         (const unsigned long long*)d_keys, opt->ratio, of);
    if (tn > 0) hipLaunchKernelGGL(k_stereo_emit, dim3(tn, nf), dim3(64), 0, s, inf, gate, cam, (const int*)o.match, eo);
  }
  HIP_TRY(hipGetLastError());
  if ((rc = h->timer_stop()) != SLSLAM_OK) return rc;

  // ---- one download
  char* h_out = hb + y.in_bytes;
  HIP_TRY(hipMemcpyAsync(h_out, d_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->timer_read()) != SLSLAM_OK) return rc;
  const int* st = reinterpret_cast<const int*>(h_out + y.o_status);
  for (int f = 0; f < F; ++f) {
    const slslam::Span& sp = span[(size_t)f];
    slslam_stereo_result& r = out[f];
    r.status = sp.n == 0 || sp.m == 0 ? SLSLAM_STEREO_EMPTY : SLSLAM_STEREO_OK;
    r.num_matched = slslam::match_scatter(h_out, y.out, (size_t)f, sp,
                                          {r.match, r.best, r.best_distance, r.second_distance, r.num_admissible, r.best_left});
    const size_t n = (size_t)sp.n, a0 = (size_t)sp.a0;
    if (r.segment_status && n > 0) std::memcpy(r.segment_status, st + a0, 4 * n);
    for (size_t i = 0; i < n; ++i) {                       // only the rows of MATCHED segments
      if (st[a0 + i] != kMatched) continue;
      if (r.observations) std::memcpy(r.observations + 8 * i, h_out + y.o_obs + 64 * (a0 + i), 64);
      if (r.disparity) std::memcpy(r.disparity + 2 * i, h_out + y.o_disp + 16 * (a0 + i), 16);
    }
  }
  return SLSLAM_OK;
}

extern "C" int slslam_match_stereo(int D, const slslam_stereo_match_options* opt, const slslam_stereo_frame* frame,
                                   slslam_stereo_result* out) {
  if (!shape_valid(D, 1, 1) || !options_valid(opt) || !frame || !out || !frame_valid(*frame, kMaxSegments))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_stereo_matcher* h = nullptr;
  int rc = slslam_stereo_matcher_create(-1, D, 1, std::max(std::max(frame->num_left, frame->num_right), 1), &h);
  if (rc == SLSLAM_OK) rc = slslam_stereo_matcher_run(h, opt, 1, frame, out);
  slslam_stereo_matcher_destroy(h);
  return rc;
}

// slslam_amd/csrc/track_api.hip — the line tracker (include/slslam_hip.h: slslam_line_tracker_*, slslam_track_lines): the link between the
// stereo matcher, which gives a frame's observations no identity, and everything keyed by a feature id.  Per run, whatever the
// number of frames:
//   upload   one block [FrameDesc T | segments | flags | descriptors], each region with room for the carried frame in front
//   carry in k_track_copy: the carried frame from the handle's carried block into that room
//   pairs    k_gated_pairs<Pairs> (gated_pairs.h): the temporal gate, then the descriptor chains of the groups somebody admits
//   finish   k_mutual_finish (mutual_match.h): mutual and ratio tests, matches, the number continued
//   status   k_track_status: segment_status, the rank and the count of the NEW segments of every frame
//   prefix   k_track_prefix: the NEW segments before every frame
//   ids      k_track_ids: id and age of every segment
//   carry out k_track_copy: the last frame into the carried block
//   download one block [the matchers' result block | segment_status | id | age | rank | num_new | new_before]
// The frame index lies in the grid.  The kernels are in line_track.h, the layout, the validation and the id rule in
// line_track_layout.h, the scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "line_track.h"

using namespace slslam_track;
using slslam::device_present;
using slslam::kMaxGridY;

static_assert(kMaxD == SLSLAM_TRACK_MAX_D && kMaxSegments == SLSLAM_TRACK_MAX_SEGMENTS, "the header's limits are the kernels'");
static_assert(kContinued == SLSLAM_TRACK_CONTINUED && kNew == SLSLAM_TRACK_NEW && kShort == SLSLAM_TRACK_SHORT &&
              kInvalid == SLSLAM_TRACK_INVALID, "the header's statuses are the kernels'");

struct slslam_line_tracker : slslam::TimedHandle {
  int D = 0, max_frames = 0, max_segments = 0;
  int next_id = 0, carried = 0;                          // the state: the carried frame's segments lie in `carry`
  slslam::BlockPair block;
  slslam::GrowBuf carry{slslam::Mem::kDevice};
};

extern "C" void slslam_line_track_default_options(slslam_line_track_options* opt) {
  if (!opt) return;
  opt->max_tan2 = 0.03;
  opt->max_shift = 40.0;
  opt->max_offset = 12.0;
  opt->min_overlap = 0.5;
  opt->min_length = 8.0;
  opt->ratio = 1.5;
  opt->max_distance = 0.25;
}

extern "C" int slslam_line_tracker_create(int device, int D, int max_frames, int max_segments, slslam_line_tracker** out) {
  if (!out || !shape_valid(D, max_frames, max_segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_tracker* h = new (std::nothrow) slslam_line_tracker();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->device = device;
  h->D = D; h->max_frames = max_frames; h->max_segments = max_segments;
  *out = h;
  return SLSLAM_OK;
}

extern "C" void slslam_line_tracker_destroy(slslam_line_tracker* h) { delete h; }

extern "C" int slslam_line_tracker_stats(const slslam_line_tracker* h, long long* calls, long long* allocations) {
  return slslam::handle_stats(h, calls, allocations);
}

extern "C" int slslam_line_tracker_timing(slslam_line_tracker* h, int enable, double* kernel_ms) {
  return slslam::handle_timing(h, enable, kernel_ms);
}

extern "C" int slslam_line_tracker_reset(slslam_line_tracker* h, int next_id) {
  if (!h || next_id < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  h->next_id = next_id;
  h->carried = 0;
  return SLSLAM_OK;
}

extern "C" int slslam_line_tracker_state(const slslam_line_tracker* h, int* next_id, int* carried_segments) {
  if (!h) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (next_id) *next_id = h->next_id;
  if (carried_segments) *carried_segments = h->carried;
  return SLSLAM_OK;
}

extern "C" int slslam_line_tracker_run(slslam_line_tracker* h, const slslam_line_track_options* opt, int num_frames,
                                       const slslam_line_track_frame* frames, slslam_line_track_result* out) {
  // ---- every argument before anything is written, the device is asked or the state changes
  if (!h || !options_valid(opt) || num_frames < 0 || (num_frames > 0 && (!frames || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  long long segments = 0;
  for (int f = 0; f < F; ++f) {
    if (!frame_valid(frames[f], h->max_segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
    segments += frames[f].num_segments;
  }
  if (!ids_fit(h->next_id, segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = h->stream;
  if (F == 0) return SLSLAM_OK;                          // (changes nothing, the count of runs included)
  ++h->calls;

  // ---- layout: [carried | frame 0 | ... ] in every region.  The blocks: made for the tracker's capacity at the first run, larger
  // only when a run exceeds them; the carried block with them, once
  const int D = h->D, C = h->carried;
  std::vector<slslam::Span> span((size_t)F);
  size_t S = (size_t)C;
  int maxN = 0, maxM = 0;
  {
    long long prev0 = 0;
    int prevn = C;
    for (int f = 0; f < F; ++f) {
      span[(size_t)f] = slslam::Span{(long long)S, prev0, frames[f].num_segments, prevn};
      maxN = std::max(maxN, frames[f].num_segments); maxM = std::max(maxM, prevn);
      prev0 = (long long)S; prevn = frames[f].num_segments;
      S += (size_t)frames[f].num_segments;
    }
  }
  const CallLayout y = call_layout((size_t)F, S, (size_t)D);
  const CarryLayout cy = carry_layout((size_t)h->max_segments, (size_t)D);
  const size_t capF = (size_t)std::max(F, h->max_frames), capS = (capF + 1) * (size_t)h->max_segments;
  if ((rc = h->block.fit(call_layout(capF, capS, (size_t)D).bytes, y.bytes, &h->allocations)) != SLSLAM_OK) return rc;
  if (!h->carry.p) {                                     // (with the blocks' first making: the same event)
    long long unused = 0;
    HIP_TRY(h->carry.need(cy.bytes, &unused));
  }

  // ---- one upload
  char* hb = h->block.host.p;
  char* dv = h->block.dev.p;
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(hb);
  float* seg = reinterpret_cast<float*>(hb + y.off_seg);
  int* ok = reinterpret_cast<int*>(hb + y.off_ok);
  float* desc = reinterpret_cast<float*>(hb + y.off_desc);
  for (int f = 0; f < F; ++f) {
    const slslam_line_track_frame& fr = frames[f];
    const slslam::Span& sp = span[(size_t)f];
    fd[f].span = sp;
    fd[f].warp = warp_of(fr.predict);
    slslam::gated::fill_side(seg, desc, ok, (size_t)sp.a0, fr.segments, fr.descriptors, (size_t)sp.n, D);
  }
  HIP_TRY(hipMemcpyAsync(dv, hb, y.in_bytes, hipMemcpyHostToDevice, s));
  In in;
  in.frames = reinterpret_cast<const FrameDesc*>(dv);
  in.seg = reinterpret_cast<const float4*>(dv + y.off_seg);
  in.ok = reinterpret_cast<const int*>(dv + y.off_ok);
  in.desc = reinterpret_cast<const float*>(dv + y.off_desc);
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(dv + y.off_keys);
  char* d_out = dv + y.off_out;
  const Out o = slslam::match_bind(d_out, y.out);
  Ids ids;
  ids.status = reinterpret_cast<int*>(d_out + y.o_status);
  ids.id = reinterpret_cast<int*>(d_out + y.o_id);
  ids.age = reinterpret_cast<int*>(d_out + y.o_age);
  ids.rank = reinterpret_cast<int*>(d_out + y.o_rank);
  ids.num_new = reinterpret_cast<int*>(d_out + y.o_new);
  ids.new_before = reinterpret_cast<int*>(d_out + y.o_before);
  // the carried block, the front of the regions, the last frame
  char* cb = h->carry.p;
  const FrameRef kept{reinterpret_cast<float4*>(cb + cy.off_seg), reinterpret_cast<int*>(cb + cy.off_ok),
                      reinterpret_cast<float*>(cb + cy.off_desc), reinterpret_cast<int*>(cb + cy.off_id),
                      reinterpret_cast<int*>(cb + cy.off_age)};
  const FrameRef front{reinterpret_cast<float4*>(dv + y.off_seg), reinterpret_cast<int*>(dv + y.off_ok),
                       reinterpret_cast<float*>(dv + y.off_desc), ids.id, ids.age};
  const slslam::Span& last = span[(size_t)F - 1];
  const FrameRef tail{front.seg + last.a0, front.ok + last.a0, front.desc + (size_t)last.a0 * (size_t)D, ids.id + last.a0,
                      ids.age + last.a0};
  if ((rc = slslam::match_clear(o, (size_t)F, d_keys, S, s)) != SLSLAM_OK) return rc;

  // ---- seven launches for all frames
  const Gate gate = gate_of(*opt);
  if ((rc = h->timer_start()) != SLSLAM_OK) return rc;
  const auto copy_grid = [D](int n) { return dim3((unsigned)std::min((n * D + 63) / 64, 256)); };
  if (C > 0) hipLaunchKernelGGL(k_track_copy, copy_grid(C), dim3(64), 0, s, front, kept, C, D);
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
  }
  hipLaunchKernelGGL(k_track_status, dim3((unsigned)F), dim3(64), 0, s, in, gate, (const int*)o.match, ids);
  hipLaunchKernelGGL(k_track_prefix, dim3(1), dim3(kScanWidth), 0, s, F, ids);
  for (int f0 = 0; f0 < F && tn > 0; f0 += kMaxGridY)
    hipLaunchKernelGGL(k_track_ids, dim3(tn, (unsigned)std::min(F - f0, kMaxGridY)), dim3(64), 0, s, in.frames, f0, (const int*)o.match, ids,
                       h->next_id);
  if (last.n > 0) hipLaunchKernelGGL(k_track_copy, copy_grid(last.n), dim3(64), 0, s, kept, tail, last.n, D);
  HIP_TRY(hipGetLastError());
  if ((rc = h->timer_stop()) != SLSLAM_OK) return rc;

  // ---- one download
  char* h_out = hb + y.in_bytes;
  HIP_TRY(hipMemcpyAsync(h_out, d_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->timer_read()) != SLSLAM_OK) return rc;
  const int* num_new = reinterpret_cast<const int*>(h_out + y.o_new);
  const int* new_before = reinterpret_cast<const int*>(h_out + y.o_before);
  for (int f = 0; f < F; ++f) {
    const slslam::Span& sp = span[(size_t)f];
    slslam_line_track_result& r = out[f];
    r.status = sp.n == 0 || sp.m == 0 ? SLSLAM_TRACK_EMPTY : SLSLAM_TRACK_OK;
    r.num_continued = slslam::match_scatter(h_out, y.out, (size_t)f, sp,
                                            {r.match, r.best, r.best_distance, r.second_distance, r.num_admissible, r.best_row});
    r.num_new = num_new[f];
    const size_t nb = 4 * (size_t)sp.n, no = 4 * (size_t)sp.a0;
    if (r.id && sp.n > 0) std::memcpy(r.id, h_out + y.o_id + no, nb);
    if (r.age && sp.n > 0) std::memcpy(r.age, h_out + y.o_age + no, nb);
    if (r.segment_status && sp.n > 0) std::memcpy(r.segment_status, h_out + y.o_status + no, nb);
  }
  h->next_id += new_before[F];
  h->carried = last.n;
  return SLSLAM_OK;
}

extern "C" int slslam_track_lines(int D, const slslam_line_track_options* opt, int num_frames, const slslam_line_track_frame* frames,
                                  slslam_line_track_result* out) {
  if (!shape_valid(D, 1, 1) || !options_valid(opt) || num_frames < 0 || (num_frames > 0 && (!frames || !out)))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  int most = 1;
  long long segments = 0;
  for (int f = 0; f < num_frames; ++f) {
    if (!frame_valid(frames[f], kMaxSegments)) return SLSLAM_ERR_INVALID_ARGUMENT;
    most = std::max(most, frames[f].num_segments);
    segments += frames[f].num_segments;
  }
  if (!ids_fit(0, segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_line_tracker* h = nullptr;
  int rc = slslam_line_tracker_create(-1, D, std::max(num_frames, 1), most, &h);
  if (rc == SLSLAM_OK) rc = slslam_line_tracker_run(h, opt, num_frames, frames, out);
  slslam_line_tracker_destroy(h);
  return rc;
}

// slslam_amd/csrc/match_api.hip — the line matcher (include/slslam_hip.h: slslam_line_matcher_*, slslam_match_lines): the link in front of
// the pose estimator.  Per call, whatever the number of frames:
//   upload   one block [FrameDesc F | doubles: per frame pose 12, observations 8 K, lines 6 L, extents 2 L]
//   lines    k_match_lines: the per-line part of the reprojection error, and of the overlap test, under each frame's pose
//   pairs    k_match_pairs: every observation against every line of its frame -> per observation (best, second, count), per line the key
//            of its best observation
//   finish   k_mutual_finish (mutual_match.h): mutual and ratio tests, matches, num_matched
//   download one block [num_matched F | match, best_line, num_admissible, best_error, second_error: Ktot each | best_observation Ltot]
// The frame index lies in the grid.  The kernels are in line_match.h, the scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "line_match.h"

using namespace slslam_match;
using slslam::device_present;
using slslam::kMaxGridY;

namespace {

// Where everything of a call lies: the upload (the same offsets on the host and on the device), the device's work arrays behind it,
// and the result block (on the host behind the upload)
struct CallLayout {
  size_t off_d = 0, in_bytes = 0;                        // upload: FrameDesc[F] at 0, doubles at off_d
  size_t off_soa = 0, off_lbest = 0, off_out = 0;
  slslam::MatchBlock out;
  slslam::BlockBytes bytes;
};

CallLayout call_layout(long long F, long long Ktot, long long Ltot) {
  CallLayout y;
  slslam::Carve c;
  const size_t doubles = 8 * (size_t)(12 * F + 8 * Ktot + 8 * Ltot);
  c.take(sizeof(FrameDesc) * (size_t)F);
  y.off_d = c.take(doubles);
  y.in_bytes = y.off_d + doubles;
  y.out = slslam::match_block((size_t)F, (size_t)Ktot, (size_t)Ltot);
  y.bytes.host = c.at + y.out.bytes;
  y.off_soa = c.take(8 * (size_t)kLineValuesExt * (size_t)Ltot);
  y.off_lbest = c.take(8 * (size_t)Ltot);
  y.off_out = c.at;
  y.bytes.dev = y.off_out + y.out.bytes;
  return y;
}

// sizes, then pointers of one frame; max_k / max_l < 0: no maximum
bool frame_valid(const slslam_match_frame& f, int max_k, int max_l) {
  const int K = f.num_observations, L = f.num_lines;
  if (K < 0 || L < 0 || (max_k >= 0 && K > max_k) || (max_l >= 0 && L > max_l)) return false;
  if (K > 0 && !f.observations) return false;
  if (L > 0 && !f.lines) return false;
  if (K > 0 && L > 0 && !f.pose) return false;
  return true;
}

bool thresholds_valid(double baseline, double error_thr, double ratio, double margin) {
  return !std::isnan(baseline) && !std::isnan(error_thr) && !std::isnan(ratio) && margin >= 0.0;
}

}  // namespace

struct slslam_line_matcher : slslam::Handle {
  int max_frames = 0, max_observations = 0, max_lines = 0;
  slslam::BlockPair block;
};

extern "C" int slslam_line_matcher_create(int device, int max_frames, int max_observations, int max_lines, slslam_line_matcher** out) {
  if (!out || max_frames < 1 || max_observations < 1 || max_lines < 1) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_matcher* m = new (std::nothrow) slslam_line_matcher();
  if (!m) return SLSLAM_ERR_NO_MEMORY;
  m->device = device;
  m->max_frames = max_frames; m->max_observations = max_observations; m->max_lines = max_lines;
  *out = m;
  return SLSLAM_OK;
}

extern "C" void slslam_line_matcher_destroy(slslam_line_matcher* m) { delete m; }

extern "C" int slslam_line_matcher_stats(const slslam_line_matcher* m, long long* calls, long long* allocations) {
  return slslam::handle_stats(m, calls, allocations);
}

extern "C" int slslam_line_matcher_run(slslam_line_matcher* m, int num_frames, const slslam_match_frame* frames, double baseline,
                                       double error_thr, double ratio, double margin, slslam_match_result* out) {
  // ---- every argument before anything is written or the device is asked
  if (!m || num_frames < 0 || (num_frames > 0 && (!frames || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!thresholds_valid(baseline, error_thr, ratio, margin)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  for (int f = 0; f < F; ++f)
    if (!frame_valid(frames[f], m->max_observations, m->max_lines)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = m->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = m->stream;
  ++m->calls;
  if (F == 0) return SLSLAM_OK;

  // ---- layout
  std::vector<FrameDesc> fd((size_t)F);
  std::vector<int> status((size_t)F);
  long long nd = 0, Ktot = 0, Ltot = 0;
  int maxK = 0, maxL = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_match_frame& fr = frames[f];
    FrameDesc& d = fd[(size_t)f];
    const int K = fr.num_observations, L = fr.num_lines;
    d.span.n = K; d.span.m = L; d.pad = 0;
    int st = K == 0 || L == 0 ? SLSLAM_MATCH_EMPTY : SLSLAM_MATCH_OK;
    for (int q = 0; st == SLSLAM_MATCH_OK && q < 12; ++q)
      if (!std::isfinite(fr.pose[q])) st = SLSLAM_MATCH_INVALID_POSE;
    status[(size_t)f] = st;
    d.run = st == SLSLAM_MATCH_OK ? 1 : 0;
    d.pose = nd; nd += 12;
    d.obs = nd; nd += 8LL * K;
    d.lines = nd; if (d.run) nd += 6LL * L;
    d.ext = -1; if (d.run && fr.extents) { d.ext = nd; nd += 2LL * L; }
    d.span.a0 = Ktot; Ktot += K;
    d.span.j0 = Ltot; Ltot += L;
    maxK = std::max(maxK, K); maxL = std::max(maxL, L);
  }
  // the blocks: made for the matcher's capacity at the first run, larger only when a call exceeds them
  const long long capF = std::max<long long>(F, m->max_frames);
  const CallLayout y = call_layout(F, Ktot, Ltot);
  if ((rc = m->block.fit(call_layout(capF, capF * m->max_observations, capF * m->max_lines).bytes, y.bytes, &m->allocations)) != SLSLAM_OK)
    return rc;

  // ---- one upload
  char* h = m->block.host.p;
  char* dv = m->block.dev.p;
  std::memcpy(h, fd.data(), sizeof(FrameDesc) * (size_t)F);
  double* hd = reinterpret_cast<double*>(h + y.off_d);
  for (int f = 0; f < F; ++f) {
    const slslam_match_frame& fr = frames[f];
    const FrameDesc& d = fd[(size_t)f];
    if (d.run) std::memcpy(hd + d.pose, fr.pose, 96);
    else std::memset(hd + d.pose, 0, 96);
    if (d.span.n > 0) std::memcpy(hd + d.obs, fr.observations, 64 * (size_t)d.span.n);
    if (d.run) std::memcpy(hd + d.lines, fr.lines, 48 * (size_t)d.span.m);
    if (d.ext >= 0) std::memcpy(hd + d.ext, fr.extents, 16 * (size_t)d.span.m);
  }
  const size_t up_bytes = y.off_d + 8 * (size_t)nd;
  HIP_TRY(hipMemcpyAsync(dv, h, up_bytes, hipMemcpyHostToDevice, s));
  const FrameDesc* d_fd = reinterpret_cast<const FrameDesc*>(dv);
  const double* d_dd = reinterpret_cast<const double*>(dv + y.off_d);
  double* d_soa = reinterpret_cast<double*>(dv + y.off_soa);
  unsigned long long* d_lbest = reinterpret_cast<unsigned long long*>(dv + y.off_lbest);
  char* d_out = dv + y.off_out;
  const Out o = slslam::match_bind(d_out, y.out);
  if ((rc = slslam::match_clear(o, (size_t)F, d_lbest, (size_t)Ltot, s)) != SLSLAM_OK) return rc;

  // ---- three launches for all frames
  const unsigned tk = (unsigned)((maxK + 63) / 64), tl = (unsigned)((maxL + 63) / 64);
  for (int f0 = 0; f0 < F; f0 += kMaxGridY) {
    const unsigned nf = (unsigned)std::min(F - f0, kMaxGridY);
    Out of = o;
    of.num_matched += f0;
    if (tk > 0 && tl > 0)                                        // (a frame that runs has observations and lines)
      hipLaunchKernelGGL(k_match_lines, dim3(tl, nf), dim3(64), 0, s, d_fd + f0, d_dd, baseline, margin, Ltot, d_soa);
    if (tk > 0)
      hipLaunchKernelGGL(k_match_pairs, dim3(tk, nf), dim3(64), 0, s, d_fd + f0, d_dd, (const double*)d_soa, Ltot, error_thr, d_lbest, of);
    if (std::max(tk, tl) > 0)
      hipLaunchKernelGGL(slslam::k_mutual_finish<FrameDesc>, dim3(std::max(tk, tl), nf), dim3(64), 0, s, d_fd + f0,
                         (const unsigned long long*)d_lbest, ratio, of);
  }
  HIP_TRY(hipGetLastError());

  // ---- one download
  char* h_out = h + slslam::align256(y.in_bytes);
  if ((rc = slslam::match_download(h_out, d_out, y.out, s)) != SLSLAM_OK) return rc;
  for (int f = 0; f < F; ++f) {
    slslam_match_result& r = out[f];
    r.status = status[(size_t)f];
    r.num_matched = slslam::match_scatter(h_out, y.out, (size_t)f, fd[(size_t)f].span,
                                          {r.match, r.best_line, r.best_error, r.second_error, r.num_admissible, r.best_observation});
  }
  return SLSLAM_OK;
}

extern "C" int slslam_match_lines(const slslam_match_frame* frame, double baseline, double error_thr, double ratio, double margin,
                                  slslam_match_result* out) {
  if (!frame || !out || !frame_valid(*frame, -1, -1) || !thresholds_valid(baseline, error_thr, ratio, margin)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_line_matcher* m = nullptr;
  int rc = slslam_line_matcher_create(-1, 1, std::max(frame->num_observations, 1), std::max(frame->num_lines, 1), &m);
  if (rc == SLSLAM_OK) rc = slslam_line_matcher_run(m, 1, frame, baseline, error_thr, ratio, margin, out);
  slslam_line_matcher_destroy(m);
  return rc;
}

// slslam_amd/csrc/match_api.hip — the line matcher (include/slslam_hip.h: slslam_line_matcher_*, slslam_match_lines): the link in front of
// the pose estimator.  Per call, whatever the number of frames:
//   upload   one block [FrameDesc F | doubles: per frame pose 12, observations 8 K, lines 6 L, extents 2 L]
//   lines    k_match_lines: the per-line part of the reprojection error, and of the overlap test, under each frame's pose
//   pairs    k_match_pairs: every observation against every line of its frame -> per observation (best, second, count), per line the key
//            of its best observation
//   finish   k_match_finish: mutual and ratio tests, matches, num_matched
//   download one block [num_matched F | match, best_line, num_admissible, best_error, second_error: Ktot each | best_observation Ltot]
// The frame index lies in the grid.  The kernels are in line_match.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "grow_buf.h"
#include "hip_status.h"
#include "line_match.h"

using namespace slslam_match;
using slslam::align256;
using slslam::GrowBuf;
using slslam::Mem;

namespace {

constexpr int kMaxGrid = 65535;         // what the y dimension of a grid takes: frames go in slices of it

// Where everything of a call lies: the upload (the same offsets on the host and on the device), the device's work arrays behind it,
// and the result block (the same offsets on the device and on the host)
struct Layout {
  size_t off_d = 0, in_bytes = 0;                        // upload: FrameDesc[F] at 0, doubles at off_d
  size_t off_soa = 0, off_lbest = 0, off_out = 0, dev_bytes = 0;
  size_t o_match = 0, o_line = 0, o_count = 0, o_best = 0, o_second = 0, o_obs = 0, out_bytes = 0;   // in the result block; num_matched[F] at 0
  size_t host_bytes = 0;                                 // upload, then the result block at align256(in_bytes)
  long long Ktot = 0, Ltot = 0;
};

Layout make_layout(long long F, long long Ktot, long long Ltot) {
  Layout y;
  y.Ktot = Ktot; y.Ltot = Ltot;
  y.off_d = align256(sizeof(FrameDesc) * (size_t)F);
  y.in_bytes = y.off_d + 8 * (size_t)(12 * F + 8 * Ktot + 8 * Ltot);
  y.o_match = align256(4 * (size_t)F);
  y.o_line = y.o_match + align256(4 * (size_t)Ktot);
  y.o_count = y.o_line + align256(4 * (size_t)Ktot);
  y.o_best = y.o_count + align256(4 * (size_t)Ktot);
  y.o_second = y.o_best + align256(4 * (size_t)Ktot);
  y.o_obs = y.o_second + align256(4 * (size_t)Ktot);
  y.out_bytes = y.o_obs + align256(4 * (size_t)Ltot);
  y.off_soa = align256(y.in_bytes);
  y.off_lbest = y.off_soa + align256(8 * (size_t)kLineValuesExt * (size_t)Ltot);
  y.off_out = y.off_lbest + align256(8 * (size_t)Ltot);
  y.dev_bytes = y.off_out + y.out_bytes;
  y.host_bytes = align256(y.in_bytes) + y.out_bytes;
  return y;
}

bool device_present() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
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

struct slslam_line_matcher {
  int device = -1;
  int max_frames = 0, max_observations = 0, max_lines = 0;
  GrowBuf d_block{Mem::kDevice}, h_block{Mem::kPinned};
  hipStream_t stream = nullptr;
  long long calls = 0, allocations = 0;
  ~slslam_line_matcher() {
    if (stream) (void)hipStreamDestroy(stream);
  }
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
  if (!m) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (calls) *calls = m->calls;
  if (allocations) *allocations = m->allocations;
  return SLSLAM_OK;
}

extern "C" int slslam_line_matcher_run(slslam_line_matcher* m, int num_frames, const slslam_match_frame* frames, double baseline,
                                       double error_thr, double ratio, double margin, slslam_match_result* out) {
  // ---- every argument before anything is written or the device is asked
  if (!m || num_frames < 0 || (num_frames > 0 && (!frames || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!thresholds_valid(baseline, error_thr, ratio, margin)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  for (int f = 0; f < F; ++f)
    if (!frame_valid(frames[f], m->max_observations, m->max_lines)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (m->device >= 0) HIP_TRY(hipSetDevice(m->device));
  else HIP_TRY(hipGetDevice(&m->device));
  if (!m->stream) HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
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
    d.K = fr.num_observations; d.L = fr.num_lines; d.pad = 0;
    int st = d.K == 0 || d.L == 0 ? SLSLAM_MATCH_EMPTY : SLSLAM_MATCH_OK;
    for (int q = 0; st == SLSLAM_MATCH_OK && q < 12; ++q)
      if (!std::isfinite(fr.pose[q])) st = SLSLAM_MATCH_INVALID_POSE;
    status[(size_t)f] = st;
    d.run = st == SLSLAM_MATCH_OK ? 1 : 0;
    d.pose = nd; nd += 12;
    d.obs = nd; nd += 8LL * d.K;
    d.lines = nd; if (d.run) nd += 6LL * d.L;
    d.ext = -1; if (d.run && fr.extents) { d.ext = nd; nd += 2LL * d.L; }
    d.k0 = Ktot; Ktot += d.K;
    d.l0 = Ltot; Ltot += d.L;
    maxK = std::max(maxK, d.K); maxL = std::max(maxL, d.L);
  }
  // the blocks: made for the matcher's capacity at the first run, larger only when a call exceeds them
  const long long capF = std::max<long long>(F, m->max_frames);
  const Layout cap = make_layout(capF, capF * m->max_observations, capF * m->max_lines);
  const Layout y = make_layout(F, Ktot, Ltot);
  if (m->d_block.n < y.dev_bytes || m->h_block.n < y.host_bytes || !m->d_block.p || !m->h_block.p) {
    long long unused = 0;
    HIP_TRY(m->d_block.need(std::max(cap.dev_bytes, y.dev_bytes), &unused));
    HIP_TRY(m->h_block.need(std::max(cap.host_bytes, y.host_bytes), &unused));
    ++m->allocations;
  }

  // ---- one upload
  char* h = m->h_block.p;
  char* dv = m->d_block.p;
  std::memcpy(h, fd.data(), sizeof(FrameDesc) * (size_t)F);
  double* hd = reinterpret_cast<double*>(h + y.off_d);
  for (int f = 0; f < F; ++f) {
    const slslam_match_frame& fr = frames[f];
    const FrameDesc& d = fd[(size_t)f];
    if (d.run) std::memcpy(hd + d.pose, fr.pose, 96);
    else std::memset(hd + d.pose, 0, 96);
    if (d.K > 0) std::memcpy(hd + d.obs, fr.observations, 64 * (size_t)d.K);
    if (d.run) std::memcpy(hd + d.lines, fr.lines, 48 * (size_t)d.L);
    if (d.ext >= 0) std::memcpy(hd + d.ext, fr.extents, 16 * (size_t)d.L);
  }
  const size_t up_bytes = y.off_d + 8 * (size_t)nd;
  HIP_TRY(hipMemcpyAsync(dv, h, up_bytes, hipMemcpyHostToDevice, s));
  const FrameDesc* d_fd = reinterpret_cast<const FrameDesc*>(dv);
  const double* d_dd = reinterpret_cast<const double*>(dv + y.off_d);
  double* d_soa = reinterpret_cast<double*>(dv + y.off_soa);
  unsigned long long* d_lbest = reinterpret_cast<unsigned long long*>(dv + y.off_lbest);
  char* d_out = dv + y.off_out;
  Out o;
  o.num_matched = reinterpret_cast<int*>(d_out);
  o.match = reinterpret_cast<int*>(d_out + y.o_match);
  o.best_line = reinterpret_cast<int*>(d_out + y.o_line);
  o.num_admissible = reinterpret_cast<int*>(d_out + y.o_count);
  o.best_error = reinterpret_cast<float*>(d_out + y.o_best);
  o.second_error = reinterpret_cast<float*>(d_out + y.o_second);
  o.best_observation = reinterpret_cast<int*>(d_out + y.o_obs);
  HIP_TRY(hipMemsetAsync(o.num_matched, 0, 4 * (size_t)F, s));
  if (Ltot > 0) HIP_TRY(hipMemsetAsync(d_lbest, 0xff, 8 * (size_t)Ltot, s));

  // ---- three launches for all frames
  const unsigned tk = (unsigned)((maxK + 63) / 64), tl = (unsigned)((maxL + 63) / 64);
  for (int f0 = 0; f0 < F; f0 += kMaxGrid) {
    const unsigned nf = (unsigned)std::min(F - f0, kMaxGrid);
    Out of = o;
    of.num_matched += f0;
    if (tk > 0 && tl > 0)                                        // (a frame that runs has observations and lines)
      hipLaunchKernelGGL(k_match_lines, dim3(tl, nf), dim3(64), 0, s, d_fd + f0, d_dd, baseline, margin, Ltot, d_soa);
    if (tk > 0)
      hipLaunchKernelGGL(k_match_pairs, dim3(tk, nf), dim3(64), 0, s, d_fd + f0, d_dd, (const double*)d_soa, Ltot, error_thr, d_lbest, of);
    if (std::max(tk, tl) > 0)
      hipLaunchKernelGGL(k_match_finish, dim3(std::max(tk, tl), nf), dim3(64), 0, s, d_fd + f0, (const unsigned long long*)d_lbest, ratio, of);
  }
  HIP_TRY(hipGetLastError());

  // ---- one download
  char* h_out = h + align256(y.in_bytes);
  HIP_TRY(hipMemcpyAsync(h_out, d_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int* r_nm = reinterpret_cast<const int*>(h_out);
  for (int f = 0; f < F; ++f) {
    const FrameDesc& d = fd[(size_t)f];
    slslam_match_result& r = out[f];
    r.status = status[(size_t)f];
    r.num_matched = r_nm[f];
    const size_t kb = 4 * (size_t)d.K, ko = 4 * (size_t)d.k0;
    if (r.match && d.K > 0) std::memcpy(r.match, h_out + y.o_match + ko, kb);
    if (r.best_line && d.K > 0) std::memcpy(r.best_line, h_out + y.o_line + ko, kb);
    if (r.num_admissible && d.K > 0) std::memcpy(r.num_admissible, h_out + y.o_count + ko, kb);
    if (r.best_error && d.K > 0) std::memcpy(r.best_error, h_out + y.o_best + ko, kb);
    if (r.second_error && d.K > 0) std::memcpy(r.second_error, h_out + y.o_second + ko, kb);
    if (r.best_observation && d.L > 0) std::memcpy(r.best_observation, h_out + y.o_obs + 4 * (size_t)d.l0, 4 * (size_t)d.L);
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

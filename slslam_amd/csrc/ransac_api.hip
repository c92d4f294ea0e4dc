// slslam_amd/csrc/ransac_api.hip — SLAM::ransac_motion (reference src/slam.cpp:363-423) for many frames at once: the one RANSAC
// front of the library (ransac_front.h) and the stateless entry points of include/slslam_hip.h, each a thin caller of it.
//
//   generate   k_frames_generate: the motion of every pre-drawn trial from its sample (SLAM::vo_angle_axis_approx), lane <-> trial
//   score      k_frames_score: the scoring loop (:396-413) whose body is SLAM::reprojection_error (:691-726).  One 64-lane wave
//              scores one hypothesis against 64 lines (lane <-> line): the pose is wave-uniform (scalar loads), observations and
//              lines are read coalesced, the inlier set of the block is one __ballot() word and its popcount the block's score
//   loop       one download of the scores, then the adaptive trial loop of every frame on the host (ransac_loop.h)
// The frame index lies in the grid, so the launch count does not depend on the number of frames.  The bodies (bit-identical to the
// reference's float/double mix) are in ransac_device.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "ransac_device.h"
#include "ransac_front.h"

using namespace slslam_ransac;
using slslam::align256;
using slslam::device_present;

namespace {

constexpr int kMaxGrid = 65535;         // what the y and z dimensions of a grid take: frames go in slices of it, hypotheses stride

// blockIdx = (64 trials, frame)
__global__ __launch_bounds__(64) void k_frames_generate(const FrameDesc* __restrict__ fr, const double* __restrict__ dd,
                                                        const int* __restrict__ di, double baseline, double* poses, int* valid) {
  const FrameDesc fd = fr[blockIdx.y];
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= fd.H) return;
  valid[fd.hyp + h] = generate_trial(fd.s, di + fd.smp + (long long)h * fd.s, dd + fd.o0, dd + fd.o1, baseline, poses + 12 * (fd.hyp + h));
}

// blockIdx = (64-line block, hypothesis (strided), frame).  valid == nullptr: the poses are the caller's, every one is scored
__global__ __launch_bounds__(64) void k_frames_score(const FrameDesc* __restrict__ fr, const double* __restrict__ dd, const double* __restrict__ poses,
                                                     const int* __restrict__ valid, double baseline, double thr, int* scores,
                                                     unsigned long long* bits) {
  const FrameDesc fd = fr[blockIdx.z];
  const int blk = blockIdx.x, lane = threadIdx.x;
  if (blk >= fd.words) return;
  const int k = blk * 64 + lane;
  for (int h = blockIdx.y; h < fd.H; h += gridDim.y) {
    const long long g = fd.hyp + h;
    const double* T = poses + 12 * g;
    // `if ( num_sol == 0 ) continue;` (slam.cpp:394) and `if ( motion[j].t.norm() > 1 ) continue;` (:398-399)
    if ((valid && !valid[g]) || pose_skipped(T)) {
      if (blk == 0 && lane == 0) scores[g] = -1;
      if (lane == 0) bits[fd.bits + (long long)h * fd.words + blk] = 0ull;
      continue;
    }
    const bool inlier = k < fd.K && line_inlier(T, dd + fd.o1 + 8 * (long long)k, dd + fd.ln + 6 * (long long)k, baseline, thr);
    const unsigned long long m = __ballot(inlier);
    if (lane == 0) {
      bits[fd.bits + (long long)h * fd.words + blk] = m;
      atomicAdd(&scores[g], __popcll(m));
    }
  }
}

// Lays the frames out, stages them into one host block [FrameDesc F | doubles | ints] and enqueues its upload.  Of each frame at most
// max_trials + 1 trials are kept: the trial loop reads no further.  lines == nullptr: generate only.  poses != nullptr: frame f's
// hypotheses are poses[f] ([12 H], uploaded from where they lie) and nothing is generated.
int front_upload(Workspace& ws, int F, const slslam_ransac_trials* frames, const double* const* lines, const double* const* poses,
                 long long max_trials, Front* fr) {
  fr->fd.assign((size_t)F, FrameDesc{});
  long long nd = 0, ni = 0, nh = 0, nb = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    FrameDesc& d = fr->fd[(size_t)f];
    // ransac_trial = comm_size: without common lines the loop body never runs
    d.H = tr.num_lines > 0 ? (int)std::max(0LL, std::min<long long>(tr.num_trials, max_trials + 1)) : 0;
    d.K = d.H > 0 ? tr.num_lines : 0; d.s = tr.sample_size; d.words = (d.K + 63) / 64;
    d.o0 = nd; if (!poses) nd += 8LL * d.K;
    d.o1 = nd; nd += 8LL * d.K;
    d.ln = nd; if (lines) nd += 6LL * d.K;
    d.smp = ni; if (!poses) ni += (long long)d.H * d.s;
    d.hyp = nh; nh += d.H;
    d.bits = nb; if (lines) nb += (long long)d.H * d.words;
    fr->maxH = std::max(fr->maxH, d.H); fr->maxW = std::max(fr->maxW, d.words); fr->maxK = std::max(fr->maxK, d.K);
  }
  const size_t off_d = align256(sizeof(FrameDesc) * (size_t)F), off_i = off_d + align256(8 * (size_t)nd), in_bytes = off_i + 4 * (size_t)ni;
  const size_t w_bits = align256(96 * (size_t)nh), w_valid = w_bits + align256(8 * (size_t)nb),
               w_scores = w_valid + align256(4 * (size_t)nh), work_bytes = w_scores + 4 * (size_t)nh;
  HIP_TRY(ws.h_in.need(in_bytes, &ws.allocations));
  HIP_TRY(ws.d_in.need(in_bytes, &ws.allocations));
  HIP_TRY(ws.d_work.need(work_bytes, &ws.allocations));
  if (F > 0) std::memcpy(ws.h_in.p, fr->fd.data(), sizeof(FrameDesc) * (size_t)F);
  double* hd = ws.h_in.at<double>(off_d);
  for (int f = 0; f < F; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    const FrameDesc& d = fr->fd[(size_t)f];
    if (d.H == 0) continue;
    std::memcpy(hd + d.o1, tr.observations1, 64 * (size_t)d.K);
    if (lines) std::memcpy(hd + d.ln, lines[f], 48 * (size_t)d.K);
    if (poses) continue;
    std::memcpy(hd + d.o0, tr.observations0, 64 * (size_t)d.K);
    std::memcpy(ws.h_in.at<int>(off_i) + d.smp, tr.samples, 4 * (size_t)d.H * d.s);
  }
  fr->d_fd = ws.d_in.at<FrameDesc>(0);
  fr->d_dd = ws.d_in.at<double>(off_d);
  fr->d_di = ws.d_in.at<int>(off_i);
  fr->d_poses = ws.d_work.at<double>(0);
  fr->d_bits = ws.d_work.at<unsigned long long>(w_bits);
  fr->d_valid = ws.d_work.at<int>(w_valid);
  fr->d_scores = ws.d_work.at<int>(w_scores);
  fr->nh = nh;
  if (nh > 0) HIP_TRY(hipMemcpyAsync(ws.d_in.p, ws.h_in.p, in_bytes, hipMemcpyHostToDevice, ws.stream));
  for (int f = 0; poses && f < F; ++f)
    if (fr->fd[(size_t)f].H > 0)
      HIP_TRY(hipMemcpyAsync(fr->d_poses + 12 * fr->fd[(size_t)f].hyp, poses[f], 96 * (size_t)fr->fd[(size_t)f].H, hipMemcpyHostToDevice, ws.stream));
  return SLSLAM_OK;
}

// Every frame's trials -> poses, valid.  `baseline` as SLAM::vo_angle_axis_approx takes it
int front_generate(Workspace& ws, const Front& fr, double baseline) {
  const int F = (int)fr.fd.size();
  for (int f0 = 0; fr.nh > 0 && f0 < F; f0 += kMaxGrid)
    hipLaunchKernelGGL(k_frames_generate, dim3((unsigned)((fr.maxH + 63) / 64), (unsigned)std::min(F - f0, kMaxGrid)), dim3(64), 0, ws.stream,
                       fr.d_fd + f0, fr.d_dd, fr.d_di, baseline, fr.d_poses, fr.d_valid);
  HIP_TRY(hipGetLastError());
  return SLSLAM_OK;
}

// Every frame's hypotheses against its lines -> scores, bits.  use_valid: skip the trials front_generate found degenerate
int front_score(Workspace& ws, const Front& fr, bool use_valid, double baseline, double thr) {
  const int F = (int)fr.fd.size();
  if (fr.nh == 0) return SLSLAM_OK;
  HIP_TRY(hipMemsetAsync(fr.d_scores, 0, 4 * (size_t)fr.nh, ws.stream));
  for (int f0 = 0; f0 < F; f0 += kMaxGrid)
    hipLaunchKernelGGL(k_frames_score, dim3((unsigned)fr.maxW, (unsigned)std::min(fr.maxH, kMaxGrid), (unsigned)std::min(F - f0, kMaxGrid)), dim3(64), 0,
                       ws.stream, fr.d_fd + f0, fr.d_dd, (const double*)fr.d_poses, use_valid ? (const int*)fr.d_valid : nullptr, baseline, thr,
                       fr.d_scores, fr.d_bits);
  HIP_TRY(hipGetLastError());
  return SLSLAM_OK;
}

// sizes, then pointers, then every sample index of one frame
bool frame_valid(const slslam_ransac_trials& tr, const double* lines, bool scored) {
  const int H = tr.num_trials, K = tr.num_lines, s = tr.sample_size;
  if (H < 0 || K < 0 || s < 1 || s > 16) return false;
  if (H == 0 || (scored && K == 0)) return true;       // comm_size == 0: the reference's trial loop never runs, whatever the sample array holds
  if (K == 0 || !tr.samples || !tr.observations0 || !tr.observations1 || (scored && !lines)) return false;
  for (long long i = 0; i < (long long)H * s; ++i)
    if (tr.samples[i] < 0 || tr.samples[i] >= K) return false;
  return true;
}

}  // namespace

namespace slslam_ransac {

bool trials_valid(int F, const slslam_ransac_trials* frames, const double* const* lines, bool scored) {
  for (int f = 0; f < F; ++f)
    if (!frame_valid(frames[f], scored ? lines[f] : nullptr, scored)) return false;
  return true;
}

int front_ransac(Workspace& ws, int F, const slslam_ransac_trials* frames, const double* const* lines, double baseline, double thr,
                 double prob_free_outliers, int max_trials, const int* best_in, Front* fr) {
  int rc = front_upload(ws, F, frames, lines, nullptr, max_trials, fr);
  // every pre-drawn trial at once: its motion from its sample (the reference passes -baseline, slam.cpp:391-392) ...
  if (rc == SLSLAM_OK) rc = front_generate(ws, *fr, -baseline);
  // ... and its score against all common lines
  if (rc == SLSLAM_OK) rc = front_score(ws, *fr, true, baseline, thr);
  if (rc != SLSLAM_OK) return rc;
  fr->scores.assign((size_t)std::max<long long>(fr->nh, 1), 0);
  if (fr->nh > 0) {
    HIP_TRY(hipMemcpyAsync(fr->scores.data(), fr->d_scores, 4 * (size_t)fr->nh, hipMemcpyDeviceToHost, ws.stream));
    HIP_TRY(hipStreamSynchronize(ws.stream));
  }
  // the adaptive trial loop of the reference (slam.cpp:363, :415-423), replayed in trial order over the scores
  fr->loop.resize((size_t)F);
  for (int f = 0; f < F; ++f) {
    const FrameDesc& d = fr->fd[(size_t)f];
    const int best = best_in ? best_in[f] : -1;
    fr->loop[(size_t)f] = d.H > 0 ? run_trial_loop(fr->scores.data() + d.hyp, d.H, d.K, d.s, prob_free_outliers, max_trials, best) : TrialLoop{ best, -1, 0 };
  }
  return SLSLAM_OK;
}

}  // namespace slslam_ransac

extern "C" int slslam_ransac_score(const slslam_ransac_frame* f, double baseline, double thr, int* scores,
                                   unsigned long long* inlier_bits) {
  if (!f || !scores || f->num_hypotheses < 0 || f->num_lines < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int H = f->num_hypotheses, K = f->num_lines;
  if (H > 0 && !f->poses) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (K > 0 && (!f->observations || !f->lines)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (H == 0) return SLSLAM_OK;
  if (K == 0) {
    for (int h = 0; h < H; ++h) {
      const double* t = f->poses + 12 * (size_t)h + 9;
      scores[h] = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) > 1.0 ? -1 : 0;
    }
    return SLSLAM_OK;
  }
  // the score step alone, over the caller's poses
  const slslam_ransac_trials tr{ H, 1, K, nullptr, nullptr, f->observations };
  Workspace ws(slslam::Mem::kHost);
  Front fr;
  int rc = front_upload(ws, 1, &tr, &f->lines, &f->poses, INT_MAX, &fr);
  if (rc == SLSLAM_OK) rc = front_score(ws, fr, false, baseline, thr);
  if (rc != SLSLAM_OK) return rc;
  HIP_TRY(hipMemcpy(scores, fr.d_scores, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost));
  if (inlier_bits) HIP_TRY(hipMemcpy(inlier_bits, fr.d_bits, sizeof(unsigned long long) * (size_t)H * fr.fd[0].words, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

extern "C" int slslam_ransac_generate(const slslam_ransac_trials* tr, double baseline, double* poses, int* valid) {
  if (!tr || !poses || !valid || !trials_valid(1, tr, nullptr, false)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  const int H = tr->num_trials;
  if (H == 0) return SLSLAM_OK;
  // the generate step alone; `baseline` is passed as given
  Workspace ws(slslam::Mem::kHost);
  Front fr;
  int rc = front_upload(ws, 1, tr, nullptr, nullptr, INT_MAX, &fr);
  if (rc == SLSLAM_OK) rc = front_generate(ws, fr, baseline);
  if (rc != SLSLAM_OK) return rc;
  HIP_TRY(hipMemcpy(poses, fr.d_poses, sizeof(double) * 12 * (size_t)H, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(valid, fr.d_valid, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

extern "C" int slslam_ransac_motion(const slslam_ransac_trials* tr, const double* lines, double baseline, double error_thr,
                                    double prob_free_outliers, int max_trials, int* best_score_io, int* trial_cnt,
                                    double* best_pose, unsigned long long* best_inlier_bits) {
  if (!tr) return SLSLAM_ERR_INVALID_ARGUMENT;
  return slslam_ransac_motion_batch(1, tr, &lines, baseline, error_thr, prob_free_outliers, max_trials, best_score_io, trial_cnt, best_pose,
                                    &best_inlier_bits);
}

// Many frames at once (replay of a sequence, several cameras): one upload, two launches for all frames, one download of every
// frame's scores, then the per-frame trial loops on the host and one gather of the winners.
extern "C" int slslam_ransac_motion_batch(int num_frames, const slslam_ransac_trials* frames, const double* const* lines,
                                          double baseline, double error_thr, double prob_free_outliers, int max_trials,
                                          int* best_score_io, int* trial_cnt, double* best_pose,
                                          unsigned long long* const* best_inlier_bits) {
  if (num_frames < 0 || (num_frames > 0 && (!frames || !lines || !best_score_io || !trial_cnt || !best_pose)))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!trials_valid(num_frames, frames, lines, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (num_frames == 0) return SLSLAM_OK;
  Workspace ws(slslam::Mem::kHost);
  Front fr;
  const int rc = front_ransac(ws, num_frames, frames, lines, baseline, error_thr, prob_free_outliers, max_trials, best_score_io, &fr);
  if (rc != SLSLAM_OK) return rc;
  for (int f = 0; f < num_frames; ++f) {
    const FrameDesc& d = fr.fd[(size_t)f];
    const TrialLoop& tl = fr.loop[(size_t)f];
    trial_cnt[f] = tl.trial_cnt;
    best_score_io[f] = tl.best;
    if (tl.best_h < 0) continue;
    HIP_TRY(hipMemcpy(best_pose + 12 * (size_t)f, fr.d_poses + 12 * (d.hyp + tl.best_h), sizeof(double) * 12, hipMemcpyDeviceToHost));
    if (best_inlier_bits && best_inlier_bits[f])
      HIP_TRY(hipMemcpy(best_inlier_bits[f], fr.d_bits + d.bits + (long long)tl.best_h * d.words, sizeof(unsigned long long) * d.words, hipMemcpyDeviceToHost));
  }
  return SLSLAM_OK;
}

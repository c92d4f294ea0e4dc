// slslam_amd/csrc/ransac_api.hip — RANSAC hypothesis scoring.
//
// Replaces the scoring loop of SLAM::ransac_motion (reference src/slam.cpp:396-413) whose body is
// SLAM::reprojection_error (src/slam.cpp:691-726).  One 64-lane wave scores one hypothesis against 64
// lines (lane <-> line): the pose is wave-uniform (scalar loads), observations and lines are read
// coalesced, the inlier set of the block is one __ballot() word and its popcount the block's score.
// The bodies (bit-identical to the reference's float/double mix) are in ransac_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/slslam_hip.h"
#include "ransac_device.h"
#include "ransac_loop.h"

using namespace slslam_ransac;

namespace {

__global__ __launch_bounds__(64) void k_ransac_score(int H, int K, int words, const double* __restrict__ poses,
                                                     const double* __restrict__ obs, const double* __restrict__ lines,
                                                     double baseline, double thr, int* scores, unsigned long long* bits,
                                                     const int* __restrict__ valid) {
  const int h = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x;
  const int k = blk * 64 + lane;
  const double* T = poses + 12 * (long long)h;
  // `if ( num_sol == 0 ) continue;` (slam.cpp:394) and `if ( motion[j].t.norm() > 1 ) continue;` (:398-399)
  if ((valid && !valid[h]) || pose_skipped(T)) {
    if (blk == 0 && lane == 0) scores[h] = -1;
    if (bits && lane == 0) bits[(long long)h * words + blk] = 0ull;
    return;
  }
  const bool inlier = k < K && line_inlier(T, obs + 8 * (long long)k, lines + 6 * (long long)k, baseline, thr);
  const unsigned long long m = __ballot(inlier);
  if (lane == 0) {
    if (bits) bits[(long long)h * words + blk] = m;
    atomicAdd(&scores[h], __popcll(m));
  }
}

// Hypothesis generation (ransac_device.h), lane <-> trial
__global__ __launch_bounds__(64) void k_ransac_generate(int H, int s, const int* __restrict__ samples,
                                                        const double* __restrict__ obs0, const double* __restrict__ obs1,
                                                        double baseline, double* poses, int* valid) {
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= H) return;
  valid[h] = generate_trial(s, samples + (long long)h * s, obs0, obs1, baseline, poses + 12 * (long long)h);
}

}  // namespace

extern "C" int slslam_ransac_score(const slslam_ransac_frame* f, double baseline, double thr, int* scores,
                                   unsigned long long* inlier_bits) {
  if (!f || !scores || f->num_hypotheses < 0 || f->num_lines < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int H = f->num_hypotheses, K = f->num_lines;
  if (H > 0 && !f->poses) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (K > 0 && (!f->observations || !f->lines)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (H == 0) return SLSLAM_OK;
  const int words = (K + 63) / 64;
  if (K == 0) {
    for (int h = 0; h < H; ++h) {
      const double* t = f->poses + 12 * (size_t)h + 9;
      scores[h] = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) > 1.0 ? -1 : 0;
    }
    return SLSLAM_OK;
  }
  double *d_poses = nullptr, *d_obs = nullptr, *d_lines = nullptr;
  int* d_scores = nullptr;
  unsigned long long* d_bits = nullptr;
  int rc = SLSLAM_OK;
#define RS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::fprintf(stderr, "slslam: %s failed: %s\n", #expr, hipGetErrorString(_e)); rc = SLSLAM_ERR_HIP; goto done; } } while (0)
  RS_TRY(hipMalloc((void**)&d_poses, sizeof(double) * 12 * H));
  RS_TRY(hipMalloc((void**)&d_obs, sizeof(double) * 8 * K));
  RS_TRY(hipMalloc((void**)&d_lines, sizeof(double) * 6 * K));
  RS_TRY(hipMalloc((void**)&d_scores, sizeof(int) * H));
  RS_TRY(hipMalloc((void**)&d_bits, sizeof(unsigned long long) * (size_t)H * words));
  RS_TRY(hipMemcpy(d_poses, f->poses, sizeof(double) * 12 * H, hipMemcpyHostToDevice));
  RS_TRY(hipMemcpy(d_obs, f->observations, sizeof(double) * 8 * K, hipMemcpyHostToDevice));
  RS_TRY(hipMemcpy(d_lines, f->lines, sizeof(double) * 6 * K, hipMemcpyHostToDevice));
  RS_TRY(hipMemset(d_scores, 0, sizeof(int) * H));
  hipLaunchKernelGGL(k_ransac_score, dim3((unsigned)words, (unsigned)H), dim3(64), 0, 0, H, K, words, d_poses, d_obs, d_lines,
                     baseline, thr, d_scores, d_bits, (const int*)nullptr);
  RS_TRY(hipGetLastError());
  RS_TRY(hipMemcpy(scores, d_scores, sizeof(int) * H, hipMemcpyDeviceToHost));
  if (inlier_bits) RS_TRY(hipMemcpy(inlier_bits, d_bits, sizeof(unsigned long long) * (size_t)H * words, hipMemcpyDeviceToHost));
#undef RS_TRY
done:
  (void)hipFree(d_poses); (void)hipFree(d_obs); (void)hipFree(d_lines); (void)hipFree(d_scores); (void)hipFree(d_bits);
  return rc;
}


namespace {
template <typename T>
struct DevArr {
  T* p = nullptr;
  ~DevArr() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc((void**)&p, sizeof(T) * (n ? n : 1)); }
};
}  // namespace

#define RM_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::fprintf(stderr, "slslam: %s failed: %s\n", #expr, hipGetErrorString(_e)); return SLSLAM_ERR_HIP; } } while (0)

extern "C" int slslam_ransac_generate(const slslam_ransac_trials* tr, double baseline, double* poses, int* valid) {
  if (!tr || !poses || !valid || tr->num_trials < 0 || tr->num_lines < 0 || tr->sample_size < 1 || tr->sample_size > 16)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  const int H = tr->num_trials, K = tr->num_lines, s = tr->sample_size;
  if (H > 0 && (!tr->samples || !tr->observations0 || !tr->observations1 || K == 0)) return SLSLAM_ERR_INVALID_ARGUMENT;
  for (long long i = 0; i < (long long)H * s; ++i)
    if (tr->samples[i] < 0 || tr->samples[i] >= K) return SLSLAM_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (H == 0) return SLSLAM_OK;
  DevArr<double> d_o0, d_o1, d_poses;
  DevArr<int> d_smp, d_valid;
  RM_TRY(d_o0.alloc(8 * (size_t)K)); RM_TRY(d_o1.alloc(8 * (size_t)K)); RM_TRY(d_poses.alloc(12 * (size_t)H));
  RM_TRY(d_smp.alloc((size_t)H * s)); RM_TRY(d_valid.alloc(H));
  RM_TRY(hipMemcpy(d_o0.p, tr->observations0, sizeof(double) * 8 * K, hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(d_o1.p, tr->observations1, sizeof(double) * 8 * K, hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(d_smp.p, tr->samples, sizeof(int) * (size_t)H * s, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_ransac_generate, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, 0, H, s, d_smp.p, d_o0.p, d_o1.p, baseline,
                     d_poses.p, d_valid.p);
  RM_TRY(hipGetLastError());
  RM_TRY(hipMemcpy(poses, d_poses.p, sizeof(double) * 12 * H, hipMemcpyDeviceToHost));
  RM_TRY(hipMemcpy(valid, d_valid.p, sizeof(int) * H, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

extern "C" int slslam_ransac_motion(const slslam_ransac_trials* tr, const double* lines, double baseline, double error_thr,
                                    double prob_free_outliers, int max_trials, int* best_score_io, int* trial_cnt,
                                    double* best_pose, unsigned long long* best_inlier_bits) {
  if (!tr || !best_score_io || !trial_cnt || !best_pose || tr->num_trials < 0 || tr->num_lines < 0 || tr->sample_size < 1 ||
      tr->sample_size > 16)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  const int H = tr->num_trials, K = tr->num_lines, s = tr->sample_size;
  if (H > 0 && K > 0 && (!tr->samples || !tr->observations0 || !tr->observations1 || !lines)) return SLSLAM_ERR_INVALID_ARGUMENT;
  // comm_size == 0: the reference's trial loop never runs (ransac_trial = 0), whatever the sample array holds
  for (long long i = 0; K > 0 && i < (long long)H * s; ++i)
    if (tr->samples[i] < 0 || tr->samples[i] >= K) return SLSLAM_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  *trial_cnt = 0;
  if (H == 0 || K == 0) return SLSLAM_OK;                     // ransac_trial = comm_size = 0: the loop body never runs
  const int words = (K + 63) / 64;
  DevArr<double> d_o0, d_o1, d_lines, d_poses;
  DevArr<int> d_smp, d_valid, d_scores;
  DevArr<unsigned long long> d_bits;
  RM_TRY(d_o0.alloc(8 * (size_t)K)); RM_TRY(d_o1.alloc(8 * (size_t)K)); RM_TRY(d_lines.alloc(6 * (size_t)K));
  RM_TRY(d_poses.alloc(12 * (size_t)H)); RM_TRY(d_smp.alloc((size_t)H * s)); RM_TRY(d_valid.alloc(H)); RM_TRY(d_scores.alloc(H));
  RM_TRY(d_bits.alloc((size_t)H * words));
  RM_TRY(hipMemcpy(d_o0.p, tr->observations0, sizeof(double) * 8 * K, hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(d_o1.p, tr->observations1, sizeof(double) * 8 * K, hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(d_lines.p, lines, sizeof(double) * 6 * K, hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(d_smp.p, tr->samples, sizeof(int) * (size_t)H * s, hipMemcpyHostToDevice));
  RM_TRY(hipMemset(d_scores.p, 0, sizeof(int) * H));
  // every pre-drawn trial at once: motion from its sample (the reference passes -baseline, slam.cpp:391-392) ...
  hipLaunchKernelGGL(k_ransac_generate, dim3((unsigned)((H + 63) / 64)), dim3(64), 0, 0, H, s, d_smp.p, d_o0.p, d_o1.p, -baseline,
                     d_poses.p, d_valid.p);
  // ... and its score against all common lines
  hipLaunchKernelGGL(k_ransac_score, dim3((unsigned)words, (unsigned)H), dim3(64), 0, 0, H, K, words, d_poses.p, d_o1.p, d_lines.p,
                     baseline, error_thr, d_scores.p, d_bits.p, (const int*)d_valid.p);
  RM_TRY(hipGetLastError());
  std::vector<int> scores(H);
  RM_TRY(hipMemcpy(scores.data(), d_scores.p, sizeof(int) * H, hipMemcpyDeviceToHost));
  // the adaptive trial loop of the reference (slam.cpp:363, :415-423), replayed in trial order over the scores
  const TrialLoop tl = run_trial_loop(scores.data(), H, K, s, prob_free_outliers, max_trials, *best_score_io);
  const int best_h = tl.best_h;
  *trial_cnt = tl.trial_cnt;
  *best_score_io = tl.best;
  if (best_h >= 0) {
    RM_TRY(hipMemcpy(best_pose, d_poses.p + 12 * (size_t)best_h, sizeof(double) * 12, hipMemcpyDeviceToHost));
    if (best_inlier_bits)
      RM_TRY(hipMemcpy(best_inlier_bits, d_bits.p + (size_t)best_h * words, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost));
  }
  return SLSLAM_OK;
}


// Many frames at once (replay of a sequence, several cameras): one device allocation, one upload, two launches
// per frame enqueued back to back without host synchronisation, one download of every frame's scores, then the
// per-frame trial loops on the host and one gather of the winners.  Per frame the results are those of
// slslam_ransac_motion.
extern "C" int slslam_ransac_motion_batch(int num_frames, const slslam_ransac_trials* frames, const double* const* lines,
                                          double baseline, double error_thr, double prob_free_outliers, int max_trials,
                                          int* best_score_io, int* trial_cnt, double* best_pose,
                                          unsigned long long* const* best_inlier_bits) {
  if (num_frames < 0 || (num_frames > 0 && (!frames || !lines || !best_score_io || !trial_cnt || !best_pose)))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  struct Off { size_t o0, o1, ln, smp, poses, valid, scores, bits; int H, K, s, words; };
  std::vector<Off> off(num_frames);
  size_t nd = 0, ni = 0, nb = 0;       // doubles, ints, 64-bit words
  for (int f = 0; f < num_frames; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    if (tr.num_trials < 0 || tr.num_lines < 0 || tr.sample_size < 1 || tr.sample_size > 16) return SLSLAM_ERR_INVALID_ARGUMENT;
    const int H = tr.num_trials, K = tr.num_lines, s = tr.sample_size;
    if (H > 0 && K > 0 && (!tr.samples || !tr.observations0 || !tr.observations1 || !lines[f])) return SLSLAM_ERR_INVALID_ARGUMENT;
    for (long long i = 0; K > 0 && i < (long long)H * s; ++i)      // a frame without common lines runs no trials
      if (tr.samples[i] < 0 || tr.samples[i] >= K) return SLSLAM_ERR_INVALID_ARGUMENT;
    Off& o = off[f];
    o.H = H; o.K = K; o.s = s; o.words = (K + 63) / 64;
    o.o0 = nd; nd += 8 * (size_t)K; o.o1 = nd; nd += 8 * (size_t)K; o.ln = nd; nd += 6 * (size_t)K; o.poses = nd; nd += 12 * (size_t)H;
    o.smp = ni; ni += (size_t)H * s; o.valid = ni; ni += H; o.scores = ni; ni += H;
    o.bits = nb; nb += (size_t)H * o.words;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  for (int f = 0; f < num_frames; ++f) trial_cnt[f] = 0;
  if (num_frames == 0) return SLSLAM_OK;
  std::vector<double> hd(nd ? nd : 1, 0.0);
  std::vector<int> hi(ni ? ni : 1, 0);
  for (int f = 0; f < num_frames; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    const Off& o = off[f];
    if (o.H == 0 || o.K == 0) continue;
    std::copy(tr.observations0, tr.observations0 + 8 * (size_t)o.K, hd.begin() + o.o0);
    std::copy(tr.observations1, tr.observations1 + 8 * (size_t)o.K, hd.begin() + o.o1);
    std::copy(lines[f], lines[f] + 6 * (size_t)o.K, hd.begin() + o.ln);
    std::copy(tr.samples, tr.samples + (size_t)o.H * o.s, hi.begin() + o.smp);
  }
  DevArr<double> dd;
  DevArr<int> di;
  DevArr<unsigned long long> db;
  RM_TRY(dd.alloc(nd)); RM_TRY(di.alloc(ni)); RM_TRY(db.alloc(nb));
  RM_TRY(hipMemcpy(dd.p, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice));
  RM_TRY(hipMemcpy(di.p, hi.data(), sizeof(int) * hi.size(), hipMemcpyHostToDevice));     // scores arrive zeroed
  for (int f = 0; f < num_frames; ++f) {
    const Off& o = off[f];
    if (o.H == 0 || o.K == 0) continue;
    hipLaunchKernelGGL(k_ransac_generate, dim3((unsigned)((o.H + 63) / 64)), dim3(64), 0, 0, o.H, o.s, di.p + o.smp, dd.p + o.o0,
                       dd.p + o.o1, -baseline, dd.p + o.poses, di.p + o.valid);
    hipLaunchKernelGGL(k_ransac_score, dim3((unsigned)o.words, (unsigned)o.H), dim3(64), 0, 0, o.H, o.K, o.words, dd.p + o.poses,
                       dd.p + o.o1, dd.p + o.ln, baseline, error_thr, di.p + o.scores, db.p + o.bits, (const int*)(di.p + o.valid));
  }
  RM_TRY(hipGetLastError());
  RM_TRY(hipMemcpy(hi.data(), di.p, sizeof(int) * hi.size(), hipMemcpyDeviceToHost));
  for (int f = 0; f < num_frames; ++f) {
    const Off& o = off[f];
    if (o.H == 0 || o.K == 0) continue;
    const int* scores = hi.data() + o.scores;
    const TrialLoop tl = run_trial_loop(scores, o.H, o.K, o.s, prob_free_outliers, max_trials, best_score_io[f]);
    const int best_h = tl.best_h;
    trial_cnt[f] = tl.trial_cnt;
    best_score_io[f] = tl.best;
    if (best_h >= 0) {
      RM_TRY(hipMemcpy(best_pose + 12 * (size_t)f, dd.p + o.poses + 12 * (size_t)best_h, sizeof(double) * 12, hipMemcpyDeviceToHost));
      if (best_inlier_bits && best_inlier_bits[f])
        RM_TRY(hipMemcpy(best_inlier_bits[f], db.p + o.bits + (size_t)best_h * o.words, sizeof(unsigned long long) * o.words,
                         hipMemcpyDeviceToHost));
    }
  }
  return SLSLAM_OK;
}

// slslam_amd/csrc/frame_api.hip — the per-frame pose estimator (include/slslam_hip.h: slslam_pose_estimator_*).
//
// SLAM::pose_estimation (reference src/slam.cpp:244-319) after its merge by feature id, for many frames per call:
//   RANSAC      the library's one RANSAC front (ransac_front.h, compiled in ransac_api.hip) on the estimator's buffers and stream: two
//               launches for all frames, one download of the scores, the adaptive trial loops on the host, best_score starting at -1 (:283)
//   pack        k_frame_pack: one wave per solvable frame writes its motion-only window (:590-640) into device memory
//   solve       the estimator's refillable fused motion-only LBA batch, refilled from those device windows (lba_resident.h)
//   finish      k_frame_finish: gc_wt_to_Rt of the solved camera (:668-674) and the final inlier set under it (:305-312), with the
//               refined pose, the summaries and the RANSAC winners gathered into one result block - one download
//   covariance  (slslam_pose_estimator_set_covariance, off by default) behind the solve: slslam_lba_batch_covariance of the batch, cameras
//               only, and k_frame_covariance: one wave per slot gathers the 6 x 6 block, its status, the residual variance and the
//               solved parameters into a third part of the result block - the same one download
// Two host round trips per call, whatever the number of frames.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "ransac_device.h"
#include "ransac_front.h"
#include "gc_convert.h"
#include "index_word.h"
#include "lba_resident.h"

using namespace slslam_ransac;
using slslam::align256;
using slslam::GrowBuf;
using slslam::Mem;

namespace {

constexpr int kMaxFeatNum = 5;          // max_feat_num (reference src/parameter.h:25): the fewest common lines / RANSAC inliers accepted

// Per frame, what the trial loop decided (uploaded after it)
struct FramePlan {
  int best_h, slot;
  long long outb;                       // first word of the frame's bits in the result block (RANSAC winner, then final set: words each)
};
// Per slot of the batch: its frame (-1: a placeholder) and where its window lies
struct SlotDesc {
  int frame, n, best_h, pad;            // frame, inliers = lines of the window, the winning trial
  long long exp_off;                    // the window's parameters in the batch's export (6 C + 4 L per window, slots in order)
};
// Per frame, what comes back
struct FrameOut {
  double ransac_pose[12];
  double pose[12];
  double initial_cost, final_cost, fixed_cost;
  int n_success, n_unsuccess, termination, nfree, nkept, num_inliers, built, pad;
};

// Per frame, with covariance enabled: the third part of the result block (zeros for a frame without a slot)
struct FrameCov {
  double constraint[6];
  double cov[36];
  double sigma2;
  int status, dof;
};

// Window slot i lies at a fixed stride in the window buffers: words [2 Lcap], observations [16 Lcap], parameters [12 + 4 Lcap]
struct WinBufs { unsigned* words; double* obs; double* par; int cap_lines; };

// One wave per slot: the motion-only window of the slot's frame (reference src/slam.cpp:590-640, slslam_pack_motion_only) -
// camera 0 = gc_Rt_to_wt(RANSAC pose), free; camera 1 = identity, constant; per inlier in ascending line order (camera 0, obs1) then
// (camera 1, obs0); every line constant, gc_av_to_orth(line).  The winner's inlier word is the ballot of its lines (k_frames_score):
// a lane's place among the inliers is the popcount of the word below it.  A placeholder slot gets a one-line window of the same shape.
__global__ __launch_bounds__(64) void k_frame_pack(const SlotDesc* __restrict__ slots, const FrameDesc* __restrict__ fr, const double* __restrict__ dd,
                                                   const double* __restrict__ poses, const unsigned long long* __restrict__ bits, WinBufs wb) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const SlotDesc sd = slots[i];
  unsigned* words = wb.words + (long long)i * 2 * wb.cap_lines;
  double* obs = wb.obs + (long long)i * 16 * wb.cap_lines;
  double* par = wb.par + (long long)i * (12 + 4 * (long long)wb.cap_lines);
  if (lane == 0) {
    double I[12] = { 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0 };
    slslam_gc::Rt_to_wt(I, par + 6);                                   // camera 1: pose_t() (:591)
  }
  if (sd.frame < 0) {
    if (lane == 0) { words[0] = slslam::index_word(0, 0, 0, 1); words[1] = slslam::index_word(1, 0, 1, 1); }
    if (lane < 6) par[lane] = 0.0;
    if (lane < 4) par[12 + lane] = 0.5;
    if (lane < 16) obs[lane] = 0.25 * (double)((lane & 3) + 1);
    return;
  }
  const FrameDesc fd = fr[sd.frame];
  if (lane == 0) slslam_gc::Rt_to_wt(poses + 12 * (fd.hyp + sd.best_h), par);   // camera 0: the RANSAC estimate (:590)
  const unsigned long long* wbits = bits + fd.bits + (long long)sd.best_h * fd.words;
  int base = 0;
  for (int w = 0; w < fd.words; ++w) {
    const unsigned long long m = wbits[w];
    const int k = 64 * w + lane;
    if ((m >> lane) & 1ull) {
      const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
      words[2 * pos] = slslam::index_word(0, pos, 0, 1);              // :593-607
      words[2 * pos + 1] = slslam::index_word(1, pos, 1, 1);
      const double* o1 = dd + fd.o1 + 8 * (long long)k;
      const double* o0 = dd + fd.o0 + 8 * (long long)k;
      double* ob = obs + 16 * (long long)pos;
      for (int q = 0; q < 8; ++q) { ob[q] = o1[q]; ob[8 + q] = o0[q]; }
      slslam_gc::av_to_orth(dd + fd.ln + 6 * (long long)k, par + 12 + 4 * (long long)pos);
    }
    base += __popcll(m);
  }
}

// blockIdx = (64-line block, frame): the RANSAC winner's pose and bits; for a solved frame gc_wt_to_Rt of camera 0 (:668-674), its
// summary, and the final inlier set under the refined pose (:305-312: every common line, no |t| test)
__global__ __launch_bounds__(64) void k_frame_finish(const FrameDesc* __restrict__ fr, const FramePlan* __restrict__ plans,
                                                     const SlotDesc* __restrict__ slots, const double* __restrict__ dd,
                                                     const double* __restrict__ poses, const unsigned long long* __restrict__ bits,
                                                     const double* __restrict__ exported, const slslam::LMState* __restrict__ state,
                                                     const slslam::WinDesc* __restrict__ wins, double baseline, double thr, FrameOut* out,
                                                     unsigned long long* out_bits) {
  const int f = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x;
  const FrameDesc fd = fr[f];
  const FramePlan pl = plans[f];
  if (blk >= fd.words || pl.best_h < 0) return;
  FrameOut& o = out[f];
  if (lane == 0) out_bits[pl.outb + blk] = bits[fd.bits + (long long)pl.best_h * fd.words + blk];
  if (blk == 0 && lane < 12) o.ransac_pose[lane] = poses[12 * (fd.hyp + pl.best_h) + lane];
  if (pl.slot < 0) return;
  const SlotDesc sd = slots[pl.slot];
  double T[12];
  slslam_gc::wt_to_Rt(exported + sd.exp_off, T);
  if (blk == 0 && lane == 0) {
    for (int q = 0; q < 12; ++q) o.pose[q] = T[q];
    const slslam::LMState st = state[pl.slot];
    const slslam::WinDesc wd = wins[pl.slot];
    o.initial_cost = st.initial_cost;
    o.final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;      // (slslam_lba_batch_get_summary)
    o.fixed_cost = st.fixed_cost;
    o.n_success = st.n_success; o.n_unsuccess = st.n_unsuccess;
    o.termination = st.status == slslam::kRunning ? SLSLAM_NO_CONVERGENCE : st.status;
    o.nfree = wd.nfree_params; o.nkept = wd.nkept;
    o.built = wd.C == 2 ? 1 : 0;
  }
  const int k = blk * 64 + lane;
  const bool inlier = k < fd.K && line_inlier(T, dd + fd.o1 + 8 * (long long)k, dd + fd.ln + 6 * (long long)k, baseline, thr);
  const unsigned long long m = __ballot(inlier);
  if (lane == 0) {
    out_bits[pl.outb + fd.words + blk] = m;
    atomicAdd(&o.num_inliers, __popcll(m));
  }
}

// One wave per slot: the slot's covariance block (k_lba_covariance: row-major 6 x 6 at the front of the window's slot, zeros when
// singular) and status, the residual variance 2 (final cost - fixed cost) / dof of the kept blocks with dof = 4 nkept - 6, and the solved
// camera 0 from the export, into the frame's FrameCov.  A placeholder slot writes nothing.
__global__ __launch_bounds__(64) void k_frame_covariance(const SlotDesc* __restrict__ slots, int nslots, const int* __restrict__ cov_hdr,
                                                         int hdr_ints, const double* __restrict__ cov_cam, long long cam_stride,
                                                         const double* __restrict__ exported, const slslam::LMState* __restrict__ state,
                                                         const slslam::WinDesc* __restrict__ wins, FrameCov* out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= nslots) return;
  const SlotDesc sd = slots[i];
  if (sd.frame < 0) return;
  FrameCov& o = out[sd.frame];
  const int status = cov_hdr[(long long)i * hdr_ints] == SLSLAM_COV_OK && cov_hdr[(long long)i * hdr_ints + 1] == 1 ? SLSLAM_COV_OK : SLSLAM_COV_SINGULAR;
  if (lane < 36) o.cov[lane] = status == SLSLAM_COV_OK ? cov_cam[(long long)i * cam_stride + lane] : 0.0;
  else if (lane < 42) o.constraint[lane - 36] = exported[sd.exp_off + (lane - 36)];
  else if (lane == 42) {
    const slslam::LMState st = state[i];
    const int dof = 4 * wins[i].nkept - 6;
    const double final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;      // (as k_frame_finish: the summary's)
    o.sigma2 = 2.0 * (final_cost - st.fixed_cost) / (double)dof;
    o.status = status; o.dof = dof;
  }
}

}  // namespace

struct slslam_pose_estimator {
  int device = -1;
  slslam_solver_options opt;
  int cap_frames = 0, cap_lines = 0;               // what the batch and the window buffers hold
  slslam_lba_batch* batch = nullptr;
  Workspace ws{Mem::kPinned};                      // the RANSAC front's buffers, the stream of every call, the allocation counter
  GrowBuf d_win{Mem::kDevice}, d_export{Mem::kDevice}, d_small{Mem::kDevice}, d_out{Mem::kDevice};
  GrowBuf h_small{Mem::kPinned}, h_out{Mem::kPinned};
  long long calls = 0, finalizes = 0, refills = 0;
  bool want_cov = false, last_cov = false;         // slslam_pose_estimator_set_covariance; whether the last run gathered covariances ...
  size_t off_cov = 0;                              // ... and where its FrameCov[F] lie in h_out
  // the last call, for slslam_pose_estimator_window
  std::vector<int> slot_of_frame, n_of_frame;
  std::vector<long long> exp_off_of_frame;
  void drop_batch() { if (batch) { slslam_lba_batch_destroy(batch); batch = nullptr; } }
  ~slslam_pose_estimator() {
    drop_batch();
    if (ws.stream) (void)hipStreamDestroy(ws.stream);
  }
};

extern "C" int slslam_pose_estimator_create(int device, const slslam_solver_options* opt, int max_frames, int max_lines,
                                            slslam_pose_estimator** out) {
  if (!out || max_frames < 1 || max_lines < kMaxFeatNum || max_lines > 0xfffe) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_pose_estimator* e = new (std::nothrow) slslam_pose_estimator();
  if (!e) return SLSLAM_ERR_NO_MEMORY;
  if (opt) e->opt = *opt; else slslam_default_options(&e->opt);
  // the estimator's batch is a refillable one on the fused motion-only path, built on the device
  e->opt.lba_fused_motion_only = 1;
  e->opt.reuse_elimination = 0;
  e->opt.device_build = 0;
  if (e->opt.refill_headroom_percent <= 0) e->opt.refill_headroom_percent = 10;
  e->device = device;
  e->cap_frames = max_frames; e->cap_lines = max_lines;
  *out = e;
  return SLSLAM_OK;
}

extern "C" void slslam_pose_estimator_destroy(slslam_pose_estimator* e) { delete e; }

extern "C" int slslam_pose_estimator_stats(const slslam_pose_estimator* e, long long* calls, long long* allocations, long long* finalizes,
                                           long long* refills) {
  if (!e) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (calls) *calls = e->calls;
  if (allocations) *allocations = e->ws.allocations;
  if (finalizes) *finalizes = e->finalizes;
  if (refills) *refills = e->refills;
  return SLSLAM_OK;
}

namespace {

// The batch: cap_frames windows of the motion-only shape with cap_lines lines each (placeholder values), finalized once; every
// call refills all its windows.  A new one only when a call needs more frames or lines than it holds.
int ensure_batch(slslam_pose_estimator* e, int frames, int lines) {
  if (e->batch && frames <= e->cap_frames && lines <= e->cap_lines) return SLSLAM_OK;
  e->drop_batch();
  e->cap_frames = std::max(e->cap_frames, frames);
  e->cap_lines = std::max(e->cap_lines, lines);
  const int L = e->cap_lines, M = 2 * L;
  std::vector<int> cam((size_t)M), line((size_t)M), fixed(2 * (size_t)M);
  std::vector<double> obs(8 * (size_t)M), par(12 + 4 * (size_t)L, 0.5);
  for (int l = 0; l < L; ++l) {
    cam[2 * (size_t)l] = 0; line[2 * (size_t)l] = l; fixed[4 * (size_t)l] = 0; fixed[4 * (size_t)l + 1] = 1;
    cam[2 * (size_t)l + 1] = 1; line[2 * (size_t)l + 1] = l; fixed[4 * (size_t)l + 2] = 1; fixed[4 * (size_t)l + 3] = 1;
  }
  for (size_t q = 0; q < obs.size(); ++q) obs[q] = 0.25 * (double)((q & 3) + 1);
  for (int a = 0; a < 12; ++a) par[(size_t)a] = 0.0;
  slslam_lba_window w;
  w.num_cameras = 2; w.num_lines = L; w.num_observations = M;
  w.camera_index = cam.data(); w.line_index = line.data(); w.fixed_index = fixed.data(); w.observations = obs.data(); w.parameters = par.data();
  slslam_lba_batch* b = nullptr;
  int rc = slslam_lba_batch_create(e->device, &b);
  for (int i = 0; rc == SLSLAM_OK && i < e->cap_frames; ++i) rc = slslam_lba_batch_add(b, &w, nullptr);
  if (rc == SLSLAM_OK) rc = slslam_lba_batch_finalize(b, &e->opt);
  int path = -1;
  if (rc == SLSLAM_OK) rc = slslam_lba_batch_path(b, &path);
  if (rc == SLSLAM_OK && path != SLSLAM_PATH_FUSED_MOTION_ONLY) rc = SLSLAM_ERR_UNSUPPORTED;
  if (rc != SLSLAM_OK) { if (b) slslam_lba_batch_destroy(b); return rc; }
  e->batch = b;
  ++e->finalizes;
  return SLSLAM_OK;
}

}  // namespace

extern "C" int slslam_pose_estimator_run(slslam_pose_estimator* e, int num_frames, const slslam_ransac_trials* frames, const double* const* lines,
                                         double baseline, double error_thr, double prob_free_outliers, int max_trials,
                                         slslam_pose_estimate* out) {
  // ---- every argument before anything is written or the device is asked (as slslam_ransac_motion_batch)
  if (!e || num_frames < 0 || (num_frames > 0 && (!frames || !lines || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  for (int f = 0; f < F; ++f)
    if (frames[f].num_lines > 0xfffe) return SLSLAM_ERR_INVALID_ARGUMENT;        // (the windows' index words hold 16-bit line indices)
  if (!trials_valid(F, frames, lines, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = slslam::use_device(e->device);
  if (rc != SLSLAM_OK) return rc;
  if (!e->ws.stream) HIP_TRY(hipStreamCreateWithFlags(&e->ws.stream, hipStreamNonBlocking));
  hipStream_t s = e->ws.stream;
  ++e->calls;
  e->last_cov = false;
  const bool with_cov = e->want_cov;
  e->slot_of_frame.assign((size_t)F, -1); e->n_of_frame.assign((size_t)F, 0); e->exp_off_of_frame.assign((size_t)F, 0);

  // ---- RANSAC of every frame (best_score = -1, slam.cpp:283); a frame with fewer than 5 common lines runs nothing (:275)
  std::vector<slslam_ransac_trials> gated(frames, frames + F);
  for (slslam_ransac_trials& tr : gated)
    if (tr.num_lines < kMaxFeatNum) tr.num_trials = 0;
  Front fr;
  rc = front_ransac(e->ws, F, gated.data(), lines, baseline, error_thr, prob_free_outliers, max_trials, nullptr, &fr);
  if (rc != SLSLAM_OK) return rc;
  const std::vector<FrameDesc>& fd = fr.fd;
  const std::vector<TrialLoop>& loop = fr.loop;
  const FrameDesc* d_fd = fr.d_fd;
  const double *d_dd = fr.d_dd, *d_poses = fr.d_poses;
  const unsigned long long* d_bits = fr.d_bits;
  const int maxW = fr.maxW, maxK = fr.maxK;

  // ---- statuses, the solvable frames' slots, where each frame's bits lie in the result block
  std::vector<FramePlan> plan((size_t)F);
  std::vector<int> slot_frame;
  long long nob = 0;
  for (int f = 0; f < F; ++f) {
    FramePlan& pl = plan[(size_t)f];
    pl.best_h = loop[(size_t)f].best_h;
    pl.slot = -1;
    pl.outb = nob; nob += 2LL * fd[(size_t)f].words;
    if (loop[(size_t)f].best >= kMaxFeatNum) { pl.slot = (int)slot_frame.size(); slot_frame.push_back(f); }
  }
  const int S = (int)slot_frame.size();
  if (S > 0) rc = ensure_batch(e, S, maxK);
  if (rc != SLSLAM_OK) return rc;
  const int B = S > 0 ? e->cap_frames : 0;
  std::vector<SlotDesc> slot((size_t)B);
  long long exp_total = 0;
  for (int i = 0; i < B; ++i) {
    SlotDesc& sd = slot[(size_t)i];
    sd.frame = i < S ? slot_frame[(size_t)i] : -1;
    sd.n = i < S ? loop[(size_t)sd.frame].best : 1;                   // (the score is the popcount of the winner's inlier bits)
    sd.best_h = i < S ? loop[(size_t)sd.frame].best_h : 0; sd.pad = 0;
    sd.exp_off = exp_total; exp_total += 12 + 4LL * sd.n;
    if (i < S) { e->slot_of_frame[(size_t)sd.frame] = i; e->n_of_frame[(size_t)sd.frame] = sd.n; e->exp_off_of_frame[(size_t)sd.frame] = sd.exp_off; }
  }
  // ---- the small tables (plans, slots) up, the result block [FrameOut F | bits] zeroed
  const size_t off_slots = align256(sizeof(FramePlan) * (size_t)F), small_bytes = off_slots + sizeof(SlotDesc) * (size_t)B;
  // (with covariance: [FrameOut F | bits | FrameCov F])
  const size_t off_bits = align256(sizeof(FrameOut) * (size_t)F), off_cov = align256(off_bits + 8 * (size_t)nob);
  const size_t out_bytes = with_cov ? off_cov + sizeof(FrameCov) * (size_t)F : off_bits + 8 * (size_t)nob;
  HIP_TRY(e->h_small.need(small_bytes, &e->ws.allocations));
  HIP_TRY(e->d_small.need(small_bytes, &e->ws.allocations));
  HIP_TRY(e->h_out.need(out_bytes, &e->ws.allocations));
  HIP_TRY(e->d_out.need(out_bytes, &e->ws.allocations));
  if (F > 0) std::memcpy(e->h_small.p, plan.data(), sizeof(FramePlan) * (size_t)F);
  if (B > 0) std::memcpy(e->h_small.p + off_slots, slot.data(), sizeof(SlotDesc) * (size_t)B);
  if (F > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_small.p, e->h_small.p, small_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(e->d_out.p, 0, out_bytes, s));
  }
  const FramePlan* d_plan = e->d_small.at<FramePlan>(0);
  const SlotDesc* d_slot = e->d_small.at<SlotDesc>(off_slots);

  // ---- pack, refill, solve, export
  const slslam::LMState* d_state = nullptr;
  const slslam::WinDesc* d_wins = nullptr;
  if (S > 0) {
    const size_t Lc = (size_t)e->cap_lines, nw = (size_t)B;
    const size_t o_obs = align256(4 * 2 * Lc * nw), o_par = o_obs + align256(8 * 16 * Lc * nw), win_bytes = o_par + 8 * (12 + 4 * Lc) * nw;
    HIP_TRY(e->d_win.need(win_bytes, &e->ws.allocations));
    HIP_TRY(e->d_export.need(8 * (size_t)exp_total, &e->ws.allocations));
    WinBufs wb{ e->d_win.at<unsigned>(0), e->d_win.at<double>(o_obs), e->d_win.at<double>(o_par), e->cap_lines };
    hipLaunchKernelGGL(k_frame_pack, dim3((unsigned)B), dim3(64), 0, s, d_slot, d_fd, d_dd, d_poses, d_bits, wb);
    HIP_TRY(hipGetLastError());
    std::vector<slslam_lba_window> wins((size_t)B);
    std::vector<const unsigned*> packed((size_t)B);
    for (int i = 0; i < B; ++i) {
      slslam_lba_window& w = wins[(size_t)i];
      const int n = slot[(size_t)i].n;
      w.num_cameras = 2; w.num_lines = n; w.num_observations = 2 * n;
      w.camera_index = nullptr; w.line_index = nullptr; w.fixed_index = nullptr;
      w.observations = wb.obs + (size_t)i * 16 * Lc;
      w.parameters = wb.par + (size_t)i * (12 + 4 * Lc);
      packed[(size_t)i] = wb.words + (size_t)i * 2 * Lc;
    }
    if ((rc = slslam::lba_refill_resident(e->batch, wins.data(), packed.data(), B, S, s)) != SLSLAM_OK) return rc;
    ++e->refills;
    if ((rc = slslam_lba_batch_solve(e->batch, s)) != SLSLAM_OK) return rc;
    if ((rc = slslam_lba_batch_export_device(e->batch, e->d_export.at<double>(0), s)) != SLSLAM_OK) return rc;
    if ((rc = slslam::lba_device_results(e->batch, &d_state, &d_wins)) != SLSLAM_OK) return rc;
    if (with_cov) {
      const int* d_hdr = nullptr;
      const double* d_cov = nullptr;
      int hdr_ints = 0;
      long long cam_stride = 0;
      long long cov_allocs[2] = { 0, 0 };
      (void)slslam_lba_batch_covariance_stats(e->batch, nullptr, &cov_allocs[0]);
      if ((rc = slslam_lba_batch_covariance(e->batch, s, /*with_lines=*/0)) != SLSLAM_OK) return rc;
      (void)slslam_lba_batch_covariance_stats(e->batch, nullptr, &cov_allocs[1]);
      e->ws.allocations += cov_allocs[1] - cov_allocs[0];             // (the batch's covariance buffers count as the estimator's)
      if ((rc = slslam::lba_device_covariance(e->batch, &d_hdr, &hdr_ints, &d_cov, &cam_stride)) != SLSLAM_OK) return rc;
      if (cam_stride < 36) return SLSLAM_ERR_UNSUPPORTED;
      hipLaunchKernelGGL(k_frame_covariance, dim3((unsigned)S), dim3(64), 0, s, d_slot, S, d_hdr, hdr_ints, d_cov, cam_stride,
                         e->d_export.at<const double>(0), d_state, d_wins, e->d_out.at<FrameCov>(off_cov));
      HIP_TRY(hipGetLastError());
    }
  }

  // ---- finish every frame in one launch, one download
  FrameOut* d_o = e->d_out.at<FrameOut>(0);
  if (F > 0 && maxW > 0)
    hipLaunchKernelGGL(k_frame_finish, dim3((unsigned)maxW, (unsigned)F), dim3(64), 0, s, d_fd, d_plan, d_slot, d_dd, d_poses, d_bits,
                       e->d_export.at<const double>(0), d_state, d_wins, baseline, error_thr, d_o, e->d_out.at<unsigned long long>(off_bits));
  HIP_TRY(hipGetLastError());
  if (F > 0) HIP_TRY(hipMemcpyAsync(e->h_out.p, e->d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int f = 0; f < F; ++f)
    if (plan[(size_t)f].slot >= 0 && !e->h_out.at<FrameOut>(0)[f].built) return SLSLAM_ERR_UNSUPPORTED;     // (the device build refused a window)

  // ---- the caller's results
  for (int f = 0; f < F; ++f) {
    const FrameDesc& d = fd[(size_t)f];
    const FrameOut& o = e->h_out.at<FrameOut>(0)[f];
    const TrialLoop& tl = loop[(size_t)f];
    slslam_pose_estimate& r = out[f];
    const int words_k = (frames[f].num_lines + 63) / 64;
    r.status = frames[f].num_lines < kMaxFeatNum ? SLSLAM_POSE_TOO_FEW_FEATURES : tl.best < kMaxFeatNum ? SLSLAM_POSE_RANSAC_FAILED : SLSLAM_POSE_OK;
    r.trial_cnt = tl.trial_cnt;
    r.ransac_score = tl.best;
    for (int q = 0; q < 12; ++q) r.ransac_pose[q] = tl.best_h >= 0 ? o.ransac_pose[q] : (q == 0 || q == 4 || q == 8 ? 1.0 : 0.0);
    const unsigned long long* ob = e->h_out.at<unsigned long long>(off_bits) + plan[(size_t)f].outb;
    if (r.ransac_inlier_bits)
      for (int w = 0; w < words_k; ++w) r.ransac_inlier_bits[w] = tl.best_h >= 0 && w < d.words ? ob[w] : 0ull;
    std::memset(&r.summary, 0, sizeof(r.summary));
    if (r.status == SLSLAM_POSE_OK) {
      r.summary.num_successful_steps = o.n_success; r.summary.num_unsuccessful_steps = o.n_unsuccess;
      r.summary.initial_cost = o.initial_cost; r.summary.final_cost = o.final_cost; r.summary.fixed_cost = o.fixed_cost;
      r.summary.termination_type = o.termination; r.summary.num_free_parameters = o.nfree; r.summary.num_residual_blocks = o.nkept;
      for (int q = 0; q < 12; ++q) r.pose[q] = o.pose[q];
      r.num_inliers = o.num_inliers;
    } else {
      for (int q = 0; q < 12; ++q) r.pose[q] = r.ransac_pose[q];
      r.num_inliers = 0;
    }
    if (r.inlier_bits)
      for (int w = 0; w < words_k; ++w) r.inlier_bits[w] = r.status == SLSLAM_POSE_OK ? ob[d.words + w] : 0ull;
  }
  e->last_cov = with_cov; e->off_cov = off_cov;
  return SLSLAM_OK;
}

extern "C" int slslam_pose_estimator_set_covariance(slslam_pose_estimator* e, int enable) {
  if (!e) return SLSLAM_ERR_INVALID_ARGUMENT;
  e->want_cov = enable != 0;
  return SLSLAM_OK;
}

extern "C" int slslam_pose_estimator_get_covariance(const slslam_pose_estimator* e, int frame, int* status, double constraint[6], double cov[36],
                                                    double* sigma2, int* dof) {
  if (!e || frame < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!e->last_cov) return SLSLAM_ERR_STATE;                                    // (no run yet, or the last one had covariance disabled or failed)
  if (frame >= (int)e->slot_of_frame.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (e->slot_of_frame[(size_t)frame] < 0) return SLSLAM_ERR_STATE;
  const FrameCov& c = e->h_out.at<FrameCov>(e->off_cov)[frame];
  if (status) *status = c.status;
  if (constraint) std::memcpy(constraint, c.constraint, sizeof(c.constraint));
  if (cov) std::memcpy(cov, c.cov, sizeof(c.cov));
  if (sigma2) *sigma2 = c.sigma2;
  if (dof) *dof = c.dof;
  return SLSLAM_OK;
}

extern "C" int slslam_pose_estimator_window(const slslam_pose_estimator* e, int frame, unsigned int* index_words, double* observations,
                                            double* parameters, double* solved_camera, int* num_lines) {
  if (!e || !num_lines || frame < 0 || frame >= (int)e->slot_of_frame.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int i = e->slot_of_frame[(size_t)frame];
  if (i < 0) return SLSLAM_ERR_STATE;
  const int n = e->n_of_frame[(size_t)frame];
  *num_lines = n;
  const size_t Lc = (size_t)e->cap_lines, nw = (size_t)e->cap_frames;
  const size_t o_obs = align256(4 * 2 * Lc * nw), o_par = o_obs + align256(8 * 16 * Lc * nw);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->ws.stream));
  if (index_words) HIP_TRY(hipMemcpy(index_words, e->d_win.at<unsigned>(0) + (size_t)i * 2 * Lc, 4 * 2 * (size_t)n, hipMemcpyDeviceToHost));
  if (observations) HIP_TRY(hipMemcpy(observations, e->d_win.at<double>(o_obs) + (size_t)i * 16 * Lc, 8 * 16 * (size_t)n, hipMemcpyDeviceToHost));
  if (parameters) HIP_TRY(hipMemcpy(parameters, e->d_win.at<double>(o_par) + (size_t)i * (12 + 4 * Lc), 8 * (12 + 4 * (size_t)n), hipMemcpyDeviceToHost));
  if (solved_camera) HIP_TRY(hipMemcpy(solved_camera, e->d_export.at<double>(0) + e->exp_off_of_frame[(size_t)frame], 8 * 6, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

// slslam_amd/csrc/frame_api.hip — the per-frame pose estimator (include/slslam_hip.h: slslam_pose_estimator_*).
//
// SLAM::pose_estimation (reference src/slam.cpp:244-319) after its merge by feature id, for many frames per call:
//   RANSAC      generate + score every frame's trials, one launch each (frame index in the grid; bodies of ransac_device.h),
//               one download of the scores, the adaptive trial loop on the host (ransac_loop.h), best_score starting at -1 (:283)
//   pack        k_frame_pack: one wave per solvable frame writes its motion-only window (:590-640) into device memory
//   solve       the estimator's refillable fused motion-only LBA batch, refilled from those device windows (lba_resident.h)
//   finish      k_frame_finish: gc_wt_to_Rt of the solved camera (:668-674) and the final inlier set under it (:305-312), with the
//               refined pose, the summaries and the RANSAC winners gathered into one result block - one download
// Two host round trips per call, whatever the number of frames.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "ransac_device.h"
#include "ransac_loop.h"
#include "gc_convert.h"
#include "index_word.h"
#include "lba_resident.h"

using namespace slslam_ransac;

namespace {

constexpr int kMaxFeatNum = 5;          // max_feat_num (reference src/parameter.h:25): the fewest common lines / RANSAC inliers accepted

// Per frame, where its inputs and RANSAC work lie (uploaded with the inputs)
struct FrameDesc {
  long long o0, o1, ln;                 // doubles: obs0 [8K], obs1 [8K], lines [6K]
  long long smp;                        // ints: samples [H s]
  long long hyp;                        // first hypothesis of the frame in poses [12] / valid / scores
  long long bits;                       // first 64-bit word of the frame's hypothesis inlier bits ([H words])
  long long outb;                       // first word of the frame's bits in the result block (RANSAC winner, then final set: 2 words each)
  int H, K, s, words;                   // trials scored (<= max_trials + 1), common lines, sample size, (K + 63) / 64
};
// Per frame, what the trial loop decided (uploaded after it)
struct FramePlan { int best_h, slot; };
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

// Window slot i lies at a fixed stride in the window buffers: words [2 Lcap], observations [16 Lcap], parameters [12 + 4 Lcap]
struct WinBufs { unsigned* words; double* obs; double* par; int cap_lines; };

__global__ __launch_bounds__(64) void k_frames_generate(const FrameDesc* __restrict__ fr, const double* __restrict__ dd,
                                                        const int* __restrict__ di, double baseline, double* poses, int* valid) {
  const FrameDesc fd = fr[blockIdx.y];
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= fd.H) return;
  valid[fd.hyp + h] = generate_trial(fd.s, di + fd.smp + (long long)h * fd.s, dd + fd.o0, dd + fd.o1, baseline, poses + 12 * (fd.hyp + h));
}

// k_ransac_score of every frame: blockIdx = (64-line block, hypothesis, frame)
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
    if (!valid[g] || pose_skipped(T)) {
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
  if (lane == 0) out_bits[fd.outb + blk] = bits[fd.bits + (long long)pl.best_h * fd.words + blk];
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
    out_bits[fd.outb + fd.words + blk] = m;
    atomicAdd(&o.num_inliers, __popcll(m));
  }
}

// A device buffer that only grows (its contents are not kept); every allocation is counted
struct DBuf {
  char* p = nullptr;
  size_t n = 0;
  ~DBuf() { if (p) (void)hipFree(p); }
  hipError_t need(size_t bytes, long long* allocs) {
    if (bytes <= n && p) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; n = 0; }
    const size_t want = std::max<size_t>(bytes + bytes / 8, 256);
    const hipError_t e = hipMalloc((void**)&p, want);
    if (e == hipSuccess) { n = want; ++*allocs; }
    return e;
  }
  template <typename T> T* at(size_t byte_off) const { return reinterpret_cast<T*>(p + byte_off); }
};
// ... and its page-locked host counterpart
struct HBuf {
  char* p = nullptr;
  size_t n = 0;
  ~HBuf() { if (p) (void)hipHostFree(p); }
  hipError_t need(size_t bytes, long long* allocs) {
    if (bytes <= n && p) return hipSuccess;
    if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
    const size_t want = std::max<size_t>(bytes + bytes / 8, 256);
    const hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
    if (e == hipSuccess) { n = want; ++*allocs; }
    return e;
  }
  template <typename T> T* at(size_t byte_off) const { return reinterpret_cast<T*>(p + byte_off); }
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct slslam_pose_estimator {
  int device = -1;
  slslam_solver_options opt;
  int cap_frames = 0, cap_lines = 0;               // what the batch and the window buffers hold
  slslam_lba_batch* batch = nullptr;
  hipStream_t stream = nullptr;
  DBuf d_in, d_work, d_win, d_export, d_small, d_out;
  HBuf h_in, h_small, h_out;
  long long calls = 0, allocations = 0, finalizes = 0, refills = 0;
  // the last call, for slslam_pose_estimator_window
  std::vector<int> slot_of_frame, n_of_frame;
  std::vector<long long> exp_off_of_frame;
  void drop_batch() { if (batch) { slslam_lba_batch_destroy(batch); batch = nullptr; } }
  ~slslam_pose_estimator() {
    drop_batch();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

#define FE_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { std::fprintf(stderr, "slslam: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    return (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? SLSLAM_ERR_NO_DEVICE : SLSLAM_ERR_HIP; } } while (0)

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
  if (allocations) *allocations = e->allocations;
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
  for (int f = 0; f < F; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    if (tr.num_trials < 0 || tr.num_lines < 0 || tr.num_lines > 0xfffe || tr.sample_size < 1 || tr.sample_size > 16) return SLSLAM_ERR_INVALID_ARGUMENT;
    const int H = tr.num_trials, K = tr.num_lines, s = tr.sample_size;
    if (H > 0 && K > 0 && (!tr.samples || !tr.observations0 || !tr.observations1 || !lines[f])) return SLSLAM_ERR_INVALID_ARGUMENT;
    for (long long i = 0; K > 0 && i < (long long)H * s; ++i)
      if (tr.samples[i] < 0 || tr.samples[i] >= K) return SLSLAM_ERR_INVALID_ARGUMENT;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (e->device >= 0) FE_TRY(hipSetDevice(e->device));
  else FE_TRY(hipGetDevice(&e->device));
  if (!e->stream) FE_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  hipStream_t s = e->stream;
  ++e->calls;
  e->slot_of_frame.assign((size_t)F, -1); e->n_of_frame.assign((size_t)F, 0); e->exp_off_of_frame.assign((size_t)F, 0);

  // ---- layout of the inputs: one block [FrameDesc F | doubles | ints], one upload
  // (a frame with fewer than 5 common lines runs nothing (:275); of the others only the trials the loop can reach are scored)
  std::vector<FrameDesc> fd((size_t)F);
  long long nd = 0, ni = 0, nh = 0, nb = 0, nob = 0;
  int maxH = 0, maxW = 0, maxK = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    FrameDesc& d = fd[(size_t)f];
    const int K = tr.num_lines;
    const bool runs = K >= kMaxFeatNum;
    d.K = runs ? K : 0; d.s = tr.sample_size; d.words = (d.K + 63) / 64;
    d.H = runs ? std::max(0, (int)std::min<long long>(tr.num_trials, (long long)max_trials + 1)) : 0;
    d.o0 = nd; nd += 8LL * d.K; d.o1 = nd; nd += 8LL * d.K; d.ln = nd; nd += 6LL * d.K;
    d.smp = ni; ni += (long long)d.H * d.s;
    d.hyp = nh; nh += d.H;
    d.bits = nb; nb += (long long)d.H * d.words;
    d.outb = nob; nob += 2LL * d.words;
    maxH = std::max(maxH, d.H); maxW = std::max(maxW, d.words); maxK = std::max(maxK, d.K);
  }
  const size_t off_d = align256(sizeof(FrameDesc) * (size_t)F), off_i = off_d + align256(8 * (size_t)nd), in_bytes = off_i + 4 * (size_t)ni;
  const size_t w_poses = 0, w_bits = align256(96 * (size_t)nh), w_valid = w_bits + align256(8 * (size_t)nb), w_scores = w_valid + align256(4 * (size_t)nh),
               work_bytes = w_scores + 4 * (size_t)nh;
  FE_TRY(e->h_in.need(in_bytes, &e->allocations));
  FE_TRY(e->d_in.need(in_bytes, &e->allocations));
  FE_TRY(e->d_work.need(work_bytes, &e->allocations));
  if (F > 0) std::memcpy(e->h_in.p, fd.data(), sizeof(FrameDesc) * (size_t)F);
  for (int f = 0; f < F; ++f) {
    const slslam_ransac_trials& tr = frames[f];
    const FrameDesc& d = fd[(size_t)f];
    if (d.K > 0 && d.H > 0) {
      std::memcpy(e->h_in.at<double>(off_d) + d.o0, tr.observations0, 64 * (size_t)d.K);
      std::memcpy(e->h_in.at<double>(off_d) + d.o1, tr.observations1, 64 * (size_t)d.K);
      std::memcpy(e->h_in.at<double>(off_d) + d.ln, lines[f], 48 * (size_t)d.K);
      std::memcpy(e->h_in.at<int>(off_i) + d.smp, tr.samples, 4 * (size_t)d.H * d.s);
    }
  }
  const FrameDesc* d_fd = e->d_in.at<FrameDesc>(0);
  const double* d_dd = e->d_in.at<double>(off_d);
  const int* d_di = e->d_in.at<int>(off_i);
  double* d_poses = e->d_work.at<double>(w_poses);
  unsigned long long* d_bits = e->d_work.at<unsigned long long>(w_bits);
  int* d_valid = e->d_work.at<int>(w_valid);
  int* d_scores = e->d_work.at<int>(w_scores);

  // ---- RANSAC of every frame: two launches, one download of the scores
  std::vector<int> scores((size_t)std::max<long long>(nh, 1), 0);
  if (F > 0) FE_TRY(hipMemcpyAsync(e->d_in.p, e->h_in.p, in_bytes, hipMemcpyHostToDevice, s));
  if (nh > 0) {
    FE_TRY(hipMemsetAsync(d_scores, 0, 4 * (size_t)nh, s));
    // the reference passes -baseline to the generator (slam.cpp:391-392)
    hipLaunchKernelGGL(k_frames_generate, dim3((unsigned)((maxH + 63) / 64), (unsigned)F), dim3(64), 0, s, d_fd, d_dd, d_di, -baseline, d_poses, d_valid);
    hipLaunchKernelGGL(k_frames_score, dim3((unsigned)maxW, (unsigned)std::min(maxH, 65535), (unsigned)F), dim3(64), 0, s, d_fd, d_dd, (const double*)d_poses,
                       (const int*)d_valid, baseline, error_thr, d_scores, d_bits);
    FE_TRY(hipGetLastError());
    FE_TRY(hipMemcpyAsync(scores.data(), d_scores, 4 * (size_t)nh, hipMemcpyDeviceToHost, s));
    FE_TRY(hipStreamSynchronize(s));
  }

  // ---- the trial loops (best_score = -1, slam.cpp:283), statuses, the solvable frames' slots
  std::vector<FramePlan> plan((size_t)F);
  std::vector<TrialLoop> loop((size_t)F);
  std::vector<int> slot_frame;
  for (int f = 0; f < F; ++f) {
    const FrameDesc& d = fd[(size_t)f];
    loop[(size_t)f] = d.K > 0 ? run_trial_loop(scores.data() + d.hyp, d.H, d.K, d.s, prob_free_outliers, max_trials, -1) : TrialLoop{ -1, -1, 0 };
    plan[(size_t)f].best_h = loop[(size_t)f].best_h;
    plan[(size_t)f].slot = -1;
    if (d.K > 0 && loop[(size_t)f].best >= kMaxFeatNum) { plan[(size_t)f].slot = (int)slot_frame.size(); slot_frame.push_back(f); }
  }
  const int S = (int)slot_frame.size();
  int rc = SLSLAM_OK;
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
  const size_t off_bits = align256(sizeof(FrameOut) * (size_t)F), out_bytes = off_bits + 8 * (size_t)nob;
  FE_TRY(e->h_small.need(small_bytes, &e->allocations));
  FE_TRY(e->d_small.need(small_bytes, &e->allocations));
  FE_TRY(e->h_out.need(out_bytes, &e->allocations));
  FE_TRY(e->d_out.need(out_bytes, &e->allocations));
  if (F > 0) std::memcpy(e->h_small.p, plan.data(), sizeof(FramePlan) * (size_t)F);
  if (B > 0) std::memcpy(e->h_small.p + off_slots, slot.data(), sizeof(SlotDesc) * (size_t)B);
  if (F > 0) {
    FE_TRY(hipMemcpyAsync(e->d_small.p, e->h_small.p, small_bytes, hipMemcpyHostToDevice, s));
    FE_TRY(hipMemsetAsync(e->d_out.p, 0, out_bytes, s));
  }
  const FramePlan* d_plan = e->d_small.at<FramePlan>(0);
  const SlotDesc* d_slot = e->d_small.at<SlotDesc>(off_slots);

  // ---- pack, refill, solve, export
  const slslam::LMState* d_state = nullptr;
  const slslam::WinDesc* d_wins = nullptr;
  if (S > 0) {
    const size_t Lc = (size_t)e->cap_lines, nw = (size_t)B;
    const size_t o_obs = align256(4 * 2 * Lc * nw), o_par = o_obs + align256(8 * 16 * Lc * nw), win_bytes = o_par + 8 * (12 + 4 * Lc) * nw;
    FE_TRY(e->d_win.need(win_bytes, &e->allocations));
    FE_TRY(e->d_export.need(8 * (size_t)exp_total, &e->allocations));
    WinBufs wb{ e->d_win.at<unsigned>(0), e->d_win.at<double>(o_obs), e->d_win.at<double>(o_par), e->cap_lines };
    hipLaunchKernelGGL(k_frame_pack, dim3((unsigned)B), dim3(64), 0, s, d_slot, d_fd, d_dd, (const double*)d_poses, (const unsigned long long*)d_bits, wb);
    FE_TRY(hipGetLastError());
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
  }

  // ---- finish every frame in one launch, one download
  FrameOut* d_o = e->d_out.at<FrameOut>(0);
  if (F > 0 && maxW > 0)
    hipLaunchKernelGGL(k_frame_finish, dim3((unsigned)maxW, (unsigned)F), dim3(64), 0, s, d_fd, d_plan, d_slot, d_dd, (const double*)d_poses,
                       (const unsigned long long*)d_bits, (const double*)e->d_export.at<double>(0), d_state, d_wins, baseline, error_thr, d_o,
                       e->d_out.at<unsigned long long>(off_bits));
  FE_TRY(hipGetLastError());
  if (F > 0) FE_TRY(hipMemcpyAsync(e->h_out.p, e->d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
  FE_TRY(hipStreamSynchronize(s));
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
    const unsigned long long* ob = e->h_out.at<unsigned long long>(off_bits) + d.outb;
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
  FE_TRY(hipSetDevice(e->device));
  FE_TRY(hipStreamSynchronize(e->stream));
  if (index_words) FE_TRY(hipMemcpy(index_words, e->d_win.at<unsigned>(0) + (size_t)i * 2 * Lc, 4 * 2 * (size_t)n, hipMemcpyDeviceToHost));
  if (observations) FE_TRY(hipMemcpy(observations, e->d_win.at<double>(o_obs) + (size_t)i * 16 * Lc, 8 * 16 * (size_t)n, hipMemcpyDeviceToHost));
  if (parameters) FE_TRY(hipMemcpy(parameters, e->d_win.at<double>(o_par) + (size_t)i * (12 + 4 * Lc), 8 * (12 + 4 * (size_t)n), hipMemcpyDeviceToHost));
  if (solved_camera) FE_TRY(hipMemcpy(solved_camera, e->d_export.at<double>(0) + e->exp_off_of_frame[(size_t)frame], 8 * 6, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

// slslam_amd/csrc/ransac_front.h — what ransac_api.hip lends the pose estimator (frame_api.hip): the batched RANSAC front every
// entry point runs through.  One validator, one layout with one upload, one kernel pair (frame index in the grid), one download of
// the scores and the adaptive trial loop per frame (ransac_loop.h).  Internal: not part of the C ABI.
#ifndef SLSLAM_RANSAC_FRONT_H_
#define SLSLAM_RANSAC_FRONT_H_

#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/slslam_hip.h"
#include "grow_buf.h"
#include "ransac_loop.h"

namespace slslam_ransac {

// Per frame, where its inputs and RANSAC work lie (uploaded with the inputs).  A frame that runs nothing has H = K = words = 0.
struct FrameDesc {
  long long o0, o1, ln;                 // doubles: obs0 [8K], obs1 [8K], lines [6K]
  long long smp;                        // ints: samples [H s]
  long long hyp;                        // first hypothesis of the frame in poses [12] / valid / scores
  long long bits;                       // first 64-bit word of the frame's hypothesis inlier bits ([H words])
  int H, K, s, words;                   // trials scored (<= max_trials + 1), common lines, sample size, (K + 63) / 64
};

// The buffers of a front call and the stream it runs on.  The pose estimator keeps one (page-locked staging, its own stream); a
// stateless entry point makes one that lives for the call (plain host staging, the null stream).  Plain host staging relies on
// hipMemcpyAsync reading unpinned memory before it returns or, at the latest, before the stream's next synchronise: a caller
// synchronises the stream before its workspace dies.
struct Workspace {
  slslam::GrowBuf d_in{slslam::Mem::kDevice}, d_work{slslam::Mem::kDevice}, h_in;
  hipStream_t stream = nullptr;
  long long allocations = 0;
  explicit Workspace(slslam::Mem host) : h_in(host) {}
};

// What a front call hands back: the layout, the device arrays it describes (valid until the workspace's next call) and, from
// front_ransac, every frame's scores and trial loop.
struct Front {
  std::vector<FrameDesc> fd;            // [F]
  const FrameDesc* d_fd = nullptr;
  const double* d_dd = nullptr;         // the doubles FrameDesc's o0 / o1 / ln index
  const int* d_di = nullptr;            // the ints FrameDesc's smp indexes
  double* d_poses = nullptr;            // [12 nh], indexed by hyp
  unsigned long long* d_bits = nullptr;
  int *d_valid = nullptr, *d_scores = nullptr;
  long long nh = 0;                     // hypotheses of all frames
  int maxH = 0, maxW = 0, maxK = 0;
  std::vector<int> scores;              // [nh]
  std::vector<TrialLoop> loop;          // [F]
};

// True when every frame's sizes, pointers and sample indices can be run.  scored: the trials are scored against lines[f] (a frame
// without trials or without common lines runs nothing, whatever its arrays hold); otherwise they are only generated (lines is not
// read, and trials need common lines to draw from).  Touches neither an output nor the device.
bool trials_valid(int F, const slslam_ransac_trials* frames, const double* const* lines, bool scored);

// SLAM::ransac_motion of every frame up to the winners' gather: layout, one upload, generate (with -baseline, as the reference calls
// it), score, one download of the scores, the trial loops.  Of each frame at most max_trials + 1 trials are run: the trial loop
// reads no further.  best_in[f] = the best score frame f starts from (nullptr: -1 each).  The frames must be trials_valid.
int front_ransac(Workspace& ws, int F, const slslam_ransac_trials* frames, const double* const* lines, double baseline, double thr,
                 double prob_free_outliers, int max_trials, const int* best_in, Front* fr);

}  // namespace slslam_ransac

#endif  // SLSLAM_RANSAC_FRONT_H_

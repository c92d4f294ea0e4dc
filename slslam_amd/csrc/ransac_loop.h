// slslam_amd/csrc/ransac_loop.h — the adaptive trial loop of SLAM::ransac_motion (reference src/slam.cpp:363, :415-423), replayed
// on the host in trial order over scores the device computed for every pre-drawn trial.  Called from one place, the RANSAC front
// (ransac_front.h, ransac_api.hip) that every entry point and the pose estimator run through.  It stays on the host: its pow / log feed an int truncation, and device libm
// does not promise the host's last bit.
#ifndef SLSLAM_RANSAC_LOOP_H_
#define SLSLAM_RANSAC_LOOP_H_

#include <algorithm>
#include <cmath>

namespace slslam_ransac {

struct TrialLoop {
  int best;        // best score (the incoming one when no trial beat it)
  int best_h;      // the trial that set it, or -1
  int trial_cnt;   // trials executed
};

// scores[H] of the trials in draw order, K common lines, s samples per trial; best_in = the running best the caller starts from
inline TrialLoop run_trial_loop(const int* scores, int H, int K, int s, double prob_free_outliers, int max_trials, int best_in) {
  int best = best_in, best_h = -1, ransac_trial = K, t = 0;
  for (; t < ransac_trial && t <= max_trials && t < H; ++t) {
    if (scores[t] > best) {
      best = scores[t]; best_h = t;
      const double prob_s_outliers = 1 - std::pow(best / (double)K, s);
      ransac_trial = (int)(std::log(1 - prob_free_outliers) / std::log(std::min(1 - 1e-6, std::max(1e-6, prob_s_outliers))));
    }
  }
  return TrialLoop{ best, best_h, t };
}

}  // namespace slslam_ransac

#endif  // SLSLAM_RANSAC_LOOP_H_

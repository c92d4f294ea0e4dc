// slslam_amd/host/place_filter.h — the Bayes filter over "which keyframe am I at, or none" and the loop decision on its posterior:
// the host half of the place recogniser (include/slslam_hip.h: slslam_place_filter_*; the device half is csrc/place_recognition.h).
// Mirrors voctree_t::trans_prob / calc_post_prob / isLoopClosing of the reference's src/voctree_bf.h.  O(21 N) per step, serial from
// frame to frame, plain C++: needs no device and no HIP header.
//
// States: -1 ("no place") and the visible documents 0 .. N-1; arrays hold state s at index s + 1.
//   trans(s, j), the float the reference returns for "from j to s":
//     j = -1:  0.9f to -1, 0.1f / (float)N to a document;
//     j >= 0:  0.1f to -1, (float)gauss[|s - j|] to a document with |s - j| < 10, else 0;
//     gauss[d] = 1 / sqrt(2 pi sigma^2) * exp(-d^2 / (2 sigma^2)) in double.
//   post[s] = likelihood[s] * sum_{j = -1}^{N - 1} trans(s, j) * prev[j]: j ascending, a float sum of float products; a prev[j] the last
//     step did not have (the visible set has grown) counts as 0.  Terms whose trans is 0 add nothing and are skipped: 21 terms at most
//     for a document.  Normalised by the double sum of the float products post[s]; when that sum is 0, uniform 1 / (N + 1).
//   Before the first update all mass is on -1.
// Decision (isLoopClosing without its dead branches): false while N < min_docs; else the lowest a with a + seq_len <= N - 1 and
//   sum_{d = a}^{a + seq_len} post[d] >= (float)threshold (a float sum, d ascending) closes a loop and reports the argmax document of that
//   window, the lowest on ties.
// The reference's presets (recent, sigma, threshold, seq_len; min_docs = recent): indoor 40, 1.0, 0.7, 10; outdoor 100, 0.8, 0.8, 15;
// outdoor long-loop 300, 0.8, 0.5, 5.
#ifndef SLSLAM_PLACE_FILTER_H_
#define SLSLAM_PLACE_FILTER_H_

#include <vector>

namespace slslam {

class PlaceFilter {
 public:
  PlaceFilter(double sigma, double threshold, int seq_len, int min_docs);
  // likelihood[N + 1].  Returns whether a loop closes; *keyframe = the reported document, or -1.
  bool update(int num_docs, const float* likelihood, int* keyframe);
  const std::vector<float>& posterior() const { return post_; }   // [N + 1] of the last update ([1] = {1} before the first)

 private:
  float gauss_[10];
  float threshold_;
  int seq_len_, min_docs_;
  std::vector<float> post_, prev_;
};

}  // namespace slslam

#endif  // SLSLAM_PLACE_FILTER_H_

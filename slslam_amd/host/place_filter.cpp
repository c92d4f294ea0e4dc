// slslam_amd/host/place_filter.cpp — see place_filter.h.  Every sum here has a stated order and a stated precision: no contraction.
#include "place_filter.h"

#include <cmath>
#include <new>

#include "../../include/slslam_hip.h"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF      // (hipcc contracts across statements by default; g++ does not contract for a baseline x86-64)
#endif

namespace slslam {

PlaceFilter::PlaceFilter(double sigma, double threshold, int seq_len, int min_docs)
    : threshold_((float)threshold), seq_len_(seq_len), min_docs_(min_docs), post_(1, 1.0f) {
  const double pi = 3.1415926535897932384626433832795;
  for (int d = 0; d < 10; ++d)
    gauss_[d] = (float)(1.0 / std::sqrt(2.0 * pi * sigma * sigma) * std::exp(-1.0 * ((double)(d * d) / (2.0 * sigma * sigma))));
}

bool PlaceFilter::update(int num_docs, const float* likelihood, int* keyframe) {
  const int N = num_docs;
  prev_.swap(post_);
  const int P = (int)prev_.size() - 1;                       // documents the last posterior has
  post_.assign((size_t)N + 1, 0.0f);
  const float* prev = prev_.data() + 1;                      // prev[j], j = -1 .. P - 1
  float* post = post_.data() + 1;
  const float to_doc = N > 0 ? 0.1f / (float)N : 0.0f;
  double eta = 0.0;
  {
    float belief = 0.0f;
    float t = 0.9f * prev[-1];
    belief = belief + t;
    for (int j = 0; j < N && j < P; ++j) {
      t = 0.1f * prev[j];
      belief = belief + t;
    }
    post[-1] = likelihood[0] * belief;
    eta += post[-1];
  }
  for (int s = 0; s < N; ++s) {
    float belief = 0.0f;
    float t = to_doc * prev[-1];
    belief = belief + t;
    const int j1 = s + 9 < P - 1 ? s + 9 : P - 1;
    for (int j = s - 9 > 0 ? s - 9 : 0; j <= j1; ++j) {
      t = gauss_[j > s ? j - s : s - j] * prev[j];
      belief = belief + t;
    }
    post[s] = likelihood[s + 1] * belief;
    eta += post[s];
  }
  for (int s = -1; s < N; ++s) post[s] = eta != 0.0 ? (float)(post[s] / eta) : 1.0f / (float)(N + 1);

  if (keyframe) *keyframe = -1;
  if (N < min_docs_) return false;
  for (int a = 0; a + seq_len_ <= N - 1; ++a) {
    float sum = 0.0f, best = post[a];
    int arg = a;
    for (int d = a; d <= a + seq_len_; ++d) {
      sum = sum + post[d];
      if (post[d] > best) { best = post[d]; arg = d; }
    }
    if (sum >= threshold_) {
      if (keyframe) *keyframe = arg;
      return true;
    }
  }
  return false;
}

}  // namespace slslam

struct slslam_place_filter {
  slslam::PlaceFilter f;
  slslam_place_filter(double sigma, double threshold, int seq_len, int min_docs) : f(sigma, threshold, seq_len, min_docs) {}
};

extern "C" int slslam_place_filter_create(double sigma, double threshold, int seq_len, int min_docs, slslam_place_filter** out) {
  if (!out || !(sigma > 0.0) || !std::isfinite(sigma) || std::isnan(threshold) || seq_len < 0 || min_docs < 0)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_place_filter* p = new (std::nothrow) slslam_place_filter(sigma, threshold, seq_len, min_docs);
  if (!p) return SLSLAM_ERR_NO_MEMORY;
  *out = p;
  return SLSLAM_OK;
}

extern "C" void slslam_place_filter_destroy(slslam_place_filter* filter) { delete filter; }

extern "C" int slslam_place_filter_update(slslam_place_filter* filter, int num_docs, const float* likelihood, float* posterior, int* loop,
                                          int* keyframe) {
  if (!filter || num_docs < 0 || !likelihood) return SLSLAM_ERR_INVALID_ARGUMENT;
  int kf = -1;
  bool lc = false;
  try {
    lc = filter->f.update(num_docs, likelihood, &kf);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  if (posterior)
    for (int i = 0; i <= num_docs; ++i) posterior[i] = filter->f.posterior()[(size_t)i];
  if (loop) *loop = lc ? 1 : 0;
  if (keyframe) *keyframe = kf;
  return SLSLAM_OK;
}

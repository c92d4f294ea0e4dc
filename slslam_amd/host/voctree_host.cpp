// slslam_amd/host/voctree_host.cpp — see voctree_host.h.  Also the three entry points of the trainer that need no device:
// slslam_voctree_centres, slslam_voctree_key, slslam_voctree_save.
#include "voctree_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/slslam_hip.h"

#pragma STDC FP_CONTRACT OFF

namespace slslam_voctree_host {

unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

unsigned long long key(unsigned long long seed, unsigned long long m) { return splitmix64(seed ^ splitmix64(m)); }

long long quantise(float f) { return std::llrint((double)f * 1073741824.0); }

bool values_valid(const float* f, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!(std::fabs(f[i]) <= 16.0f)) return false;                 // (a NaN fails the comparison, an infinity exceeds 16)
  return true;
}

void centres(size_t rows, int D, const long long* acc, const float* prev, float* out) {
  for (size_t r = 0; r < rows; ++r) {
    const long long* a = acc + r * (size_t)D;
    double n2 = 0.0;
    for (int i = 0; i < D; ++i) {
      const double s = (double)a[i];
      const double p = s * s;
      n2 = n2 + p;
    }
    float* o = out + r * (size_t)D;
    if (n2 == 0.0) {
      if (o != prev + r * (size_t)D) std::memcpy(o, prev + r * (size_t)D, sizeof(float) * (size_t)D);
      continue;
    }
    const double norm = std::sqrt(n2);
    for (int i = 0; i < D; ++i) o[i] = (float)((double)a[i] / norm);
  }
}

void partition(size_t n, const int* node, size_t num_nodes, int* perm, long long* start) {
  std::fill(start, start + num_nodes + 1, 0LL);
  for (size_t m = 0; m < n; ++m) ++start[(size_t)node[m] + 1];
  for (size_t j = 0; j < num_nodes; ++j) start[j + 1] += start[j];
  std::vector<long long> at(start, start + num_nodes);
  for (size_t m = 0; m < n; ++m) perm[at[(size_t)node[m]]++] = (int)m;
}

void initial_centres(int K, int D, size_t num_nodes, const long long* start, const int* perm, const unsigned long long* keys,
                     const float* desc, const float* parent, float* out) {
  const size_t KD = (size_t)K * (size_t)D;
  std::vector<std::pair<unsigned long long, int>> cand;
  std::vector<long long> acc((size_t)D);
  std::vector<float> zero((size_t)D, 0.0f);
  for (size_t j = 0; j < num_nodes; ++j) {
    float* o = out + j * KD;
    const size_t members = (size_t)(start[j + 1] - start[j]);
    if (members == 0) {
      for (int c = 0; c < K; ++c) std::memcpy(o + (size_t)c * D, parent + j * (size_t)D, sizeof(float) * (size_t)D);
      continue;
    }
    cand.clear();
    for (long long p = start[j]; p < start[j + 1]; ++p) cand.emplace_back(keys[perm[p]], perm[p]);
    const size_t picks = std::min(members, (size_t)K);
    std::partial_sort(cand.begin(), cand.begin() + (long)picks, cand.end());             // by (key, m)
    for (size_t c = 0; c < picks; ++c) {
      const float* f = desc + (size_t)cand[c].second * (size_t)D;
      for (int i = 0; i < D; ++i) acc[(size_t)i] = quantise(f[i]);
      centres(1, D, acc.data(), zero.data(), o + c * (size_t)D);
    }
    for (size_t c = picks; c < (size_t)K; ++c) std::memcpy(o + c * (size_t)D, o, sizeof(float) * (size_t)D);
  }
}

}  // namespace slslam_voctree_host

extern "C" int slslam_voctree_centres(long long rows, int D, const long long* acc, const float* prev, float* out) {
  if (rows < 0 || D < 1 || D > SLSLAM_PLACE_MAX_D || (rows > 0 && (!acc || !prev || !out))) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_voctree_host::centres((size_t)rows, D, acc, prev, out);
  return SLSLAM_OK;
}

extern "C" unsigned long long slslam_voctree_key(unsigned long long seed, unsigned long long m) {
  return slslam_voctree_host::key(seed, m);
}

extern "C" int slslam_voctree_save(const char* path, int K, int L, int D, const float* nodes) {
  if (!path || !nodes || K < 2 || K > SLSLAM_PLACE_MAX_K || L < 1 || L > SLSLAM_PLACE_MAX_L || D < 1 || D > SLSLAM_PLACE_MAX_D)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  size_t num_int = 0, level = 1;
  for (int l = 0; l < L; ++l) { num_int += level; level *= (size_t)K; }
  if (level > ((size_t)1 << 24)) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::FILE* fp = std::fopen(path, "wb");
  if (!fp) return SLSLAM_ERR_INVALID_ARGUMENT;
  const size_t want = num_int * (size_t)K * (size_t)D;
  const bool ok = std::fwrite(nodes, sizeof(float), want, fp) == want;
  return (std::fclose(fp) == 0 && ok) ? SLSLAM_OK : SLSLAM_ERR_INVALID_ARGUMENT;
}

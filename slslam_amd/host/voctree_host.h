// slslam_amd/host/voctree_host.h — the host half of the vocabulary-tree trainer (include/slslam_hip.h: slslam_voctree_train; DESIGN.md
// 6.5): the fixed point, the keys, centre(acc, prev), the stable partition of the descriptors by node and the initial centres of a
// level.  Plain C++, no device: IEEE sqrt and division here are what numpy computes, which keeps the trees bit-identical to the
// contract in numpy.  The assignment and the sums are the device's (csrc/voctree_train.h).
#ifndef SLSLAM_VOCTREE_HOST_H_
#define SLSLAM_VOCTREE_HOST_H_

#include <cstddef>

namespace slslam_voctree_host {

unsigned long long splitmix64(unsigned long long x);
unsigned long long key(unsigned long long seed, unsigned long long m);
long long quantise(float f);                                       // q(f) = llrint((double)f * 2^30)
// every value finite and |f| <= 16
bool values_valid(const float* f, size_t count);
// out (may be prev) [rows][D] = centre(acc [rows][D], prev [rows][D])
void centres(size_t rows, int D, const long long* acc, const float* prev, float* out);
// stable counting sort of 0 .. n-1 by node: perm [n] (members of a node ascending), start [num_nodes + 1]
void partition(size_t n, const int* node, size_t num_nodes, int* perm, long long* start);
// the initial centres out [num_nodes][K][D] of a level; parent: the centres of the level above as rows [num_nodes][D] (NULL at the root)
void initial_centres(int K, int D, size_t num_nodes, const long long* start, const int* perm, const unsigned long long* keys,
                     const float* desc, const float* parent, float* out);

}  // namespace slslam_voctree_host

#endif  // SLSLAM_VOCTREE_HOST_H_

// slslam_amd/csrc/voctree_train_api.hip — slslam_voctree_train and its test hook slslam_debug_voctree_step (include/slslam_hip.h; DESIGN.md
// 6.5).  The descriptors go up once.  Per level the host (host/voctree_host.h) partitions the descriptors by node, picks the initial
// centres and uploads permutation, nodes and centres; per update the device assigns and accumulates (k_voctree_step, voctree_train.h),
// `changed` comes back, then the level's accumulators, the host makes the centres (IEEE sqrt and division, as the contract wants) and
// uploads them.  A level ends with the download of labels, member counts and the blocks' distortion sums.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "../host/voctree_host.h"
#include "call_block.h"
#include "voctree_train.h"

using namespace slslam_vtrain;
namespace vh = slslam_voctree_host;
using slslam::GrowBuf;
using slslam::Mem;

namespace {

constexpr long long kMaxDescriptors = 1LL << 24, kMaxAccValues = 1LL << 27;

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// a failed allocation is the caller's out-of-memory status, any other HIP error the usual one
#define HIP_TRY_MEM(expr)                                                                    \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e == hipErrorOutOfMemory) { (void)hipGetLastError(); return SLSLAM_ERR_NO_MEMORY; }  \
    if (_e != hipSuccess) return slslam::hip_status(_e, #expr, __FILE__, __LINE__);          \
  } while (0)

bool shape_valid(int K, int D) {
  return K >= 2 && K <= slslam_place::kMaxK && D >= 1 && D <= slslam_place::kMaxD;
}

// the device block of a level of at most `rows` accumulator rows over n descriptors, and its page-locked mirror
struct Layout {
  size_t o_desc = 0, o_node = 0, o_label = 0, o_perm = 0, o_centres = 0, o_acc = 0, o_count = 0, o_changed = 0, o_partial = 0, bytes = 0;
};

Layout layout(size_t n, size_t D, size_t centre_floats, size_t rows) {
  Layout y;
  slslam::Carve c;
  y.o_desc = c.take(4 * n * D);
  y.o_node = c.take(4 * n);
  y.o_label = c.take(4 * n);
  y.o_perm = c.take(4 * n);
  y.o_centres = c.take(4 * centre_floats);
  y.o_acc = c.take(8 * rows * D);
  y.o_count = c.take(8 * rows);                                       // (changed follows count: one memset clears both)
  y.o_changed = c.take(256);
  y.o_partial = c.take(8 * (size_t)step_blocks((long long)n));
  y.bytes = c.at;
  return y;
}

struct Session {
  int K = 0, D = 0;
  size_t n = 0;
  Layout y;
  GrowBuf dev{Mem::kDevice}, pin{Mem::kPinned};                       // (the mirror holds node .. partial, not the descriptors)
  hipStream_t stream = nullptr;
  ~Session() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  template <typename T> T* d(size_t off) const { return reinterpret_cast<T*>(dev.p + off); }
  template <typename T> T* h(size_t off) const { return reinterpret_cast<T*>(pin.p + (off - y.o_node)); }
};

int open_session(Session* s, int device, int K, int D, size_t n, const float* desc, size_t centre_floats, size_t rows) {
  if (!slslam::device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  s->K = K; s->D = D; s->n = n;
  s->y = layout(n, (size_t)D, centre_floats, rows);
  long long unused = 0;
  HIP_TRY_MEM(s->dev.need(s->y.bytes, &unused));
  HIP_TRY_MEM(s->pin.need(s->y.bytes - s->y.o_node, &unused));
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_TRY(hipFuncSetAttribute((const void*)k_voctree_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)step_lds_bytes(K, D)));
  HIP_TRY(hipMemcpyAsync(s->d<float>(s->y.o_desc), desc, 4 * n * (size_t)D, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return SLSLAM_OK;
}

// node and perm of the level are in the mirror: up they go
int upload_partition(const Session& s) {
  HIP_TRY(hipMemcpyAsync(s.d<int>(s.y.o_node), s.h<int>(s.y.o_node), 4 * s.n, hipMemcpyHostToDevice, s.stream));
  HIP_TRY(hipMemcpyAsync(s.d<int>(s.y.o_perm), s.h<int>(s.y.o_perm), 4 * s.n, hipMemcpyHostToDevice, s.stream));
  return SLSLAM_OK;
}

// one assignment (and accumulation) of a level of `rows` accumulator rows; *changed comes back
int launch_step(const Session& s, const float* d_centres, size_t rows, bool accumulate, unsigned* changed) {
  const Layout& y = s.y;
  if (accumulate) HIP_TRY(hipMemsetAsync(s.dev.p + y.o_acc, 0, 8 * rows * (size_t)s.D, s.stream));
  HIP_TRY(hipMemsetAsync(s.dev.p + y.o_count, 0, y.o_changed + 256 - y.o_count, s.stream));
  Step a;
  a.K = s.K; a.D = s.D; a.n = (long long)s.n;
  a.centres = d_centres;
  a.desc = s.d<float>(y.o_desc);
  a.perm = s.d<int>(y.o_perm);
  a.node = s.d<int>(y.o_node);
  a.label = s.d<int>(y.o_label);
  a.acc = s.d<unsigned long long>(y.o_acc);
  a.count = s.d<unsigned long long>(y.o_count);
  a.changed = s.d<unsigned>(y.o_changed);
  a.partial = s.d<double>(y.o_partial);
  a.accumulate = accumulate ? 1 : 0;
  hipLaunchKernelGGL(k_voctree_step, dim3(step_blocks(a.n)), dim3(kStepThreads), step_lds_bytes(s.K, s.D), s.stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s.h<unsigned>(y.o_changed), a.changed, 4, hipMemcpyDeviceToHost, s.stream));
  HIP_TRY(hipStreamSynchronize(s.stream));
  *changed = *s.h<unsigned>(y.o_changed);
  return SLSLAM_OK;
}

int train(int device, const slslam_voctree_train_options& o, size_t n, const float* desc, size_t num_int, float* nodes, int* words,
          slslam_voctree_train_report* rep) {
  const int K = o.K, L = o.L, D = o.D;
  const size_t KD = (size_t)K * (size_t)D;
  size_t last_nodes = 1;
  for (int l = 1; l < L; ++l) last_nodes *= (size_t)K;
  std::vector<unsigned long long> keys(n);
  std::vector<long long> start(last_nodes + 1);
  for (size_t m = 0; m < n; ++m) keys[m] = vh::key(o.seed, m);

  Session s;
  int rc = open_session(&s, device, K, D, n, desc, num_int * KD, last_nodes * (size_t)K);
  if (rc != SLSLAM_OK) return rc;
  const Layout& y = s.y;
  int* h_node = s.h<int>(y.o_node);
  int* h_label = s.h<int>(y.o_label);
  int* h_perm = s.h<int>(y.o_perm);
  std::fill(h_node, h_node + n, 0);

  size_t num_nodes = 1, off = 0;                                      // of the level, and the level's first node in the tree
  for (int l = 0; l < L; ++l) {
    const size_t rows = num_nodes * (size_t)K;
    float* h_c = nodes + off * KD;                                    // the level's centres [num_nodes][K][D] = rows [rows][D]
    float* d_c = s.d<float>(y.o_centres) + off * KD;
    auto t0 = std::chrono::steady_clock::now();
    vh::partition(n, h_node, num_nodes, h_perm, start.data());
    vh::initial_centres(K, D, num_nodes, start.data(), h_perm, keys.data(), desc, l == 0 ? nullptr : nodes + (off - num_nodes / (size_t)K) * KD,
                        h_c);
    if ((rc = upload_partition(s)) != SLSLAM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_c, h_c, 4 * rows * (size_t)D, hipMemcpyHostToDevice, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    rep->setup_ms[l] = ms_since(t0);

    int its = 0;
    unsigned changed = 0;
    for (;;) {
      const bool last = its == o.max_iterations;
      t0 = std::chrono::steady_clock::now();
      if ((rc = launch_step(s, d_c, rows, !last, &changed)) != SLSLAM_OK) return rc;
      rep->kernel_ms[l] += ms_since(t0);
      if (its == 0) changed = (unsigned)n;                            // (the first assignment changes every label)
      if (last || (its >= 1 && changed == 0)) break;
      t0 = std::chrono::steady_clock::now();
      HIP_TRY(hipMemcpyAsync(s.h<long long>(y.o_acc), s.d<long long>(y.o_acc), 8 * rows * (size_t)D, hipMemcpyDeviceToHost, s.stream));
      HIP_TRY(hipStreamSynchronize(s.stream));
      rep->download_ms[l] += ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      vh::centres(rows, D, s.h<long long>(y.o_acc), h_c, h_c);
      rep->centre_ms[l] += ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      HIP_TRY(hipMemcpyAsync(d_c, h_c, 4 * rows * (size_t)D, hipMemcpyHostToDevice, s.stream));
      HIP_TRY(hipStreamSynchronize(s.stream));
      rep->upload_ms[l] += ms_since(t0);
      ++its;
    }

    t0 = std::chrono::steady_clock::now();
    const size_t blocks = step_blocks((long long)n);
    HIP_TRY(hipMemcpyAsync(h_label, s.d<int>(y.o_label), 4 * n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h<long long>(y.o_count), s.d<long long>(y.o_count), 8 * rows, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h<double>(y.o_partial), s.d<double>(y.o_partial), 8 * blocks, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    rep->download_ms[l] += ms_since(t0);
    const long long* cnt = s.h<long long>(y.o_count);
    long long empty = 0;
    for (size_t r = 0; r < rows; ++r) empty += cnt[r] == 0 ? 1 : 0;
    double dsum = 0.0;
    for (size_t b = 0; b < blocks; ++b) dsum += s.h<double>(y.o_partial)[b];
    rep->iterations[l] = its;
    rep->changed[l] = (long long)changed;
    rep->empty_children[l] = empty;
    rep->distortion[l] = dsum / (double)n;
    for (size_t m = 0; m < n; ++m) h_node[m] = h_node[m] * K + h_label[m];
    off += num_nodes;
    num_nodes = rows;
  }
  if (words) std::memcpy(words, h_node, 4 * n);
  return SLSLAM_OK;
}

}  // namespace

extern "C" int slslam_voctree_train(int device, const slslam_voctree_train_options* options, long long n, const float* descriptors,
                                    float* nodes, int* words, slslam_voctree_train_report* report) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!options || !descriptors || !nodes || n < 1 || n > kMaxDescriptors || !shape_valid(options->K, options->D) || options->L < 1 ||
      options->L > slslam_place::kMaxL || options->max_iterations < 0 || options->max_iterations > 1000)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  size_t num_int = 0, leaves = 1;
  for (int l = 0; l < options->L; ++l) { num_int += leaves; leaves *= (size_t)options->K; }
  if (leaves > ((size_t)1 << 24) || leaves * (size_t)options->D > (size_t)kMaxAccValues) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!vh::values_valid(descriptors, (size_t)n * (size_t)options->D)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc;
  try {
    // the outputs are the caller's only after the last level: a failure on the way leaves them as they were
    std::vector<float> out(num_int * (size_t)options->K * (size_t)options->D);
    std::vector<int> w((size_t)n);
    slslam_voctree_train_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.levels = options->L;
    rc = train(device, *options, (size_t)n, descriptors, num_int, out.data(), w.data(), &rep);
    if (rc == SLSLAM_OK) {
      std::memcpy(nodes, out.data(), sizeof(float) * out.size());
      if (words) std::memcpy(words, w.data(), sizeof(int) * w.size());
      rep.total_ms = ms_since(t0);
      if (report) *report = rep;
    }
  } catch (const std::bad_alloc&) {
    rc = SLSLAM_ERR_NO_MEMORY;
  }
  return rc;
}

extern "C" int slslam_debug_voctree_step(int device, int K, int D, long long num_nodes, const float* centres, long long n,
                                         const float* descriptors, const int* node, int* label, long long* acc, long long* count) {
  if (!centres || !descriptors || !node || !label || !acc || !count || n < 1 || n > kMaxDescriptors || !shape_valid(K, D) || num_nodes < 1 ||
      num_nodes > (1LL << 24) || num_nodes * K * D > kMaxAccValues)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  for (long long m = 0; m < n; ++m)
    if (node[m] < 0 || node[m] >= num_nodes) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!vh::values_valid(descriptors, (size_t)n * (size_t)D)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const size_t rows = (size_t)num_nodes * (size_t)K;
  try {
    std::vector<long long> start((size_t)num_nodes + 1);
    Session s;
    int rc = open_session(&s, device, K, D, (size_t)n, descriptors, rows * (size_t)D, rows);
    if (rc != SLSLAM_OK) return rc;
    const Layout& y = s.y;
    std::memcpy(s.h<int>(y.o_node), node, 4 * (size_t)n);
    vh::partition((size_t)n, node, (size_t)num_nodes, s.h<int>(y.o_perm), start.data());
    if ((rc = upload_partition(s)) != SLSLAM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s.d<float>(y.o_centres), centres, 4 * rows * (size_t)D, hipMemcpyHostToDevice, s.stream));
    unsigned changed = 0;
    if ((rc = launch_step(s, s.d<float>(y.o_centres), rows, true, &changed)) != SLSLAM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s.h<int>(y.o_label), s.d<int>(y.o_label), 4 * (size_t)n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h<long long>(y.o_acc), s.d<long long>(y.o_acc), 8 * rows * (size_t)D, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h<long long>(y.o_count), s.d<long long>(y.o_count), 8 * rows, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    std::memcpy(label, s.h<int>(y.o_label), 4 * (size_t)n);
    std::memcpy(acc, s.h<long long>(y.o_acc), 8 * rows * (size_t)D);
    std::memcpy(count, s.h<long long>(y.o_count), 8 * rows);
    return SLSLAM_OK;
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
}

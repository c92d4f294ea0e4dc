// slslam_amd/csrc/call_block.h — the scaffold of an entry point that is "a handle, one upload block, a few launches, one download
// block": whether there is a device, the handle's device and stream, the events of a handle that times its launches, its device
// block with the page-locked mirror, and the matchers' result block on the device (its layout and scatter need no HIP: call_layout.h).  Internal: not part of the C ABI.
#ifndef SLSLAM_CALL_BLOCK_H_
#define SLSLAM_CALL_BLOCK_H_

#include <hip/hip_runtime.h>

#include <algorithm>

#include "call_layout.h"
#include "grow_buf.h"
#include "hip_status.h"
#include "mutual_match.h"

namespace slslam {

// Devices the runtime reports; 0 also when asking fails
inline int device_count() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess ? ndev : 0;
}

inline bool device_present() { return device_count() > 0; }

constexpr int kMaxGridY = 65535;        // what the y dimension of a grid takes: problems go in slices of it

// The device of a handle: dev >= 0 is made current, dev < 0 adopts the current one
inline int use_device(int& dev) {
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (dev >= 0) HIP_TRY(hipSetDevice(dev));
  else HIP_TRY(hipGetDevice(&dev));
  return SLSLAM_OK;
}

// What a handle with a stream of its own holds
struct Handle {
  int device = -1;
  hipStream_t stream = nullptr;         // non-blocking, made at the first call that reaches the device
  long long calls = 0, allocations = 0;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  int ensure(int& dev) {
    const int rc = use_device(dev);
    if (rc != SLSLAM_OK) return rc;
    if (!stream) HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return SLSLAM_OK;
  }
  int ensure() { return ensure(device); }
};

// The *_stats(calls, allocations) getter of any handle that counts the two
template <typename H>
int handle_stats(const H* h, long long* calls, long long* allocations) {
  if (!h) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (calls) *calls = h->calls;
  if (allocations) *allocations = h->allocations;
  return SLSLAM_OK;
}

// A handle whose runs can time their launches by two events on its stream.  With timing off no member touches the runtime, and
// last_kernel_ms keeps what the last timed run left.
struct TimedHandle : Handle {
  bool timing = false;
  double last_kernel_ms = 0.0;          // the last timed run's launches
  hipEvent_t ev0 = nullptr, ev1 = nullptr;              // made at the first timed run
  ~TimedHandle() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  // before the launches
  int timer_start() {
    if (!timing) return SLSLAM_OK;
    if (!ev0) {
      HIP_TRY(hipEventCreate(&ev0));
      HIP_TRY(hipEventCreate(&ev1));
    }
    HIP_TRY(hipEventRecord(ev0, stream));
    return SLSLAM_OK;
  }
  // after them
  int timer_stop() {
    if (timing) HIP_TRY(hipEventRecord(ev1, stream));
    return SLSLAM_OK;
  }
  // after the caller's hipStreamSynchronize
  int timer_read() {
    if (!timing) return SLSLAM_OK;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    last_kernel_ms = ms;
    return SLSLAM_OK;
  }
};

// The *_timing(enable, kernel_ms) of any TimedHandle: enable < 0 leaves the switch as it is
template <typename H>
int handle_timing(H* h, int enable, double* kernel_ms) {
  if (!h) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (enable >= 0) h->timing = enable != 0;
  if (kernel_ms) *kernel_ms = h->last_kernel_ms;
  return SLSLAM_OK;
}

// A device block and its page-locked mirror
struct BlockPair {
  GrowBuf dev{Mem::kDevice}, host{Mem::kPinned};
  // Made for `capacity` at the first use, larger only when a call's `need` exceeds them; either way one event in *allocations
  int fit(const BlockBytes& capacity, const BlockBytes& need, long long* allocations) {
    if (dev.p && host.p && dev.n >= need.dev && host.n >= need.host) return SLSLAM_OK;
    long long unused = 0;
    HIP_TRY(dev.need(std::max(capacity.dev, need.dev), &unused));
    HIP_TRY(host.need(std::max(capacity.host, need.host), &unused));
    ++*allocations;
    return SLSLAM_OK;
  }
};

// ---- the matchers' result block on the device
inline MatchOut match_bind(char* d_out, const MatchBlock& b) {
  MatchOut o;
  o.num_matched = reinterpret_cast<int*>(d_out);
  o.match = reinterpret_cast<int*>(d_out + b.o_match);
  o.best = reinterpret_cast<int*>(d_out + b.o_best);
  o.num_admissible = reinterpret_cast<int*>(d_out + b.o_count);
  o.best_value = reinterpret_cast<float*>(d_out + b.o_best_value);
  o.second_value = reinterpret_cast<float*>(d_out + b.o_second_value);
  o.best_row = reinterpret_cast<int*>(d_out + b.o_best_row);
  return o;
}

// Before the launches: nothing matched, no column has a best row
inline int match_clear(const MatchOut& o, size_t P, unsigned long long* d_keys, size_t cols, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(o.num_matched, 0, 4 * P, s));
  if (cols > 0) HIP_TRY(hipMemsetAsync(d_keys, 0xff, 8 * cols, s));
  return SLSLAM_OK;
}

// After them: the block is on the host when this returns
inline int match_download(char* h_out, const char* d_out, const MatchBlock& b, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(h_out, d_out, b.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SLSLAM_OK;
}

}  // namespace slslam

#endif  // SLSLAM_CALL_BLOCK_H_

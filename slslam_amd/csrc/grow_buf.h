// slslam_amd/csrc/grow_buf.h — a buffer that only grows (its contents are not kept over a growth), in device, page-locked host or
// plain host memory; every allocation is counted.  Used by every handle that keeps its blocks between calls.  Internal: not part of
// the C ABI.
#ifndef SLSLAM_GROW_BUF_H_
#define SLSLAM_GROW_BUF_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "call_layout.h"

namespace slslam {

enum class Mem { kDevice, kPinned, kHost };

struct GrowBuf {
  const Mem mem;
  char* p = nullptr;
  size_t n = 0;
  explicit GrowBuf(Mem m) : mem(m) {}
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { release(); }
  hipError_t need(size_t bytes, long long* allocs) {
    if (bytes <= n && p) return hipSuccess;
    release();
    const size_t want = std::max<size_t>(bytes + bytes / 8, 256);
    hipError_t e = hipSuccess;
    if (mem == Mem::kDevice) e = hipMalloc((void**)&p, want);
    else if (mem == Mem::kPinned) e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
    else if (!(p = (char*)std::malloc(want))) e = hipErrorOutOfMemory;
    if (e == hipSuccess) { n = want; ++*allocs; }
    return e;
  }
  template <typename T> T* at(size_t byte_off) const { return reinterpret_cast<T*>(p + byte_off); }

 private:
  void release() {
    if (!p) return;
    if (mem == Mem::kDevice) (void)hipFree(p);
    else if (mem == Mem::kPinned) (void)hipHostFree(p);
    else std::free(p);
    p = nullptr; n = 0;
  }
};

}  // namespace slslam

#endif  // SLSLAM_GROW_BUF_H_

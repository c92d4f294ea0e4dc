// slslam_amd/csrc/hip_status.h — a failed HIP call as the C ABI reports it: one message format and one status mapping for every
// entry point of the library.  Internal: not part of the C ABI.
#ifndef SLSLAM_HIP_STATUS_H_
#define SLSLAM_HIP_STATUS_H_

#include <hip/hip_runtime.h>

#include <cstdio>

#include "../../include/slslam_hip.h"

namespace slslam {

inline int hip_status(hipError_t e, const char* what, const char* file, int line) {
  std::fprintf(stderr, "slslam: %s failed: %s (%s:%d)\n", what, hipGetErrorString(e), file, line);
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? SLSLAM_ERR_NO_DEVICE : SLSLAM_ERR_HIP;
}

}  // namespace slslam

// In a function that returns a slslam status: leave it with that status when the HIP call fails
#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return slslam::hip_status(_e, #expr, __FILE__, __LINE__);          \
  } while (0)

#endif  // SLSLAM_HIP_STATUS_H_

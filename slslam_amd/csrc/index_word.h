// slslam_amd/csrc/index_word.h — the narrowed index word of an observation, the one codec of the device build (lba_device_build.h),
// the host narrowing (lba_api.hip) and the pose estimator's window pack (frame_api.hip).
#ifndef SLSLAM_INDEX_WORD_H_
#define SLSLAM_INDEX_WORD_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slslam {

// The narrowed index word of an observation (RawWin::packed, slslam_pack_indices): line | camera << 16 | camera constant << 24 | line
// constant << 25.
__host__ __device__ inline uint32_t index_word(int camera, int line, int camera_const, int line_const) {
  return ((uint32_t)line & 0xffffu) | ((uint32_t)camera & 0xffu) << 16 | (camera_const ? 1u << 24 : 0u) | (line_const ? 1u << 25 : 0u);
}
__host__ __device__ inline int word_line(uint32_t v) { return (int)(v & 0xffffu); }
__host__ __device__ inline int word_camera(uint32_t v) { return (int)((v >> 16) & 0xffu); }
__host__ __device__ inline int word_camera_const(uint32_t v) { return (int)((v >> 24) & 1u); }
__host__ __device__ inline int word_line_const(uint32_t v) { return (int)((v >> 25) & 1u); }
// nonzero: a caller's word names a line >= L or a camera >= C, or sets a bit above the flags
__host__ __device__ inline unsigned word_bad(uint32_t v, int C, int L) {
  return (unsigned)(word_line(v) >= L) | (unsigned)(word_camera(v) >= C) | (v >> 26);
}

}  // namespace slslam

#endif  // SLSLAM_INDEX_WORD_H_

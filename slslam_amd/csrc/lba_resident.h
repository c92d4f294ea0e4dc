// slslam_amd/csrc/lba_resident.h — what lba_api.hip lends the pose estimator (frame_api.hip): a refill of a fused motion-only batch
// from windows that already lie in device memory, and the device-side view of the solved batch.  Internal: not part of the C ABI.
#ifndef SLSLAM_LBA_RESIDENT_H_
#define SLSLAM_LBA_RESIDENT_H_

#include <hip/hip_runtime.h>

#include "../../include/slslam_hip.h"
#include "lba_types.h"

namespace slslam {

// Replaces all windows of a refillable batch on the fused motion-only path by `n` windows (n = the batch's window count) whose
// observations, parameters and narrowed index words (packed[i]) are DEVICE pointers; camera_index / line_index / fixed_index are not read.
// The windows go straight to the device build on `s`: no staging copy, no page-locked lookup, and no host shape check - the caller
// builds motion-only windows by construction.  Windows [n_used, n) are placeholders: their LM state is parked, so the solve skips them.
// SLSLAM_ERR_UNSUPPORTED: not such a batch, or the windows cannot take this path (nothing touched).
int lba_refill_resident(slslam_lba_batch* b, const slslam_lba_window* windows, const unsigned int* const* packed, int n, int n_used,
                        hipStream_t s);

// The batch's LM states and window descriptors on the device ([window count] each; a window the device build could not take has C == 0).
int lba_device_results(const slslam_lba_batch* b, const LMState** state, const WinDesc** wins);

// Where the slslam_lba_batch_covariance call enqueued last left its results on the device: hdr [window count][hdr_ints] (status | free
// cameras | ...), cov_cam [window count][cam_stride] with the window's row-major (6F)^2 block at the front of its slot.
// SLSLAM_ERR_STATE: no such call is enqueued (none was made, or a download or a refill came after it).
int lba_device_covariance(const slslam_lba_batch* b, const int** hdr, int* hdr_ints, const double** cov_cam, long long* cam_stride);

}  // namespace slslam

#endif  // SLSLAM_LBA_RESIDENT_H_

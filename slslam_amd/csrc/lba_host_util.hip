// slslam_amd/csrc/lba_host_util.hip — host utilities of the LBA path's C ABI (include/slslam_hip.h): page-locked memory and the
// narrowed index words.  No kernel.
#include <hip/hip_runtime.h>

#include "../../include/slslam_hip.h"
#include "lba_batch.h"
#include "call_block.h"
#include "pinned_registry.h"

// ------------------------------------------------------------------------------------------
// Page-locked host memory the GPU reads and writes in place (include/slslam_hip.h)
extern "C" int slslam_pinned_alloc(size_t bytes, void** out) {
  if (!out) return SLSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  HIP_TRY(PinnedRegistry::get().alloc(bytes, out));
  return SLSLAM_OK;
}
extern "C" int slslam_pinned_free(void* p) {
  if (!p) return SLSLAM_OK;
  return PinnedRegistry::get().free(p) == 0 ? SLSLAM_OK : SLSLAM_ERR_INVALID_ARGUMENT;
}
extern "C" int slslam_pinned_register(void* p, size_t bytes) {
  if (!p || !bytes) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  HIP_TRY(PinnedRegistry::get().register_range(p, bytes));
  return SLSLAM_OK;
}
extern "C" int slslam_pinned_unregister(void* p) {
  if (!p) return SLSLAM_OK;
  return PinnedRegistry::get().unregister_range(p) == 0 ? SLSLAM_OK : SLSLAM_ERR_INVALID_ARGUMENT;
}
extern "C" int slslam_pinned_contains(const void* p, size_t bytes) { return PinnedRegistry::get().contains(p, bytes) ? 1 : 0; }
extern "C" int slslam_pack_indices(int n, const int* camera_index, const int* line_index, const int* fixed_index, unsigned int* packed) {
  if (n < 0 || (n > 0 && (!camera_index || !line_index || !fixed_index || !packed))) return SLSLAM_ERR_INVALID_ARGUMENT;
  // (what the word's fields hold: cameras 0 - 255, lines 0 - 65534)
  const unsigned oob = narrow_indices((size_t)n, camera_index, line_index, fixed_index, nullptr, 0x100, 0xffff, packed);
  return oob ? SLSLAM_ERR_UNSUPPORTED : SLSLAM_OK;
}

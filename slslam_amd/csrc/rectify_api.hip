// slslam_amd/csrc/rectify_api.hip — the image rectifier (include/slslam_hip.h: slslam_image_rectifier_*, slslam_rectify_images,
// slslam_rectify_smooth_taps, slslam_stereo_rectify): from the raw, distorted images of a stereo rig to the rectified and optionally
// smoothed images that slslam_line_detector_run and slslam_line_descriptor_run take.  Once per handle, at the first call that reaches
// the device: the maps of its cameras (k_rect_map), kept resident; their valid bytes come back once and stay on the host.  Per call,
// whatever the number of frames:
//   upload   one block [FrameDesc F | the source pixels of every frame, rows of src_width bytes]
//   launch   k_rect_remap, or k_rect_smooth when the handle smooths: one launch, sized by the largest frame of the call
//   download one block [the output pixels of every frame, rows of dst_width bytes]
// The kernels are in image_rectify.h, the layout, the validation, the taps and the rig in image_rectify_layout.h, the scaffold in
// call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "image_rectify.h"

using namespace slslam_rect;
using slslam::device_present;

static_assert(kConstant == SLSLAM_RECTIFY_BORDER_CONSTANT && kReplicate == SLSLAM_RECTIFY_BORDER_REPLICATE, "the header's modes are the kernel's");
static_assert(kSubBits == SLSLAM_RECTIFY_SUBPIXEL_BITS && kMaxRadius == SLSLAM_RECTIFY_MAX_RADIUS && kNoCoord == SLSLAM_RECTIFY_NO_COORD &&
              kTileW == SLSLAM_RECTIFY_TILE_WIDTH && kTileH == SLSLAM_RECTIFY_TILE_HEIGHT && kMaxSide == SLSLAM_LSD_MAX_SIDE,
              "the header's constants are the kernel's");
static_assert(sizeof(Camera) == sizeof(slslam_rectify_camera) && sizeof(Camera) == 22 * 8 + 16, "slslam_rectify_camera, field for field");
static_assert(sizeof(Rig) == sizeof(slslam_stereo_rig) && sizeof(Rig) == 30 * 8 + 8 * 4 + 16, "slslam_stereo_rig, field for field");
static_assert(sizeof(FrameDesc) == 24 && sizeof(CamDesc) == 24, "the layout the kernels index");

namespace {

Options options_of(const slslam_rectify_options& o) { return Options{o.border_mode, o.border_value, o.smooth_sigma}; }

bool options_valid(const slslam_rectify_options* o) { return o && slslam_rect::options_valid(options_of(*o)); }

std::vector<Camera> cameras_of(int num, const slslam_rectify_camera* cams) {
  std::vector<Camera> out((size_t)num);
  std::memcpy(out.data(), cams, sizeof(Camera) * (size_t)num);
  return out;
}

bool cameras_valid(int num, const slslam_rectify_camera* cams) {
  if (num < 1 || num > kMaxCameras || !cams) return false;
  return slslam_rect::cameras_valid(num, cameras_of(num, cams).data());
}

}  // namespace

struct slslam_image_rectifier : slslam::TimedHandle {
  Options opt;
  Taps taps;
  std::vector<Camera> cams;
  std::vector<CamDesc> desc;
  long long max_frames = 0, max_pixels = 0;
  slslam::BlockPair block;
  // the maps: made at the first call that reaches the device
  bool mapped = false;
  size_t map_pixels = 0;                // of all cameras, each at a multiple of 256
  slslam::GrowBuf map_dev{slslam::Mem::kDevice};
  std::vector<unsigned char> valid;     // the valid bytes of all cameras, as on the device
  std::vector<int> num_valid;
  size_t off_q = 0, off_sx = 0, off_sy = 0, off_valid = 0, off_desc = 0;

  Maps maps() const {
    return Maps{map_dev.at<int2>(off_q), map_dev.at<unsigned char>(off_valid), map_dev.at<double>(off_sx), map_dev.at<double>(off_sy)};
  }

  int ensure_maps() {
    if (mapped) return SLSLAM_OK;
    slslam::Carve c;
    off_q = c.take(8 * map_pixels);
    off_sx = c.take(8 * map_pixels);
    off_sy = c.take(8 * map_pixels);
    off_valid = c.take(map_pixels);
    off_desc = c.take(sizeof(CamDesc) * desc.size());
    long long unused = 0;
    HIP_TRY(map_dev.need(c.at, &unused));
    HIP_TRY(hipMemcpyAsync(map_dev.p + off_desc, desc.data(), sizeof(CamDesc) * desc.size(), hipMemcpyHostToDevice, stream));
    for (size_t k = 0; k < cams.size(); ++k) {
      const long long n = (long long)cams[k].dst_width * cams[k].dst_height;
      hipLaunchKernelGGL(k_rect_map, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, cams[k], desc[k].map0, maps());
    }
    HIP_TRY(hipGetLastError());
    valid.assign(map_pixels, 0);
    HIP_TRY(hipMemcpyAsync(valid.data(), map_dev.p + off_valid, map_pixels, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    num_valid.assign(cams.size(), 0);
    for (size_t k = 0; k < cams.size(); ++k) {
      const size_t n = (size_t)cams[k].dst_width * (size_t)cams[k].dst_height;
      int count = 0;
      for (size_t i = 0; i < n; ++i) count += valid[(size_t)desc[k].map0 + i];
      num_valid[k] = count;
    }
    mapped = true;
    return SLSLAM_OK;
  }
};

extern "C" void slslam_rectify_default_options(slslam_rectify_options* opt) {
  if (!opt) return;
  opt->border_mode = SLSLAM_RECTIFY_BORDER_CONSTANT;
  opt->border_value = 0;
  opt->smooth_sigma = 0.0;
}

extern "C" int slslam_rectify_smooth_taps(double sigma, int* radius, int* taps) {
  Taps t;
  if (!radius || !taps || !smooth_taps(sigma, &t)) return SLSLAM_ERR_INVALID_ARGUMENT;
  *radius = t.radius;
  std::memcpy(taps, t.t, sizeof(t.t));
  return SLSLAM_OK;
}

extern "C" int slslam_stereo_rectify(const slslam_stereo_rig* rig, slslam_rectify_camera* left, slslam_rectify_camera* right, double* baseline,
                                     double* intrinsics) {
  if (!rig || !left || !right || !baseline || !intrinsics) return SLSLAM_ERR_INVALID_ARGUMENT;
  Rig g;
  std::memcpy(&g, rig, sizeof(g));
  Camera l, r;
  double b, k[4];
  if (!stereo_rectify(g, &l, &r, &b, k)) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::memcpy(left, &l, sizeof(l));
  std::memcpy(right, &r, sizeof(r));
  *baseline = b;
  std::memcpy(intrinsics, k, sizeof(k));
  return SLSLAM_OK;
}

extern "C" int slslam_image_rectifier_create(int device, const slslam_rectify_options* opt, int num_cameras, const slslam_rectify_camera* cameras,
                                             int max_frames, long long max_pixels, slslam_image_rectifier** out) {
  if (!out || !options_valid(opt) || !cameras_valid(num_cameras, cameras) || !capacity_valid(max_frames, max_pixels))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_image_rectifier* h = new (std::nothrow) slslam_image_rectifier();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->device = device;
  h->opt = options_of(*opt);
  smooth_taps(h->opt.smooth_sigma, &h->taps);
  h->cams = cameras_of(num_cameras, cameras);
  h->desc.resize((size_t)num_cameras);
  for (int k = 0; k < num_cameras; ++k) {
    const Camera& c = h->cams[(size_t)k];
    h->desc[(size_t)k] = CamDesc{(long long)h->map_pixels, c.src_width, c.src_height, c.dst_width, c.dst_height};
    h->map_pixels += align_map((size_t)c.dst_width * (size_t)c.dst_height);
  }
  h->max_frames = max_frames; h->max_pixels = max_pixels;
  *out = h;
  return SLSLAM_OK;
}

extern "C" void slslam_image_rectifier_destroy(slslam_image_rectifier* h) { delete h; }

extern "C" int slslam_image_rectifier_stats(const slslam_image_rectifier* h, long long* calls, long long* allocations) {
  return slslam::handle_stats(h, calls, allocations);
}

extern "C" int slslam_image_rectifier_timing(slslam_image_rectifier* h, int enable, double* kernel_ms) {
  return slslam::handle_timing(h, enable, kernel_ms);
}

extern "C" int slslam_image_rectifier_get_map(slslam_image_rectifier* h, int camera, int* qx, int* qy, unsigned char* valid, double* sx,
                                              double* sy) {
  if (!h || camera < 0 || camera >= (int)h->cams.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  if ((rc = h->ensure_maps()) != SLSLAM_OK) return rc;
  const Camera& c = h->cams[(size_t)camera];
  const size_t n = (size_t)c.dst_width * (size_t)c.dst_height, m0 = (size_t)h->desc[(size_t)camera].map0;
  if (qx || qy) {
    std::vector<int> q(2 * n);
    HIP_TRY(hipMemcpy(q.data(), h->map_dev.p + h->off_q + 8 * m0, 8 * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      if (qx) qx[i] = q[2 * i];
      if (qy) qy[i] = q[2 * i + 1];
    }
  }
  if (valid) std::memcpy(valid, h->valid.data() + m0, n);
  if (sx) HIP_TRY(hipMemcpy(sx, h->map_dev.p + h->off_sx + 8 * m0, 8 * n, hipMemcpyDeviceToHost));
  if (sy) HIP_TRY(hipMemcpy(sy, h->map_dev.p + h->off_sy + 8 * m0, 8 * n, hipMemcpyDeviceToHost));
  return SLSLAM_OK;
}

extern "C" int slslam_image_rectifier_run(slslam_image_rectifier* h, int num_frames, const slslam_rectify_frame* frames,
                                          const slslam_rectify_result* results) {
  // ---- every argument before anything is written or the device is asked
  if (!h || num_frames < 0 || (num_frames > 0 && (!frames || !results))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames, C = (int)h->cams.size();
  size_t src_bytes = 0, dst_bytes = 0;
  long long max_dst = 0;
  int max_tiles = 0;
  for (int f = 0; f < F; ++f) {
    if (!frame_valid(frames[f].camera, C, frames[f].stride, frames[f].image, h->cams.data())) return SLSLAM_ERR_INVALID_ARGUMENT;
    const Camera& c = h->cams[(size_t)frames[f].camera];
    if (!result_valid(results[f].stride, results[f].image, c)) return SLSLAM_ERR_INVALID_ARGUMENT;
    src_bytes += slslam::align256((size_t)c.src_width * (size_t)c.src_height);
    dst_bytes += slslam::align256((size_t)c.dst_width * (size_t)c.dst_height);
    max_dst = std::max(max_dst, (long long)c.dst_width * c.dst_height);
    max_tiles = std::max(max_tiles, ((c.dst_width + kTileW - 1) / kTileW) * ((c.dst_height + kTileH - 1) / kTileH));
  }
  if (F > slslam::kMaxGridY || (long long)src_bytes > 4 * kMaxCapacityPixels || (long long)dst_bytes > 4 * kMaxCapacityPixels)
    return SLSLAM_ERR_UNSUPPORTED;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = h->stream;
  ++h->calls;
  if (F == 0) return SLSLAM_OK;
  if ((rc = h->ensure_maps()) != SLSLAM_OK) return rc;

  // ---- layout.  The blocks: made for the handle's capacity at the first run, larger only when a call exceeds them
  const CallLayout y = call_layout((size_t)F, src_bytes, dst_bytes);
  const size_t capF = (size_t)std::max<long long>(F, h->max_frames), capN = capF * slslam::align256((size_t)h->max_pixels);
  const CallLayout cap = call_layout(capF, capN, capN);
  if ((rc = h->block.fit(cap.bytes, y.bytes, &h->allocations)) != SLSLAM_OK) return rc;

  // ---- one upload: the images with their src_width bytes per row, the stride stays here
  char* hb = h->block.host.p;
  char* dv = h->block.dev.p;
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(hb);
  unsigned char* px = reinterpret_cast<unsigned char*>(hb + y.off_src);
  size_t src_at = 0, dst_at = 0;
  for (int f = 0; f < F; ++f) {
    const Camera& c = h->cams[(size_t)frames[f].camera];
    fd[f] = FrameDesc{(long long)src_at, (long long)dst_at, frames[f].camera, 0};
    slslam::pack_rows(px + src_at, frames[f].image, c.src_width, c.src_height, (int)frames[f].stride);
    src_at += slslam::align256((size_t)c.src_width * (size_t)c.src_height);
    dst_at += slslam::align256((size_t)c.dst_width * (size_t)c.dst_height);
  }
  HIP_TRY(hipMemcpyAsync(dv, hb, y.in_bytes, hipMemcpyHostToDevice, s));

  const Maps m = h->maps();
  Call call;
  call.frames = reinterpret_cast<const FrameDesc*>(dv);
  call.cams = h->map_dev.at<CamDesc>(h->off_desc);
  call.q = m.q;
  call.valid = m.valid;
  call.src = reinterpret_cast<const unsigned char*>(dv + y.off_src);
  call.dst = reinterpret_cast<unsigned char*>(dv + y.off_out);
  call.border_mode = h->opt.border_mode;
  call.border_value = h->opt.border_value;

  if ((rc = h->timer_start()) != SLSLAM_OK) return rc;
  if (h->taps.radius > 0)
    hipLaunchKernelGGL(k_rect_smooth, dim3((unsigned)max_tiles, (unsigned)F), dim3(kBlock), 0, s, call, h->taps);
  else
    hipLaunchKernelGGL(k_rect_remap, dim3((unsigned)((max_dst + kBlock - 1) / kBlock), (unsigned)F), dim3(kBlock), 0, s, call);
  HIP_TRY(hipGetLastError());
  if ((rc = h->timer_stop()) != SLSLAM_OK) return rc;

  // ---- one download
  char* ho = hb + y.off_out;
  HIP_TRY(hipMemcpyAsync(ho, dv + y.off_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->timer_read()) != SLSLAM_OK) return rc;
  for (int f = 0; f < F; ++f) {
    const Camera& c = h->cams[(size_t)frames[f].camera];
    const slslam_rectify_result& r = results[f];
    const unsigned char* from = reinterpret_cast<const unsigned char*>(ho) + fd[f].dst0;
    for (int row = 0; row < c.dst_height; ++row)
      std::memcpy(r.image + (size_t)row * (size_t)r.stride, from + (size_t)row * (size_t)c.dst_width, (size_t)c.dst_width);
    // validity is the camera's alone: the bytes came back with the maps
    if (r.valid) std::memcpy(r.valid, h->valid.data() + (size_t)h->desc[(size_t)frames[f].camera].map0, (size_t)c.dst_width * (size_t)c.dst_height);
    if (r.num_valid) *r.num_valid = h->num_valid[(size_t)frames[f].camera];
  }
  return SLSLAM_OK;
}

extern "C" int slslam_rectify_images(const slslam_rectify_options* opt, int num_cameras, const slslam_rectify_camera* cameras, int num_frames,
                                     const slslam_rectify_frame* frames, const slslam_rectify_result* results) {
  if (!options_valid(opt) || !cameras_valid(num_cameras, cameras) || num_frames < 0 || (num_frames > 0 && (!frames || !results)))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  long long max_pixels = 1;
  const std::vector<Camera> cams = cameras_of(num_cameras, cameras);
  for (int f = 0; f < num_frames; ++f) {
    if (!frame_valid(frames[f].camera, num_cameras, frames[f].stride, frames[f].image, cams.data())) return SLSLAM_ERR_INVALID_ARGUMENT;
    const Camera& c = cams[(size_t)frames[f].camera];
    if (!result_valid(results[f].stride, results[f].image, c)) return SLSLAM_ERR_INVALID_ARGUMENT;
    max_pixels = std::max(max_pixels, std::max((long long)c.src_width * c.src_height, (long long)c.dst_width * c.dst_height));
  }
  if (!capacity_valid(std::max(num_frames, 1), max_pixels)) return SLSLAM_ERR_UNSUPPORTED;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_image_rectifier* h = nullptr;
  int rc = slslam_image_rectifier_create(-1, opt, num_cameras, cameras, std::max(num_frames, 1), max_pixels, &h);
  if (rc == SLSLAM_OK) rc = slslam_image_rectifier_run(h, num_frames, frames, results);
  slslam_image_rectifier_destroy(h);
  return rc;
}

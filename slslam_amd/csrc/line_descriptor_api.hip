// slslam_amd/csrc/line_descriptor_api.hip — the MSLD line descriptor (include/slslam_hip.h: slslam_line_descriptor_*, slslam_describe_lines):
// what makes the [n, D] descriptors the place recogniser, the tree trainer and the descriptor matcher take, from grey images and line
// segments.  Per call, whatever the number of frames:
//   upload   one block [FrameDesc F | SegDesc S | WeightRow M w | the pixels of every frame, rows of `width` bytes]
//   launch   k_line_descriptor: one wave per segment
//   download one block [descriptors S D | status S | num_samples S | polarity S]
// The segment index lies in the grid, the frame in the segment.  The kernel is in line_descriptor.h, the layout and the validation in
// line_descriptor_layout.h, the scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "line_descriptor.h"

using namespace slslam_msld;
using slslam::device_present;

static_assert(kOk == SLSLAM_MSLD_OK && kFlat == SLSLAM_MSLD_FLAT && kTooShort == SLSLAM_MSLD_TOO_SHORT && kOutside == SLSLAM_MSLD_OUTSIDE &&
              kInvalid == SLSLAM_MSLD_INVALID, "the header's statuses are the kernel's");
static_assert(kMaxBands == SLSLAM_MSLD_MAX_BANDS && kMaxBandWidth == SLSLAM_MSLD_MAX_BAND_WIDTH && kMaxRows == SLSLAM_MSLD_MAX_ROWS &&
              kMaxSide == SLSLAM_MSLD_MAX_SIDE, "the header's limits are the kernel's");

namespace {

bool options_valid(const slslam_msld_options* o) { return o && slslam_msld::options_valid(o->bands, o->band_width, o->orient); }

bool frame_valid(const slslam_msld_frame& f) {
  return slslam_msld::frame_valid(f.width, f.height, f.stride, f.image, f.num_segments, f.segments);
}

}  // namespace

struct slslam_line_descriptor : slslam::TimedHandle {
  slslam_msld_options opt;
  int rows = 0;
  long long max_frames = 0, max_pixels = 0, max_segments = 0;
  WeightRow table[kMaxRows];
  slslam::BlockPair block;
};

extern "C" void slslam_msld_default_options(slslam_msld_options* opt) {
  if (!opt) return;
  opt->bands = 9;
  opt->band_width = 5;
  opt->orient = 1;
}

extern "C" int slslam_line_descriptor_create(int device, const slslam_msld_options* opt, int max_frames, long long max_pixels,
                                             int max_segments, slslam_line_descriptor** out) {
  if (!out || !options_valid(opt) || max_frames < 1 || max_pixels < 1 || max_segments < 1) return SLSLAM_ERR_INVALID_ARGUMENT;
  // the capacity the first run allocates: no more segments than a call may hold, no frame larger than an image may be, 4 GiB of pixels
  if (max_pixels > (long long)kMaxSide * kMaxSide || (long long)max_frames * max_segments > kMaxSegments ||
      (long long)max_frames * max_pixels > kMaxCapacityPixels)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_descriptor* h = new (std::nothrow) slslam_line_descriptor();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->device = device;
  h->opt = *opt;
  h->rows = weight_table(opt->bands, opt->band_width, h->table);
  h->max_frames = max_frames; h->max_pixels = max_pixels; h->max_segments = max_segments;
  *out = h;
  return SLSLAM_OK;
}

extern "C" void slslam_line_descriptor_destroy(slslam_line_descriptor* h) { delete h; }

extern "C" int slslam_line_descriptor_stats(const slslam_line_descriptor* h, long long* calls, long long* allocations) {
  return slslam::handle_stats(h, calls, allocations);
}

extern "C" int slslam_line_descriptor_timing(slslam_line_descriptor* h, int enable, double* kernel_ms) {
  return slslam::handle_timing(h, enable, kernel_ms);
}

extern "C" int slslam_line_descriptor_run(slslam_line_descriptor* h, int num_frames, const slslam_msld_frame* frames,
                                          const slslam_msld_result* results) {
  // ---- every argument before anything is written or the device is asked
  if (!h || num_frames < 0 || (num_frames > 0 && (!frames || !results))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  long long Stot = 0, pixels = 0;
  for (int f = 0; f < F; ++f) {
    if (!frame_valid(frames[f])) return SLSLAM_ERR_INVALID_ARGUMENT;
    Stot += frames[f].num_segments;
    pixels += (long long)slslam::align256((size_t)frames[f].width * (size_t)frames[f].height);
  }
  if (Stot > kMaxSegments) return SLSLAM_ERR_UNSUPPORTED;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = h->stream;
  ++h->calls;
  if (F == 0) return SLSLAM_OK;

  // ---- layout.  The blocks: made for the handle's capacity at the first run, larger only when a call exceeds them
  const int M = h->opt.bands, D = 8 * M;
  const size_t S = (size_t)Stot;
  const CallLayout y = call_layout((size_t)F, S, (size_t)h->rows, (size_t)pixels, (size_t)D);
  const size_t capF = (size_t)std::max<long long>(F, h->max_frames);
  const CallLayout cap = call_layout(capF, capF * (size_t)h->max_segments, (size_t)h->rows,
                                     capF * slslam::align256((size_t)h->max_pixels), (size_t)D);
  if ((rc = h->block.fit(cap.bytes, y.bytes, &h->allocations)) != SLSLAM_OK) return rc;

  // ---- one upload: the images with their `width` bytes per row, the stride stays here
  char* hb = h->block.host.p;
  char* dv = h->block.dev.p;
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(hb);
  SegDesc* sg = reinterpret_cast<SegDesc*>(hb + y.off_seg);
  std::memcpy(hb + y.off_table, h->table, sizeof(WeightRow) * (size_t)h->rows);
  unsigned char* px = reinterpret_cast<unsigned char*>(hb + y.off_pixels);
  std::vector<size_t> first((size_t)F);
  size_t at = 0, k = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_msld_frame& fr = frames[f];
    fd[f].image = (long long)at;
    fd[f].width = fr.width; fd[f].height = fr.height;
    slslam::pack_rows(px + at, fr.image, fr.width, fr.height, fr.stride);
    at += slslam::align256((size_t)fr.width * (size_t)fr.height);
    first[(size_t)f] = k;
    for (int i = 0; i < fr.num_segments; ++i, ++k) {
      const float* c = fr.segments + 4 * (size_t)i;
      SegDesc& d = sg[k];
      d.x0 = c[0]; d.y0 = c[1]; d.x1 = c[2]; d.y1 = c[3];
      d.status = segment_status(fr.width, fr.height, c, &d.length, &d.num_samples);
      d.frame = f;
      d.pad = 0;
    }
  }
  if (S > 0) {
    HIP_TRY(hipMemcpyAsync(dv, hb, y.in_bytes, hipMemcpyHostToDevice, s));
    char* d_out = dv + y.off_out;
    Out o;
    o.descriptors = reinterpret_cast<float*>(d_out);
    o.status = reinterpret_cast<int*>(d_out + y.o_status);
    o.num_samples = reinterpret_cast<int*>(d_out + y.o_samples);
    o.polarity = reinterpret_cast<float*>(d_out + y.o_polarity);
    if ((rc = h->timer_start()) != SLSLAM_OK) return rc;
    hipLaunchKernelGGL(k_line_descriptor, dim3((unsigned)S), dim3(kWave), 0, s, reinterpret_cast<const FrameDesc*>(dv),
                       reinterpret_cast<const SegDesc*>(dv + y.off_seg), reinterpret_cast<const WeightRow*>(dv + y.off_table),
                       reinterpret_cast<const unsigned char*>(dv + y.off_pixels), M, h->rows, h->opt.orient, o);
    HIP_TRY(hipGetLastError());
    if ((rc = h->timer_stop()) != SLSLAM_OK) return rc;

    // ---- one download
    HIP_TRY(hipMemcpyAsync(hb + y.off_out, d_out, y.out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = h->timer_read()) != SLSLAM_OK) return rc;
  }
  const char* ho = hb + y.off_out;
  for (int f = 0; f < F; ++f) {
    const slslam_msld_result& r = results[f];
    const size_t n = (size_t)frames[f].num_segments, k0 = first[(size_t)f];
    if (n == 0) continue;
    if (r.descriptors) std::memcpy(r.descriptors, ho + 4 * k0 * (size_t)D, 4 * n * (size_t)D);
    if (r.status) std::memcpy(r.status, ho + y.o_status + 4 * k0, 4 * n);
    if (r.num_samples) std::memcpy(r.num_samples, ho + y.o_samples + 4 * k0, 4 * n);
    if (r.polarity) std::memcpy(r.polarity, ho + y.o_polarity + 4 * k0, 4 * n);
  }
  return SLSLAM_OK;
}

extern "C" int slslam_describe_lines(const slslam_msld_options* opt, const slslam_msld_frame* frame, const slslam_msld_result* result) {
  if (!options_valid(opt) || !frame || !result || !frame_valid(*frame)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_line_descriptor* h = nullptr;
  int rc = slslam_line_descriptor_create(-1, opt, 1, (long long)frame->width * frame->height, std::max(frame->num_segments, 1), &h);
  if (rc == SLSLAM_OK) rc = slslam_line_descriptor_run(h, 1, frame, result);
  slslam_line_descriptor_destroy(h);
  return rc;
}

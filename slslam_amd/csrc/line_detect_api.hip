// slslam_amd/csrc/line_detect_api.hip — the line segment detector (include/slslam_hip.h: slslam_line_detector_*, slslam_detect_lines): what
// makes the segments that slslam_line_descriptor_run, the matchers and the triangulator take, from grey images.  Per call, whatever the
// number of frames:
//   upload   one block [FrameDesc F | the pixels of every frame, rows of `width` bytes]
//   launch   the eleven kernels of line_detect.h, sized by what the host knows: pixels, tiles, component slots
//   download one block [FrameOut F | segments | length | thickness | strength | pixels | label], and the label planes behind it when a
//            frame asks for its plane
// The kernels are in line_detect.h, the layout and the validation in line_detect_layout.h, the scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "line_detect.h"

using namespace slslam_lsd;
using slslam::device_present;

static_assert(kOk == SLSLAM_LSD_OK && kSmall == SLSLAM_LSD_SMALL && kIsotropic == SLSLAM_LSD_ISOTROPIC && kShort == SLSLAM_LSD_SHORT &&
              kThick == SLSLAM_LSD_THICK, "the header's statuses are the kernel's");
static_assert(kMaxSide == SLSLAM_LSD_MAX_SIDE && kTile == SLSLAM_LSD_TILE, "the header's limits are the kernel's");
static_assert(sizeof(Comp) == 128 && sizeof(FrameOut) == 48 && sizeof(FrameDesc) == 32, "the layout the kernels index");

namespace {

Options options_of(const slslam_line_detect_options& o) {
  return Options{o.grad_threshold, o.tol_num, o.tol_den, o.min_pixels, o.min_length, o.max_thickness, o.max_segments};
}

bool options_valid(const slslam_line_detect_options* o) { return o && slslam_lsd::options_valid(options_of(*o)); }

bool frame_valid(const slslam_line_detect_frame& f) { return slslam_lsd::frame_valid(f.width, f.height, f.stride, f.image); }

}  // namespace

struct slslam_line_detector : slslam::TimedHandle {
  Options opt;
  long long max_frames = 0, max_pixels = 0;
  slslam::BlockPair block;
};

extern "C" void slslam_line_detect_default_options(slslam_line_detect_options* opt) {
  if (!opt) return;
  opt->grad_threshold = 24;
  opt->tol_num = 11;
  opt->tol_den = 64;
  opt->min_pixels = 12;
  opt->min_length = 10.0;
  opt->max_thickness = 3.0;
  opt->max_segments = 512;
}

extern "C" int slslam_line_detector_create(int device, const slslam_line_detect_options* opt, int max_frames, long long max_pixels,
                                           slslam_line_detector** out) {
  if (!out || !options_valid(opt) || !capacity_valid(max_frames, max_pixels, opt->max_segments)) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_detector* h = new (std::nothrow) slslam_line_detector();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->device = device;
  h->opt = options_of(*opt);
  h->max_frames = max_frames; h->max_pixels = max_pixels;
  *out = h;
  return SLSLAM_OK;
}

extern "C" void slslam_line_detector_destroy(slslam_line_detector* h) { delete h; }

extern "C" int slslam_line_detector_stats(const slslam_line_detector* h, long long* calls, long long* allocations) {
  return slslam::handle_stats(h, calls, allocations);
}

extern "C" int slslam_line_detector_timing(slslam_line_detector* h, int enable, double* kernel_ms) {
  return slslam::handle_timing(h, enable, kernel_ms);
}

extern "C" int slslam_line_detector_run(slslam_line_detector* h, int num_frames, const slslam_line_detect_frame* frames,
                                        const slslam_line_detect_result* results) {
  // ---- every argument before anything is written or the device is asked
  if (!h || num_frames < 0 || (num_frames > 0 && (!frames || !results))) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  const size_t S = (size_t)h->opt.max_segments;
  size_t pixels = 0, comps = 0;
  int max_chunks = 0, max_tiles = 0, max_comps = 0;
  bool labels = false;
  for (int f = 0; f < F; ++f) {
    if (!frame_valid(frames[f])) return SLSLAM_ERR_INVALID_ARGUMENT;
    const size_t n = (size_t)frames[f].width * (size_t)frames[f].height;
    pixels += align_chunk(n);
    comps += comp_capacity(n, h->opt.min_pixels);
    max_chunks = std::max(max_chunks, (int)(align_chunk(n) / kChunk));
    max_tiles = std::max(max_tiles, ((frames[f].width + kTile - 1) / kTile) * ((frames[f].height + kTile - 1) / kTile));
    max_comps = std::max(max_comps, (int)comp_capacity(n, h->opt.min_pixels));
    labels = labels || results[f].labels != nullptr;
  }
  if ((long long)F * (long long)S > kMaxCallSegments || F > slslam::kMaxGridY || (long long)pixels > 4 * kMaxCapacityPixels) return SLSLAM_ERR_UNSUPPORTED;
  int rc = h->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = h->stream;
  ++h->calls;
  if (F == 0) return SLSLAM_OK;

  // ---- layout.  The blocks: made for the handle's capacity at the first run, larger only when a call exceeds them
  const CallLayout y = call_layout((size_t)F, pixels, comps, S, labels);
  const size_t capF = (size_t)std::max<long long>(F, h->max_frames), capN = (size_t)h->max_pixels;
  const CallLayout cap = call_layout(capF, capF * align_chunk(capN), capF * comp_capacity(capN, h->opt.min_pixels), S, labels);
  if ((rc = h->block.fit(cap.bytes, y.bytes, &h->allocations)) != SLSLAM_OK) return rc;

  // ---- one upload: the images with their `width` bytes per row, the stride stays here
  char* hb = h->block.host.p;
  char* dv = h->block.dev.p;
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(hb);
  unsigned char* px = reinterpret_cast<unsigned char*>(hb + y.off_pixels);
  size_t at = 0, comp0 = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_line_detect_frame& fr = frames[f];
    const size_t n = (size_t)fr.width * (size_t)fr.height;
    fd[f].first = (long long)at;
    fd[f].comp0 = (long long)comp0;
    fd[f].width = fr.width; fd[f].height = fr.height;
    fd[f].comp_cap = (int)comp_capacity(n, h->opt.min_pixels);
    fd[f].chunk0 = (int)(at / kChunk);
    slslam::pack_rows(px + at, fr.image, fr.width, fr.height, fr.stride);
    at += align_chunk(n);
    comp0 += comp_capacity(n, h->opt.min_pixels);
  }
  HIP_TRY(hipMemcpyAsync(dv, hb, y.in_bytes, hipMemcpyHostToDevice, s));

  char* d_out = dv + y.off_out;
  Planes P;
  P.frames = reinterpret_cast<const FrameDesc*>(dv);
  P.pixels = reinterpret_cast<const unsigned char*>(dv + y.off_pixels);
  P.links = reinterpret_cast<unsigned char*>(dv + y.off_links);
  P.count = reinterpret_cast<int*>(dv + y.off_count);
  P.parent = reinterpret_cast<int*>(d_out + y.o_labels);
  P.chunks = reinterpret_cast<int2*>(dv + y.off_chunks);
  P.comps = reinterpret_cast<Comp*>(dv + y.off_comp);
  P.out = reinterpret_cast<FrameOut*>(d_out);
  Segments G;
  G.segments = reinterpret_cast<float*>(d_out + y.o_segments);
  G.length = reinterpret_cast<double*>(d_out + y.o_length);
  G.thickness = reinterpret_cast<double*>(d_out + y.o_thickness);
  G.strength = reinterpret_cast<double*>(d_out + y.o_strength);
  G.npix = reinterpret_cast<int*>(d_out + y.o_npix);
  G.label = reinterpret_cast<int*>(d_out + y.o_label);

  if ((rc = h->timer_start()) != SLSLAM_OK) return rc;
  const Options& o = h->opt;
  const dim3 per_chunk((unsigned)max_chunks, (unsigned)F), per_tile((unsigned)max_tiles, (unsigned)F), per_frame((unsigned)F);
  const dim3 per_comp((unsigned)((max_comps + kBlock - 1) / kBlock), (unsigned)F), block(kBlock);
  hipLaunchKernelGGL(k_links, per_chunk, block, 0, s, P, o.grad_threshold * o.grad_threshold, o.tol_num, o.tol_den);
  hipLaunchKernelGGL(k_tile, per_tile, block, 0, s, P);
  hipLaunchKernelGGL(k_border, per_chunk, block, 0, s, P);
  hipLaunchKernelGGL(k_compress, per_chunk, block, 0, s, P);
  hipLaunchKernelGGL(k_count, per_chunk, block, 0, s, P, o.min_pixels);
  hipLaunchKernelGGL(k_scan, per_frame, block, 0, s, P);
  hipLaunchKernelGGL(k_assign, per_chunk, block, 0, s, P, o.min_pixels);
  hipLaunchKernelGGL(k_sums, per_chunk, block, 0, s, P);
  hipLaunchKernelGGL(k_fit, per_comp, block, 0, s, P);
  hipLaunchKernelGGL(k_extent, per_chunk, block, 0, s, P);
  hipLaunchKernelGGL(k_emit, per_frame, block, 0, s, P, G, o.min_length, o.max_thickness, o.max_segments);
  HIP_TRY(hipGetLastError());
  if ((rc = h->timer_stop()) != SLSLAM_OK) return rc;

  // ---- one download
  char* ho = hb + y.in_bytes;
  HIP_TRY(hipMemcpyAsync(ho, d_out, labels ? y.out_bytes_labels : y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->timer_read()) != SLSLAM_OK) return rc;
  const FrameOut* fo = reinterpret_cast<const FrameOut*>(ho);
  for (int f = 0; f < F; ++f) {
    const slslam_line_detect_result& r = results[f];
    const size_t n = (size_t)fo[f].num_written, k0 = (size_t)f * S;
    if (r.num_components) *r.num_components = fo[f].num_components;
    if (r.num_ok) *r.num_ok = fo[f].num_ok;
    if (r.num_written) *r.num_written = fo[f].num_written;
    if (r.status_counts) std::memcpy(r.status_counts, fo[f].counts, sizeof(fo[f].counts));
    if (r.segments && n) std::memcpy(r.segments, ho + y.o_segments + 16 * k0, 16 * n);
    if (r.length && n) std::memcpy(r.length, ho + y.o_length + 8 * k0, 8 * n);
    if (r.thickness && n) std::memcpy(r.thickness, ho + y.o_thickness + 8 * k0, 8 * n);
    if (r.strength && n) std::memcpy(r.strength, ho + y.o_strength + 8 * k0, 8 * n);
    if (r.pixels && n) std::memcpy(r.pixels, ho + y.o_npix + 4 * k0, 4 * n);
    if (r.label && n) std::memcpy(r.label, ho + y.o_label + 4 * k0, 4 * n);
    if (r.labels)
      std::memcpy(r.labels, ho + y.o_labels + 4 * (size_t)fd[f].first, 4 * (size_t)frames[f].width * (size_t)frames[f].height);
  }
  return SLSLAM_OK;
}

extern "C" int slslam_detect_lines(const slslam_line_detect_options* opt, const slslam_line_detect_frame* frame,
                                   const slslam_line_detect_result* result) {
  if (!options_valid(opt) || !frame || !result || !frame_valid(*frame)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_line_detector* h = nullptr;
  int rc = slslam_line_detector_create(-1, opt, 1, (long long)frame->width * frame->height, &h);
  if (rc == SLSLAM_OK) rc = slslam_line_detector_run(h, 1, frame, result);
  slslam_line_detector_destroy(h);
  return rc;
}

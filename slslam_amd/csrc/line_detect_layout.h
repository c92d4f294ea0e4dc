// slslam_amd/csrc/line_detect_layout.h — the host half of the line segment detector (include/slslam_hip.h: slslam_line_detector_*): the
// limits, the validation of options and frames, and where everything of a call lies in its one block.  Plain C++ with no HIP in it, so
// that tests/host_cxx/line_detect_layout_check.cpp runs it on the host under the sanitizers; the kernels are in line_detect.h.
// Internal: not part of the C ABI.
#ifndef SLSLAM_LINE_DETECT_LAYOUT_H_
#define SLSLAM_LINE_DETECT_LAYOUT_H_

#include <cmath>
#include <cstddef>

#include "call_layout.h"

namespace slslam_lsd {

constexpr int kMaxSide = 8192, kMaxThreshold = 1024, kMaxTolerance = 1 << 20, kMaxSegments = 1 << 20;
constexpr long long kMaxCallSegments = 1LL << 24;       // max_frames x max_segments a handle may be created for
constexpr long long kMaxCapacityPixels = 1LL << 30;    // max_frames x max_pixels a handle may be created for: about 21 bytes a pixel
constexpr int kTile = 32;                               // the side of a labelling tile: 1024 parents in LDS
constexpr int kBlock = 256, kChunk = 1024;              // a block of the per-pixel passes takes kChunk pixels, four a thread

// per-component status: the values of SLSLAM_LSD_* (the api file asserts it), the index of status_counts
enum Status { kOk = 0, kSmall = 1, kIsotropic = 2, kShort = 3, kThick = 4 };
// the bits of a pixel's link byte: strong, and the four forward links
enum Link { kStrong = 1, kEast = 2, kSouthWest = 4, kSouth = 8, kSouthEast = 16 };

struct Options {
  int grad_threshold, tol_num, tol_den, min_pixels;
  double min_length, max_thickness;
  int max_segments;
};

// A frame of the call, as the kernels see it.  A plane (pixels, link bytes, counts, labels) holds the frames one behind the other, each
// at a multiple of kChunk elements; `first` is the frame's offset in every plane.
struct FrameDesc {
  long long first;
  long long comp0;                      // its first slot among the fitted components of all frames
  int width, height;
  int comp_cap;                         // slots it has: floor(width height / min_pixels), which a frame cannot exceed
  int chunk0;                           // its first chunk among the chunks of all frames
};

// A component that is fitted (pixels >= min_pixels), in label order within its frame
struct Comp {
  long long sw, swu, swv, swuu, swuv, swvv, sgx, sgy;    // step 4, about the root pixel
  long long tmin_key, tmax_key;         // the order-preserving image of the extent's two doubles
  int n, root;
  double cx, cy, ex, ey, thickness;     // step 5; ex = ey = 0: isotropic
};

// What a frame's kernels leave for the host (num_fitted is the device's own)
struct FrameOut {
  int num_components, num_ok, num_written, num_fitted;
  int counts[5];
  int pad[3];
};

inline size_t align_chunk(size_t pixels) { return (pixels + (size_t)kChunk - 1) / (size_t)kChunk * (size_t)kChunk; }

inline bool options_valid(const Options& o) {
  if (o.grad_threshold < 1 || o.grad_threshold > kMaxThreshold) return false;
  if (o.tol_num < 0 || o.tol_num > kMaxTolerance || o.tol_den < 1 || o.tol_den > kMaxTolerance) return false;
  if (o.min_pixels < 1 || o.max_segments < 1 || o.max_segments > kMaxSegments) return false;
  // (a NaN fails both comparisons)
  if (!(o.min_length >= 0.0) || !std::isfinite(o.min_length) || !(o.max_thickness >= 0.0) || !std::isfinite(o.max_thickness)) return false;
  return true;
}

inline bool frame_valid(int width, int height, long long stride, const void* image) {
  return width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide && stride >= width && image != nullptr;
}

inline bool capacity_valid(int max_frames, long long max_pixels, int max_segments) {
  return max_frames >= 1 && max_pixels >= 1 && max_pixels <= (long long)kMaxSide * kMaxSide &&
         (long long)max_frames * max_pixels <= kMaxCapacityPixels && (long long)max_frames * max_segments <= kMaxCallSegments;
}

// slots for the fitted components of a frame of `pixels` pixels: a component that is fitted has at least min_pixels of them
inline size_t comp_capacity(size_t pixels, int min_pixels) { return pixels / (size_t)min_pixels + 1; }

// Where everything of a call lies.  The device block: the upload [FrameDesc F | pixels], the scratch [link bytes | counts | chunk counts
// | Comp], the result block [FrameOut F | segments | length | thickness | strength | pixels | label | label planes].  The label planes
// are the labelling's parents themselves and lie last, so that a call that wants none downloads the block without them.  The host block:
// the upload, then the result block - with the label planes only when `labels` is set.
struct CallLayout {
  size_t off_pixels = 0, in_bytes = 0;
  size_t off_links = 0, off_count = 0, off_chunks = 0, off_comp = 0;
  size_t off_out = 0;
  size_t o_segments = 0, o_length = 0, o_thickness = 0, o_strength = 0, o_npix = 0, o_label = 0, o_labels = 0;      // within the result block
  size_t out_bytes = 0, out_bytes_labels = 0;          // of the result block without / with the label planes
  slslam::BlockBytes bytes;
};

// F frames of `pixels` plane elements (the sum of align_chunk(width height)) and `comps` component slots in all, S segments a frame
inline CallLayout call_layout(size_t F, size_t pixels, size_t comps, size_t S, bool labels) {
  CallLayout y;
  slslam::Carve c;
  c.take(sizeof(FrameDesc) * F);
  y.off_pixels = c.take(pixels);
  y.in_bytes = c.at;
  y.off_links = c.take(pixels);
  y.off_count = c.take(4 * pixels);
  y.off_chunks = c.take(8 * (pixels / (size_t)kChunk));
  y.off_comp = c.take(sizeof(Comp) * comps);
  y.off_out = c.at;
  slslam::Carve o;
  o.take(sizeof(FrameOut) * F);
  y.o_segments = o.take(16 * F * S);
  y.o_length = o.take(8 * F * S);
  y.o_thickness = o.take(8 * F * S);
  y.o_strength = o.take(8 * F * S);
  y.o_npix = o.take(4 * F * S);
  y.o_label = o.take(4 * F * S);
  y.out_bytes = o.at;
  y.o_labels = o.take(4 * pixels);
  y.out_bytes_labels = o.at;
  y.bytes.dev = y.off_out + y.out_bytes_labels;
  y.bytes.host = y.in_bytes + (labels ? y.out_bytes_labels : y.out_bytes);
  return y;
}

}  // namespace slslam_lsd

#endif  // SLSLAM_LINE_DETECT_LAYOUT_H_

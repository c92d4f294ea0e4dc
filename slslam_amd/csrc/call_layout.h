// slslam_amd/csrc/call_layout.h — where things lie in the one block a call uploads, works in and downloads: the builder every layout is
// made with, the result block the matchers (mutual_match.h) share, with its scatter into the caller's arrays, the image copy of the
// detector and the descriptor, and the limits, validation and upload of a gated problem (stereo matcher, tracker).  Plain C++ with
// no HIP in it, so that tests/host_cxx/call_block_check.cpp checks it on the host; the HIP half is call_block.h.  Internal: not part of
// the C ABI.
#ifndef SLSLAM_CALL_LAYOUT_H_
#define SLSLAM_CALL_LAYOUT_H_

#include <cmath>
#include <cstddef>
#include <cstring>

namespace slslam {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Regions one behind the other, each at a multiple of 256 bytes: no offset is written as a sum of the one before it
struct Carve {
  size_t at = 0;                        // the next region's offset; after the last take, the bytes of them all
  size_t take(size_t bytes) {
    const size_t off = at;
    at += align256(bytes);
    return off;
  }
};

// What a call's layout asks of the handle's device block and of its page-locked mirror
struct BlockBytes {
  size_t dev = 0, host = 0;
};

// One matching problem among those of a call: n rows (observations, query descriptors) against m columns (map lines, keyframe descriptors)
struct Span {
  long long a0, j0;                     // its first row / column among those of all problems
  int n, m;
};

// The matchers' result block, the same offsets on the device and on the host: num_matched [P] at 0, five arrays over all rows, one over
// all columns
struct MatchBlock {
  size_t o_match = 0, o_best = 0, o_count = 0, o_best_value = 0, o_second_value = 0, o_best_row = 0, bytes = 0;
};

inline MatchBlock match_block(size_t P, size_t rows, size_t cols) {
  MatchBlock b;
  Carve c;
  c.take(4 * P);
  b.o_match = c.take(4 * rows);
  b.o_best = c.take(4 * rows);
  b.o_count = c.take(4 * rows);
  b.o_best_value = c.take(4 * rows);
  b.o_second_value = c.take(4 * rows);
  b.o_best_row = c.take(4 * cols);
  b.bytes = c.at;
  return b;
}

// The caller's arrays of one problem, any of them may be NULL: the tail of slslam_match_result and of slslam_descriptor_result
struct MatchArrays {
  int *match, *best;                    // [n]
  float *best_value, *second_value;     // [n]
  int* num_admissible;                  // [n]
  int* best_row;                        // [m]
};

// Problem p's part of the downloaded block into the caller's arrays; returns its num_matched
inline int match_scatter(const char* h_out, const MatchBlock& b, size_t p, const Span& s, const MatchArrays& r) {
  const size_t nb = 4 * (size_t)s.n, no = 4 * (size_t)s.a0;
  if (r.match && s.n > 0) std::memcpy(r.match, h_out + b.o_match + no, nb);
  if (r.best && s.n > 0) std::memcpy(r.best, h_out + b.o_best + no, nb);
  if (r.num_admissible && s.n > 0) std::memcpy(r.num_admissible, h_out + b.o_count + no, nb);
  if (r.best_value && s.n > 0) std::memcpy(r.best_value, h_out + b.o_best_value + no, nb);
  if (r.second_value && s.n > 0) std::memcpy(r.second_value, h_out + b.o_second_value + no, nb);
  if (r.best_row && s.m > 0) std::memcpy(r.best_row, h_out + b.o_best_row + 4 * (size_t)s.j0, 4 * (size_t)s.m);
  int num_matched;
  std::memcpy(&num_matched, h_out + 4 * p, 4);
  return num_matched;
}

// An image into the upload with `width` bytes per row: the stride stays with the caller
inline void pack_rows(unsigned char* dst, const unsigned char* image, int width, int height, int stride) {
  for (int r = 0; r < height; ++r) std::memcpy(dst + (size_t)r * (size_t)width, image + (size_t)r * (size_t)stride, (size_t)width);
}

// ---- a gated problem (gated_pairs.h): segments with descriptors of D floats, rows against columns in groups of kGroup.  The stereo
// matcher and the line tracker take its limits and its validation by `using`.
namespace gated {

constexpr int kMaxD = 128, kMaxSegments = 512;
constexpr int kGroup = 8;                                // columns whose chains a lane carries at a time
constexpr int kMaxGroups = kMaxSegments / kGroup;        // 64: the groups of a problem are the bits of one 64-bit word

inline bool shape_valid(int D, int max_frames, int max_segments) {
  return D >= 8 && D <= kMaxD && D % 8 == 0 && max_frames >= 1 && max_segments >= 1 && max_segments <= kMaxSegments;
}

// valid: the four floats and the D descriptor floats are finite
inline int segment_ok(const float* seg, const float* desc, int D) {
  for (int q = 0; q < 4; ++q)
    if (!std::isfinite(seg[q])) return 0;
  for (int i = 0; i < D; ++i)
    if (!std::isfinite(desc[i])) return 0;
  return 1;
}

// n segments and their descriptors to places a0 .. a0 + n - 1 of the upload's regions, with their flags
inline void fill_side(float* seg, float* desc, int* ok, size_t a0, const float* src_seg, const float* src_desc, size_t n, int D) {
  if (n == 0) return;
  std::memcpy(seg + 4 * a0, src_seg, 16 * n);
  std::memcpy(desc + a0 * (size_t)D, src_desc, 4 * n * (size_t)D);
  for (size_t i = 0; i < n; ++i) ok[a0 + i] = segment_ok(src_seg + 4 * i, src_desc + i * (size_t)D, D);
}

}  // namespace gated

}  // namespace slslam

#endif  // SLSLAM_CALL_LAYOUT_H_

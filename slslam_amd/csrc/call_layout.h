// slslam_amd/csrc/call_layout.h — where things lie in the one block a call uploads, works in and downloads: the builder every layout is
// made with, and the result block the two matchers (mutual_match.h) share, with its scatter into the caller's arrays.  Plain C++ with
// no HIP in it, so that tests/host_cxx/call_block_check.cpp checks it on the host; the HIP half is call_block.h.  Internal: not part of
// the C ABI.
#ifndef SLSLAM_CALL_LAYOUT_H_
#define SLSLAM_CALL_LAYOUT_H_

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

}  // namespace slslam

#endif  // SLSLAM_CALL_LAYOUT_H_

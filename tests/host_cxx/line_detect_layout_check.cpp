// tests/host_cxx/line_detect_layout_check.cpp — the host half of the line segment detector (slslam_amd/csrc/line_detect_layout.h) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_line_detect_cpu.py: the validation of options, frames and
// capacities at their limits, and the call's layout, filled the way a run fills it (a write past a region is an error the sanitizer
// sees).  Arguments: min_pixels, max_segments, then "width height" per frame; it prints the frames' descriptors ("frame first comp0
// width height comp_cap chunk0") and the sizes ("size name bytes") for the test to compare with the layout computed in numpy.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/line_detect_layout.h"

using namespace slslam_lsd;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main(int argc, char** argv) {
  // ---- options
  const Options good{24, 11, 64, 12, 10.0, 3.0, 512};
  CHECK(options_valid(good));
  CHECK(options_valid(Options{1, 0, 1, 1, 0.0, 0.0, 1}) && options_valid(Options{kMaxThreshold, kMaxTolerance, kMaxTolerance, 1 << 30, 1e9, 1e9, kMaxSegments}));
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Options o = good; o.grad_threshold = 0; CHECK(!options_valid(o));
  o = good; o.grad_threshold = kMaxThreshold + 1; CHECK(!options_valid(o));
  o = good; o.tol_num = -1; CHECK(!options_valid(o));
  o = good; o.tol_num = kMaxTolerance + 1; CHECK(!options_valid(o));
  o = good; o.tol_den = 0; CHECK(!options_valid(o));
  o = good; o.tol_den = kMaxTolerance + 1; CHECK(!options_valid(o));
  o = good; o.min_pixels = 0; CHECK(!options_valid(o));
  o = good; o.min_length = -1.0; CHECK(!options_valid(o));
  o = good; o.min_length = nan; CHECK(!options_valid(o));
  o = good; o.min_length = inf; CHECK(!options_valid(o));
  o = good; o.max_thickness = -1.0; CHECK(!options_valid(o));
  o = good; o.max_thickness = nan; CHECK(!options_valid(o));
  o = good; o.max_thickness = inf; CHECK(!options_valid(o));
  o = good; o.max_segments = 0; CHECK(!options_valid(o));
  o = good; o.max_segments = kMaxSegments + 1; CHECK(!options_valid(o));
  // the largest terms of a link test stay inside 64 bits: tol x (2 x 255^2)^2
  CHECK((long double)kMaxTolerance * 130050.0L * 130050.0L < 9.2e18L);
  // ... and so do the sums of a component of a whole 8192 x 8192 image: w <= 360, u^2 <= 8191^2
  CHECK(360.0L * 8191.0L * 8191.0L * 8192.0L * 8192.0L < 9.2e18L);

  // ---- frames and capacities
  unsigned char px[4] = {0, 0, 0, 0};
  CHECK(frame_valid(2, 2, 2, px) && frame_valid(2, 2, 100, px) && frame_valid(kMaxSide, kMaxSide, kMaxSide, px) && frame_valid(1, 1, 1, px));
  CHECK(!frame_valid(0, 2, 2, px) && !frame_valid(2, 0, 2, px) && !frame_valid(kMaxSide + 1, 2, kMaxSide + 1, px));
  CHECK(!frame_valid(2, kMaxSide + 1, 2, px) && !frame_valid(2, 2, 1, px) && !frame_valid(2, 2, 2, nullptr));
  CHECK(capacity_valid(1, 1, 1) && capacity_valid(16, (long long)kMaxSide * kMaxSide, kMaxSegments));
  CHECK(!capacity_valid(0, 1, 1) && !capacity_valid(1, 0, 1) && !capacity_valid(1, (long long)kMaxSide * kMaxSide + 1, 1));
  CHECK(!capacity_valid(17, (long long)kMaxSide * kMaxSide, 1) && !capacity_valid(17, 100, kMaxSegments));
  CHECK(align_chunk(0) == 0 && align_chunk(1) == (size_t)kChunk && align_chunk(kChunk) == (size_t)kChunk && align_chunk(kChunk + 1) == 2 * (size_t)kChunk);
  CHECK(comp_capacity(11, 12) == 1 && comp_capacity(12, 12) == 2 && comp_capacity(100, 1) == 101);
  CHECK(kTile * kTile == kChunk && kChunk % kBlock == 0 && kChunk / kBlock == 4);
  CHECK(sizeof(Comp) == 128 && sizeof(FrameOut) == 48 && sizeof(FrameDesc) == 32);

  // ---- the layout of the frames given
  CHECK(argc >= 4);
  const int min_pixels = std::atoi(argv[1]);
  const size_t S = (size_t)std::atoi(argv[2]), F = (size_t)(argc - 3);
  CHECK(min_pixels >= 1 && S >= 1);
  std::vector<FrameDesc> fd(F);
  size_t pixels = 0, comps = 0;
  for (size_t f = 0; f < F; ++f) {
    int w = 0, h = 0;
    CHECK(std::sscanf(argv[3 + f], "%d %d", &w, &h) == 2 && frame_valid(w, h, w, px));
    const size_t n = (size_t)w * (size_t)h;
    fd[f] = FrameDesc{(long long)pixels, (long long)comps, w, h, (int)comp_capacity(n, min_pixels), (int)(pixels / kChunk)};
    // a frame cannot have more fitted components than slots: each has at least min_pixels pixels
    CHECK((size_t)fd[f].comp_cap * (size_t)min_pixels > n);
    pixels += align_chunk(n);
    comps += comp_capacity(n, min_pixels);
    std::printf("frame %lld %lld %d %d %d %d\n", fd[f].first, fd[f].comp0, fd[f].width, fd[f].height, fd[f].comp_cap, fd[f].chunk0);
  }
  const CallLayout y = call_layout(F, pixels, comps, S, false), z = call_layout(F, pixels, comps, S, true);
  // regions in order, each at a multiple of 256 bytes, none overlapping; the label planes last
  CHECK(y.off_pixels >= sizeof(FrameDesc) * F && y.in_bytes >= y.off_pixels + pixels && y.off_links == y.in_bytes);
  CHECK(y.off_count >= y.off_links + pixels && y.off_chunks >= y.off_count + 4 * pixels && y.off_comp >= y.off_chunks + 8 * (pixels / kChunk));
  CHECK(y.off_out >= y.off_comp + sizeof(Comp) * comps);
  CHECK(y.o_segments >= sizeof(FrameOut) * F && y.o_length >= y.o_segments + 16 * F * S && y.o_thickness >= y.o_length + 8 * F * S);
  CHECK(y.o_strength >= y.o_thickness + 8 * F * S && y.o_npix >= y.o_strength + 8 * F * S && y.o_label >= y.o_npix + 4 * F * S);
  CHECK(y.out_bytes >= y.o_label + 4 * F * S && y.o_labels == y.out_bytes && y.out_bytes_labels >= y.o_labels + 4 * pixels);
  for (size_t off : {y.off_pixels, y.in_bytes, y.off_links, y.off_count, y.off_chunks, y.off_comp, y.off_out, y.o_segments, y.o_length,
                     y.o_thickness, y.o_strength, y.o_npix, y.o_label, y.o_labels, y.out_bytes_labels})
    CHECK(off % 256 == 0);
  CHECK(y.bytes.dev == y.off_out + y.out_bytes_labels && z.bytes.dev == y.bytes.dev);
  CHECK(y.bytes.host == y.in_bytes + y.out_bytes && z.bytes.host == y.in_bytes + y.out_bytes_labels && z.off_out == y.off_out);
  std::printf("size in_bytes %zu\nsize out_bytes %zu\nsize out_bytes_labels %zu\nsize dev %zu\nsize host %zu\nsize host_labels %zu\n", y.in_bytes,
              y.out_bytes, y.out_bytes_labels, y.bytes.dev, y.bytes.host, z.bytes.host);

  // the host block as a run fills and reads it: the descriptors, every frame's pixels, every frame's part of every result array
  std::vector<char> block(z.bytes.host);
  std::memcpy(block.data(), fd.data(), sizeof(FrameDesc) * F);
  char* ho = block.data() + z.in_bytes;
  for (size_t f = 0; f < F; ++f) {
    const size_t n = (size_t)fd[f].width * (size_t)fd[f].height;
    std::memset(block.data() + z.off_pixels + fd[f].first, 1, n);
    reinterpret_cast<FrameOut*>(ho)[f] = FrameOut{};
    std::memset(ho + z.o_segments + 16 * f * S, 2, 16 * S);
    std::memset(ho + z.o_length + 8 * f * S, 3, 8 * S);
    std::memset(ho + z.o_thickness + 8 * f * S, 4, 8 * S);
    std::memset(ho + z.o_strength + 8 * f * S, 5, 8 * S);
    std::memset(ho + z.o_npix + 4 * f * S, 6, 4 * S);
    std::memset(ho + z.o_label + 4 * f * S, 7, 4 * S);
    std::memset(ho + z.o_labels + 4 * (size_t)fd[f].first, 8, 4 * n);
  }
  CHECK(block[z.off_pixels + pixels - 1] == 0 || block[z.off_pixels + pixels - 1] == 1);
  CHECK(ho[z.o_segments - 1] == 0 && ho[z.o_segments] == 2);

  std::printf("line detect layout ok\n");
  return 0;
}

// tests/host_cxx/line_descriptor_layout_check.cpp — the host half of the MSLD line descriptor (slslam_amd/csrc/line_descriptor_layout.h)
// as a stand-alone program, built with -fsanitize=address,undefined by tests/test_line_descriptor_cpu.py: the validation of options,
// frames and segments, the weight table at its limits (written into an array of exactly M w rows, so that a row too many is an error
// the sanitizer sees), and the call's layout.  Arguments: "M w" pairs; it prints their tables ("row M w r wa wb f band") and the
// statuses of the test's segment list ("segment status N") for the test to compare with the numpy reference.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/line_descriptor_layout.h"

using namespace slslam_msld;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main(int argc, char** argv) {
  // ---- options
  CHECK(options_valid(9, 5, 1) && options_valid(1, 1, 0) && options_valid(16, 9, 1));
  CHECK(!options_valid(0, 5, 1) && !options_valid(17, 1, 1) && !options_valid(9, 0, 1) && !options_valid(9, 10, 1));
  CHECK(!options_valid(9, 5, 2) && !options_valid(9, 5, -1));
  CHECK(kMaxBands * kMaxBandWidth == kMaxRows);

  // ---- every table: M w rows and no more, bands from -1 (0 at w = 1) to M - 1 rising by at most 1, weights in [0, 1] that sum to f,
  // symmetric about the middle row
  for (int m = 1; m <= kMaxBands; ++m)
    for (int w = 1; w <= kMaxBandWidth; ++w) {
      std::vector<WeightRow> t((size_t)(m * w));
      CHECK(weight_table(m, w, t.data()) == m * w);
      const int rows = m * w;
      CHECK(t[0].band == (w == 1 ? 0 : -1) && t[(size_t)rows - 1].band == m - 1);
      for (int r = 0; r < rows; ++r) {
        const WeightRow& a = t[(size_t)r];
        const WeightRow& b = t[(size_t)(rows - 1 - r)];
        CHECK(a.wa >= 0.f && a.wb >= 0.f && a.f > 0.f && a.f <= 1.f);
        CHECK(std::fabs((double)a.wa + (double)a.wb - (double)a.f) <= 1e-7);
        CHECK(a.f == b.f);
        if (a.wb == 0.f && b.wb == 0.f)                   // a row in the middle of its band, and so is its mirror image
          CHECK(a.wa == b.wa && a.band + b.band == m - 1);
        else
          CHECK(std::fabs((double)a.wa - (double)b.wb) <= 1e-7 && a.band + b.band == m - 2);
        if (r > 0) CHECK(a.band - t[(size_t)r - 1].band == 0 || a.band - t[(size_t)r - 1].band == 1);
      }
      if (rows % 2 == 1) CHECK(t[(size_t)rows / 2].f == 1.f);
    }
  for (int i = 1; i < argc; ++i) {
    int m = 0, w = 0;
    CHECK(std::sscanf(argv[i], "%d %d", &m, &w) == 2 && options_valid(m, w, 1));
    std::vector<WeightRow> t((size_t)(m * w));
    weight_table(m, w, t.data());
    for (int r = 0; r < m * w; ++r)
      std::printf("row %d %d %d %.9g %.9g %.9g %d\n", m, w, r, (double)t[(size_t)r].wa, (double)t[(size_t)r].wb, (double)t[(size_t)r].f,
                  t[(size_t)r].band);
  }

  // ---- frames
  unsigned char px[4] = {0, 0, 0, 0};
  float sg[4] = {0, 0, 1, 1};
  CHECK(frame_valid(2, 2, 2, px, 1, sg) && frame_valid(2, 2, 100, px, 0, nullptr) && frame_valid(kMaxSide, kMaxSide, kMaxSide, px, 0, nullptr));
  CHECK(!frame_valid(0, 2, 2, px, 0, nullptr) && !frame_valid(2, 0, 2, px, 0, nullptr) && !frame_valid(kMaxSide + 1, 2, kMaxSide + 1, px, 0, nullptr));
  CHECK(!frame_valid(2, kMaxSide + 1, 2, px, 0, nullptr) && !frame_valid(2, 2, 1, px, 0, nullptr) && !frame_valid(2, 2, 2, nullptr, 0, nullptr));
  CHECK(!frame_valid(2, 2, 2, px, -1, sg) && !frame_valid(2, 2, 2, px, 1, nullptr));

  // ---- segments of a 16 x 12 image: the list of tests/test_line_descriptor_cpu.py (STATUS_SEGMENTS), in its order
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float segs[][4] = {
      {2, 3, 12, 3}, {2, 3, std::nextafterf(12.f, 0.f), 3}, {2, 3, std::nextafterf(12.f, 99.f), 3}, {2, 3, 4, 3},
      {2, 3, std::nextafterf(4.f, 0.f), 3}, {5, 5, 5, 5}, {0, 0, 15, 11}, {-0.01f, 3, 9, 3}, {2, 3, 15.01f, 3}, {2, 3, 9, 11.5f},
      {2, -1, 2, -1}, {2, 3, nan, 3}, {inf, 3, 9, 3}, {-5, nan, 9, 3}};
  for (const auto& s : segs) {
    double length = -1.0;
    int n = -1;
    const int st = segment_status(16, 12, s, &length, &n);
    CHECK((st == kOk) == (n >= 2) && (st == kOk || n == 0) && length >= 0.0);
    if (st == kOk) CHECK(n == (int)std::floor(length) && length >= 2.0);
    std::printf("segment %d %d\n", st, n);
  }

  // ---- the layout: regions in order, each at a multiple of 256 bytes, none overlapping, the result block behind the upload
  const size_t F = 3, S = 131, rows = 45, pixels = 64 * 48 + 320 * 240 + 97 * 33 + 700, D = 72;
  const CallLayout y = call_layout(F, S, rows, pixels, D);
  CHECK(y.off_seg >= sizeof(FrameDesc) * F && y.off_table >= y.off_seg + sizeof(SegDesc) * S);
  CHECK(y.off_pixels >= y.off_table + sizeof(WeightRow) * rows && y.in_bytes >= y.off_pixels + pixels && y.off_out == y.in_bytes);
  CHECK(y.o_status >= 4 * S * D && y.o_samples >= y.o_status + 4 * S && y.o_polarity >= y.o_samples + 4 * S && y.out_bytes >= y.o_polarity + 4 * S);
  for (size_t off : {y.off_seg, y.off_table, y.off_pixels, y.off_out, y.o_status, y.o_samples, y.o_polarity, y.out_bytes}) CHECK(off % 256 == 0);
  CHECK(y.bytes.dev == y.off_out + y.out_bytes && y.bytes.host == y.bytes.dev);
  const CallLayout z = call_layout(0, 0, rows, 0, D);
  CHECK(z.out_bytes == 0 && z.bytes.dev == z.off_out);
  CHECK(sizeof(SegDesc) == 40 && sizeof(FrameDesc) == 16 && sizeof(WeightRow) == 16);

  // the blocks as a run fills them: every descriptor inside its region (the sanitizer sees a write past it)
  std::vector<char> block(y.bytes.host);
  FrameDesc* fd = reinterpret_cast<FrameDesc*>(block.data());
  SegDesc* sd = reinterpret_cast<SegDesc*>(block.data() + y.off_seg);
  for (size_t f = 0; f < F; ++f) fd[f] = FrameDesc{(long long)f, 1, 1};
  for (size_t k = 0; k < S; ++k) sd[k] = SegDesc{0, 0, 1, 1, 1.5, 0, 0, kTooShort, 0};
  weight_table(9, 5, reinterpret_cast<WeightRow*>(block.data() + y.off_table));
  block[y.off_pixels + pixels - 1] = 1;
  block[y.off_out + y.out_bytes - 1] = 1;

  std::printf("line descriptor layout ok\n");
  return 0;
}

// tests/host_cxx/stereo_match_layout_check.cpp — the host half of the stereo line matcher (slslam_amd/csrc/stereo_match_layout.h) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_stereo_match_cpu.py: the validation of options, shapes,
// frames and segments, the call's layout (its offsets are printed, "layout F A J D name offset ...", for the test to compare with its
// own restatement), and the contract's arithmetic - the very functions the kernels call - on the pairs of the file named by the first
// argument.  Its lines: "gate min_disparity max_disparity max_tan2 min_rows min_overlap fx fy cx cy", then "pair" and the eight floats of
// a left and a right segment; numbers as C hexadecimal floats.  Per pair it prints "pair <admits> <status of the left segment alone>
// obs[8] disp[2]" in hexadecimal, which the test compares with tests/stereo_match_reference.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/stereo_match_layout.h"

using namespace slslam_stereo;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                      \
    }                                                                \
  } while (0)

static slslam_stereo_match_options good() {
  return slslam_stereo_match_options{0.0, 128.0, 0.03, 3.0, 0.5, 1.5, 0.25, 1.0, 1.0, 0.0, 0.0};
}

int main(int argc, char** argv) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- options
  slslam_stereo_match_options o = good();
  CHECK(options_valid(&o) && !options_valid(nullptr));
  o = good(); o.min_disparity = 129.0; CHECK(!options_valid(&o));
  o = good(); o.min_disparity = o.max_disparity = 5.0; CHECK(options_valid(&o));
  o = good(); o.min_disparity = -inf; CHECK(!options_valid(&o));
  o = good(); o.max_disparity = inf; CHECK(!options_valid(&o));
  o = good(); o.max_tan2 = -1e-9; CHECK(!options_valid(&o));
  o = good(); o.max_tan2 = nan; CHECK(!options_valid(&o));
  o = good(); o.max_tan2 = 0.0; CHECK(options_valid(&o));
  o = good(); o.min_rows = -1.0; CHECK(!options_valid(&o));
  o = good(); o.min_rows = 0.0; CHECK(options_valid(&o));
  o = good(); o.min_overlap = 1.5; CHECK(!options_valid(&o));
  o = good(); o.min_overlap = -0.1; CHECK(!options_valid(&o));
  o = good(); o.min_overlap = 1.0; CHECK(options_valid(&o));
  o = good(); o.ratio = nan; CHECK(!options_valid(&o));
  o = good(); o.ratio = 0.0; o.max_distance = inf; CHECK(options_valid(&o));
  o = good(); o.max_distance = nan; CHECK(!options_valid(&o));
  o = good(); o.fx = 0.0; CHECK(!options_valid(&o));
  o = good(); o.fy = inf; CHECK(!options_valid(&o));
  o = good(); o.cx = nan; CHECK(!options_valid(&o));
  o = good(); o.fx = -406.05; o.cy = -3.0; CHECK(options_valid(&o));

  // ---- shapes, frames, segments
  CHECK(shape_valid(8, 1, 1) && shape_valid(72, 64, 512) && shape_valid(128, 1, 512));
  CHECK(!shape_valid(0, 1, 1) && !shape_valid(12, 1, 1) && !shape_valid(136, 1, 1) && !shape_valid(72, 0, 1) && !shape_valid(72, 1, 0) &&
        !shape_valid(72, 1, 513));
  float seg[8] = {0, 0, 1, 1, 2, 2, 3, 3}, desc[16] = {0};
  slslam_stereo_frame f{2, seg, desc, 1, seg, desc};
  CHECK(frame_valid(f, 2) && !frame_valid(f, 1));
  f.num_left = -1; CHECK(!frame_valid(f, 2));
  f = slslam_stereo_frame{2, nullptr, desc, 1, seg, desc}; CHECK(!frame_valid(f, 2));
  f = slslam_stereo_frame{2, seg, nullptr, 1, seg, desc}; CHECK(!frame_valid(f, 2));
  f = slslam_stereo_frame{2, seg, desc, 1, nullptr, desc}; CHECK(!frame_valid(f, 2));
  f = slslam_stereo_frame{2, seg, desc, 1, seg, nullptr}; CHECK(!frame_valid(f, 2));
  f = slslam_stereo_frame{0, nullptr, nullptr, 0, nullptr, nullptr}; CHECK(frame_valid(f, 1));
  f = slslam_stereo_frame{0, nullptr, nullptr, 3, seg, desc}; CHECK(!frame_valid(f, 2));
  {
    std::vector<float> s4(4, 1.0f), d8(8, 0.5f);                   // exactly D floats: a read past them is an error the sanitizer sees
    CHECK(segment_ok(s4.data(), d8.data(), 8) == 1);
    d8[7] = std::numeric_limits<float>::infinity(); CHECK(segment_ok(s4.data(), d8.data(), 8) == 0);
    d8[7] = 0.0f; s4[3] = std::numeric_limits<float>::quiet_NaN(); CHECK(segment_ok(s4.data(), d8.data(), 8) == 0);
  }

  // ---- the layout: regions in order, each at a multiple of 256 bytes, none overlapping; the result block behind the upload on the
  // host, behind the keys on the device
  const size_t shapes[][4] = {{3, 131, 97, 72}, {1, 512, 512, 128}, {2, 0, 0, 8}, {64, 64 * 300, 64 * 300, 72}};
  for (const auto& sh : shapes) {
    const size_t F = sh[0], A = sh[1], J = sh[2], D = sh[3];
    const CallLayout y = call_layout(F, A, J, D);
    CHECK(y.off_lseg >= sizeof(FrameDesc) * F && y.off_rseg >= y.off_lseg + 16 * A && y.off_lok >= y.off_rseg + 16 * J);
    CHECK(y.off_rok >= y.off_lok + 4 * A && y.off_ldesc >= y.off_rok + 4 * J && y.off_rdesc >= y.off_ldesc + 4 * A * D);
    CHECK(y.in_bytes >= y.off_rdesc + 4 * J * D && y.off_keys == y.in_bytes && y.off_out >= y.off_keys + 8 * J);
    CHECK(y.o_status >= y.out.bytes && y.o_obs >= y.o_status + 4 * A && y.o_disp >= y.o_obs + 64 * A && y.out_bytes >= y.o_disp + 16 * A);
    for (size_t off : {y.off_lseg, y.off_rseg, y.off_lok, y.off_rok, y.off_ldesc, y.off_rdesc, y.in_bytes, y.off_keys, y.off_out, y.o_status,
                       y.o_obs, y.o_disp, y.out_bytes})
      CHECK(off % 256 == 0);
    CHECK(y.bytes.host == y.in_bytes + y.out_bytes && y.bytes.dev == y.off_out + y.out_bytes);
    std::printf("layout %zu %zu %zu %zu lseg %zu rseg %zu lok %zu rok %zu ldesc %zu rdesc %zu in %zu keys %zu out %zu status %zu obs %zu disp %zu "
                "out_bytes %zu host %zu dev %zu\n", F, A, J, D, y.off_lseg, y.off_rseg, y.off_lok, y.off_rok, y.off_ldesc, y.off_rdesc,
                y.in_bytes, y.off_keys, y.off_out, y.o_status, y.o_obs, y.o_disp, y.out_bytes, y.bytes.host, y.bytes.dev);
    if (F > 3) continue;
    // the host block as a run fills it: the last byte of every region (the sanitizer sees a write past the block)
    std::vector<char> block(y.bytes.host);
    FrameDesc* fd = reinterpret_cast<FrameDesc*>(block.data());
    for (size_t i = 0; i < F; ++i) fd[i].span = slslam::Span{0, 0, 0, 0};
    if (A > 0) block[y.off_ldesc + 4 * A * D - 1] = 1;
    if (J > 0) block[y.off_rdesc + 4 * J * D - 1] = 1;
    if (A > 0) block[y.in_bytes + y.o_disp + 16 * A - 1] = 1;
    block[y.in_bytes + y.out_bytes - 1] = 1;
  }
  CHECK(sizeof(FrameDesc) == 24);

  // ---- the contract's arithmetic on the test's pairs
  if (argc > 1) {
    std::FILE* in = std::fopen(argv[1], "r");
    CHECK(in != nullptr);
    char line[1024];
    Gate g = gate_of(good());
    Camera cam = camera_of(good());
    while (std::fgets(line, sizeof line, in)) {
      char* p = line;
      char* word = std::strtok(p, " \n");
      if (!word) continue;
      double v[9];
      const int want = std::strcmp(word, "gate") == 0 ? 9 : 8;
      for (int i = 0; i < want; ++i) {
        const char* t = std::strtok(nullptr, " \n");
        CHECK(t != nullptr);
        v[i] = std::strtod(t, nullptr);
      }
      if (want == 9) {
        g = Gate{v[0], v[1], v[2], v[3], v[4], inf};
        cam = Camera{v[5], v[6], v[7], v[8]};
        continue;
      }
      const Segment a = segment_of((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
      const Segment b = segment_of((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
      // the staged slope gives the same segment
      const Segment b2 = segment_with((float)v[4], (float)v[5], (float)v[6], (float)v[7], slope_of((float)v[4], (float)v[5], (float)v[6], (float)v[7]));
      CHECK(std::memcmp(&b, &b2, sizeof b) == 0);
      const bool adm = gate_admits(a, b, g);
      double obs[8] = {0}, disp[2] = {0};
      if (adm) emit_row(a, b, cam, obs, disp);
      std::printf("pair %d %d", adm ? 1 : 0, status_of(1, a, g, adm ? 0 : -1));
      for (double x : obs) std::printf(" %a", x);
      std::printf(" %a %a\n", disp[0], disp[1]);
    }
    std::fclose(in);
  }
  std::printf("stereo match layout ok\n");
  return 0;
}

// tests/host_cxx/line_track_layout_check.cpp — the host half of the line tracker (slslam_amd/csrc/line_track_layout.h) as a stand-alone
// program, built with -fsanitize=address,undefined by tests/test_line_track_cpu.py: the validation of options, shapes and frames, the
// run's layout (its offsets are printed, "layout F S D name offset ...", for the test to compare with its own restatement), and the
// contract's arithmetic - the very functions the kernels call - on the file named by the first argument.  Its lines, numbers as C
// hexadecimal floats: "gate max_tan2 max_shift max_offset min_overlap min_length predict[6]", then "pair" and the four floats of a row
// and of a column: printed is "pair <admits> <the row is short>".  "ids next_id C T id age ..." (the carried frame) followed by T
// lines "frame n status match ...": printed per frame is "idage id age ...", the id rule over regions laid out as a run lays them out.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../slslam_amd/csrc/line_track_layout.h"

using namespace slslam_track;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                      \
    }                                                                \
  } while (0)

static slslam_line_track_options good() { return slslam_line_track_options{0.03, 40.0, 12.0, 0.5, 8.0, 1.5, 0.25}; }

static int run_ids(std::FILE* in, char* first) {
  // the regions of a run: [carried | frame 0 | ...]
  std::strtok(first, " \n");
  const int next_id = std::atoi(std::strtok(nullptr, " \n")), C = std::atoi(std::strtok(nullptr, " \n")), T = std::atoi(std::strtok(nullptr, " \n"));
  std::vector<int> status((size_t)C, -1), match((size_t)C, -1), rank((size_t)C, 0), id((size_t)C), age((size_t)C);
  for (int i = 0; i < C; ++i) {
    id[(size_t)i] = std::atoi(std::strtok(nullptr, " \n"));
    age[(size_t)i] = std::atoi(std::strtok(nullptr, " \n"));
  }
  std::vector<FrameDesc> fd((size_t)T);
  std::vector<int> new_before((size_t)T + 1, 0);
  long long prev0 = 0;
  int prevn = C;
  std::vector<char> line(1 << 16);
  for (int t = 0; t < T; ++t) {
    CHECK(std::fgets(line.data(), (int)line.size(), in) != nullptr);
    CHECK(std::strcmp(std::strtok(line.data(), " \n"), "frame") == 0);
    const int n = std::atoi(std::strtok(nullptr, " \n"));
    fd[(size_t)t].span = slslam::Span{(long long)status.size(), prev0, n, prevn};
    fd[(size_t)t].warp = warp_of(nullptr);
    prev0 = (long long)status.size(); prevn = n;
    int fresh = 0;
    for (int a = 0; a < n; ++a) {
      const int st = std::atoi(std::strtok(nullptr, " \n")), m = std::atoi(std::strtok(nullptr, " \n"));
      CHECK(status_of(st != kInvalid, st == kShort, m) == st);
      status.push_back(st); match.push_back(m); rank.push_back(fresh);
      id.push_back(-7); age.push_back(-7);
      if (st == kNew) ++fresh;
    }
    new_before[(size_t)t + 1] = new_before[(size_t)t] + fresh;
  }
  for (int t = 0; t < T; ++t) {
    std::string out = "idage";
    for (int a = 0; a < fd[(size_t)t].span.n; ++a) {
      const IdAge r = id_of(fd.data(), t, a, status.data(), match.data(), rank.data(), new_before.data(), id.data(), age.data(), next_id);
      out += " " + std::to_string(r.id) + " " + std::to_string(r.age);
    }
    std::printf("%s\n", out.c_str());
  }
  return 0;
}

int main(int argc, char** argv) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- options
  slslam_line_track_options o = good();
  CHECK(options_valid(&o) && !options_valid(nullptr));
  o = good(); o.max_tan2 = -1e-9; CHECK(!options_valid(&o));
  o = good(); o.max_tan2 = nan; CHECK(!options_valid(&o));
  o = good(); o.max_tan2 = 0.0; CHECK(options_valid(&o));
  o = good(); o.max_shift = -1.0; CHECK(!options_valid(&o));
  o = good(); o.max_shift = inf; CHECK(!options_valid(&o));
  o = good(); o.max_shift = 0.0; CHECK(options_valid(&o));
  o = good(); o.max_offset = -1.0; CHECK(!options_valid(&o));
  o = good(); o.max_offset = nan; CHECK(!options_valid(&o));
  o = good(); o.min_overlap = 1.5; CHECK(!options_valid(&o));
  o = good(); o.min_overlap = -0.1; CHECK(!options_valid(&o));
  o = good(); o.min_overlap = 1.0; CHECK(options_valid(&o));
  o = good(); o.min_length = -1.0; CHECK(!options_valid(&o));
  o = good(); o.min_length = inf; CHECK(!options_valid(&o));
  o = good(); o.ratio = nan; CHECK(!options_valid(&o));
  o = good(); o.ratio = 0.0; o.max_distance = inf; CHECK(options_valid(&o));
  o = good(); o.max_distance = nan; CHECK(!options_valid(&o));
  {
    const Gate g = gate_of(good());
    CHECK(g.max_shift2 == 1600.0 && g.max_offset2 == 144.0 && g.min_length2 == 64.0 && g.max_tan2 == 0.03 && g.max_distance == 0.25);
  }

  // ---- shapes, frames, segments, ids
  CHECK(shape_valid(8, 1, 1) && shape_valid(72, 64, 512) && shape_valid(128, 1, 512));
  CHECK(!shape_valid(0, 1, 1) && !shape_valid(12, 1, 1) && !shape_valid(136, 1, 1) && !shape_valid(72, 0, 1) && !shape_valid(72, 1, 0) &&
        !shape_valid(72, 1, 513));
  float seg[8] = {0, 0, 1, 1, 2, 2, 3, 3}, desc[16] = {0};
  double pre[6] = {1, 0, 3, 0, 1, -2};
  slslam_line_track_frame f{2, seg, desc, nullptr};
  CHECK(frame_valid(f, 2) && !frame_valid(f, 1));
  f.predict = pre; CHECK(frame_valid(f, 2));
  pre[5] = inf; CHECK(!frame_valid(f, 2));
  pre[5] = nan; CHECK(!frame_valid(f, 2));
  f = slslam_line_track_frame{-1, seg, desc, nullptr}; CHECK(!frame_valid(f, 2));
  f = slslam_line_track_frame{2, nullptr, desc, nullptr}; CHECK(!frame_valid(f, 2));
  f = slslam_line_track_frame{2, seg, nullptr, nullptr}; CHECK(!frame_valid(f, 2));
  f = slslam_line_track_frame{0, nullptr, nullptr, nullptr}; CHECK(frame_valid(f, 1));
  CHECK(ids_fit(0, 0) && ids_fit(INT_MAX, 0) && !ids_fit(INT_MAX, 1) && ids_fit(INT_MAX - 512, 512) && !ids_fit(INT_MAX - 512, 513) &&
        !ids_fit(-1, 0) && !ids_fit(0, (long long)INT_MAX + 1));
  {
    std::vector<float> s4(4, 1.0f), d8(8, 0.5f);                   // exactly D floats: a read past them is an error the sanitizer sees
    CHECK(segment_ok(s4.data(), d8.data(), 8) == 1);
    d8[7] = std::numeric_limits<float>::infinity(); CHECK(segment_ok(s4.data(), d8.data(), 8) == 0);
    d8[7] = 0.0f; s4[3] = std::numeric_limits<float>::quiet_NaN(); CHECK(segment_ok(s4.data(), d8.data(), 8) == 0);
  }
  CHECK(status_of(0, true, 3) == kInvalid && status_of(1, true, 3) == kShort && status_of(1, false, 0) == kContinued &&
        status_of(1, false, -1) == kNew);

  // ---- the layout: regions in order, each at a multiple of 256 bytes, none overlapping; the result block behind the upload on the
  // host, behind the keys on the device
  const size_t shapes[][3] = {{3, 131, 72}, {1, 1024, 128}, {2, 0, 8}, {512, 513 * 300, 72}};
  for (const auto& sh : shapes) {
    const size_t F = sh[0], S = sh[1], D = sh[2];
    const CallLayout y = call_layout(F, S, D);
    CHECK(y.off_seg >= sizeof(FrameDesc) * F && y.off_ok >= y.off_seg + 16 * S && y.off_desc >= y.off_ok + 4 * S);
    CHECK(y.in_bytes >= y.off_desc + 4 * S * D && y.off_keys == y.in_bytes && y.off_out >= y.off_keys + 8 * S);
    CHECK(y.o_status >= y.out.bytes && y.o_id >= y.o_status + 4 * S && y.o_age >= y.o_id + 4 * S && y.o_rank >= y.o_age + 4 * S);
    CHECK(y.o_new >= y.o_rank + 4 * S && y.o_before >= y.o_new + 4 * F && y.out_bytes >= y.o_before + 4 * (F + 1));
    for (size_t off : {y.off_seg, y.off_ok, y.off_desc, y.in_bytes, y.off_keys, y.off_out, y.o_status, y.o_id, y.o_age, y.o_rank, y.o_new,
                       y.o_before, y.out_bytes})
      CHECK(off % 256 == 0);
    CHECK(y.bytes.host == y.in_bytes + y.out_bytes && y.bytes.dev == y.off_out + y.out_bytes);
    std::printf("layout %zu %zu %zu seg %zu ok %zu desc %zu in %zu keys %zu out %zu status %zu id %zu age %zu rank %zu new %zu before %zu "
                "out_bytes %zu host %zu dev %zu\n", F, S, D, y.off_seg, y.off_ok, y.off_desc, y.in_bytes, y.off_keys, y.off_out, y.o_status,
                y.o_id, y.o_age, y.o_rank, y.o_new, y.o_before, y.out_bytes, y.bytes.host, y.bytes.dev);
    if (F > 3) continue;
    // the host block as a run fills it: the last byte of every region (the sanitizer sees a write past the block)
    std::vector<char> block(y.bytes.host);
    FrameDesc* fd = reinterpret_cast<FrameDesc*>(block.data());
    for (size_t i = 0; i < F; ++i) fd[i] = FrameDesc{slslam::Span{0, 0, 0, 0}, warp_of(nullptr)};
    if (S > 0) block[y.off_desc + 4 * S * D - 1] = 1;
    block[y.in_bytes + y.o_before + 4 * (F + 1) - 1] = 1;
    block[y.in_bytes + y.out_bytes - 1] = 1;
  }
  CHECK(sizeof(FrameDesc) == 72);
  {
    const CarryLayout c = carry_layout(512, 128);
    CHECK(c.off_seg == 0 && c.off_ok == 8192 && c.off_desc == 8192 + 2048 && c.off_id == c.off_desc + 512 * 512 &&
          c.off_age == c.off_id + 2048 && c.bytes == c.off_age + 2048);
  }

  // ---- the contract's arithmetic on the test's pairs and frames
  if (argc > 1) {
    std::FILE* in = std::fopen(argv[1], "r");
    CHECK(in != nullptr);
    std::vector<char> line(1 << 16);
    Gate g = gate_of(good());
    Warp w = warp_of(nullptr);
    while (std::fgets(line.data(), (int)line.size(), in)) {
      if (std::strncmp(line.data(), "ids ", 4) == 0) {
        if (run_ids(in, line.data()) != 0) return 1;
        continue;
      }
      char* word = std::strtok(line.data(), " \n");
      if (!word) continue;
      double v[11];
      const int want = std::strcmp(word, "gate") == 0 ? 11 : 8;
      for (int i = 0; i < want; ++i) {
        const char* t = std::strtok(nullptr, " \n");
        CHECK(t != nullptr);
        v[i] = std::strtod(t, nullptr);
      }
      if (want == 11) {
        slslam_line_track_options q{v[0], v[1], v[2], v[3], v[4], 1.5, inf};
        CHECK(options_valid(&q));
        g = gate_of(q);
        w = warp_of(v + 5);
        continue;
      }
      const Segment a = segment_of(ends_of((float)v[0], (float)v[1], (float)v[2], (float)v[3]));
      const Ends e = ends_of((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
      const Segment b = segment_of(warped(e, w));
      const bool adm = gate_admits(a, b, g);
      std::printf("pair %d %d\n", adm ? 1 : 0, is_short(a, g) ? 1 : 0);
    }
    std::fclose(in);
  }
  std::printf("line track layout ok\n");
  return 0;
}

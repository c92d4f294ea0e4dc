// tests/host_cxx/image_rectify_layout_check.cpp — the host half of the image rectifier (slslam_amd/csrc/image_rectify_layout.h) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_image_rectify_cpu.py: the validation of options, cameras,
// frames and capacities at their limits, the taps, slslam_stereo_rectify's construction, the map and the remap of a camera, and the
// call's layout, filled the way a run fills it (a write past a region is an error the sanitizer sees).  Arguments: the 22 doubles and 4
// sizes of a camera, then the camera index (0 or 1: the same camera twice) of every frame of a call.  It prints the map ("map qx qy
// valid sx sy", the doubles in hex), the frames ("frame src0 dst0 camera"), the sizes ("size name bytes") and the taps ("taps sigma
// radius t0 .. t7") for the test to compare with numpy and the library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/image_rectify_layout.h"

using namespace slslam_rect;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      return 1;                                                      \
    }                                                                \
  } while (0)

static Camera identity(int w, int h) {
  Camera c{};
  c.fx = c.fy = c.fx2 = c.fy2 = 1.0;
  c.R[0] = c.R[4] = c.R[8] = 1.0;
  c.src_width = c.dst_width = w;
  c.src_height = c.dst_height = h;
  return c;
}

int main(int argc, char** argv) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- options
  CHECK(options_valid(Options{kConstant, 0, 0.0}) && options_valid(Options{kReplicate, 255, kMaxSigma}));
  CHECK(!options_valid(Options{2, 0, 0.0}) && !options_valid(Options{-1, 0, 0.0}) && !options_valid(Options{0, 256, 0.0}));
  CHECK(!options_valid(Options{0, -1, 0.0}) && !options_valid(Options{0, 0, -0.1}) && !options_valid(Options{0, 0, nan}));
  CHECK(!options_valid(Options{0, 0, inf}) && !options_valid(Options{0, 0, kMaxSigma + 0.5}));

  // ---- cameras, frames, capacities
  Camera id = identity(16, 12);
  CHECK(camera_valid(id) && camera_valid(identity(kMaxSide, kMaxSide)) && camera_valid(identity(1, 1)));
  Camera b = id; b.fx = 0.0; CHECK(!camera_valid(b));
  b = id; b.fy2 = -1.0; CHECK(!camera_valid(b));
  b = id; b.k3 = nan; CHECK(!camera_valid(b));
  b = id; b.R[8] = inf; CHECK(!camera_valid(b));
  b = id; b.cy2 = nan; CHECK(!camera_valid(b));
  b = id; b.src_width = 0; CHECK(!camera_valid(b));
  b = id; b.dst_height = kMaxSide + 1; CHECK(!camera_valid(b));
  std::vector<Camera> many(5, identity(kMaxSide, kMaxSide));
  CHECK(cameras_valid(4, many.data()) && !cameras_valid(5, many.data()) && !cameras_valid(0, many.data()) && !cameras_valid(1, nullptr));
  CHECK(!cameras_valid(kMaxCameras + 1, many.data()));
  unsigned char px[4] = {0, 0, 0, 0};
  CHECK(frame_valid(0, 1, 16, px, &id) && frame_valid(0, 1, 100, px, &id));
  CHECK(!frame_valid(-1, 1, 16, px, &id) && !frame_valid(1, 1, 16, px, &id) && !frame_valid(0, 1, 15, px, &id) && !frame_valid(0, 1, 16, nullptr, &id));
  CHECK(!frame_valid(0, 1, (long long)INT_MAX + 1, px, &id));
  CHECK(result_valid(16, px, id) && !result_valid(15, px, id) && !result_valid(16, nullptr, id));
  CHECK(capacity_valid(1, 1) && capacity_valid(16, (long long)kMaxSide * kMaxSide));
  CHECK(!capacity_valid(0, 1) && !capacity_valid(1, 0) && !capacity_valid(1, (long long)kMaxSide * kMaxSide + 1) && !capacity_valid(17, (long long)kMaxSide * kMaxSide));
  CHECK(sizeof(Camera) == 192 && sizeof(Rig) == 288 && sizeof(FrameDesc) == 24 && sizeof(CamDesc) == 24);
  CHECK(align_map(0) == 0 && align_map(1) == 256 && align_map(256) == 256 && align_map(257) == 512);
  // the arithmetic of the remap and of the two passes stays inside 31 bits
  CHECK(256LL * 256 * 255 + 32768 < (1LL << 31) && (16384LL * 255 + 32) < (1LL << 31) && ((16384LL * 255 + 32) >> 6) == 65280);
  CHECK(16384LL * 65280 + (1LL << 21) < (1LL << 31));
  // the tile of the smoothing kernel with the widest halo: what its LDS arrays are made for
  CHECK((kTileW + 2 * kMaxRadius) * (kTileH + 2 * kMaxRadius) == 2340 && kTileW * (kTileH + 2 * kMaxRadius) * 2 == 3840);

  // ---- taps
  Taps t;
  CHECK(smooth_taps(0.0, &t) && t.radius == 0 && t.t[0] == 16384);
  CHECK(!smooth_taps(-1.0, &t) && !smooth_taps(nan, &t) && !smooth_taps(kMaxSigma + 1.0, &t));
  for (double sigma : {0.28, 0.6, 0.95, 1.28, 1.6, 1.95, 2.4}) {
    CHECK(smooth_taps(sigma, &t));
    int sum = t.t[0];
    for (int i = 1; i <= kMaxRadius; ++i) {
      sum += 2 * t.t[i];
      CHECK(t.t[i] <= t.t[i - 1] && t.t[i] >= 0 && (i <= t.radius || t.t[i] == 0));
    }
    CHECK(sum == 16384 && t.radius >= 1 && t.radius <= kMaxRadius);
    std::printf("taps %.17g %d %d %d %d %d %d %d %d %d\n", sigma, t.radius, t.t[0], t.t[1], t.t[2], t.t[3], t.t[4], t.t[5], t.t[6], t.t[7]);
  }
  CHECK(smooth_taps(kMaxSigma, &t) && t.radius == kMaxRadius);

  // ---- the rig: a rectified one gives identities; a turned one orthonormal rotations and the centre along +x
  Rig g{};
  const double k[4] = {400.0, 402.0, 320.0, 240.0};
  std::memcpy(g.left_k, k, sizeof(k));
  std::memcpy(g.right_k, k, sizeof(k));
  g.R[0] = g.R[4] = g.R[8] = 1.0;
  g.t[0] = -0.12;
  g.left_width = g.right_width = g.dst_width = 640;
  g.left_height = g.right_height = g.dst_height = 480;
  Camera l, r;
  double base = 0.0, kk[4];
  CHECK(stereo_rectify(g, &l, &r, &base, kk));
  for (int i = 0; i < 9; ++i) CHECK(l.R[i] == (i % 4 == 0 ? 1.0 : 0.0) && r.R[i] == l.R[i]);
  CHECK(base == 0.12 && kk[0] == 401.0 && kk[1] == 401.0 && kk[2] == 320.0 && kk[3] == 240.0 && l.fx2 == 401.0 && r.cy2 == 240.0);
  const double c = std::cos(0.03), s = std::sin(0.03);
  const double Ry[9] = {c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c};
  std::memcpy(g.R, Ry, sizeof(Ry));
  g.t[0] = -0.12; g.t[1] = 0.01; g.t[2] = 0.02;
  g.has_principal = 1; g.cx2 = 300.5; g.cy2 = 200.25;
  CHECK(stereo_rectify(g, &l, &r, &base, kk) && kk[2] == 300.5 && kk[3] == 200.25);
  for (const Camera* cam : {&l, &r})
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double dot = 0.0;
        for (int q = 0; q < 3; ++q) dot += cam->R[3 * i + q] * cam->R[3 * j + q];
        CHECK(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-14);
      }
  const double ctr[3] = {-(Ry[0] * g.t[0] + Ry[3] * g.t[1] + Ry[6] * g.t[2]), -(Ry[1] * g.t[0] + Ry[4] * g.t[1] + Ry[7] * g.t[2]),
                         -(Ry[2] * g.t[0] + Ry[5] * g.t[1] + Ry[8] * g.t[2])};
  for (int i = 0; i < 3; ++i) {
    const double v = l.R[3 * i] * ctr[0] + l.R[3 * i + 1] * ctr[1] + l.R[3 * i + 2] * ctr[2];
    CHECK(std::fabs(v - (i == 0 ? base : 0.0)) <= 1e-14);
  }
  Rig bad = g; bad.t[0] = bad.t[1] = bad.t[2] = 0.0; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));
  bad = g; std::memcpy(bad.R, id.R, sizeof(id.R)); bad.t[0] = 0.0; bad.t[1] = 0.0; bad.t[2] = -0.1; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));
  bad = g; bad.left_k[0] = 0.0; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));
  bad = g; bad.right_dist[4] = nan; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));
  bad = g; bad.cx2 = nan; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));
  bad = g; bad.dst_width = 0; CHECK(!stereo_rectify(bad, &l, &r, &base, kk));

  // ---- the camera given: its map, printed, and a remap of a source under both border modes
  CHECK(argc >= 28);
  Camera cam{};
  double* members[22] = {&cam.fx, &cam.fy, &cam.cx, &cam.cy, &cam.k1, &cam.k2, &cam.p1, &cam.p2, &cam.k3,
                         &cam.R[0], &cam.R[1], &cam.R[2], &cam.R[3], &cam.R[4], &cam.R[5], &cam.R[6], &cam.R[7], &cam.R[8],
                         &cam.fx2, &cam.fy2, &cam.cx2, &cam.cy2};
  for (int i = 0; i < 22; ++i) *members[i] = std::strtod(argv[1 + i], nullptr);
  cam.src_width = std::atoi(argv[23]); cam.src_height = std::atoi(argv[24]);
  cam.dst_width = std::atoi(argv[25]); cam.dst_height = std::atoi(argv[26]);
  CHECK(camera_valid(cam));
  const size_t ns = (size_t)cam.src_width * (size_t)cam.src_height, nd = (size_t)cam.dst_width * (size_t)cam.dst_height;
  std::vector<unsigned char> src(ns), dst(nd), valid(nd);
  std::vector<int> qx(nd), qy(nd);
  for (size_t i = 0; i < ns; ++i) src[i] = (unsigned char)(i * 37 + 11);
  int num_valid = 0;
  for (int v = 0; v < cam.dst_height; ++v)
    for (int u = 0; u < cam.dst_width; ++u) {
      const size_t i = (size_t)v * (size_t)cam.dst_width + (size_t)u;
      double sx, sy;
      valid[i] = (unsigned char)map_pixel(cam, u, v, &sx, &sy, &qx[i], &qy[i]);
      num_valid += valid[i];
      CHECK((qx[i] == kNoCoord) == (qy[i] == kNoCoord) && (qx[i] == kNoCoord) == std::isnan(sx) && (!valid[i] || qx[i] != kNoCoord));
      CHECK(qx[i] == kNoCoord || (qx[i] >= -kSub && qx[i] <= kSub * cam.src_width && qy[i] >= -kSub && qy[i] <= kSub * cam.src_height));
      std::printf("map %d %d %d %a %a\n", qx[i], qy[i], (int)valid[i], sx, sy);
    }
  for (int mode : {kConstant, kReplicate})
    for (size_t i = 0; i < nd; ++i) {                           // (a read outside the source is an error the sanitizer sees)
      dst[i] = remap_pixel(src.data(), cam.src_width, cam.src_height, qx[i], qy[i], valid[i], mode, 99);
      if (!valid[i] && (mode == kConstant || qx[i] == kNoCoord)) CHECK(dst[i] == 99);
    }
  std::printf("num_valid %d\n", num_valid);

  // ---- the layout of the frames given, over the camera twice
  const Camera cams[2] = {cam, cam};
  const size_t F = (size_t)(argc - 27);
  std::vector<FrameDesc> fd(F);
  size_t src_at = 0, dst_at = 0;
  for (size_t f = 0; f < F; ++f) {
    const int which = std::atoi(argv[27 + f]);
    CHECK(frame_valid(which, 2, cam.src_width, src.data(), cams));
    fd[f] = FrameDesc{(long long)src_at, (long long)dst_at, which, 0};
    src_at += slslam::align256(ns);
    dst_at += slslam::align256(nd);
    std::printf("frame %lld %lld %d\n", fd[f].src0, fd[f].dst0, fd[f].camera);
  }
  const CallLayout y = call_layout(F, src_at, dst_at);
  CHECK(y.off_src >= sizeof(FrameDesc) * F && y.in_bytes >= y.off_src + src_at && y.off_out == y.in_bytes && y.out_bytes >= dst_at);
  CHECK(y.bytes.dev == y.off_out + y.out_bytes && y.bytes.host == y.bytes.dev);
  for (size_t off : {y.off_src, y.in_bytes, y.off_out, y.out_bytes}) CHECK(off % 256 == 0);
  std::printf("size off_src %zu\nsize in_bytes %zu\nsize off_out %zu\nsize out_bytes %zu\nsize dev %zu\nsize host %zu\n", y.off_src, y.in_bytes,
              y.off_out, y.out_bytes, y.bytes.dev, y.bytes.host);
  // the host block as a run fills and reads it
  std::vector<char> block(y.bytes.host);
  std::memcpy(block.data(), fd.data(), sizeof(FrameDesc) * F);
  for (size_t f = 0; f < F; ++f) {
    slslam::pack_rows(reinterpret_cast<unsigned char*>(block.data()) + y.off_src + fd[f].src0, src.data(), cam.src_width, cam.src_height, cam.src_width);
    std::memset(block.data() + y.off_out + fd[f].dst0, 2, nd);
  }
  CHECK(block[y.off_src] == (char)src[0] && block[y.off_out] == 2 && block[y.off_out + dst_at - slslam::align256(nd) + nd - 1] == 2);

  std::printf("image rectify layout ok\n");
  return 0;
}

// slslam_amd/csrc/image_rectify_layout.h — the host half of the image rectifier (include/slslam_hip.h: slslam_image_rectifier_*): the
// limits, the validation of options, cameras and frames, the map of one output pixel (the one text of it: k_rect_map compiles the same
// function for the device), the smoothing taps, where everything of a call lies in its one block, and slslam_stereo_rectify.  Plain C++
// with no HIP in it, so that tests/host_cxx/image_rectify_layout_check.cpp runs it on the host under the sanitizers; the kernels are in
// image_rectify.h.  Internal: not part of the C ABI.
#ifndef SLSLAM_IMAGE_RECTIFY_LAYOUT_H_
#define SLSLAM_IMAGE_RECTIFY_LAYOUT_H_

#include <climits>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "call_layout.h"

#ifdef __HIPCC__
#define SLSLAM_RECT_HD __host__ __device__
#else
#define SLSLAM_RECT_HD
#endif

namespace slslam_rect {

constexpr int kMaxSide = 8192;                           // SLSLAM_LSD_MAX_SIDE: what the detector takes
constexpr int kSubBits = 8, kSub = 1 << kSubBits;        // the map's subpixel bits
constexpr int kMaxRadius = 7, kTapBits = 14;             // taps sum to 1 << kTapBits
constexpr double kMaxSigma = 16.0;
constexpr int kMaxCameras = 64;
constexpr long long kMaxMapPixels = 1LL << 28;           // the output pixels of all cameras of a handle: 25 bytes each on the device
constexpr long long kMaxCapacityPixels = 1LL << 30;      // max_frames x max_pixels a handle may be created for
constexpr int kNoCoord = INT_MIN;                        // qx = qy of a pixel that has no source coordinates
constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = 16;                  // the smoothing kernel's tile of output pixels: a wave takes a row of it

enum Border { kConstant = 0, kReplicate = 1 };

struct Options {
  int border_mode, border_value;
  double smooth_sigma;
};

// slslam_rectify_camera, field for field (the api file asserts the size)
struct Camera {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  double R[9];
  double fx2, fy2, cx2, cy2;
  int src_width, src_height, dst_width, dst_height;
};

// A camera as the per-call kernels see it: where its map lies among the maps of all cameras, and the four sizes
struct CamDesc {
  long long map0;
  int src_width, src_height, dst_width, dst_height;
};

// A frame of the call, as the kernels see it: where its source and its output lie among those of all frames
struct FrameDesc {
  long long src0, dst0;
  int camera, pad;
};

struct Taps {
  int radius;                           // 0: no smoothing
  int t[kMaxRadius + 1];
};

inline bool options_valid(const Options& o) {
  if (o.border_mode != kConstant && o.border_mode != kReplicate) return false;
  if (o.border_value < 0 || o.border_value > 255) return false;
  return std::isfinite(o.smooth_sigma) && o.smooth_sigma >= 0.0 && o.smooth_sigma <= kMaxSigma;
}

inline bool side_valid(int s) { return s >= 1 && s <= kMaxSide; }

inline bool camera_valid(const Camera& c) {
  for (double v : {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3, c.fx2, c.fy2, c.cx2, c.cy2})
    if (!std::isfinite(v)) return false;
  for (double v : c.R)
    if (!std::isfinite(v)) return false;
  if (!(c.fx > 0.0) || !(c.fy > 0.0) || !(c.fx2 > 0.0) || !(c.fy2 > 0.0)) return false;
  return side_valid(c.src_width) && side_valid(c.src_height) && side_valid(c.dst_width) && side_valid(c.dst_height);
}

inline size_t align_map(size_t pixels) { return (pixels + 255) / 256 * 256; }

// every camera valid and their output pixels together within kMaxMapPixels
inline bool cameras_valid(int num, const Camera* cams) {
  if (num < 1 || num > kMaxCameras || !cams) return false;
  long long total = 0;
  for (int c = 0; c < num; ++c) {
    if (!camera_valid(cams[c])) return false;
    total += (long long)align_map((size_t)cams[c].dst_width * (size_t)cams[c].dst_height);
  }
  return total <= kMaxMapPixels;
}

inline bool capacity_valid(int max_frames, long long max_pixels) {
  return max_frames >= 1 && max_pixels >= 1 && max_pixels <= (long long)kMaxSide * kMaxSide &&
         (long long)max_frames * max_pixels <= kMaxCapacityPixels;
}

// a frame of the camera `c`: its image has the camera's source size
inline bool frame_valid(int camera, int num_cameras, long long stride, const void* image, const Camera* cams) {
  return camera >= 0 && camera < num_cameras && image != nullptr && stride >= cams[camera].src_width && stride <= (long long)INT_MAX;
}

inline bool result_valid(long long stride, const void* image, const Camera& c) { return image != nullptr && stride >= c.dst_width; }

// ---- the map of one output pixel (include/slslam_hip.h, "map" and "quantise").  fp64, every operation rounded on its own, in the
// order written.  Returns the valid flag; a pixel without source coordinates gets qx = qy = kNoCoord and sx = sy = NaN.
SLSLAM_RECT_HD inline int map_pixel(const Camera& c, int u, int v, double* sx_out, double* sy_out, int* qx_out, int* qy_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xr = ((double)u - c.cx2) / c.fx2, yr = ((double)v - c.cy2) / c.fy2;
  const double X = (c.R[0] * xr + c.R[3] * yr) + c.R[6];
  const double Y = (c.R[1] * xr + c.R[4] * yr) + c.R[7];
  const double Z = (c.R[2] * xr + c.R[5] * yr) + c.R[8];
  double sx = 0.0, sy = 0.0;
  bool coords = Z > 0.0;
  if (coords) {
    const double x = X / Z, y = Y / Z;
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    const double xd = x * rad + ((2.0 * c.p1) * x * y + c.p2 * (r2 + 2.0 * (x * x)));
    const double yd = y * rad + (c.p1 * (r2 + 2.0 * (y * y)) + (2.0 * c.p2) * x * y);
    sx = c.fx * xd + c.cx;
    sy = c.fy * yd + c.cy;
    // (x - x is 0 for a finite x and NaN for an infinity or a NaN: the test needs no library call on the device)
    coords = (sx - sx == 0.0) && (sy - sy == 0.0);
  }
  if (!coords) {
    const double nan = __builtin_nan("");
    *sx_out = nan; *sy_out = nan;
    *qx_out = kNoCoord; *qy_out = kNoCoord;
    return 0;
  }
  double fqx = __builtin_floor(sx * (double)kSub + 0.5), fqy = __builtin_floor(sy * (double)kSub + 0.5);
  // kept in 32 bits: beyond [-256, 256 side] both neighbours clamp to the same border pixel, so the remap reads the same value
  const double hx = (double)kSub * (double)c.src_width, hy = (double)kSub * (double)c.src_height;
  fqx = fqx < -(double)kSub ? -(double)kSub : (fqx > hx ? hx : fqx);
  fqy = fqy < -(double)kSub ? -(double)kSub : (fqy > hy ? hy : fqy);
  *sx_out = sx; *sy_out = sy;
  *qx_out = (int)fqx; *qy_out = (int)fqy;
  return (sx >= -0.5 && sx < (double)c.src_width - 0.5 && sy >= -0.5 && sy < (double)c.src_height - 0.5) ? 1 : 0;
}

// ---- the remap of one output pixel from its map entry: integers only.  src: the camera's source image, sw bytes a row
SLSLAM_RECT_HD inline int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

SLSLAM_RECT_HD inline unsigned char remap_pixel(const unsigned char* src, int sw, int sh, int qx, int qy, int valid, int border_mode,
                                                int border_value) {
  if (!valid && (border_mode == kConstant || qx == kNoCoord)) return (unsigned char)border_value;
  const int ix = qx >> kSubBits, ax = qx & (kSub - 1), iy = qy >> kSubBits, ay = qy & (kSub - 1);
  const int x0 = clampi(ix, 0, sw - 1), x1 = clampi(ix + 1, 0, sw - 1), y0 = clampi(iy, 0, sh - 1), y1 = clampi(iy + 1, 0, sh - 1);
  const unsigned char* r0 = src + (size_t)y0 * (size_t)sw;
  const unsigned char* r1 = src + (size_t)y1 * (size_t)sw;
  const int p00 = r0[x0], p01 = r0[x1], p10 = r1[x0], p11 = r1[x1];
  return (unsigned char)(((kSub - ax) * (kSub - ay) * p00 + ax * (kSub - ay) * p01 + (kSub - ax) * ay * p10 + ax * ay * p11 + 32768) >> 16);
}

// ---- the smoothing taps: radius = min(7, ceil(3 sigma)), t_i = floor(w_i / sum w 16384 + 0.5) for i >= 1 with w_i = exp(-i i / (2 sigma
// sigma)), the centre tap what is left of 16384.  sigma = 0: radius 0, t_0 = 16384.  False when sigma is out of range.
inline bool smooth_taps(double sigma, Taps* out) {
  if (!std::isfinite(sigma) || sigma < 0.0 || sigma > kMaxSigma) return false;
  Taps t{};
  if (sigma > 0.0) {
    const double r = std::ceil(3.0 * sigma);
    t.radius = r < 1.0 ? 1 : (r > (double)kMaxRadius ? kMaxRadius : (int)r);
    double w[kMaxRadius + 1], sum = 1.0;
    w[0] = 1.0;
    for (int i = 1; i <= t.radius; ++i) {
      w[i] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
      sum += 2.0 * w[i];
    }
    int side = 0;
    for (int i = 1; i <= t.radius; ++i) {
      t.t[i] = (int)std::floor(w[i] / sum * (double)(1 << kTapBits) + 0.5);
      side += t.t[i];
    }
    t.t[0] = (1 << kTapBits) - 2 * side;
  } else {
    t.t[0] = 1 << kTapBits;
  }
  *out = t;
  return true;
}

// ---- where everything of a call lies.  The device block: the upload [FrameDesc F | the source pixels of every frame, rows of
// src_width bytes], then the result block [the output pixels of every frame, rows of dst_width bytes].  A frame's source and output
// begin at multiples of 256 bytes.  The host block: the upload, then the result block.
struct CallLayout {
  size_t off_src = 0, in_bytes = 0, off_out = 0, out_bytes = 0;
  slslam::BlockBytes bytes;
};

// F frames with src_bytes / dst_bytes in all: the sums of align256(source pixels) / align256(output pixels)
inline CallLayout call_layout(size_t F, size_t src_bytes, size_t dst_bytes) {
  CallLayout y;
  slslam::Carve c;
  c.take(sizeof(FrameDesc) * F);
  y.off_src = c.take(src_bytes);
  y.in_bytes = c.at;
  y.off_out = c.take(dst_bytes);
  y.out_bytes = c.at - y.off_out;
  y.bytes.dev = c.at;
  y.bytes.host = c.at;
  return y;
}

// ---- slslam_stereo_rectify (include/slslam_hip.h): Fusiello's construction, fp64, every step as stated there
struct Rig {
  double left_k[4], left_dist[5];       // fx fy cx cy; k1 k2 p1 p2 k3
  double right_k[4], right_dist[5];
  double R[9], t[3];                    // x_right = R x_left + t
  int left_width, left_height, right_width, right_height, dst_width, dst_height;
  int has_principal, pad;
  double cx2, cy2;                      // read when has_principal != 0
};

template <size_t N>
inline bool all_finite(const double (&a)[N]) {
  for (double v : a)
    if (!std::isfinite(v)) return false;
  return true;
}

inline bool stereo_rectify(const Rig& g, Camera* left, Camera* right, double* baseline, double* intrinsics) {
  if (!all_finite(g.left_k) || !all_finite(g.left_dist) || !all_finite(g.right_k) || !all_finite(g.right_dist) || !all_finite(g.R) ||
      !all_finite(g.t))
    return false;
  if (g.has_principal && (!std::isfinite(g.cx2) || !std::isfinite(g.cy2))) return false;
  if (!side_valid(g.left_width) || !side_valid(g.left_height) || !side_valid(g.right_width) || !side_valid(g.right_height) ||
      !side_valid(g.dst_width) || !side_valid(g.dst_height))
    return false;
  if (!(g.left_k[0] > 0.0) || !(g.left_k[1] > 0.0) || !(g.right_k[0] > 0.0) || !(g.right_k[1] > 0.0)) return false;
  const double* R = g.R;
  // the right camera's centre in the left camera: c = -R^T t
  const double c[3] = {-(R[0] * g.t[0] + R[3] * g.t[1] + R[6] * g.t[2]), -(R[1] * g.t[0] + R[4] * g.t[1] + R[7] * g.t[2]),
                       -(R[2] * g.t[0] + R[5] * g.t[1] + R[8] * g.t[2])};
  const double b = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  if (!(b > 0.0)) return false;
  const double e1[3] = {c[0] / b, c[1] / b, c[2] / b};                            // the new x: along the baseline
  double e2[3] = {-e1[1], e1[0], 0.0};                                            // the new y: (0, 0, 1) x e1
  const double n2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1]);
  if (!(n2 > 0.0)) return false;                                                   // the baseline along the optical axis
  e2[0] /= n2; e2[1] /= n2;
  const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};   // e1 x e2
  const double Rl[9] = {e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], e3[0], e3[1], e3[2]};
  double Rr[9];                                                                   // Rl R^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rr[3 * i + j] = Rl[3 * i] * R[3 * j] + Rl[3 * i + 1] * R[3 * j + 1] + Rl[3 * i + 2] * R[3 * j + 2];
  const double f = ((g.left_k[0] + g.left_k[1]) + (g.right_k[0] + g.right_k[1])) / 4.0;
  const double cx2 = g.has_principal ? g.cx2 : g.left_k[2], cy2 = g.has_principal ? g.cy2 : g.left_k[3];
  for (int side = 0; side < 2; ++side) {
    Camera& o = side ? *right : *left;
    const double* k = side ? g.right_k : g.left_k;
    const double* dist = side ? g.right_dist : g.left_dist;
    o.fx = k[0]; o.fy = k[1]; o.cx = k[2]; o.cy = k[3];
    o.k1 = dist[0]; o.k2 = dist[1]; o.p1 = dist[2]; o.p2 = dist[3]; o.k3 = dist[4];
    for (int i = 0; i < 9; ++i) o.R[i] = side ? Rr[i] : Rl[i];
    o.fx2 = f; o.fy2 = f; o.cx2 = cx2; o.cy2 = cy2;
    o.src_width = side ? g.right_width : g.left_width;
    o.src_height = side ? g.right_height : g.left_height;
    o.dst_width = g.dst_width; o.dst_height = g.dst_height;
  }
  *baseline = b;
  intrinsics[0] = f; intrinsics[1] = f; intrinsics[2] = cx2; intrinsics[3] = cy2;
  return true;
}

}  // namespace slslam_rect

#endif  // SLSLAM_IMAGE_RECTIFY_LAYOUT_H_

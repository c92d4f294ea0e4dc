// slslam_amd/csrc/image_rectify.h — the kernels of the image rectifier (include/slslam_hip.h: slslam_image_rectifier_*).
//   k_rect_map     once per camera, outside the per-call path: one thread per output pixel evaluates map_pixel (image_rectify_layout.h)
//                  in fp64 and writes (qx, qy) as one int2, the valid byte and sx, sy.
//   k_rect_remap   per call without smoothing: the frame in the grid's y, one thread per output pixel in row-major order, so a wave reads
//                  64 consecutive map entries (512 bytes) and stores 64 consecutive bytes; the four source reads are gathers.
//   k_rect_smooth  per call with smoothing, one launch: a block takes a tile of kTileW x kTileH output pixels, remaps the tile and a halo
//                  of `radius` pixels into LDS (a halo pixel outside the output takes the clamped pixel's remap), runs the horizontal
//                  pass over the tile's columns and every row of tile and halo into 16 bits in LDS, and the vertical pass from there.
//                  6180 bytes of LDS a block, no scratch.
// Integers only on the per-call path.  No launch is sized by a count made on the device.  Internal: not part of the C ABI.
#ifndef SLSLAM_IMAGE_RECTIFY_H_
#define SLSLAM_IMAGE_RECTIFY_H_

#include <hip/hip_runtime.h>

#include "image_rectify_layout.h"

namespace slslam_rect {

// The maps of all cameras, one plane each; a camera's part begins at its CamDesc::map0
struct Maps {
  int2* q;
  unsigned char* valid;
  double *sx, *sy;
};

__global__ __launch_bounds__(kBlock) void k_rect_map(Camera cam, long long map0, Maps m) {
  const long long n = (long long)cam.dst_width * cam.dst_height;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int v = (int)(i / cam.dst_width), u = (int)(i - (long long)v * cam.dst_width);
  double sx, sy;
  int qx, qy;
  const int ok = map_pixel(cam, u, v, &sx, &sy, &qx, &qy);
  m.q[map0 + i] = make_int2(qx, qy);
  m.valid[map0 + i] = (unsigned char)ok;
  m.sx[map0 + i] = sx;
  m.sy[map0 + i] = sy;
}

// What a per-call kernel is given
struct Call {
  const FrameDesc* frames;
  const CamDesc* cams;
  const int2* q;
  const unsigned char* valid;
  const unsigned char* src;             // the source pixels of every frame
  unsigned char* dst;                   // the output pixels of every frame
  int border_mode, border_value;
};

__global__ __launch_bounds__(kBlock) void k_rect_remap(Call c) {
  const FrameDesc fd = c.frames[blockIdx.y];
  const CamDesc cd = c.cams[fd.camera];
  const long long n = (long long)cd.dst_width * cd.dst_height;
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int2 q = c.q[cd.map0 + i];
  c.dst[fd.dst0 + i] = remap_pixel(c.src + fd.src0, cd.src_width, cd.src_height, q.x, q.y, c.valid[cd.map0 + i], c.border_mode, c.border_value);
}

constexpr int kRawW = kTileW + 2 * kMaxRadius, kRawH = kTileH + 2 * kMaxRadius;

__global__ __launch_bounds__(kBlock) void k_rect_smooth(Call c, Taps taps) {
  __shared__ unsigned char raw[kRawH * kRawW];           // the remapped tile with its halo, rows of tile_w + 2 radius bytes
  __shared__ unsigned short hor[kRawH * kTileW];         // the horizontal pass, the value x 256, rows of kTileW
  const FrameDesc fd = c.frames[blockIdx.y];
  const CamDesc cd = c.cams[fd.camera];
  const int tiles_x = (cd.dst_width + kTileW - 1) / kTileW, tiles_y = (cd.dst_height + kTileH - 1) / kTileH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;      // (the grid's x is sized for the call's largest frame; uniform over the block)
  const int x0 = ((int)blockIdx.x % tiles_x) * kTileW, y0 = ((int)blockIdx.x / tiles_x) * kTileH;
  const int r = taps.radius, rw = kTileW + 2 * r, rh = kTileH + 2 * r;
  const unsigned char* src = c.src + fd.src0;
  // remap loop: (kTileW + 2 radius) x (kTileH + 2 radius) pixels of tile and halo, kBlock a pass
  for (int i = threadIdx.x; i < rw * rh; i += kBlock) {
    const int ly = i / rw, lx = i - ly * rw;
    const int gx = clampi(x0 + lx - r, 0, cd.dst_width - 1), gy = clampi(y0 + ly - r, 0, cd.dst_height - 1);
    const long long at = cd.map0 + (long long)gy * cd.dst_width + gx;
    const int2 q = c.q[at];
    raw[i] = remap_pixel(src, cd.src_width, cd.src_height, q.x, q.y, c.valid[at], c.border_mode, c.border_value);
  }
  __syncthreads();
  // horizontal loop: kTileW x (kTileH + 2 radius) values, kBlock a pass; the tap loop inside runs `radius` times
  for (int i = threadIdx.x; i < kTileW * rh; i += kBlock) {
    const int ly = i / kTileW, lx = i - ly * kTileW;
    const unsigned char* row = raw + ly * rw + lx + r;
    int acc = taps.t[0] * (int)row[0];
    for (int k = 1; k <= r; ++k) acc += taps.t[k] * ((int)row[-k] + (int)row[k]);
    hor[i] = (unsigned short)((acc + 32) >> 6);
  }
  __syncthreads();
  // vertical loop: the tile's kTileW x kTileH pixels, kBlock a pass
  for (int i = threadIdx.x; i < kTileW * kTileH; i += kBlock) {
    const int ly = i / kTileW, lx = i - ly * kTileW;
    const int gx = x0 + lx, gy = y0 + ly;
    if (gx >= cd.dst_width || gy >= cd.dst_height) continue;
    const unsigned short* col = hor + (ly + r) * kTileW + lx;
    int acc = taps.t[0] * (int)col[0];
    for (int k = 1; k <= r; ++k) acc += taps.t[k] * ((int)col[-k * kTileW] + (int)col[k * kTileW]);
    c.dst[fd.dst0 + (long long)gy * cd.dst_width + gx] = (unsigned char)((acc + (1 << 21)) >> 22);
  }
}

}  // namespace slslam_rect

#endif  // SLSLAM_IMAGE_RECTIFY_H_

// slslam_amd/csrc/line_descriptor.h — the MSLD line descriptor on the device (include/slslam_hip.h: slslam_line_descriptor_*; the contract
// is written there).  One launch per call: a block of one wave per segment, whatever the number of frames.
//   lane <-> sample along the line, 64 samples per pass, ceil(N / 64) passes
//   a lane walks the M w support rows of its sample.  A row adds to band i0 and to band i0 + 1 and i0 only rises along the rows, so two
//   open sets of four sums are all a lane keeps; when i0 moves on, band i0 of the pass is complete in every lane.
//   a complete band is summed over the lanes at once - first and second moment about the band's value at sample 0, in fp64 - and lane b
//   keeps the moments of band b: no array is indexed by a band, and the two halves of the descriptor end up one band per lane.
// fp64: the sample positions (a coordinate reaches 8192, where a float resolves 1 / 1024 pixel) and the moments (N reaches thousands
// and the variance is a difference of them; about sample 0 a constant band has moments of exactly 0).  fp32: the gradients, their
// interpolation, the weights and the band sums of one sample.  Every pixel is read at clamped coordinates: no read leaves the image.
#ifndef SLSLAM_LINE_DESCRIPTOR_H_
#define SLSLAM_LINE_DESCRIPTOR_H_

#include <hip/hip_runtime.h>

#include "line_descriptor_layout.h"

namespace slslam_msld {

struct Out {
  float* descriptors;                   // [S D]
  int* status;                          // [S]
  int* num_samples;                     // [S]
  float* polarity;                      // [S]
};

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// gx and gy at the integer pixel (x, y) clamped to the image: central differences over the replicated border
__device__ inline void pixel_gradient(const unsigned char* __restrict__ img, int W, int H, int x, int y, float& gx, float& gy) {
  x = clampi(x, W - 1);
  y = clampi(y, H - 1);
  const unsigned char* row = img + (size_t)y * (size_t)W;
  const int xl = x > 0 ? x - 1 : 0, xr = x < W - 1 ? x + 1 : W - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y < H - 1 ? y + 1 : H - 1;
  gx = 0.5f * ((float)row[xr] - (float)row[xl]);
  gy = 0.5f * ((float)img[(size_t)yd * (size_t)W + (size_t)x] - (float)img[(size_t)yu * (size_t)W + (size_t)x]);
}

struct BandMoments {
  float shift[4];                       // lane b: band b's four sums at sample 0
  double m1[4], m2[4];                  // lane b: sums over the samples of (v - shift) and of its square
};

// Band `band` of pass `pass` is complete in v[4] of every lane: into lane `band`'s moments
__device__ inline void band_done(int band, int bands, int pass, int lane, bool active, const float* v, BandMoments& bm) {
  if (band < 0 || band >= bands) return;                 // (the same in every lane)
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float s0 = pass == 0 ? __shfl(v[c], 0) : __shfl(bm.shift[c], band);
    const double d = active ? (double)v[c] - (double)s0 : 0.0;
    const double t1 = wave_sum(d), t2 = wave_sum(d * d);
    if (lane == band) {
      if (pass == 0) bm.shift[c] = s0;
      bm.m1[c] += t1;
      bm.m2[c] += t2;
    }
  }
}

__global__ __launch_bounds__(kWave) void k_line_descriptor(const FrameDesc* __restrict__ frames, const SegDesc* __restrict__ segs,
                                                           const WeightRow* __restrict__ table, const unsigned char* __restrict__ pixels,
                                                           int bands, int rows, int orient, Out out) {
  const size_t seg = blockIdx.x;
  const int lane = (int)threadIdx.x;
  const int D = 8 * bands;
  const SegDesc sd = segs[seg];
  float* desc = out.descriptors + seg * (size_t)D;
  if (sd.status != kOk) {                                // (refused on the host: the same in every lane)
    for (int i = lane; i < D; i += kWave) desc[i] = 0.f;
    if (lane == 0) {
      out.status[seg] = sd.status;
      out.num_samples[seg] = 0;
      out.polarity[seg] = 0.f;
    }
    return;
  }
  const FrameDesc fd = frames[sd.frame];
  const unsigned char* img = pixels + fd.image;
  const int W = fd.width, H = fd.height, N = sd.num_samples;
  const double L = sd.length;
  const double dlx = ((double)sd.x1 - (double)sd.x0) / L, dly = ((double)sd.y1 - (double)sd.y0) / L;      // d_L; d_perp = (-dly, dlx)
  const float flx = (float)dlx, fly = (float)dly;
  const double rho0 = -0.5 * (double)(rows - 1);

  BandMoments bm;
#pragma unroll
  for (int c = 0; c < 4; ++c) { bm.shift[c] = 0.f; bm.m1[c] = 0.0; bm.m2[c] = 0.0; }
  double pol = 0.0;

  const int passes = (N + kWave - 1) / kWave;
  for (int pass = 0; pass < passes; ++pass) {
    const int j = pass * kWave + lane;
    const bool active = j < N;
    const int jc = active ? j : N - 1;                   // (a lane past the end walks the last sample and adds nothing)
    const double s = 0.5 * L + (double)jc - 0.5 * (double)(N - 1);
    const double bx = (double)sd.x0 + s * dlx, by = (double)sd.y0 + s * dly;
    float cur[4] = {0.f, 0.f, 0.f, 0.f}, nxt[4] = {0.f, 0.f, 0.f, 0.f};
    float psum = 0.f;
    int band = table[0].band;
    for (int r = 0; r < rows; ++r) {
      const WeightRow wr = table[r];                     // (the same address in every lane)
      if (wr.band != band) {
        band_done(band, bands, pass, lane, active, cur, bm);
#pragma unroll
        for (int c = 0; c < 4; ++c) { cur[c] = nxt[c]; nxt[c] = 0.f; }
        band = wr.band;
      }
      const double rho = rho0 + (double)r;
      const double x = bx - rho * dly, y = by + rho * dlx;
      const double xf = floor(x), yf = floor(y);
      const float ax = (float)(x - xf), ay = (float)(y - yf);
      const int ix = (int)xf, iy = (int)yf;
      float gx00, gy00, gx10, gy10, gx01, gy01, gx11, gy11;
      pixel_gradient(img, W, H, ix, iy, gx00, gy00);
      pixel_gradient(img, W, H, ix + 1, iy, gx10, gy10);
      pixel_gradient(img, W, H, ix, iy + 1, gx01, gy01);
      pixel_gradient(img, W, H, ix + 1, iy + 1, gx11, gy11);
      const float gx0 = gx00 + ax * (gx10 - gx00), gx1 = gx01 + ax * (gx11 - gx01);
      const float gy0 = gy00 + ax * (gy10 - gy00), gy1 = gy01 + ax * (gy11 - gy01);
      const float gx = gx0 + ay * (gx1 - gx0), gy = gy0 + ay * (gy1 - gy0);
      const float gl = gx * flx + gy * fly, gp = gy * flx - gx * fly;
      const float comp[4] = {fmaxf(gp, 0.f), fmaxf(-gp, 0.f), fmaxf(gl, 0.f), fmaxf(-gl, 0.f)};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        cur[c] += wr.wa * comp[c];
        nxt[c] += wr.wb * comp[c];
      }
      psum += wr.f * gp;
    }
    band_done(band, bands, pass, lane, active, cur, bm);
    band_done(band + 1, bands, pass, lane, active, nxt, bm);
    pol += active ? (double)psum : 0.0;
  }

  // ---- lane b < M holds band b: means, standard deviations, the two norms, the flip, the write
  const double polarity = wave_sum(pol);
  const bool flip = orient != 0 && polarity < 0.0;
  const bool mine = lane < bands;
  const double inv_n = 1.0 / (double)N;
  double mean[4], sdev[4], qm = 0.0, qs = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double e = bm.m1[c] * inv_n;
    const double var = bm.m2[c] * inv_n - e * e;
    mean[c] = mine ? (double)bm.shift[c] + e : 0.0;
    sdev[c] = mine && var > 0.0 ? sqrt(var) : 0.0;
    qm += mean[c] * mean[c];
    qs += sdev[c] * sdev[c];
  }
  const double nm = sqrt(wave_sum(qm)), ns = sqrt(wave_sum(qs));
  const double km = nm > 0.0 ? 0.70710678118654752440 / nm : 0.0, ks = ns > 0.0 ? 0.70710678118654752440 / ns : 0.0;
  if (mine) {
    // the swapped segment: bands mirrored, each pair of components exchanged.  Equal to the contract's reversed rows where the table is
    // symmetric, wa[r] == wb[R-1-r]; rounded to float the two may differ in the last bit (line_descriptor_layout_check.cpp allows 1e-7),
    // which is a relative 6e-8 in a weight: far inside the tests' tolerance, and the first thing to look at if that is ever tightened
    const int b = flip ? bands - 1 - lane : lane;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cc = flip ? c ^ 1 : c;
      desc[4 * b + cc] = (float)(mean[c] * km);
      desc[4 * bands + 4 * b + cc] = (float)(sdev[c] * ks);
    }
  }
  if (lane == 0) {
    out.status[seg] = nm > 0.0 || ns > 0.0 ? kOk : kFlat;
    out.num_samples[seg] = N;
    out.polarity[seg] = (float)(flip ? -polarity : polarity);
  }
}

}  // namespace slslam_msld

#endif  // SLSLAM_LINE_DESCRIPTOR_H_

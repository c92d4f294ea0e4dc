// slslam_amd/csrc/line_detect.h — the line segment detector on the device (include/slslam_hip.h: slslam_line_detector_*; the contract is
// written there).  Eleven launches per call, whatever the number of frames: the frame is the grid's y (or its x where a block takes a
// whole frame), a chunk of kChunk pixels or a tile of kTile x kTile its x.
//   k_links     gradient, strong bit and the four forward link bits E, SW, S, SE of every pixel: one byte a pixel
//   k_tile      union-find of a tile in LDS; a pixel's parent = the smallest index of its component within the tile
//   k_border    the links that cross a tile border (E, S and both diagonals): unions on the parents in global memory, by atomicMin
//   k_compress  parent = root, the label plane; the pixels of a root counted into its word of the count plane
//   k_count     roots and fitted roots (pixels >= min_pixels) of every chunk
//   k_scan      one block a frame: the chunks' exclusive prefix sums, the frame's totals
//   k_assign    a fitted root's rank in label order = its slot among the frame's Comp; the slot is cleared and written over the count
//   k_sums      the eight int64 sums of step 4 into the slots, by atomics: a run of equal slots within a wave adds once
//   k_fit       step 5 of every slot, in fp64 without contraction
//   k_extent    t of every pixel, min and max into the slot through an order-preserving int64 image of the double
//   k_emit      one block a frame: statuses, their counts, the OK components' rank in label order, the segments
// Every find loop walks parents that only ever decrease (parent[i] <= i, a union writes the smaller root over the larger by atomicMin),
// so it ends after at most i steps and waits for nobody; a union retries only with a strictly smaller pair.  A stale parent is an
// ancestor all the same: the walk is longer, never wrong.  Integers: gradient, links, labels, sums - bit-equal to the reference
// whatever the order.  fp64: the fit, the extent, the end points.  Every pixel is read at clamped coordinates; every plane index is
// checked against the frame's pixel count before it is used.
#ifndef SLSLAM_LINE_DETECT_H_
#define SLSLAM_LINE_DETECT_H_

#include <hip/hip_runtime.h>

#include "line_detect_layout.h"

// step 5 and 6 are rounded operation by operation, as the reference evaluates them
#pragma clang fp contract(off)

namespace slslam_lsd {

constexpr int kWave = 64;

struct Planes {
  const FrameDesc* frames;
  const unsigned char* pixels;
  unsigned char* links;
  int* count;                           // k_compress: pixels of the root; from k_assign on: the root's slot, -1 without one
  int* parent;                          // the label plane
  int2* chunks;                         // per chunk (roots, fitted roots), then their exclusive prefix sums within the frame
  Comp* comps;
  FrameOut* out;
};

struct Segments {
  float* segments;                      // [F S 4]
  double *length, *thickness, *strength;
  int *npix, *label;                    // [F S]
};

__device__ inline void gradient(const unsigned char* __restrict__ img, int W, int H, int x, int y, int& gx, int& gy) {
  const unsigned char* row = img + (size_t)y * (size_t)W;
  const int xl = x > 0 ? x - 1 : 0, xr = x < W - 1 ? x + 1 : W - 1;
  const int yu = y > 0 ? y - 1 : 0, yd = y < H - 1 ? y + 1 : H - 1;
  gx = (int)row[xr] - (int)row[xl];
  gy = (int)img[(size_t)yd * (size_t)W + (size_t)x] - (int)img[(size_t)yu * (size_t)W + (size_t)x];
}

// the largest integer whose square is at most m2 (m2 <= 2 255^2): the float root, corrected
__device__ inline int isqrt(int m2) {
  int w = (int)sqrtf((float)m2);
  if (w * w > m2) --w;
  if ((w + 1) * (w + 1) <= m2) ++w;
  return w;
}

__device__ inline bool aligned(int ax, int ay, int bx, int by, long long tol_num, long long tol_den) {
  const long long dot = (long long)(ax * bx + ay * by), cross = (long long)(ax * by - ay * bx);
  return dot > 0 && tol_den * cross * cross <= tol_num * dot * dot;
}

// ---- 1. gradient and links
__global__ __launch_bounds__(kBlock) void k_links(Planes P, int thr2, int tol_num, int tol_den) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int W = fd.width, H = fd.height, N = W * H;
  const unsigned char* img = P.pixels + fd.first;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const int p = (int)blockIdx.x * kChunk + k * kBlock + (int)threadIdx.x;       // (a lane's neighbours are the neighbouring pixels)
    if (p >= N) return;
    const int y = p / W, x = p - y * W;
    int gx, gy;
    gradient(img, W, H, x, y, gx, gy);
    int bits = 0;
    if (gx * gx + gy * gy >= thr2) {
      bits = kStrong;
      const int dx[4] = {1, -1, 0, 1}, dy[4] = {0, 1, 1, 1};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nx = x + dx[q], ny = y + dy[q];
        if (nx < 0 || nx >= W || ny >= H) continue;
        int hx, hy;
        gradient(img, W, H, nx, ny, hx, hy);
        if (hx * hx + hy * hy >= thr2 && aligned(gx, gy, hx, hy, tol_num, tol_den)) bits |= kEast << q;
      }
    }
    P.links[fd.first + p] = (unsigned char)bits;
    P.parent[fd.first + p] = -1;                         // (a strong pixel's is written by k_tile)
    P.count[fd.first + p] = 0;
  }
}

// ---- 2. / 3. labelling.  find and unite on parents in LDS or in global memory: `Load` reads a parent past any cache that may be stale
struct LdsLoad {
  __device__ static int get(const int* p) { return *(const volatile int*)p; }
};
struct AgentLoad {
  __device__ static int get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

template <typename Load>
__device__ inline int find(const int* L, int i) {
  for (int q = Load::get(L + i); q < i; q = Load::get(L + i)) i = q;              // (q < i or q == i: every step goes down)
  return i;
}

// The union of the sets of a and b: the larger root gets the smaller as its parent.  Where the larger one has stopped being a root, the
// atomicMin may have replaced its parent `old` by the smaller root; old and the smaller root are then united in turn, which keeps what
// the replaced parent said.  Every retry has a strictly smaller pair.
template <typename Load>
__device__ inline void unite(int* L, int a, int b) {
  for (;;) {
    a = find<Load>(L, a);
    b = find<Load>(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }        // a > b
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(kBlock) void k_tile(Planes P) {
  __shared__ int L[kTile * kTile];
  __shared__ unsigned char lk[kTile * kTile];
  const FrameDesc fd = P.frames[blockIdx.y];
  const int W = fd.width, H = fd.height;
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;     // (the whole block)
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTile, y0 = ty * kTile;
  for (int i = (int)threadIdx.x; i < kTile * kTile; i += kBlock) {
    const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
    lk[i] = x < W && y < H ? P.links[fd.first + (long long)y * W + x] : (unsigned char)0;
    L[i] = i;
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < kTile * kTile; i += kBlock) {
    const int b = lk[i], lx = i & (kTile - 1), ly = i / kTile;
    if (!(b & kStrong)) continue;
    // a link bit is set only where the neighbour lies in the image; here it must lie in the tile as well
    if ((b & kEast) && lx + 1 < kTile) unite<LdsLoad>(L, i, i + 1);
    if (ly + 1 < kTile) {
      if ((b & kSouthWest) && lx > 0) unite<LdsLoad>(L, i, i + kTile - 1);
      if (b & kSouth) unite<LdsLoad>(L, i, i + kTile);
      if ((b & kSouthEast) && lx + 1 < kTile) unite<LdsLoad>(L, i, i + kTile + 1);
    }
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < kTile * kTile; i += kBlock) {
    if (!(lk[i] & kStrong)) continue;
    const int r = find<LdsLoad>(L, i);                   // (row-major in the tile and in the image: the smallest of the one is the smallest of the other)
    const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
    P.parent[fd.first + (long long)y * W + x] = (y0 + r / kTile) * W + x0 + (r & (kTile - 1));
  }
}

__global__ __launch_bounds__(kBlock) void k_border(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int W = fd.width, N = W * fd.height;
  int* parent = P.parent + fd.first;
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const int p = (int)blockIdx.x * kChunk + k * kBlock + (int)threadIdx.x;
    if (p >= N) return;
    const int b = P.links[fd.first + p];
    if (b < 2) continue;                                 // (no forward link)
    const int y = p / W, x = p - y * W;
    const bool right = (x & (kTile - 1)) == kTile - 1, left = (x & (kTile - 1)) == 0, bottom = (y & (kTile - 1)) == kTile - 1;
    if ((b & kEast) && right) unite<AgentLoad>(parent, p, p + 1);
    if ((b & kSouthWest) && (left || bottom)) unite<AgentLoad>(parent, p, p + W - 1);
    if ((b & kSouth) && bottom) unite<AgentLoad>(parent, p, p + W);
    if ((b & kSouthEast) && (right || bottom)) unite<AgentLoad>(parent, p, p + W + 1);
  }
}

// ---- runs of equal keys among the lanes of a wave: `end` = the lane behind the run of this lane
__device__ inline int run_end(int key, int lane, bool& head) {
  const int before = __shfl_up(key, 1);
  head = lane == 0 || before != key;
  const unsigned long long heads = __ballot(head);
  const unsigned long long later = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
  return later ? lane + 1 + __ffsll((long long)later) - 1 : kWave;
}

__device__ inline long long shfl_down64(long long v, int d) {
  const int lo = __shfl_down((int)(v & 0xffffffffll), d), hi = __shfl_down((int)(v >> 32), d);
  return ((long long)hi << 32) | (long long)(unsigned)lo;
}

// the sum of v over the run, in the run's head lane
__device__ inline long long run_sum(long long v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long o = shfl_down64(v, d);
    if (lane + d < end) v += o;
  }
  return v;
}

__device__ inline long long run_min(long long v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long o = shfl_down64(v, d);
    if (lane + d < end && o < v) v = o;
  }
  return v;
}

__device__ inline long long run_max(long long v, int lane, int end) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long o = shfl_down64(v, d);
    if (lane + d < end && o > v) v = o;
  }
  return v;
}

// ---- 4. the label plane, and the pixels of every root
__global__ __launch_bounds__(kBlock) void k_compress(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int N = fd.width * fd.height;
  int* parent = P.parent + fd.first;
  const int lane = (int)threadIdx.x & (kWave - 1);
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const int p = (int)blockIdx.x * kChunk + k * kBlock + (int)threadIdx.x;
    if ((int)blockIdx.x * kChunk + k * kBlock + ((int)threadIdx.x & ~(kWave - 1)) >= N) return;      // (the whole wave is past the frame)
    int r = -1;
    if (p < N && (P.links[fd.first + p] & kStrong)) {
      r = find<AgentLoad>(parent, p);
      __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (another walk reads the old parent or the root)
    }
    bool head;
    const int end = run_end(r, lane, head);
    if (head && r >= 0) atomicAdd(P.count + fd.first + r, end - lane);
  }
}

// ---- 5. - 7. a fitted root's slot: its rank in label order
__device__ inline int block_scan_exclusive(int v, int* total) {
  __shared__ int wsum[kBlock / kWave];
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  int inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();                                       // (wsum of an earlier scan has been read)
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    if (w < wave) base += wsum[w];
    sum += wsum[w];
  }
  *total = sum;
  return base + inc - v;
}

// a thread's four consecutive pixels: bit q of `roots`: pixel q is a root, of `fitted`: a root with at least min_pixels pixels
__device__ inline void root_flags(const Planes& P, const FrameDesc& fd, int p0, int N, int min_pixels, int& roots, int& fitted) {
  roots = fitted = 0;
  for (int q = 0; q < 4; ++q) {
    const int p = p0 + q;
    if (p >= N || P.parent[fd.first + p] != p) continue;
    roots |= 1 << q;
    if (P.count[fd.first + p] >= min_pixels) fitted |= 1 << q;
  }
}

__global__ __launch_bounds__(kBlock) void k_count(Planes P, int min_pixels) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int N = fd.width * fd.height;
  if ((int)blockIdx.x * kChunk >= N) return;
  int roots, fitted, nr, nf;
  root_flags(P, fd, (int)blockIdx.x * kChunk + 4 * (int)threadIdx.x, N, min_pixels, roots, fitted);
  block_scan_exclusive(__popc(roots), &nr);
  block_scan_exclusive(__popc(fitted), &nf);
  if (threadIdx.x == 0) P.chunks[fd.chunk0 + (int)blockIdx.x] = make_int2(nr, nf);
}

__global__ __launch_bounds__(kBlock) void k_scan(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.x];
  const int N = fd.width * fd.height, nchunks = (N + kChunk - 1) / kChunk;
  int2* c = P.chunks + fd.chunk0;
  int base_r = 0, base_f = 0;
  for (int i0 = 0; i0 < nchunks; i0 += kBlock) {
    const int i = i0 + (int)threadIdx.x;
    const int2 v = i < nchunks ? c[i] : make_int2(0, 0);
    int tr, tf;
    const int er = block_scan_exclusive(v.x, &tr), ef = block_scan_exclusive(v.y, &tf);
    if (i < nchunks) c[i] = make_int2(base_r + er, base_f + ef);
    base_r += tr;
    base_f += tf;
  }
  if (threadIdx.x == 0) {
    P.out[blockIdx.x].num_components = base_r;
    P.out[blockIdx.x].num_fitted = base_f < fd.comp_cap ? base_f : fd.comp_cap;        // (base_f min_pixels <= N: it cannot be larger)
  }
}

__global__ __launch_bounds__(kBlock) void k_assign(Planes P, int min_pixels) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int N = fd.width * fd.height;
  if ((int)blockIdx.x * kChunk >= N) return;
  const int p0 = (int)blockIdx.x * kChunk + 4 * (int)threadIdx.x;
  int roots, fitted, total;
  root_flags(P, fd, p0, N, min_pixels, roots, fitted);
  int slot = P.chunks[fd.chunk0 + (int)blockIdx.x].y + block_scan_exclusive(__popc(fitted), &total);
  for (int q = 0; q < 4; ++q) {
    if (!(roots & (1 << q))) continue;
    const int p = p0 + q;
    int mine = -1;
    if ((fitted & (1 << q)) && slot < fd.comp_cap) {
      mine = slot++;
      Comp c;
      c.sw = c.swu = c.swv = c.swuu = c.swuv = c.swvv = c.sgx = c.sgy = 0;
      c.tmin_key = 0x7fffffffffffffffll;
      c.tmax_key = -0x7fffffffffffffffll - 1;
      c.n = P.count[fd.first + p];
      c.root = p;
      c.cx = c.cy = c.ex = c.ey = c.thickness = 0.0;
      P.comps[fd.comp0 + mine] = c;
    }
    P.count[fd.first + p] = mine;
  }
}

// the slot of pixel p's component, -1 where p is not strong or the component is small
__device__ inline int slot_of(const Planes& P, const FrameDesc& fd, int p, int N) {
  if (p >= N) return -1;
  const int r = P.parent[fd.first + p];
  return r < 0 ? -1 : P.count[fd.first + r];
}

// ---- 8. the sums
__global__ __launch_bounds__(kBlock) void k_sums(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int W = fd.width, H = fd.height, N = W * H;
  const unsigned char* img = P.pixels + fd.first;
  const int lane = (int)threadIdx.x & (kWave - 1);
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const int p = (int)blockIdx.x * kChunk + k * kBlock + (int)threadIdx.x;
    if ((int)blockIdx.x * kChunk + k * kBlock + ((int)threadIdx.x & ~(kWave - 1)) >= N) return;
    const int slot = slot_of(P, fd, p, N);
    long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (slot >= 0) {
      const int root = P.parent[fd.first + p];
      const int y = p / W, x = p - y * W, yr = root / W, xr = root - yr * W;
      int gx, gy;
      gradient(img, W, H, x, y, gx, gy);
      const long long w = isqrt(gx * gx + gy * gy), u = x - xr, v = y - yr;
      s[0] = w; s[1] = w * u; s[2] = w * v; s[3] = w * u * u; s[4] = w * u * v; s[5] = w * v * v; s[6] = gx; s[7] = gy;
    }
    bool head;
    const int end = run_end(slot, lane, head);
    if (__ballot(slot >= 0) == 0ull) continue;           // (the same in every lane)
    Comp* c = P.comps + fd.comp0 + (slot >= 0 ? slot : 0);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&c->sw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long t = run_sum(s[j], lane, end);
      if (head && slot >= 0) atomicAdd(dst + j, (unsigned long long)t);
    }
  }
}

// ---- 9. the fit
__global__ __launch_bounds__(kBlock) void k_fit(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (i >= P.out[blockIdx.y].num_fitted) return;
  Comp* c = P.comps + fd.comp0 + i;
  const double sw = (double)c->sw;
  const double cx = (double)c->swu / sw, cy = (double)c->swv / sw;
  const double sxx = (double)c->swuu / sw - cx * cx, syy = (double)c->swvv / sw - cy * cy, sxy = (double)c->swuv / sw - cx * cy;
  const double h = (sxx - syy) / 2.0;
  const double rt = sqrt(h * h + sxy * sxy);
  const double lmin = (sxx + syy) / 2.0 - rt;
  double ex = h >= 0.0 ? h + rt : sxy, ey = h >= 0.0 ? sxy : rt - h;
  const double norm = sqrt(ex * ex + ey * ey);
  if (norm == 0.0) ex = ey = 0.0;
  else { ex = ex / norm; ey = ey / norm; }
  c->cx = cx; c->cy = cy; c->ex = ex; c->ey = ey;
  c->thickness = norm == 0.0 ? 0.0 : sqrt(lmin > 0.0 ? lmin : 0.0);
}

// a double as an int64 of the same order, and back
__device__ inline long long order_key(double t) {
  const long long b = __double_as_longlong(t);
  return b >= 0 ? b : b ^ 0x7fffffffffffffffll;
}
__device__ inline double order_value(long long k) { return __longlong_as_double(k >= 0 ? k : k ^ 0x7fffffffffffffffll); }

// ---- 10. the extent
__global__ __launch_bounds__(kBlock) void k_extent(Planes P) {
  const FrameDesc fd = P.frames[blockIdx.y];
  const int W = fd.width, N = W * fd.height;
  const int lane = (int)threadIdx.x & (kWave - 1);
#pragma unroll
  for (int k = 0; k < kChunk / kBlock; ++k) {
    const int p = (int)blockIdx.x * kChunk + k * kBlock + (int)threadIdx.x;
    if ((int)blockIdx.x * kChunk + k * kBlock + ((int)threadIdx.x & ~(kWave - 1)) >= N) return;
    const int slot = slot_of(P, fd, p, N);
    if (__ballot(slot >= 0) == 0ull) continue;
    Comp* c = P.comps + fd.comp0 + (slot >= 0 ? slot : 0);
    long long key = 0;
    if (slot >= 0) {
      const int root = c->root;
      const int y = p / W, x = p - y * W, yr = root / W, xr = root - yr * W;
      const double u = (double)(x - xr), v = (double)(y - yr);
      key = order_key((u - c->cx) * c->ex + (v - c->cy) * c->ey);
    }
    bool head;
    const int end = run_end(slot, lane, head);
    const long long lo = run_min(key, lane, end), hi = run_max(key, lane, end);
    if (head && slot >= 0) {
      atomicMin(&c->tmin_key, lo);
      atomicMax(&c->tmax_key, hi);
    }
  }
}

// ---- 11. statuses, counts, segments
__global__ __launch_bounds__(kBlock) void k_emit(Planes P, Segments S, double min_length, double max_thickness, int max_segments) {
  __shared__ int counts[5];
  const FrameDesc fd = P.frames[blockIdx.x];
  const int f = (int)blockIdx.x;
  const int nfit = P.out[f].num_fitted;
  if (threadIdx.x < 5) counts[threadIdx.x] = 0;
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < nfit; i0 += kBlock) {
    const int i = i0 + (int)threadIdx.x;
    int status = -1;
    double length = 0.0, tmin = 0.0, tmax = 0.0;
    const Comp* c = P.comps + fd.comp0 + (i < nfit ? i : 0);
    if (i < nfit) {
      if (c->ex == 0.0 && c->ey == 0.0) status = kIsotropic;
      else {
        tmin = order_value(c->tmin_key);
        tmax = order_value(c->tmax_key);
        length = tmax - tmin;
        status = length < min_length ? kShort : c->thickness > max_thickness ? kThick : kOk;
      }
      atomicAdd(&counts[status], 1);
    }
    int total;
    const int rank = base + block_scan_exclusive(status == kOk ? 1 : 0, &total);
    base += total;
    if (status == kOk && rank < max_segments) {
      const int xr = c->root % fd.width, yr = c->root / fd.width;
      const double bx = (double)xr + c->cx, by = (double)yr + c->cy;
      double x0 = bx + tmin * c->ex, y0 = by + tmin * c->ey, x1 = bx + tmax * c->ex, y1 = by + tmax * c->ey;
      if (!(c->ex * (double)c->sgy - c->ey * (double)c->sgx >= 0.0)) {
        double t = x0; x0 = x1; x1 = t;
        t = y0; y0 = y1; y1 = t;
      }
      const size_t o = (size_t)f * (size_t)max_segments + (size_t)rank;
      S.segments[4 * o + 0] = (float)x0; S.segments[4 * o + 1] = (float)y0;
      S.segments[4 * o + 2] = (float)x1; S.segments[4 * o + 3] = (float)y1;
      S.length[o] = length;
      S.thickness[o] = c->thickness;
      S.strength[o] = (double)c->sw / (double)c->n;
      S.npix[o] = c->n;
      S.label[o] = c->root;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FrameOut& o = P.out[f];
    o.num_ok = base;
    o.num_written = base < max_segments ? base : max_segments;
    o.counts[kOk] = counts[kOk];
    o.counts[kSmall] = o.num_components - nfit;
    o.counts[kIsotropic] = counts[kIsotropic];
    o.counts[kShort] = counts[kShort];
    o.counts[kThick] = counts[kThick];
  }
}

}  // namespace slslam_lsd

#endif  // SLSLAM_LINE_DETECT_H_

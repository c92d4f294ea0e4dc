// slslam_amd/csrc/po_covariance.h — posterior covariances of pose graphs: slslam_po_covariance and slslam_po_batch_covariance.
// Replaces nothing in the reference (its loop closures are judged by two fixed thresholds, src/slam.cpp:1215-1232); the Ceres
// counterpart is ceres::Covariance on the problem POProblem::build wires up.  Part of po_api.hip's translation unit.
//
// For a graph at its poses x, with J the Jacobian of every edge's six residuals w.r.t. the free poses (after the Huber corrector of
// po_huber_delta, no Jacobi scale, no damping) and H = J^T J:  Sigma = H^-1, of which the caller gets the 6 x 6 marginal of every pose and
// the cross blocks of the pairs it names.  Everything is fp64.  One launch sequence covers every graph of the call (work lists of
// (graph, block) items, as po_batch.h); the one-graph entry point runs the same kernels on a list of one.
//
//   k_pocov_begin      zeroes H, copies the poses the covariance is taken at, arms the graph's own LMState (the bodies below early-out on it)
//   k_pocov_linearise  po_linearise_body<kRobust, kWeighted> (blocks whitened by the edges' sqrt_information, when a graph has it) into the covariance's OWN normal matrix, scale == 1
//   k_pocov_diag / k_pocov_scale     d = 1 / sqrt(diag H),  H <- D H D  (unit diagonal: the pivot test is scale free)
//   k_pocov_potrf_diag / k_pocov_step   the blocked MFMA Cholesky of po_kernels.h (64 x 64 blocks, the diagonal blocks' inverses kept)
//   k_pocov_check      smallest pivot L_kk^2 of the unit-diagonal matrix <= 1e-10 (or a failed tile) -> SLSLAM_COV_SINGULAR
//   k_pocov_inverse    W = L^-1, block DIAGONAL by block diagonal: launch s computes every block W(k+s, k) = -linv_(k+s) sum_{k<=j<k+s}
//                      L(k+s, j) W(j, k) - it needs the diagonals before it only, all its workgroups carry the same s + 1 tile products
//                      (v_mfma_f64_16x16x4_f64) and none waits for another.  W overwrites H, which the factorisation has left dead.
//   k_pocov_blocks     one workgroup per requested block: Sigma_ab = D_a (sum_k W[k, a]^T W[k, b]) D_b over the rows below both slots;
//                      marginals and pairs through one work list, written at the caller's pose / pair index, zeros for a singular graph
#ifndef SLSLAM_PO_COVARIANCE_H_
#define SLSLAM_PO_COVARIANCE_H_

#include <algorithm>

namespace {

enum { kCovFill = 4096 };                     // matrix entries one workgroup of the fill and scale launches covers
constexpr double kCovPivot = 1e-10;           // singular rule: a pivot of the unit-diagonal matrix at or below this

struct PoCovItem { int graph, local; };
struct PoCovGraph {
  PoPtrs p;                                   // the covariance's own system: H (later W), scale == 1, g, scal, flags, st, x [6N]
  const double* x_src;                        // batch: the solve's two pose buffers and its state; one graph: nullptr (x0 is the point)
  const LMState* st_src;
  const double* x0;                           // the poses as added (batch: the point of a graph whose solve failed numerically)
  double* Lf;                                 // the Cholesky factor, n rows of ld
  double* linv;                               // inverses of its 64 x 64 diagonal blocks
  double* dsc;                                // [n] 1 / sqrt(diag H)
  const int* pa; const int* pb;               // [num_pairs] the caller's pairs
  int* status;                                // SLSLAM_COV_*
  double* cov_poses;                          // [36 N]
  double* cov_pairs;                          // [36 num_pairs]
  int num_pairs;
};

__device__ __forceinline__ void pocov_begin_body(const PoCovGraph& G, unsigned blk) {
  const PoPtrs& p = G.p;
  const int tid = threadIdx.x;
  const long long total = (long long)p.n * p.ld;
  for (int u = 0; u < kCovFill / 256; ++u) {
    const long long q = (long long)blk * kCovFill + u * 256 + tid;
    if (q < total) p.H[q] = 0.0;
  }
  if (blk != 0) return;
  for (int i = tid; i < p.n; i += 256) { p.g[i] = 0.0; p.scale[i] = 1.0; }
  const double* X = G.x0;
  if (G.st_src && G.st_src->status != SLSLAM_NUMERICAL_FAILURE) X = G.x_src + (long long)G.st_src->cur * 6 * p.N;
  for (int i = tid; i < 6 * p.N; i += 256) p.x[i] = X[i];
  if (tid < 8) p.scal[tid] = 0.0;
  if (tid == 0) { p.flags[0] = 0; p.flags[1] = 0; *G.status = SLSLAM_COV_OK; p.st->status = kRunning; p.st->cur = 0; }
}
__global__ __launch_bounds__(256) void k_pocov_begin(const PoCovGraph* gs, const PoCovItem* items) {
  const PoCovItem it = items[blockIdx.x];
  pocov_begin_body(gs[it.graph], (unsigned)it.local);
}
template <bool kRobust, bool kWeighted>
__global__ __launch_bounds__(64) void k_pocov_linearise(const PoCovGraph* gs, const PoCovItem* items) {
  const PoCovItem it = items[blockIdx.x];
  po_linearise_body<kRobust, kWeighted>(gs[it.graph].p, 0, (unsigned)it.local);
}
// d = 1 / sqrt(diag H); a free pose has an edge, so its diagonal is positive - 0 (then a zero pivot: singular) guards the rest
__global__ __launch_bounds__(256) void k_pocov_diag(const PoCovGraph* gs) {
  const PoCovGraph& G = gs[blockIdx.x];
  for (int i = threadIdx.x; i < G.p.n; i += 256) {
    const double h = G.p.H[(long long)i * G.p.ld + i];
    G.dsc[i] = (h > 0.0 && isfinite(h)) ? 1.0 / sqrt(h) : 0.0;
  }
}
__global__ __launch_bounds__(256) void k_pocov_scale(const PoCovGraph* gs, const PoCovItem* items) {
  const PoCovItem it = items[blockIdx.x];
  const PoCovGraph& G = gs[it.graph];
  const PoPtrs& p = G.p;
  const long long total = (long long)p.n * p.ld;
  for (int u = 0; u < kCovFill / 256; ++u) {
    const long long q = (long long)it.local * kCovFill + u * 256 + threadIdx.x;
    if (q >= total) continue;
    const int r = (int)(q / p.ld), c = (int)(q - (long long)r * p.ld);
    if (c <= r) p.H[q] *= G.dsc[r] * G.dsc[c];
  }
}
__global__ __launch_bounds__(256) void k_pocov_potrf_diag(const PoCovGraph* gs) {
  PoPtrs p = gs[blockIdx.x].p;
  po_potrf_diag_body<double>(p, p.H, gs[blockIdx.x].linv, 0, gs[blockIdx.x].Lf);
}
__global__ __launch_bounds__(256) void k_pocov_step(const PoCovGraph* gs, const PoCovItem* items, int bk) {
  const PoCovItem it = items[blockIdx.x];
  PoPtrs p = gs[it.graph].p;
  po_step_body<double>(p, p.H, gs[it.graph].Lf, gs[it.graph].linv, bk, (unsigned)it.local);
}
// the singular rule, per graph: the call does not fail, the graph's status says so and k_pocov_blocks writes zeros
__global__ __launch_bounds__(256) void k_pocov_check(const PoCovGraph* gs) {
  const PoCovGraph& G = gs[blockIdx.x];
  __shared__ int bad_s;
  if (threadIdx.x == 0) bad_s = G.p.flags[0] != 0;
  __syncthreads();
  int bad = 0;
  for (int i = threadIdx.x; i < G.p.n; i += 256) {
    const double l = G.Lf[(long long)i * G.p.ld + i];
    if (!(l * l > kCovPivot)) bad = 1;              // (a NaN is singular too)
  }
  if (bad) bad_s = 1;                               // (same value from every writer)
  __syncthreads();
  if (threadIdx.x == 0 && bad_s) *G.status = SLSLAM_COV_SINGULAR;
}

// acc += A(64 x 64) * B(64 x 64), both row-major tiles in LDS (leading dimension kLdT); 4 waves, wave w owns tile row w.
__device__ __forceinline__ void pocov_tile_mac_nn(const double* As, const double* Bs, int wave, int lane, v4f64 acc[4]) {
  const int rr = lane & 15, kk = lane >> 4;
  for (int k4 = 0; k4 < kNB / 4; ++k4) {
    const double a = As[(wave * 16 + rr) * kLdT + k4 * 4 + kk];
#pragma unroll
    for (int tc = 0; tc < 4; ++tc) acc[tc] = Mfma<double>::mac(a, Bs[(k4 * 4 + kk) * kLdT + tc * 16 + rr], acc[tc]);
  }
}

// Block (k + s, k) of W = L^-1 (blk = k).  s == 0: the kept inverse of the diagonal block, as a block of W (zeros above the diagonal).
__device__ __forceinline__ void pocov_inverse_body(const PoCovGraph& G, int s, unsigned blk) {
  const PoPtrs& p = G.p;
  if (p.st->status != kRunning) return;
  const int n = p.n, ld = p.ld;
  double* W = p.H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int k = (int)blk, i = k + s;
  const int c0 = k * kNB, r0 = i * kNB;
  if (s == 0) {
    const double* Li = G.linv + (size_t)k * kNB * kNB;
    for (int q = tid; q < kNB * kNB; q += 256) {
      const int r = q / kNB, c = q - r * kNB;
      if (r0 + r < n && c0 + c < n) W[(long long)(r0 + r) * ld + c0 + c] = Li[q];
    }
    return;
  }
  __shared__ double As[kNB * kLdT];
  __shared__ double Bs[kNB * kLdT];
  v4f64 acc[4];
  for (int tc = 0; tc < 4; ++tc) acc[tc] = Mfma<double>::zero();
  for (int j = k; j < i; ++j) {                     // (j < i <= the last block: block row j is full)
    __syncthreads();
    for (int q = tid; q < kNB * kNB; q += 256) {
      const int r = q / kNB, c = q - r * kNB;
      As[r * kLdT + c] = (r0 + r < n) ? G.Lf[(long long)(r0 + r) * ld + j * kNB + c] : 0.0;
      Bs[r * kLdT + c] = W[(long long)(j * kNB + r) * ld + c0 + c];
    }
    __syncthreads();
    pocov_tile_mac_nn(As, Bs, wave, lane, acc);
  }
  __syncthreads();
  const int col = lane & 15;
  const double* Li = G.linv + (size_t)i * kNB * kNB;
  for (int q = tid; q < kNB * kNB; q += 256) As[(q / kNB) * kLdT + (q % kNB)] = Li[q];
#pragma unroll
  for (int tc = 0; tc < 4; ++tc)
#pragma unroll
    for (int q = 0; q < 4; ++q) Bs[(wave * 16 + Mfma<double>::row(lane, q)) * kLdT + tc * 16 + col] = acc[tc][q];
  __syncthreads();
  for (int tc = 0; tc < 4; ++tc) acc[tc] = Mfma<double>::zero();
  pocov_tile_mac_nn(As, Bs, wave, lane, acc);
  for (int tc = 0; tc < 4; ++tc)
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + wave * 16 + Mfma<double>::row(lane, q), c = c0 + tc * 16 + col;
      if (r < n && c < n) W[(long long)r * ld + c] = -acc[tc][q];
    }
}
__global__ __launch_bounds__(256) void k_pocov_inverse(const PoCovGraph* gs, const PoCovItem* items, int s) {
  const PoCovItem it = items[blockIdx.x];
  pocov_inverse_body(gs[it.graph], s, (unsigned)it.local);
}

// One requested block: blk < N the marginal of pose blk, otherwise pair blk - N.
__device__ __forceinline__ void pocov_block_body(const PoCovGraph& G, unsigned blk) {
  const PoPtrs& p = G.p;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int a, b;
  double* out;
  if ((int)blk < p.N) { a = b = (int)blk; out = G.cov_poses + 36 * (size_t)blk; }
  else { const int k = (int)blk - p.N; a = G.pa[k]; b = G.pb[k]; out = G.cov_pairs + 36 * (size_t)k; }
  const int sa = p.slot[a], sb = p.slot[b];
  if (*G.status != SLSLAM_COV_OK || sa < 0 || sb < 0) {          // (workgroup-uniform)
    if (tid < 36) out[tid] = 0.0;
    return;
  }
  const double* W = p.H;
  double acc[36];
#pragma unroll
  for (int q = 0; q < 36; ++q) acc[q] = 0.0;
  for (int k = max(sa, sb) + tid; k < p.n; k += 256) {          // W is lower triangular: rows above both slots hold nothing
    double wa[6], wb[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      wa[i] = (sa + i <= k) ? W[(long long)k * p.ld + sa + i] : 0.0;
      wb[i] = (sb + i <= k) ? W[(long long)k * p.ld + sb + i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[6 * i + j] = fma(wa[i], wb[j], acc[6 * i + j]);
  }
  __shared__ double part[4][36];
#pragma unroll
  for (int q = 0; q < 36; ++q) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (tid < 36) {
    const int i = tid / 6, j = tid - 6 * i;
    out[tid] = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) * G.dsc[sa + i] * G.dsc[sb + j];
  }
}
__global__ __launch_bounds__(256) void k_pocov_blocks(const PoCovGraph* gs, const PoCovItem* items) {
  const PoCovItem it = items[blockIdx.x];
  pocov_block_body(gs[it.graph], (unsigned)it.local);
}

// ---- host: one plan for the graphs of a call (a batch keeps its plan; the one-graph call builds one per call)
struct PoCovInput {
  int N = 0, E = 0, n = 0, ld = 0;
  const int *d_p1 = nullptr, *d_p2 = nullptr, *d_slot = nullptr;   // device arrays of the graph
  const double* d_cons = nullptr;
  const double* d_winfo = nullptr;                                 // [36E] the edges' square-root information, or null: identity
  const double* d_x_src = nullptr; const LMState* d_st_src = nullptr; const double* d_x0 = nullptr;
  const int *pa = nullptr, *pb = nullptr;                          // host: the pairs
  int P = 0;
};
struct PoCovPlan {
  int A = 0;
  bool robust = false;
  bool weighted = false;                      // some graph has sqrt_information: the whitening instantiation of k_pocov_linearise runs
  PoCovGraph* d_graphs = nullptr;
  PoCovItem* d_items = nullptr;
  int fill_off = 0, fill_cnt = 0, edge_off = 0, edge_cnt = 0, block_off = 0, block_cnt = 0;
  std::vector<int> step_off, step_cnt, inv_off, inv_cnt;
  size_t down_off = 0, down_bytes = 0;        // what comes back: [ status | per graph: marginals, pairs ]
  size_t img_off = 0, img_bytes = 0;          // what the host uploads: descriptors, work lists, pairs
  size_t o_status = 0;
  std::vector<size_t> o_poses, o_pairs;       // offsets in the down region
};

constexpr size_t kCovStepLds = kPoStepLdsTiles * kNB * kLdT * sizeof(double);

// Lays the plan out in a device block from offset carve.off on.  dev == nullptr: sizes only.  img (when given) receives the upload image,
// img_bytes long, to be copied to dev + img_off.  Returns the offset behind the plan.
size_t po_cov_layout(const std::vector<PoCovInput>& in, double huber, PoCarve carve, char* dev, std::vector<char>* img, PoCovPlan* P) {
  const int A = (int)in.size();
  P->A = A;
  P->robust = huber > 0.0;
  P->weighted = false;
  for (const PoCovInput& g : in) P->weighted = P->weighted || g.d_winfo != nullptr;
  P->down_off = carve.off;
  P->o_status = carve.take(sizeof(int) * (size_t)A) - P->down_off;
  P->o_poses.assign((size_t)A, 0); P->o_pairs.assign((size_t)A, 0);
  for (int a = 0; a < A; ++a) {
    P->o_poses[(size_t)a] = carve.take(sizeof(double) * 36 * (size_t)in[(size_t)a].N) - P->down_off;
    P->o_pairs[(size_t)a] = carve.take(sizeof(double) * 36 * (size_t)in[(size_t)a].P) - P->down_off;
  }
  P->down_bytes = carve.off - P->down_off;
  std::vector<PoCovItem> items;
  auto list = [&](int& o, int& cnt, auto&& fill) { o = (int)items.size(); fill(); cnt = (int)items.size() - o; };
  int max_blk = 0;
  for (const PoCovInput& g : in) max_blk = std::max(max_blk, (g.n + kNB - 1) / kNB);
  list(P->fill_off, P->fill_cnt, [&] {
    for (int a = 0; a < A; ++a) {
      const long long total = (long long)in[(size_t)a].n * in[(size_t)a].ld;
      for (long long k = 0; k < (total + kCovFill - 1) / kCovFill; ++k) items.push_back(PoCovItem{ a, (int)k });
    }
  });
  list(P->edge_off, P->edge_cnt, [&] {
    for (int a = 0; a < A; ++a) for (int k = 0; k < (in[(size_t)a].E + 4) / 5; ++k) items.push_back(PoCovItem{ a, k });
  });
  list(P->block_off, P->block_cnt, [&] {
    for (int a = 0; a < A; ++a) for (int k = 0; k < in[(size_t)a].N + in[(size_t)a].P; ++k) items.push_back(PoCovItem{ a, k });
  });
  const int steps = std::max(max_blk - 1, 0);
  P->step_off.assign((size_t)steps, 0); P->step_cnt.assign((size_t)steps, 0);
  for (int bk = 0; bk < steps; ++bk)
    list(P->step_off[(size_t)bk], P->step_cnt[(size_t)bk], [&] {
      for (int a = 0; a < A; ++a) {
        const int tb = (in[(size_t)a].n + kNB - 1) / kNB - 1 - bk;
        for (int t = 0; tb > 0 && t < tb * (tb + 1) / 2; ++t) items.push_back(PoCovItem{ a, t });
      }
    });
  P->inv_off.assign((size_t)max_blk, 0); P->inv_cnt.assign((size_t)max_blk, 0);
  for (int s = 0; s < max_blk; ++s)
    list(P->inv_off[(size_t)s], P->inv_cnt[(size_t)s], [&] {
      for (int a = 0; a < A; ++a) {
        const int nblk = (in[(size_t)a].n + kNB - 1) / kNB;
        for (int k = 0; k + s < nblk; ++k) items.push_back(PoCovItem{ a, k });
      }
    });
  P->img_off = carve.off;
  const size_t o_graphs = carve.take(sizeof(PoCovGraph) * (size_t)A), o_items = carve.take(sizeof(PoCovItem) * items.size());
  std::vector<size_t> o_pa((size_t)A), o_pb((size_t)A);
  for (int a = 0; a < A; ++a) { o_pa[(size_t)a] = carve.take(sizeof(int) * (size_t)in[(size_t)a].P); o_pb[(size_t)a] = carve.take(sizeof(int) * (size_t)in[(size_t)a].P); }
  P->img_bytes = carve.off - P->img_off;
  std::vector<PoCovGraph> desc((size_t)A);
  for (int a = 0; a < A; ++a) {
    const PoCovInput& g = in[(size_t)a];
    const size_t nn = (size_t)std::max(g.n, 1), nblk = (size_t)std::max((g.n + kNB - 1) / kNB, 1);
    const size_t o_H = carve.take(sizeof(double) * nn * g.ld), o_Lf = carve.take(sizeof(double) * nn * g.ld), o_linv = carve.take(sizeof(double) * kNB * kNB * nblk),
                 o_d = carve.take(sizeof(double) * nn), o_scale = carve.take(sizeof(double) * nn), o_g = carve.take(sizeof(double) * nn),
                 o_x = carve.take(sizeof(double) * 6 * (size_t)std::max(g.N, 1)), o_scal = carve.take(sizeof(double) * 8), o_flags = carve.take(sizeof(int) * 2),
                 o_st = carve.take(sizeof(LMState));
    if (!dev) continue;
    PoCovGraph& D = desc[(size_t)a];
    std::memset(&D, 0, sizeof(D));
    PoPtrs& p = D.p;
    p.p1 = g.d_p1; p.p2 = g.d_p2; p.slot = g.d_slot; p.cons = g.d_cons;
    p.x = (double*)(dev + o_x); p.scale = (double*)(dev + o_scale); p.H = (double*)(dev + o_H); p.g = (double*)(dev + o_g);
    p.scal = (double*)(dev + o_scal); p.flags = (int*)(dev + o_flags); p.st = (LMState*)(dev + o_st);
    p.N = g.N; p.E = g.E; p.n = g.n; p.ld = g.ld; p.huber = huber; p.winfo = g.d_winfo;
    D.x_src = g.d_x_src; D.st_src = g.d_st_src; D.x0 = g.d_x0;
    D.Lf = (double*)(dev + o_Lf); D.linv = (double*)(dev + o_linv); D.dsc = (double*)(dev + o_d);
    D.pa = (const int*)(dev + o_pa[(size_t)a]); D.pb = (const int*)(dev + o_pb[(size_t)a]);
    D.status = (int*)(dev + P->down_off + P->o_status) + a;
    D.cov_poses = (double*)(dev + P->down_off + P->o_poses[(size_t)a]); D.cov_pairs = (double*)(dev + P->down_off + P->o_pairs[(size_t)a]);
    D.num_pairs = g.P;
  }
  if (dev && img) {
    img->assign(P->img_bytes, 0);
    char* im = img->data() - P->img_off;
    std::memcpy(im + o_graphs, desc.data(), sizeof(PoCovGraph) * desc.size());
    if (!items.empty()) std::memcpy(im + o_items, items.data(), sizeof(PoCovItem) * items.size());
    for (int a = 0; a < A; ++a)
      if (in[(size_t)a].P > 0) {
        std::memcpy(im + o_pa[(size_t)a], in[(size_t)a].pa, sizeof(int) * (size_t)in[(size_t)a].P);
        std::memcpy(im + o_pb[(size_t)a], in[(size_t)a].pb, sizeof(int) * (size_t)in[(size_t)a].P);
      }
    P->d_graphs = (PoCovGraph*)(dev + o_graphs); P->d_items = (PoCovItem*)(dev + o_items);
  }
  return carve.off;
}

// (k_pocov_step keeps three 64 x 66 tiles in dynamic LDS, as k_po_step does: the limit is raised per device)
hipError_t po_cov_lds_attribute() {
  return hipFuncSetAttribute((const void*)k_pocov_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCovStepLds);
}

// The whole launch sequence, every step once over all graphs.
int po_cov_enqueue(const PoCovPlan& P, hipStream_t s) {
  if (P.A == 0) return SLSLAM_OK;
  const PoCovGraph* gs = P.d_graphs;
  const PoCovItem* items = P.d_items;
  const dim3 per_graph((unsigned)P.A);
  hipLaunchKernelGGL(k_pocov_begin, dim3((unsigned)P.fill_cnt), dim3(256), 0, s, gs, items + P.fill_off);
  const dim3 g_edges((unsigned)P.edge_cnt);
  if (P.weighted) {
    if (P.robust) hipLaunchKernelGGL((k_pocov_linearise<true, true>), g_edges, dim3(64), 0, s, gs, items + P.edge_off);
    else hipLaunchKernelGGL((k_pocov_linearise<false, true>), g_edges, dim3(64), 0, s, gs, items + P.edge_off);
  } else if (P.robust) hipLaunchKernelGGL((k_pocov_linearise<true, false>), g_edges, dim3(64), 0, s, gs, items + P.edge_off);
  else hipLaunchKernelGGL((k_pocov_linearise<false, false>), g_edges, dim3(64), 0, s, gs, items + P.edge_off);
  hipLaunchKernelGGL(k_pocov_diag, per_graph, dim3(256), 0, s, gs);
  hipLaunchKernelGGL(k_pocov_scale, dim3((unsigned)P.fill_cnt), dim3(256), 0, s, gs, items + P.fill_off);
  hipLaunchKernelGGL(k_pocov_potrf_diag, per_graph, dim3(256), 0, s, gs);
  for (size_t bk = 0; bk < P.step_cnt.size(); ++bk)
    if (P.step_cnt[bk] > 0) hipLaunchKernelGGL(k_pocov_step, dim3((unsigned)P.step_cnt[bk]), dim3(256), kCovStepLds, s, gs, items + P.step_off[bk], (int)bk);
  hipLaunchKernelGGL(k_pocov_check, per_graph, dim3(256), 0, s, gs);
  for (size_t d = 0; d < P.inv_cnt.size(); ++d)
    if (P.inv_cnt[d] > 0) hipLaunchKernelGGL(k_pocov_inverse, dim3((unsigned)P.inv_cnt[d]), dim3(256), 0, s, gs, items + P.inv_off[d], (int)d);
  if (P.block_cnt > 0) hipLaunchKernelGGL(k_pocov_blocks, dim3((unsigned)P.block_cnt), dim3(256), 0, s, gs, items + P.block_off);
  HIP_TRY(hipGetLastError());
  return SLSLAM_OK;
}

// pair lists as the C ABI takes them: indices in [0, N)
bool po_cov_pairs_ok(int N, int num_pairs, const int* pa, const int* pb) {
  if (num_pairs < 0 || (num_pairs > 0 && (!pa || !pb))) return false;
  for (int k = 0; k < num_pairs; ++k) if (pa[k] < 0 || pa[k] >= N || pb[k] < 0 || pb[k] >= N) return false;
  return true;
}

}  // namespace

// ceres::Covariance for ONE graph at graph->parameters, no solve, synchronous.
extern "C" int slslam_po_covariance(const slslam_po_graph* g, double po_huber_delta, int num_pairs, const int* pair_a, const int* pair_b,
                                    int* status, double* cov_poses, double* cov_pairs) {
  if (!g || !po_graph_arrays_ok(g, true) || !po_huber_ok(po_huber_delta) || !po_graph_entries_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (num_pairs < 0 || (cov_pairs && num_pairs > 0 && (!pair_a || !pair_b))) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (pair_a && pair_b && !po_cov_pairs_ok(g->num_poses, num_pairs, pair_a, pair_b)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  const int N = g->num_poses, E = g->num_edges;
  const int P = (cov_pairs && pair_a && pair_b) ? num_pairs : 0;
  if (status) *status = SLSLAM_COV_OK;
  if (cov_poses && N > 0) std::memset(cov_poses, 0, sizeof(double) * 36 * (size_t)N);
  if (cov_pairs && num_pairs > 0) std::memset(cov_pairs, 0, sizeof(double) * 36 * (size_t)num_pairs);
  if (E == 0) return SLSLAM_OK;                  // no free pose: every block is zero
  try {
    PoSymbolic S;
    po_analyse(N, E, g->pose_index_1, g->pose_index_2, false, &S);      // the free poses in index order: the inverse needs no chains
    PoCarve a;
    const size_t o_p1 = a.take(sizeof(int) * E), o_p2 = a.take(sizeof(int) * E), o_slot = a.take(sizeof(int) * N), o_cons = a.take(sizeof(double) * 6 * E),
                 o_x = a.take(sizeof(double) * 6 * N), o_winfo = a.take(g->sqrt_information ? sizeof(double) * 36 * E : 0), up_bytes = a.off;
    std::vector<PoCovInput> in(1);
    PoCovInput& I = in[0];
    I.N = N; I.E = E; I.n = S.n; I.ld = S.ld; I.pa = pair_a; I.pb = pair_b; I.P = P;
    PoCovPlan plan;
    struct Block {                          // the calling thread's cached device block, handed back on every path
      char* p = nullptr; size_t bytes = 0; int device = 0;
      ~Block() { DeviceBlockCache::give_back(p, bytes, device); }
    } blk;
    blk.bytes = po_cov_layout(in, po_huber_delta, a, nullptr, nullptr, &plan);
    HIP_TRY(hipGetDevice(&blk.device));
    HIP_TRY(DeviceBlockCache::acquire(blk.bytes, blk.device, &blk.p));
    HIP_TRY(po_cov_lds_attribute());
    I.d_p1 = (const int*)(blk.p + o_p1); I.d_p2 = (const int*)(blk.p + o_p2); I.d_slot = (const int*)(blk.p + o_slot);
    I.d_cons = (const double*)(blk.p + o_cons); I.d_x0 = (const double*)(blk.p + o_x);
    if (g->sqrt_information) I.d_winfo = (const double*)(blk.p + o_winfo);
    std::vector<char> img, up(up_bytes);
    po_cov_layout(in, po_huber_delta, a, blk.p, &img, &plan);
    std::memcpy(up.data() + o_p1, g->pose_index_1, sizeof(int) * E); std::memcpy(up.data() + o_p2, g->pose_index_2, sizeof(int) * E);
    std::memcpy(up.data() + o_slot, S.slot.data(), sizeof(int) * N); std::memcpy(up.data() + o_cons, g->constraints, sizeof(double) * 6 * E);
    std::memcpy(up.data() + o_x, g->parameters, sizeof(double) * 6 * N);
    if (g->sqrt_information) std::memcpy(up.data() + o_winfo, g->sqrt_information, sizeof(double) * 36 * E);
    HIP_TRY(hipMemcpy(blk.p, up.data(), up_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(blk.p + plan.img_off, img.data(), plan.img_bytes, hipMemcpyHostToDevice));
    const int rc = po_cov_enqueue(plan, 0);
    if (rc != SLSLAM_OK) return rc;
    std::vector<char> down(plan.down_bytes);
    HIP_TRY(hipMemcpy(down.data(), blk.p + plan.down_off, plan.down_bytes, hipMemcpyDeviceToHost));
    if (status) std::memcpy(status, down.data() + plan.o_status, sizeof(int));
    if (cov_poses) std::memcpy(cov_poses, down.data() + plan.o_poses[0], sizeof(double) * 36 * (size_t)N);
    if (P > 0) std::memcpy(cov_pairs, down.data() + plan.o_pairs[0], sizeof(double) * 36 * (size_t)P);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

#endif  // SLSLAM_PO_COVARIANCE_H_

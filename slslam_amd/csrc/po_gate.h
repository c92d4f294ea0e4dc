// slslam_amd/csrc/po_gate.h — statistics of a pose-graph edge under the posterior covariance of its two poses: slslam_po_edge_statistics,
// slslam_po_gate (the batch entry points are in po_batch.h).  Serves what the reference decides by two fixed thresholds
// (consistency_broken(), src/slam.cpp:1215-1232) and the odometry constraints it builds at src/slam.cpp:1403-1416, which it leaves
// unweighted.  Part of po_api.hip's translation unit, behind po_covariance.h.
//
// One item: poses x_a, x_b, a constraint C, the joint covariance blocks Sigma_aa, Sigma_bb, Sigma_ab (rows of a, columns of b) and a
// measurement covariance R (any of the four absent: zeros).  With Te = pose_constraint_error(x_a, x_b, C) - the solve's functor, unwhitened -
// and [Ja | Jb] its 6 x 12 Jacobian by the dual numbers of po_kernels.h:
//   S  = sigma2 (Ja Saa Ja^T + Jb Sbb Jb^T + Ja Sab Jb^T + Jb Sab^T Ja^T) + R      (the lower triangle of R is read)
//   W  lower triangular, W^T W = S^-1, by the rule of slslam_po_sqrt_information: Cholesky after scaling to unit diagonal, a scaled pivot
//      <= kCovPivot (or a diagonal entry <= 0) -> SLSLAM_COV_SINGULAR: zeros for S, W, m2, the error still written
//   m2 = |W Te|^2 = Te^T S^-1 Te
//
// po_edge_stat_body: lane <-> (item, column d of [Ja | Jb]), five items per wave, as po_linearise_body.  fp64, no atomics, every sum in
// a fixed order: the same bits run to run.
//   1  every lane evaluates the functor on duals seeded in its column: all six Te[q].v and its column Te[q].d      -> Js[item][d][.]  (LDS)
//   2  lane d: row d of the 12 x 12 joint covariance (read from the three blocks) times J^T                         -> Vs[item][d][.]
//   3  the 21 entries of the lower triangle of J V, two per lane, summed over d = 0 .. 11, times sigma2, plus R      -> Ss[item]  (mirrored)
//   4  lane d == 0 of each item: scaling, chol6_and_inverse in registers (static indices only), W and m2            -> Ws[item]
//   5  all twelve lanes copy the item's results out
#ifndef SLSLAM_PO_GATE_H_
#define SLSLAM_PO_GATE_H_

namespace {

struct PoEdgeIn { const double *xa, *xb, *c, *saa, *sbb, *sab, *r; };    // one item's inputs; saa, sbb, sab, r may be null: zeros
struct PoEdgeOut { int* status; double *err, *cov, *W, *m2; };           // one item's outputs

// ok: the lane has an item (otherwise `in` points at some valid item and nothing is written).  graph_singular: the covariance the
// blocks come from does not exist - the item is singular whatever its numbers.
__device__ __forceinline__ void po_edge_stat_body(const PoEdgeIn& in, const PoEdgeOut& out, bool ok, bool graph_singular, double sigma2) {
  const int lane = threadIdx.x;
  const int el = lane / 12, d = lane - 12 * el;
  const int e5 = el < 5 ? el : 4;                    // (lanes 60 .. 63 have no item: they read item 4's tiles and write nothing)
  __shared__ double Js[5][12][6];
  __shared__ double Vs[5][12][6];                    // step 4 reuses an item's first 36 entries for the scaled matrix
  __shared__ double Ss[5][36];
  __shared__ double Ws[5][37];                       // [36]: m2
  __shared__ int St[5];
  Dual T1[6], T2[6], C[6], Te[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    T1[i] = mk(in.xa[i], d == i ? 1.0 : 0.0);
    T2[i] = mk(in.xb[i], d == 6 + i ? 1.0 : 0.0);
    C[i] = mk(in.c[i]);
  }
  pose_constraint_error<Dual>(T1, T2, C, Te);
  if (el < 5) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Js[el][d][q] = Te[q].d;
  }
  __syncthreads();
  {
    double v[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    const bool first = d < 6;
    const int r6 = first ? d : d - 6;
    for (int dp = 0; dp < 12; ++dp) {
      const bool left = dp < 6;
      const int c6 = left ? dp : dp - 6;
      // row d of [[Saa, Sab], [Sab^T, Sbb]]
      const double* blk = first ? (left ? in.saa : in.sab) : (left ? in.sab : in.sbb);
      const int idx = (first || !left) ? 6 * r6 + c6 : 6 * c6 + r6;
      const double s = blk ? blk[idx] : 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] = fma(s, Js[e5][dp][q], v[q]);
    }
    if (el < 5) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Vs[el][d][q] = v[q];
    }
  }
  __syncthreads();
  for (int k = d; k < 21 && el < 5; k += 12) {       // entry k of the packed lower triangle: (p, q), q <= p
    int p = 0;
    while ((p + 1) * (p + 2) / 2 <= k) ++p;
    const int q = k - p * (p + 1) / 2;
    double s = 0.0;
    for (int dd = 0; dd < 12; ++dd) s = fma(Js[el][dd][p], Vs[el][dd][q], s);
    s = sigma2 * s + (in.r ? in.r[6 * p + q] : 0.0);
    Ss[el][6 * p + q] = s;
    Ss[el][6 * q + p] = s;
  }
  __syncthreads();
  if (el < 5 && d == 0) {
    double* Cs = &Vs[el][0][0];                      // (the item's V is dead; this lane alone touches Cs)
    double dsc[6];
    bool good = !graph_singular;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double h = Ss[el][7 * i];
      if (!(h > 0.0) || !isfinite(h)) good = false;
      dsc[i] = good ? 1.0 / sqrt(h) : 1.0;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) Cs[6 * i + j] = i == j ? 1.0 : dsc[i] * Ss[el][6 * i + j] * dsc[j];
    double L[21], Li[21];
    if (!chol6_and_inverse(Cs, L, Li)) good = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double l = L[(i * (i + 1)) / 2 + i];
      if (!(l * l > kCovPivot)) good = false;        // (a NaN is singular too)
    }
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double y = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double w = (good && j <= i) ? Li[(i * (i + 1)) / 2 + (j <= i ? j : 0)] * dsc[j] : 0.0;
        Ws[el][6 * i + j] = w;
        y = fma(w, Te[j].v, y);
      }
      m2 = fma(y, y, m2);
    }
    Ws[el][36] = good ? m2 : 0.0;
    St[el] = good ? SLSLAM_COV_OK : SLSLAM_COV_SINGULAR;
  }
  __syncthreads();
  if (!ok) return;
  const bool good = St[el] == SLSLAM_COV_OK;
  for (int k = d; k < 36; k += 12) {
    out.cov[k] = good ? Ss[el][k] : 0.0;
    out.W[k] = Ws[el][k];
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) if (d == q) out.err[q] = Te[q].v;
  if (d == 6) *out.status = St[el];
  if (d == 7) *out.m2 = Ws[el][36];
}

// ---- the primitive: n independent items in flat arrays
struct PoEdgeArrays {
  const double *pa, *pb, *c, *saa, *sbb, *sab, *r;   // [6n] x 3, [36n] x 4 (the last four may be null)
  int n;
  double sigma2;
  int* status; double *err, *cov, *W, *m2;            // [n], [6n], [36n], [36n], [n]
};
__global__ __launch_bounds__(64) void k_po_edge_stat(PoEdgeArrays A) {
  const int el = (int)threadIdx.x / 12;
  const long long i = (long long)blockIdx.x * 5 + el;
  const bool ok = el < 5 && i < A.n;
  const size_t s = ok ? (size_t)i : 0;               // (the launch has n >= 1: item 0 exists)
  PoEdgeIn in;
  in.xa = A.pa + 6 * s; in.xb = A.pb + 6 * s; in.c = A.c + 6 * s;
  in.saa = A.saa ? A.saa + 36 * s : nullptr; in.sbb = A.sbb ? A.sbb + 36 * s : nullptr;
  in.sab = A.sab ? A.sab + 36 * s : nullptr; in.r = A.r ? A.r + 36 * s : nullptr;
  PoEdgeOut out;
  out.status = A.status + s; out.err = A.err + 6 * s; out.cov = A.cov + 36 * s; out.W = A.W + 36 * s; out.m2 = A.m2 + s;
  po_edge_stat_body(in, out, ok, false, A.sigma2);
}

// ---- the gate: candidates of the graphs of a covariance plan.  A graph's candidates are the LAST `num` pairs of its plan (behind the
// caller's own pairs, from pair_off on), so Sigma_ab is where k_pocov_blocks has just written it, Sigma_aa / Sigma_bb are the marginals
// (zeros for the constant pose) and the poses are the plan's copy: nothing leaves the device but the results below.
struct PoGateGraph {
  const double* cons;                                // [6 num]
  const double* rmeas;                               // [36 num] or null
  double sigma2;
  int pair_off, num;
  int* cov_status;                                   // the graph's SLSLAM_COV_*, copied beside the results
  int* status; double *err, *cov, *W, *m2;
};
__global__ __launch_bounds__(64) void k_po_gate(const PoCovGraph* gs, const PoGateGraph* qs, const PoCovItem* items) {
  const PoCovItem it = items[blockIdx.x];
  const PoCovGraph& G = gs[it.graph];
  const PoGateGraph& Q = qs[it.graph];
  const int el = (int)threadIdx.x / 12;
  const int k = it.local * 5 + el;
  const bool ok = el < 5 && k < Q.num;
  const size_t s = ok ? (size_t)k : 0;               // (a listed graph has num >= 1)
  const int a = G.pa[Q.pair_off + s], b = G.pb[Q.pair_off + s];
  const int cov_status = *G.status;
  PoEdgeIn in;
  in.xa = G.p.x + 6 * (size_t)a; in.xb = G.p.x + 6 * (size_t)b; in.c = Q.cons + 6 * s;
  in.saa = G.cov_poses + 36 * (size_t)a; in.sbb = G.cov_poses + 36 * (size_t)b;
  in.sab = G.cov_pairs + 36 * ((size_t)Q.pair_off + s);
  in.r = Q.rmeas ? Q.rmeas + 36 * s : nullptr;
  PoEdgeOut out;
  out.status = Q.status + s; out.err = Q.err + 6 * s; out.cov = Q.cov + 36 * s; out.W = Q.W + 36 * s; out.m2 = Q.m2 + s;
  if (it.local == 0 && threadIdx.x == 63) *Q.cov_status = cov_status;
  po_edge_stat_body(in, out, ok, cov_status != SLSLAM_COV_OK, Q.sigma2);
}

// ---- host
struct PoGateInput {                                 // one graph of the plan (host pointers)
  int num = 0, pair_off = 0;
  const double* cons = nullptr;
  const double* rmeas = nullptr;
  double sigma2 = 1.0;
};
struct PoGatePlan {
  int A = 0, item_cnt = 0;
  PoGateGraph* d_graphs = nullptr;
  PoCovItem* d_items = nullptr;
  size_t down_off = 0, down_bytes = 0;               // what comes back, per graph: cov_status | status | err | cov | W | m2
  size_t img_off = 0, img_bytes = 0;                 // what the host uploads: descriptors, work list, constraints, R
  std::vector<size_t> o_cov_status, o_status, o_err, o_cov, o_W, o_m2;      // offsets in the down region
};

// As po_cov_layout: dev == nullptr sizes only; img receives the upload image for dev + img_off.  Returns the offset behind the plan.
size_t po_gate_layout(const std::vector<PoGateInput>& in, PoCarve carve, char* dev, std::vector<char>* img, PoGatePlan* P) {
  const int A = (int)in.size();
  P->A = A;
  P->down_off = carve.off;
  for (auto* v : { &P->o_cov_status, &P->o_status, &P->o_err, &P->o_cov, &P->o_W, &P->o_m2 }) v->assign((size_t)A, 0);
  for (int a = 0; a < A; ++a) {
    const size_t m = (size_t)in[(size_t)a].num;
    P->o_cov_status[(size_t)a] = carve.take(sizeof(int)) - P->down_off;
    P->o_status[(size_t)a] = carve.take(sizeof(int) * m) - P->down_off;
    P->o_err[(size_t)a] = carve.take(sizeof(double) * 6 * m) - P->down_off;
    P->o_cov[(size_t)a] = carve.take(sizeof(double) * 36 * m) - P->down_off;
    P->o_W[(size_t)a] = carve.take(sizeof(double) * 36 * m) - P->down_off;
    P->o_m2[(size_t)a] = carve.take(sizeof(double) * m) - P->down_off;
  }
  P->down_bytes = carve.off - P->down_off;
  std::vector<PoCovItem> items;
  for (int a = 0; a < A; ++a) for (int k = 0; k < (in[(size_t)a].num + 4) / 5; ++k) items.push_back(PoCovItem{ a, k });
  P->item_cnt = (int)items.size();
  P->img_off = carve.off;
  const size_t o_graphs = carve.take(sizeof(PoGateGraph) * (size_t)A), o_items = carve.take(sizeof(PoCovItem) * items.size());
  std::vector<size_t> o_cons((size_t)A), o_r((size_t)A);
  for (int a = 0; a < A; ++a) {
    const size_t m = (size_t)in[(size_t)a].num;
    o_cons[(size_t)a] = carve.take(sizeof(double) * 6 * m);
    o_r[(size_t)a] = carve.take(in[(size_t)a].rmeas ? sizeof(double) * 36 * m : 0);
  }
  P->img_bytes = carve.off - P->img_off;
  if (!dev || !img) return carve.off;
  img->assign(P->img_bytes, 0);
  char* im = img->data() - P->img_off;
  std::vector<PoGateGraph> desc((size_t)A);
  for (int a = 0; a < A; ++a) {
    const PoGateInput& g = in[(size_t)a];
    const size_t m = (size_t)g.num;
    PoGateGraph& D = desc[(size_t)a];
    std::memset(&D, 0, sizeof(D));
    D.cons = (const double*)(dev + o_cons[(size_t)a]);
    D.rmeas = g.rmeas ? (const double*)(dev + o_r[(size_t)a]) : nullptr;
    D.sigma2 = g.sigma2; D.pair_off = g.pair_off; D.num = g.num;
    char* down = dev + P->down_off;
    D.cov_status = (int*)(down + P->o_cov_status[(size_t)a]); D.status = (int*)(down + P->o_status[(size_t)a]);
    D.err = (double*)(down + P->o_err[(size_t)a]); D.cov = (double*)(down + P->o_cov[(size_t)a]);
    D.W = (double*)(down + P->o_W[(size_t)a]); D.m2 = (double*)(down + P->o_m2[(size_t)a]);
    if (m > 0) std::memcpy(im + o_cons[(size_t)a], g.cons, sizeof(double) * 6 * m);
    if (m > 0 && g.rmeas) std::memcpy(im + o_r[(size_t)a], g.rmeas, sizeof(double) * 36 * m);
  }
  std::memcpy(im + o_graphs, desc.data(), sizeof(PoGateGraph) * desc.size());
  if (!items.empty()) std::memcpy(im + o_items, items.data(), sizeof(PoCovItem) * items.size());
  P->d_graphs = (PoGateGraph*)(dev + o_graphs); P->d_items = (PoCovItem*)(dev + o_items);
  return carve.off;
}

// behind po_cov_enqueue of the plan the gate plan was laid out for
int po_gate_enqueue(const PoCovPlan& C, const PoGatePlan& P, hipStream_t s) {
  if (P.item_cnt == 0) return SLSLAM_OK;
  hipLaunchKernelGGL(k_po_gate, dim3((unsigned)P.item_cnt), dim3(64), 0, s, (const PoCovGraph*)C.d_graphs, (const PoGateGraph*)P.d_graphs, (const PoCovItem*)P.d_items);
  HIP_TRY(hipGetLastError());
  return SLSLAM_OK;
}

// One graph's results out of a downloaded gate region (any output may be null).
void po_gate_read(const PoGatePlan& P, const char* down, int a, int num, int* cov_status, int* status, double* error, double* cov, double* W, double* m2) {
  const size_t m = (size_t)num, g = (size_t)a;
  if (cov_status) std::memcpy(cov_status, down + P.o_cov_status[g], sizeof(int));
  if (status && m) std::memcpy(status, down + P.o_status[g], sizeof(int) * m);
  if (error && m) std::memcpy(error, down + P.o_err[g], sizeof(double) * 6 * m);
  if (cov && m) std::memcpy(cov, down + P.o_cov[g], sizeof(double) * 36 * m);
  if (W && m) std::memcpy(W, down + P.o_W[g], sizeof(double) * 36 * m);
  if (m2 && m) std::memcpy(m2, down + P.o_m2[g], sizeof(double) * m);
}

bool po_all_finite(const double* v, size_t count) {
  for (size_t i = 0; v && i < count; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}
bool po_sigma2_ok(double s) { return std::isfinite(s) && s > 0.0; }

// a candidate list as the C ABI takes it, against a graph of N poses
bool po_candidates_ok(int N, const slslam_po_candidates* c) {
  if (!c || c->num < 0 || !po_sigma2_ok(c->sigma2)) return false;
  if (c->num == 0) return true;
  if (!c->pose_a || !c->pose_b || !c->constraints) return false;
  for (int k = 0; k < c->num; ++k) {
    const int a = c->pose_a[k], b = c->pose_b[k];
    if (a < 0 || a >= N || b < 0 || b >= N || a == b) return false;
  }
  return po_all_finite(c->constraints, (size_t)6 * c->num) && po_all_finite(c->cov_meas, (size_t)36 * c->num);
}

}  // namespace

// n independent items: one upload, one launch, one download.
extern "C" int slslam_po_edge_statistics(const slslam_po_edge_items* it, int* status, double* error, double* cov, double* sqrt_information,
                                         double* mahalanobis2) {
  if (!it || it->n < 0 || !po_sigma2_ok(it->sigma2)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const size_t n = (size_t)it->n;
  if (n > 0 && (!it->pose_a || !it->pose_b || !it->constraints)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!po_all_finite(it->pose_a, 6 * n) || !po_all_finite(it->pose_b, 6 * n) || !po_all_finite(it->constraints, 6 * n) ||
      !po_all_finite(it->cov_aa, 36 * n) || !po_all_finite(it->cov_bb, 36 * n) || !po_all_finite(it->cov_ab, 36 * n) ||
      !po_all_finite(it->cov_meas, 36 * n))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  if (n == 0) return SLSLAM_OK;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  try {
    PoCarve a;
    const size_t o_pa = a.take(sizeof(double) * 6 * n), o_pb = a.take(sizeof(double) * 6 * n), o_c = a.take(sizeof(double) * 6 * n);
    const double* blocks[4] = { it->cov_aa, it->cov_bb, it->cov_ab, it->cov_meas };
    size_t o_blk[4];
    for (int q = 0; q < 4; ++q) o_blk[q] = a.take(blocks[q] ? sizeof(double) * 36 * n : 0);
    const size_t up_bytes = a.off;
    const size_t o_status = a.take(sizeof(int) * n), o_err = a.take(sizeof(double) * 6 * n), o_cov = a.take(sizeof(double) * 36 * n),
                 o_W = a.take(sizeof(double) * 36 * n), o_m2 = a.take(sizeof(double) * n), down_bytes = a.off - up_bytes;
    struct Block {                          // the calling thread's cached device block, handed back on every path
      char* p = nullptr; size_t bytes = 0; int device = 0;
      ~Block() { DeviceBlockCache::give_back(p, bytes, device); }
    } blk;
    blk.bytes = a.off;
    HIP_TRY(hipGetDevice(&blk.device));
    HIP_TRY(DeviceBlockCache::acquire(blk.bytes, blk.device, &blk.p));
    std::vector<char> img(std::max(up_bytes, down_bytes));
    std::memcpy(img.data() + o_pa, it->pose_a, sizeof(double) * 6 * n); std::memcpy(img.data() + o_pb, it->pose_b, sizeof(double) * 6 * n);
    std::memcpy(img.data() + o_c, it->constraints, sizeof(double) * 6 * n);
    for (int q = 0; q < 4; ++q) if (blocks[q]) std::memcpy(img.data() + o_blk[q], blocks[q], sizeof(double) * 36 * n);
    HIP_TRY(hipMemcpy(blk.p, img.data(), up_bytes, hipMemcpyHostToDevice));
    PoEdgeArrays A;
    A.pa = (const double*)(blk.p + o_pa); A.pb = (const double*)(blk.p + o_pb); A.c = (const double*)(blk.p + o_c);
    A.saa = blocks[0] ? (const double*)(blk.p + o_blk[0]) : nullptr; A.sbb = blocks[1] ? (const double*)(blk.p + o_blk[1]) : nullptr;
    A.sab = blocks[2] ? (const double*)(blk.p + o_blk[2]) : nullptr; A.r = blocks[3] ? (const double*)(blk.p + o_blk[3]) : nullptr;
    A.n = it->n; A.sigma2 = it->sigma2;
    A.status = (int*)(blk.p + o_status); A.err = (double*)(blk.p + o_err); A.cov = (double*)(blk.p + o_cov);
    A.W = (double*)(blk.p + o_W); A.m2 = (double*)(blk.p + o_m2);
    hipLaunchKernelGGL(k_po_edge_stat, dim3((unsigned)((n + 4) / 5)), dim3(64), 0, 0, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(img.data(), blk.p + up_bytes, down_bytes, hipMemcpyDeviceToHost));
    const char* down = img.data() - up_bytes;
    if (status) std::memcpy(status, down + o_status, sizeof(int) * n);
    if (error) std::memcpy(error, down + o_err, sizeof(double) * 6 * n);
    if (cov) std::memcpy(cov, down + o_cov, sizeof(double) * 36 * n);
    if (sqrt_information) std::memcpy(sqrt_information, down + o_W, sizeof(double) * 36 * n);
    if (mahalanobis2) std::memcpy(mahalanobis2, down + o_m2, sizeof(double) * n);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

// Candidates against ONE graph at graph->parameters: slslam_po_covariance's launch sequence with the candidates as its pairs, then
// k_po_gate; only the gate's results come back.
extern "C" int slslam_po_gate(const slslam_po_graph* g, double po_huber_delta, const slslam_po_candidates* cand, int* cov_status, int* status,
                              double* error, double* cov, double* sqrt_information, double* mahalanobis2) {
  if (!g || !po_graph_arrays_ok(g, true) || !po_huber_ok(po_huber_delta) || !po_graph_entries_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!po_candidates_ok(g->num_poses, cand)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int N = g->num_poses, E = g->num_edges, M = cand->num;
  if (M == 0) return slslam_po_covariance(g, po_huber_delta, 0, nullptr, nullptr, cov_status, nullptr, nullptr);
  if (E == 0) {                                  // no free pose: every Sigma block is zero, S = R
    std::vector<double> xa((size_t)6 * M), xb((size_t)6 * M);
    for (int k = 0; k < M; ++k) {
      std::memcpy(&xa[(size_t)6 * k], g->parameters + 6 * (size_t)cand->pose_a[k], sizeof(double) * 6);
      std::memcpy(&xb[(size_t)6 * k], g->parameters + 6 * (size_t)cand->pose_b[k], sizeof(double) * 6);
    }
    slslam_po_edge_items it = { M, xa.data(), xb.data(), cand->constraints, nullptr, nullptr, nullptr, cand->cov_meas, cand->sigma2 };
    const int rc = slslam_po_edge_statistics(&it, status, error, cov, sqrt_information, mahalanobis2);
    if (rc == SLSLAM_OK && cov_status) *cov_status = SLSLAM_COV_OK;
    return rc;
  }
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  try {
    PoSymbolic S;
    po_analyse(N, E, g->pose_index_1, g->pose_index_2, false, &S);
    PoCarve a;
    const size_t o_p1 = a.take(sizeof(int) * E), o_p2 = a.take(sizeof(int) * E), o_slot = a.take(sizeof(int) * N), o_cons = a.take(sizeof(double) * 6 * E),
                 o_x = a.take(sizeof(double) * 6 * N), o_winfo = a.take(g->sqrt_information ? sizeof(double) * 36 * E : 0), up_bytes = a.off;
    std::vector<PoCovInput> in(1);
    PoCovInput& I = in[0];
    I.N = N; I.E = E; I.n = S.n; I.ld = S.ld; I.pa = cand->pose_a; I.pb = cand->pose_b; I.P = M;
    std::vector<PoGateInput> gin(1);
    gin[0].num = M; gin[0].pair_off = 0; gin[0].cons = cand->constraints; gin[0].rmeas = cand->cov_meas; gin[0].sigma2 = cand->sigma2;
    PoCovPlan plan;
    PoGatePlan gate;
    struct Block {
      char* p = nullptr; size_t bytes = 0; int device = 0;
      ~Block() { DeviceBlockCache::give_back(p, bytes, device); }
    } blk;
    PoCarve ga;
    ga.off = po_cov_layout(in, po_huber_delta, a, nullptr, nullptr, &plan);
    blk.bytes = po_gate_layout(gin, ga, nullptr, nullptr, &gate);
    HIP_TRY(hipGetDevice(&blk.device));
    HIP_TRY(DeviceBlockCache::acquire(blk.bytes, blk.device, &blk.p));
    HIP_TRY(po_cov_lds_attribute());
    I.d_p1 = (const int*)(blk.p + o_p1); I.d_p2 = (const int*)(blk.p + o_p2); I.d_slot = (const int*)(blk.p + o_slot);
    I.d_cons = (const double*)(blk.p + o_cons); I.d_x0 = (const double*)(blk.p + o_x);
    if (g->sqrt_information) I.d_winfo = (const double*)(blk.p + o_winfo);
    std::vector<char> img, gimg, up(up_bytes);
    po_cov_layout(in, po_huber_delta, a, blk.p, &img, &plan);
    po_gate_layout(gin, ga, blk.p, &gimg, &gate);
    std::memcpy(up.data() + o_p1, g->pose_index_1, sizeof(int) * E); std::memcpy(up.data() + o_p2, g->pose_index_2, sizeof(int) * E);
    std::memcpy(up.data() + o_slot, S.slot.data(), sizeof(int) * N); std::memcpy(up.data() + o_cons, g->constraints, sizeof(double) * 6 * E);
    std::memcpy(up.data() + o_x, g->parameters, sizeof(double) * 6 * N);
    if (g->sqrt_information) std::memcpy(up.data() + o_winfo, g->sqrt_information, sizeof(double) * 36 * E);
    HIP_TRY(hipMemcpy(blk.p, up.data(), up_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(blk.p + plan.img_off, img.data(), plan.img_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(blk.p + gate.img_off, gimg.data(), gate.img_bytes, hipMemcpyHostToDevice));
    int rc = po_cov_enqueue(plan, 0);
    if (rc == SLSLAM_OK) rc = po_gate_enqueue(plan, gate, 0);
    if (rc != SLSLAM_OK) return rc;
    std::vector<char> down(gate.down_bytes);
    HIP_TRY(hipMemcpy(down.data(), blk.p + gate.down_off, gate.down_bytes, hipMemcpyDeviceToHost));
    po_gate_read(gate, down.data(), 0, M, cov_status, status, error, cov, sqrt_information, mahalanobis2);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

#endif  // SLSLAM_PO_GATE_H_

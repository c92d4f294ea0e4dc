// slslam_amd/csrc/po_batch.h — many pose graphs per call: slslam_po_batch_* runs slslam_po_solve's structured path
// (POProblem::build + ceres::Solve, reference src/slam.cpp:1236-1313, src/po_problem.cpp:40-77) for G graphs at once.
// Part of po_api.hip's translation unit (included at its end: the one-graph kernels and order_chains_first live there).
//
// Every launch of the one-graph sequence covers every graph of the batch: the kernels below are the one-graph kernels'
// bodies (po_kernels.h) behind a graph index taken from the grid (one workgroup per graph) or from a flattened work list
// (PoItem: graph + the block index the one-graph launch would have given that workgroup).  Per graph the slots, the chain
// order and the operation order are those of slslam_po_solve; only the order of the fp64 atomic sums can differ.  A graph
// early-outs on its own LMState, as in the one-graph path.  No workgroup waits for another: any batch size runs.
#ifndef SLSLAM_PO_BATCH_H_
#define SLSLAM_PO_BATCH_H_

#include <algorithm>
#include <new>

namespace {

struct PoItem { int graph, local; };        // one workgroup of a batched launch: its graph and its block index in that graph's launch
struct PoBatchGraph {
  PoPtrs p, pj;                             // the whole system and its junction block (slslam_po_solve's p / pj)
  const PoChain* chains;                    // this graph's chains, level after level
  double* Lf_j;                             // the junction block's factor: nj rows, leading dimension ld
  double* linv;                             // inverses of its 64 x 64 diagonal blocks
  int n_l1;                                 // unknowns of the level-1 chains (k_po_zero_structured)
};

__global__ __launch_bounds__(256) void k_pob_zero(const PoBatchGraph* gs, const PoItem* items) {
  const PoItem it = items[blockIdx.x];
  po_zero_structured_body(gs[it.graph].p, gs[it.graph].n_l1, (unsigned)it.local);
}
__global__ __launch_bounds__(64) void k_pob_linearise(const PoBatchGraph* gs, const PoItem* items, int mode) {
  const PoItem it = items[blockIdx.x];
  po_linearise_body(gs[it.graph].p, mode, (unsigned)it.local);
}
__global__ __launch_bounds__(256) void k_pob_prepare(const PoBatchGraph* gs, Policy pol, int first) {
  const PoPtrs p = gs[blockIdx.x].p;
  po_prepare_body(p, pol, first);
}
__global__ __launch_bounds__(64) void k_pob_chain_eliminate(const PoBatchGraph* gs, const PoItem* items) {
  const PoItem it = items[blockIdx.x];
  const PoPtrs p = gs[it.graph].p;
  po_chain_eliminate_body(p, gs[it.graph].chains + it.local);
}
__global__ __launch_bounds__(64) void k_pob_chain_backsub(const PoBatchGraph* gs, const PoItem* items) {
  const PoItem it = items[blockIdx.x];
  const PoPtrs p = gs[it.graph].p;
  po_chain_backsub_body(p, gs[it.graph].chains + it.local);
}
// the junction block: its first diagonal block, then one launch per block step over the graphs that have that step
__global__ __launch_bounds__(256) void k_pob_potrf_diag(const PoBatchGraph* gs, const int* graphs) {
  const int gi = graphs[blockIdx.x];
  PoPtrs pj = gs[gi].pj;
  po_potrf_diag_body<double>(pj, pj.H, gs[gi].linv, 0, gs[gi].Lf_j);
}
__global__ __launch_bounds__(256) void k_pob_step(const PoBatchGraph* gs, const PoItem* items, int bk) {
  const PoItem it = items[blockIdx.x];
  PoPtrs pj = gs[it.graph].pj;
  po_step_body<double>(pj, pj.H, gs[it.graph].Lf_j, gs[it.graph].linv, bk, (unsigned)it.local);
}
__global__ __launch_bounds__(1024) void k_pob_trisolve(const PoBatchGraph* gs, const int* graphs) {
  const int gi = graphs[blockIdx.x];
  const PoPtrs pj = gs[gi].pj;
  po_trisolve_body<double>(pj, gs[gi].Lf_j, gs[gi].linv);
}
__global__ __launch_bounds__(256) void k_pob_candidate(const PoBatchGraph* gs) {
  const PoPtrs p = gs[blockIdx.x].p;
  po_candidate_body(p);
}
__global__ __launch_bounds__(64) void k_pob_update(const PoBatchGraph* gs, Policy pol) {
  const PoPtrs p = gs[blockIdx.x].p;
  po_update_body(p, pol);
}

constexpr size_t kStepLds = kPoStepLdsTiles * kNB * kLdT * sizeof(double);

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

struct slslam_po_batch {
  struct Graph {
    int N = 0, E = 0;
    std::vector<int> p1, p2;
    std::vector<double> cons, x0;
    // symbolic analysis (slslam_po_solve's, done by add)
    std::vector<int> slot, level_counts;
    std::vector<PoChain> chains;
    int n_chain = 0, n = 0, kept = 0, n_l1 = 0, nj = 0, nblk_j = 0, ld = 0;
    int active = -1;                        // index among the graphs the device solves (E > 0), -1 otherwise
    // results (download)
    LMState st{};
    std::vector<IterRec> trace;
    std::vector<double> x;
  };
  int device = -1;
  bool finalized = false, have_results = false;
  std::vector<Graph> graphs;
  std::vector<int> active;                  // batch index of each graph the device solves
  Policy pol{};
  // device arena: [ states | traces | poses ] (what comes back) [ descriptors | work lists | per-graph inputs ] (what reset restores)
  // [ per-graph work arrays ]
  char* arena = nullptr;
  char* h_up = nullptr;                     // pinned image of the first two regions, as uploaded at finalize (reset copies it again)
  char* h_down = nullptr;                   // pinned landing area of the first region
  size_t up_bytes = 0, down_bytes = 0;
  std::vector<size_t> o_x;                  // per active graph: offset of its poses in the arena
  size_t o_trace = 0;
  PoBatchGraph* d_graphs = nullptr;
  PoItem* d_items = nullptr;
  int* d_jgraphs = nullptr;
  int zero_off = 0, zero_cnt = 0, edge_off = 0, edge_cnt = 0, jgraph_cnt = 0;
  std::vector<int> level_off, level_cnt, step_off, step_cnt;
  int iter_hint = -1;                       // LM iterations the slowest graph of the previous solve took
  void release() {
    if (arena) (void)hipFree(arena);
    if (h_up) (void)hipHostFree(h_up);
    if (h_down) (void)hipHostFree(h_down);
    arena = h_up = h_down = nullptr;
  }
};

#define POB_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      std::fprintf(stderr, "slslam: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? SLSLAM_ERR_NO_DEVICE : SLSLAM_ERR_HIP; \
    }                                                                                   \
  } while (0)

extern "C" int slslam_po_batch_create(int device, slslam_po_batch** out) {
  if (!out) return SLSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  slslam_po_batch* b = new (std::nothrow) slslam_po_batch();
  if (!b) return SLSLAM_ERR_NO_MEMORY;
  b->device = device;
  *out = b;
  return SLSLAM_OK;
}

extern "C" void slslam_po_batch_destroy(slslam_po_batch* b) {
  if (!b) return;
  if (b->arena || b->h_up || b->h_down) { (void)hipSetDevice(b->device); b->release(); }
  delete b;
}

extern "C" int slslam_po_batch_add(slslam_po_batch* b, const slslam_po_graph* g, int* index) {
  if (!b || !g) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (b->finalized) return SLSLAM_ERR_STATE;
  // the validation of slslam_po_solve
  const int N = g->num_poses, E = g->num_edges;
  if (N < 0 || E < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (E > 0 && (!g->pose_index_1 || !g->pose_index_2 || !g->constraints)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (N > 0 && !g->parameters) return SLSLAM_ERR_INVALID_ARGUMENT;
  for (int e = 0; e < E; ++e) {
    const int a = g->pose_index_1[e], c = g->pose_index_2[e];
    if (a < 0 || a >= N || c < 0 || c >= N || a == c) return SLSLAM_ERR_INVALID_ARGUMENT;
    for (int q = 0; q < 6; ++q) if (!std::isfinite(g->constraints[6 * (size_t)e + q])) return SLSLAM_ERR_INVALID_ARGUMENT;
  }
  for (size_t i = 0; i < (size_t)6 * N; ++i) if (!std::isfinite(g->parameters[i])) return SLSLAM_ERR_INVALID_ARGUMENT;
  try {
    slslam_po_batch::Graph G;
    G.N = N; G.E = E;
    G.p1.assign(g->pose_index_1, g->pose_index_1 + E); G.p2.assign(g->pose_index_2, g->pose_index_2 + E);
    G.cons.assign(g->constraints, g->constraints + 6 * (size_t)E);
    G.x0.assign(g->parameters, g->parameters + 6 * (size_t)N);
    if (E > 0) {
      // the symbolic analysis of slslam_po_solve's structured path: pose1 of edge 0 is constant, unreferenced poses are not in the problem
      std::vector<int> used(N, 0);
      G.slot.assign(N, -1);
      for (int e = 0; e < E; ++e) { used[G.p1[e]] = 1; used[G.p2[e]] = 1; }
      order_chains_first(N, E, G.p1.data(), G.p2.data(), used, G.p1[0], G.slot, G.chains, &G.n_chain, &G.n, &G.level_counts);
      for (int e = 0; e < E; ++e) if (G.slot[G.p1[e]] >= 0 || G.slot[G.p2[e]] >= 0) ++G.kept;
      G.ld = ((G.n + 7) / 8) * 8 + 8;
      G.nj = G.n - G.n_chain;
      G.nblk_j = (G.nj + kNB - 1) / kNB;
      const int n_level1 = G.level_counts.empty() ? 0 : G.level_counts[0];
      G.n_l1 = n_level1 > 0 ? G.chains[(size_t)n_level1 - 1].start + 6 * G.chains[(size_t)n_level1 - 1].len : 0;
    }
    if (index) *index = (int)b->graphs.size();
    b->graphs.push_back(std::move(G));
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

namespace {
// Lays the arena out, fills the pinned image and the work lists.  arena == nullptr: sizes only.
void po_batch_layout(slslam_po_batch* b, char* arena, size_t* up_bytes, size_t* down_bytes, size_t* total_bytes) {
  const int A = (int)b->active.size();
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
  char* img = b->h_up;
  auto put = [&](size_t o, const void* src, size_t bytes) { if (img && bytes) std::memcpy(img + o, src, bytes); };
  // what comes back: the LM states (also what solve polls), the traces, the poses
  const size_t o_st = take(sizeof(LMState) * (size_t)A);
  b->o_trace = take(sizeof(IterRec) * kMaxTrace * (size_t)A);
  b->o_x.assign((size_t)A, 0);
  for (int a = 0; a < A; ++a) b->o_x[(size_t)a] = take(sizeof(double) * 12 * (size_t)b->graphs[(size_t)b->active[(size_t)a]].N);
  *down_bytes = off;
  // the work lists
  std::vector<PoItem> items;
  std::vector<int> jgraphs;
  auto list = [&](int& o, int& cnt, auto&& fill) { o = (int)items.size(); fill(); cnt = (int)items.size() - o; };
  list(b->zero_off, b->zero_cnt, [&] {
    for (int a = 0; a < A; ++a) {
      const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
      const long long nz = G.n - G.n_l1, zero_items = (long long)G.E * 144 + nz * nz + G.n + 1;
      for (long long k = 0; k < (zero_items + 255) / 256; ++k) items.push_back(PoItem{ a, (int)k });
    }
  });
  list(b->edge_off, b->edge_cnt, [&] {
    for (int a = 0; a < A; ++a)
      for (int k = 0; k < (b->graphs[(size_t)b->active[(size_t)a]].E + 4) / 5; ++k) items.push_back(PoItem{ a, k });
  });
  size_t levels = 0;
  int steps = 0;
  for (int gi : b->active) {
    const auto& G = b->graphs[(size_t)gi];
    levels = std::max(levels, G.level_counts.size());
    steps = std::max(steps, G.nblk_j - 1);
  }
  for (int a = 0; a < A; ++a) if (b->graphs[(size_t)b->active[(size_t)a]].nj > 0) jgraphs.push_back(a);
  b->jgraph_cnt = (int)jgraphs.size();
  b->level_off.assign(levels, 0); b->level_cnt.assign(levels, 0);
  for (size_t lv = 0; lv < levels; ++lv)
    list(b->level_off[lv], b->level_cnt[lv], [&] {
      for (int a = 0; a < A; ++a) {
        const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
        if (lv >= G.level_counts.size()) continue;
        size_t first = 0;
        for (size_t q = 0; q < lv; ++q) first += (size_t)G.level_counts[q];
        for (int c = 0; c < G.level_counts[lv]; ++c) items.push_back(PoItem{ a, (int)first + c });
      }
    });
  b->step_off.assign((size_t)std::max(steps, 0), 0); b->step_cnt.assign((size_t)std::max(steps, 0), 0);
  for (int bk = 0; bk < steps; ++bk)
    list(b->step_off[(size_t)bk], b->step_cnt[(size_t)bk], [&] {
      for (int a = 0; a < A; ++a) {
        const int tb = b->graphs[(size_t)b->active[(size_t)a]].nblk_j - 1 - bk;
        for (int t = 0; tb > 0 && t < tb * (tb + 1) / 2; ++t) items.push_back(PoItem{ a, t });
      }
    });
  const size_t o_graphs = take(sizeof(PoBatchGraph) * (size_t)A), o_items = take(sizeof(PoItem) * items.size()),
               o_jg = take(sizeof(int) * jgraphs.size());
  put(o_items, items.data(), sizeof(PoItem) * items.size());
  put(o_jg, jgraphs.data(), sizeof(int) * jgraphs.size());
  // per graph: the inputs, then (after every graph's inputs) the work arrays
  std::vector<PoBatchGraph> desc((size_t)A);
  std::vector<size_t> o_in((size_t)A * 8);
  for (int a = 0; a < A; ++a) {
    const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
    size_t* o = &o_in[(size_t)a * 8];
    o[0] = take(sizeof(int) * G.E); o[1] = take(sizeof(int) * G.E); o[2] = take(sizeof(int) * G.N); o[3] = take(sizeof(double) * 6 * G.E);
    o[4] = take(sizeof(double) * G.n); o[5] = take(sizeof(PoChain) * (G.chains.size() + 1)); o[6] = take(sizeof(double) * 8); o[7] = take(sizeof(int) * 2);
    if (img) {
      LMState st;
      std::memset(&st, 0, sizeof(st));
      st.radius = b->pol.initial_radius; st.decrease_factor = 2.0; st.status = kRunning;
      put(o_st + sizeof(LMState) * a, &st, sizeof(st));
      put(b->o_x[(size_t)a], G.x0.data(), sizeof(double) * 6 * G.N);
      put(b->o_x[(size_t)a] + sizeof(double) * 6 * G.N, G.x0.data(), sizeof(double) * 6 * G.N);
      put(o[0], G.p1.data(), sizeof(int) * G.E); put(o[1], G.p2.data(), sizeof(int) * G.E); put(o[2], G.slot.data(), sizeof(int) * G.N);
      put(o[3], G.cons.data(), sizeof(double) * 6 * G.E);
      for (int i = 0; i < G.n; ++i) { const double one = 1.0; put(o[4] + sizeof(double) * i, &one, sizeof(double)); }
      put(o[5], G.chains.data(), sizeof(PoChain) * G.chains.size());
    }
  }
  *up_bytes = off;
  for (int a = 0; a < A; ++a) {
    const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
    const size_t* o = &o_in[(size_t)a * 8];
    const size_t o_H = take(sizeof(double) * (size_t)G.n * G.ld), o_g = take(sizeof(double) * G.n), o_d2 = take(sizeof(double) * G.n),
                 o_y = take(sizeof(double) * G.n), o_linv = take(sizeof(double) * kNB * kNB * (size_t)std::max(G.nblk_j, 1)),
                 o_Lf = take(sizeof(double) * (size_t)std::max(G.nj, 1) * G.ld);
    if (!arena) continue;
    PoBatchGraph& D = desc[(size_t)a];
    std::memset(&D, 0, sizeof(D));
    PoPtrs& p = D.p;
    p.p1 = (const int*)(arena + o[0]); p.p2 = (const int*)(arena + o[1]); p.slot = (const int*)(arena + o[2]); p.cons = (const double*)(arena + o[3]);
    p.scale = (double*)(arena + o[4]); p.scal = (double*)(arena + o[6]); p.flags = (int*)(arena + o[7]);
    p.x = (double*)(arena + b->o_x[(size_t)a]); p.st = (LMState*)(arena + o_st) + a; p.trace = (IterRec*)(arena + b->o_trace) + (size_t)kMaxTrace * a;
    p.H = (double*)(arena + o_H); p.g = (double*)(arena + o_g); p.d2 = (double*)(arena + o_d2); p.y = (double*)(arena + o_y);
    p.N = G.N; p.E = G.E; p.n = G.n; p.ld = G.ld;
    D.pj = p;                               // the junction block as a matrix of its own (same leading dimension)
    D.pj.n = G.nj; D.pj.H = p.H + (size_t)G.n_chain * G.ld + G.n_chain; D.pj.y = p.y + G.n_chain;
    D.chains = (const PoChain*)(arena + o[5]);
    D.Lf_j = (double*)(arena + o_Lf);
    D.linv = (double*)(arena + o_linv);
    D.n_l1 = G.n_l1;
  }
  put(o_graphs, desc.data(), sizeof(PoBatchGraph) * desc.size());
  if (arena) {
    b->d_graphs = (PoBatchGraph*)(arena + o_graphs); b->d_items = (PoItem*)(arena + o_items); b->d_jgraphs = (int*)(arena + o_jg);
  }
  *total_bytes = off;
}
}  // namespace

extern "C" int slslam_po_batch_finalize(slslam_po_batch* b, const slslam_solver_options* opt_in) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (b->finalized) return SLSLAM_ERR_STATE;
  slslam_solver_options opt;
  if (opt_in) opt = *opt_in; else slslam_default_options(&opt);
  if (opt.max_num_iterations < 0 || opt.max_num_iterations > 100000) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (opt.po_dense_factor || opt.po_factor_fp32) return SLSLAM_ERR_UNSUPPORTED;      // the structured fp64 factorisation only
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (b->device < 0) { if (hipGetDevice(&b->device) != hipSuccess) return SLSLAM_ERR_NO_DEVICE; }
  if (b->device >= ndev) return SLSLAM_ERR_INVALID_ARGUMENT;
  POB_TRY(hipSetDevice(b->device));
  Policy& pol = b->pol;                     // (slslam_po_solve's policy)
  std::memset(&pol, 0, sizeof(pol));
  pol.huber_delta = 0.0; pol.baseline = 0.0;
  pol.initial_radius = opt.initial_trust_region_radius; pol.max_radius = opt.max_trust_region_radius;
  pol.min_radius = opt.min_trust_region_radius; pol.min_relative_decrease = opt.min_relative_decrease;
  pol.min_lm_diagonal = opt.min_lm_diagonal; pol.max_lm_diagonal = opt.max_lm_diagonal;
  pol.function_tolerance = opt.function_tolerance; pol.gradient_tolerance = opt.gradient_tolerance;
  pol.parameter_tolerance = opt.parameter_tolerance; pol.max_num_iterations = opt.max_num_iterations;
  pol.max_invalid = opt.max_num_consecutive_invalid_steps; pol.jacobi_scaling = opt.jacobi_scaling; pol.keep_jacobian = 0;
  b->active.clear();
  for (size_t i = 0; i < b->graphs.size(); ++i) {
    b->graphs[i].active = b->graphs[i].E > 0 ? (int)b->active.size() : -1;
    if (b->graphs[i].E > 0) b->active.push_back((int)i);
  }
  if (!b->active.empty()) {
    size_t up = 0, down = 0, total = 0;
    po_batch_layout(b, nullptr, &up, &down, &total);
    hipError_t e = hipFuncSetAttribute((const void*)k_pob_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStepLds);
    if (e == hipSuccess) e = hipMalloc((void**)&b->arena, total);
    if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_up, up, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_down, down, hipHostMallocDefault);
    if (e == hipSuccess) {
      std::memset(b->h_up, 0, up);
      po_batch_layout(b, b->arena, &b->up_bytes, &b->down_bytes, &total);
      e = hipMemcpy(b->arena, b->h_up, b->up_bytes, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      std::fprintf(stderr, "slslam: slslam_po_batch_finalize: %s (%zu bytes of device memory)\n", hipGetErrorString(e), total);
      (void)hipGetLastError();
      b->release();
      return SLSLAM_ERR_HIP;
    }
  }
  b->finalized = true;
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_reset(slslam_po_batch* b, void* stream) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  b->have_results = false;
  if (b->active.empty()) return SLSLAM_OK;
  POB_TRY(hipSetDevice(b->device));
  POB_TRY(hipMemcpyAsync(b->arena, b->h_up, b->up_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_solve(slslam_po_batch* b, void* stream) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  b->have_results = false;
  const int A = (int)b->active.size();
  if (A == 0) return SLSLAM_OK;
  POB_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const PoBatchGraph* gs = b->d_graphs;
  const PoItem* items = b->d_items;
  const Policy pol = b->pol;
  auto zero_and_linearise = [&]() {
    hipLaunchKernelGGL(k_pob_zero, dim3((unsigned)b->zero_cnt), dim3(256), 0, s, gs, items + b->zero_off);
    hipLaunchKernelGGL(k_pob_linearise, dim3((unsigned)b->edge_cnt), dim3(64), 0, s, gs, items + b->edge_off, 0);
  };
  // initial evaluation: cost, gradient, column norms -> Jacobi scale
  zero_and_linearise();
  hipLaunchKernelGGL(k_pob_prepare, dim3((unsigned)A), dim3(256), 0, s, gs, pol, 1);
  // LM iterations, enqueued without host synchronisation; a finished graph early-outs on the device.  As slslam_po_solve does, the host asks
  // whether every graph has finished after one iteration more than the slowest graph of the previous solve took (8 without history), then
  // every 4, and stops enqueueing when they have.
  int next_check = b->iter_hint >= 0 ? std::min(b->iter_hint + 1, 8) : 8;
  for (int it = 0; it < pol.max_num_iterations; ++it) {
    if (it == next_check) {
      POB_TRY(hipMemcpyAsync(b->h_down, b->arena, sizeof(LMState) * (size_t)A, hipMemcpyDeviceToHost, s));
      POB_TRY(hipStreamSynchronize(s));
      const LMState* st = (const LMState*)b->h_down;
      bool running = false;
      int steps = 0;
      for (int a = 0; a < A; ++a) { running = running || st[a].status == kRunning; steps = std::max(steps, st[a].n_success + st[a].n_unsuccess); }
      if (!running) { b->iter_hint = steps; break; }
      next_check += 4;
    }
    zero_and_linearise();
    hipLaunchKernelGGL(k_pob_prepare, dim3((unsigned)A), dim3(256), 0, s, gs, pol, 0);
    for (size_t lv = 0; lv < b->level_cnt.size(); ++lv)             // level after level: the pieces, then the chains of their cut poses, ...
      if (b->level_cnt[lv] > 0)
        hipLaunchKernelGGL(k_pob_chain_eliminate, dim3((unsigned)b->level_cnt[lv]), dim3(64), 0, s, gs, items + b->level_off[lv]);
    if (b->jgraph_cnt > 0) {
      hipLaunchKernelGGL(k_pob_potrf_diag, dim3((unsigned)b->jgraph_cnt), dim3(256), 0, s, gs, (const int*)b->d_jgraphs);
      for (size_t bk = 0; bk < b->step_cnt.size(); ++bk)
        if (b->step_cnt[bk] > 0)
          hipLaunchKernelGGL(k_pob_step, dim3((unsigned)b->step_cnt[bk]), dim3(256), kStepLds, s, gs, items + b->step_off[bk], (int)bk);
      hipLaunchKernelGGL(k_pob_trisolve, dim3((unsigned)b->jgraph_cnt), dim3(1024), 0, s, gs, (const int*)b->d_jgraphs);
    }
    for (size_t lv = b->level_cnt.size(); lv-- > 0;)                 // ... and back down
      if (b->level_cnt[lv] > 0)
        hipLaunchKernelGGL(k_pob_chain_backsub, dim3((unsigned)b->level_cnt[lv]), dim3(64), 0, s, gs, items + b->level_off[lv]);
    hipLaunchKernelGGL(k_pob_candidate, dim3((unsigned)A), dim3(256), 0, s, gs);
    hipLaunchKernelGGL(k_pob_linearise, dim3((unsigned)b->edge_cnt), dim3(64), 0, s, gs, items + b->edge_off, 1);
    hipLaunchKernelGGL(k_pob_update, dim3((unsigned)A), dim3(64), 0, s, gs, pol);
  }
  POB_TRY(hipGetLastError());
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_download(slslam_po_batch* b, void* stream) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  const int A = (int)b->active.size();
  if (A > 0) {
    POB_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    POB_TRY(hipMemcpyAsync(b->h_down, b->arena, b->down_bytes, hipMemcpyDeviceToHost, s));
    POB_TRY(hipStreamSynchronize(s));
  }
  int steps = 0;
  try {
    for (int a = 0; a < A; ++a) {
      auto& G = b->graphs[(size_t)b->active[(size_t)a]];
      std::memcpy(&G.st, b->h_down + sizeof(LMState) * (size_t)a, sizeof(LMState));
      G.trace.resize(kMaxTrace);
      std::memcpy(G.trace.data(), b->h_down + b->o_trace + sizeof(IterRec) * kMaxTrace * (size_t)a, sizeof(IterRec) * kMaxTrace);
      G.x.resize((size_t)6 * G.N);
      std::memcpy(G.x.data(), b->h_down + b->o_x[(size_t)a] + sizeof(double) * 6 * G.N * (size_t)G.st.cur, sizeof(double) * 6 * G.N);
      steps = std::max(steps, G.st.n_success + G.st.n_unsuccess);
    }
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  if (A > 0) b->iter_hint = steps;
  b->have_results = true;
  return SLSLAM_OK;
}

namespace {
int po_batch_graph(const slslam_po_batch* b, int index, const slslam_po_batch::Graph** G) {
  if (!b || index < 0 || index >= (int)b->graphs.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->have_results) return SLSLAM_ERR_STATE;
  *G = &b->graphs[(size_t)index];
  return SLSLAM_OK;
}
int po_termination(const slslam_po_batch::Graph& G) {
  if (G.active < 0) return SLSLAM_FUNCTION_TOLERANCE;              // no edges: nothing to solve
  return G.st.status == kRunning ? SLSLAM_NO_CONVERGENCE : G.st.status;
}
}  // namespace

extern "C" int slslam_po_batch_get_parameters(const slslam_po_batch* b, int index, double* parameters) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  if (G->N > 0 && !parameters) return SLSLAM_ERR_INVALID_ARGUMENT;
  // a numerical failure leaves the parameters untouched (slslam_po_solve)
  const bool solved = G->active >= 0 && po_termination(*G) != SLSLAM_NUMERICAL_FAILURE;
  if (G->N > 0) std::memcpy(parameters, solved ? G->x.data() : G->x0.data(), sizeof(double) * 6 * (size_t)G->N);
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_summary(const slslam_po_batch* b, int index, slslam_summary* s) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  if (!s) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::memset(s, 0, sizeof(*s));
  s->termination_type = po_termination(*G);
  if (G->active < 0) return SLSLAM_OK;
  const LMState& st = G->st;
  s->num_successful_steps = st.n_success; s->num_unsuccessful_steps = st.n_unsuccess;
  s->initial_cost = st.initial_cost;
  s->final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;
  s->fixed_cost = st.fixed_cost;
  s->num_free_parameters = G->n; s->num_residual_blocks = G->kept;
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_trace(const slslam_po_batch* b, int index, slslam_iteration* trace, int cap, int* len) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  const int nt = G->active < 0 ? 0 : (G->st.ntrace < kMaxTrace ? G->st.ntrace : kMaxTrace);
  if (len) *len = nt;
  for (int i = 0; trace && i < nt && i < cap; ++i) {
    const IterRec& r = G->trace[(size_t)i];
    slslam_iteration& o = trace[i];
    o.iteration = r.iteration; o.step_is_valid = r.step_is_valid; o.step_is_successful = r.step_is_successful;
    o.cost = r.cost; o.cost_change = r.cost_change; o.gradient_max_norm = r.gradient_max_norm;
    o.step_norm = r.step_norm; o.relative_decrease = r.relative_decrease;
    o.trust_region_radius = r.trust_region_radius; o.model_cost_change = r.model_cost_change;
  }
  return SLSLAM_OK;
}

#endif  // SLSLAM_PO_BATCH_H_

// slslam_amd/csrc/po_batch.h — many pose graphs per call: slslam_po_batch_* runs slslam_po_solve's structured path
// (POProblem::build + ceres::Solve, reference src/slam.cpp:1236-1313, src/po_problem.cpp:40-77) for G graphs at once.
// Part of po_api.hip's translation unit (included at its end: the one-graph kernels, the symbolic analysis and the host helpers both
// paths share - validation, policy, PoSymbolic, results, PoCarve - live there).
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
  const double* x0;                         // the poses as added (the edge report of a graph whose solve failed numerically)
  double* report;                           // [2E] per edge |Te|^2, then rho' (k_pob_edge_report)
};

__global__ __launch_bounds__(256) void k_pob_zero(const PoBatchGraph* gs, const PoItem* items) {
  const PoItem it = items[blockIdx.x];
  po_zero_structured_body(gs[it.graph].p, gs[it.graph].n_l1, (unsigned)it.local);
}
// kWeighted: launched when some graph of the batch has sqrt_information; a graph without (p.winfo null) keeps identity weights
template <bool kRobust, bool kWeighted>
__global__ __launch_bounds__(64) void k_pob_linearise(const PoBatchGraph* gs, const PoItem* items, int mode) {
  const PoItem it = items[blockIdx.x];
  po_linearise_body<kRobust, kWeighted>(gs[it.graph].p, mode, (unsigned)it.local);
}
// every graph's edge report over the linearisation's work list (5 edges per workgroup), at what slslam_po_batch_get_parameters returns:
// the accepted poses, or the poses as added when the solve ended in a numerical failure
template <bool kWeighted>
__global__ __launch_bounds__(64) void k_pob_edge_report(const PoBatchGraph* gs, const PoItem* items) {
  const PoItem it = items[blockIdx.x];
  const PoBatchGraph& G = gs[it.graph];
  const LMState* st = G.p.st;
  const double* X = st->status == SLSLAM_NUMERICAL_FAILURE ? G.x0 : G.p.x + (long long)st->cur * 6 * G.p.N;
  po_edge_report_body<kWeighted>(G.p, X, G.report, G.report + G.p.E, (unsigned)it.local, 5);
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

}  // namespace

struct slslam_po_batch {
  struct Graph {
    int N = 0, E = 0;
    std::vector<int> p1, p2;
    std::vector<double> cons, x0;
    std::vector<double> winfo;              // [36E] the edges' square-root information; empty: none given (identity)
    bool weighted = false;
    PoSymbolic sym;                         // slslam_po_solve's structured analysis, done by add
    int active = -1;                        // index among the graphs the device solves (E > 0), -1 otherwise
    // results (download)
    LMState st{};
    std::vector<IterRec> trace;
    std::vector<double> x;
    std::vector<double> report;             // [2E] per edge |Te|^2, then rho'
    // covariances (po_covariance.h): the caller's pairs, and what the last downloaded slslam_po_batch_covariance call gave
    std::vector<int> cov_pa, cov_pb;
    int cov_status = SLSLAM_COV_OK;
    std::vector<double> cov_poses, cov_pairs;
    // the gate (po_gate.h): the caller's candidates, the pair lists of the covariance plan (the caller's pairs, then the candidates),
    // and what the last downloaded slslam_po_batch_gate call gave
    std::vector<int> gate_pa, gate_pb, plan_pa, plan_pb;
    std::vector<double> gate_cons, gate_r;
    double gate_sigma2 = 1.0;
    std::vector<int> gate_status;
    std::vector<double> gate_err, gate_cov, gate_W, gate_m2;
  };
  int device = -1;
  bool finalized = false, have_results = false;
  std::vector<Graph> graphs;
  std::vector<int> active;                  // batch index of each graph the device solves
  Policy pol{};
  double huber = 0.0;                       // po_huber_delta of finalize: HuberLoss on every edge of every graph, 0 = none
  bool weighted = false;                    // some active graph has sqrt_information: the whitening instantiations run (else: the ones there were)
  // device arena: [ states | traces | poses | edge reports ] (what comes back) [ descriptors | work lists | per-graph inputs ] (what reset
  // restores) [ poses as added ] (uploaded once) [ per-graph work arrays ]
  char* arena = nullptr;
  char* h_up = nullptr;                     // pinned image of the first three regions, as uploaded at finalize (reset copies the first two again)
  char* h_down = nullptr;                   // pinned landing area of the first region
  size_t up_bytes = 0, down_bytes = 0;
  size_t init_bytes = 0;                    // what finalize uploads: the image reset restores (up_bytes) and, behind it, what stays as it is
  std::vector<size_t> o_x;                  // per active graph: offset of its poses in the arena
  std::vector<size_t> o_report;             // ... and of its edge report
  size_t o_trace = 0;
  PoBatchGraph* d_graphs = nullptr;
  PoItem* d_items = nullptr;
  int* d_jgraphs = nullptr;
  int zero_off = 0, zero_cnt = 0, edge_off = 0, edge_cnt = 0, jgraph_cnt = 0;
  std::vector<int> level_off, level_cnt, step_off, step_cnt;
  int iter_hint = -1;                       // LM iterations the slowest graph of the previous solve took
  // covariances: buffers of their own, allocated by the first slslam_po_batch_covariance call and kept (grown when a pair list grew)
  std::vector<PoBatchGraph> h_desc;         // host copy of the descriptors: where each graph's arrays live in the arena
  PoCovPlan cov_plan;
  char* cov_dev = nullptr;
  char* cov_h_down = nullptr;               // pinned landing area of the plan's results
  size_t cov_dev_bytes = 0, cov_down_cap = 0;
  bool cov_dirty = true;                    // the plan has to be (re)built: first call, or a pair list was replaced
  bool cov_pending = false;                 // a covariance call is on the device, not downloaded, no solve or reset behind it
  bool cov_valid = false;                   // the graphs hold the results of the latest covariance call
  long long cov_calls = 0, cov_allocs = 0;
  PoGatePlan gate_plan;                     // laid out behind cov_plan in cov_dev, rebuilt with it
  char* gate_h_down = nullptr;              // pinned landing area of the gate's results
  size_t gate_down_cap = 0;
  bool gate_call = false;                   // the covariance call that is pending (or, after its download, valid) was a gate call
  void release() {
    if (arena) (void)hipFree(arena);
    if (h_up) (void)hipHostFree(h_up);
    if (h_down) (void)hipHostFree(h_down);
    if (cov_dev) (void)hipFree(cov_dev);
    if (cov_h_down) (void)hipHostFree(cov_h_down);
    if (gate_h_down) (void)hipHostFree(gate_h_down);
    arena = h_up = h_down = cov_dev = cov_h_down = gate_h_down = nullptr;
    cov_dev_bytes = cov_down_cap = gate_down_cap = 0;
  }
};

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
  if (b->arena || b->h_up || b->h_down || b->cov_dev || b->cov_h_down) { (void)hipSetDevice(b->device); b->release(); }
  delete b;
}

extern "C" int slslam_po_batch_add(slslam_po_batch* b, const slslam_po_graph* g, int* index) {
  if (!b || !g) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (b->finalized) return SLSLAM_ERR_STATE;
  if (!po_graph_arrays_ok(g, true) || !po_graph_entries_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int N = g->num_poses, E = g->num_edges;
  try {
    slslam_po_batch::Graph G;
    G.N = N; G.E = E;
    G.p1.assign(g->pose_index_1, g->pose_index_1 + E); G.p2.assign(g->pose_index_2, g->pose_index_2 + E);
    G.cons.assign(g->constraints, g->constraints + 6 * (size_t)E);
    G.x0.assign(g->parameters, g->parameters + 6 * (size_t)N);
    G.weighted = g->sqrt_information != nullptr;
    if (G.weighted) G.winfo.assign(g->sqrt_information, g->sqrt_information + 36 * (size_t)E);
    po_analyse(N, E, G.p1.data(), G.p2.data(), true, &G.sym);
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
  PoCarve carve;
  char* img = b->h_up;
  auto put = [&](size_t o, const void* src, size_t bytes) { if (img && bytes) std::memcpy(img + o, src, bytes); };
  // what comes back: the LM states (also what solve polls), the traces, the poses
  const size_t o_st = carve.take(sizeof(LMState) * (size_t)A);
  b->o_trace = carve.take(sizeof(IterRec) * kMaxTrace * (size_t)A);
  b->o_x.assign((size_t)A, 0);
  for (int a = 0; a < A; ++a) b->o_x[(size_t)a] = carve.take(sizeof(double) * 12 * (size_t)b->graphs[(size_t)b->active[(size_t)a]].N);
  b->o_report.assign((size_t)A, 0);
  for (int a = 0; a < A; ++a) b->o_report[(size_t)a] = carve.take(sizeof(double) * 2 * (size_t)b->graphs[(size_t)b->active[(size_t)a]].E);
  *down_bytes = carve.off;
  // the work lists
  std::vector<PoItem> items;
  std::vector<int> jgraphs;
  auto list = [&](int& o, int& cnt, auto&& fill) { o = (int)items.size(); fill(); cnt = (int)items.size() - o; };
  list(b->zero_off, b->zero_cnt, [&] {
    for (int a = 0; a < A; ++a) {
      const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
      for (long long k = 0; k < po_zero_blocks(G.sym, G.E); ++k) items.push_back(PoItem{ a, (int)k });
    }
  });
  list(b->edge_off, b->edge_cnt, [&] {
    for (int a = 0; a < A; ++a)
      for (int k = 0; k < (b->graphs[(size_t)b->active[(size_t)a]].E + 4) / 5; ++k) items.push_back(PoItem{ a, k });
  });
  size_t levels = 0;
  int steps = 0;
  for (int gi : b->active) {
    const PoSymbolic& S = b->graphs[(size_t)gi].sym;
    levels = std::max(levels, S.level_counts.size());
    steps = std::max(steps, S.nblk_j - 1);
  }
  for (int a = 0; a < A; ++a) if (b->graphs[(size_t)b->active[(size_t)a]].sym.nj > 0) jgraphs.push_back(a);
  b->jgraph_cnt = (int)jgraphs.size();
  b->level_off.assign(levels, 0); b->level_cnt.assign(levels, 0);
  for (size_t lv = 0; lv < levels; ++lv)
    list(b->level_off[lv], b->level_cnt[lv], [&] {
      for (int a = 0; a < A; ++a) {
        const PoSymbolic& S = b->graphs[(size_t)b->active[(size_t)a]].sym;
        if (lv >= S.level_counts.size()) continue;
        size_t first = 0;
        for (size_t q = 0; q < lv; ++q) first += (size_t)S.level_counts[q];
        for (int c = 0; c < S.level_counts[lv]; ++c) items.push_back(PoItem{ a, (int)first + c });
      }
    });
  b->step_off.assign((size_t)std::max(steps, 0), 0); b->step_cnt.assign((size_t)std::max(steps, 0), 0);
  for (int bk = 0; bk < steps; ++bk)
    list(b->step_off[(size_t)bk], b->step_cnt[(size_t)bk], [&] {
      for (int a = 0; a < A; ++a) {
        const int tb = b->graphs[(size_t)b->active[(size_t)a]].sym.nblk_j - 1 - bk;
        for (int t = 0; tb > 0 && t < tb * (tb + 1) / 2; ++t) items.push_back(PoItem{ a, t });
      }
    });
  const size_t o_graphs = carve.take(sizeof(PoBatchGraph) * (size_t)A), o_items = carve.take(sizeof(PoItem) * items.size()),
               o_jg = carve.take(sizeof(int) * jgraphs.size());
  put(o_items, items.data(), sizeof(PoItem) * items.size());
  put(o_jg, jgraphs.data(), sizeof(int) * jgraphs.size());
  // per graph: the inputs, then (after every graph's inputs) the work arrays
  std::vector<PoBatchGraph> desc((size_t)A);
  std::vector<size_t> o_in((size_t)A * 10);    // (the ninth and tenth: the poses as added and the edges' weights, behind what reset restores)
  const LMState st = lm_initial_state(b->pol);
  for (int a = 0; a < A; ++a) {
    const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
    const PoSymbolic& S = G.sym;
    size_t* o = &o_in[(size_t)a * 10];
    o[0] = carve.take(sizeof(int) * G.E); o[1] = carve.take(sizeof(int) * G.E); o[2] = carve.take(sizeof(int) * G.N); o[3] = carve.take(sizeof(double) * 6 * G.E);
    o[4] = carve.take(sizeof(double) * S.n); o[5] = carve.take(sizeof(PoChain) * (S.chains.size() + 1)); o[6] = carve.take(sizeof(double) * 8); o[7] = carve.take(sizeof(int) * 2);
    if (img) {
      put(o_st + sizeof(LMState) * a, &st, sizeof(st));
      put(b->o_x[(size_t)a], G.x0.data(), sizeof(double) * 6 * G.N);
      put(b->o_x[(size_t)a] + sizeof(double) * 6 * G.N, G.x0.data(), sizeof(double) * 6 * G.N);
      put(o[0], G.p1.data(), sizeof(int) * G.E); put(o[1], G.p2.data(), sizeof(int) * G.E); put(o[2], S.slot.data(), sizeof(int) * G.N);
      put(o[3], G.cons.data(), sizeof(double) * 6 * G.E);
      for (int i = 0; i < S.n; ++i) { const double one = 1.0; put(o[4] + sizeof(double) * i, &one, sizeof(double)); }
      put(o[5], S.chains.data(), sizeof(PoChain) * S.chains.size());
    }
  }
  *up_bytes = carve.off;
  // uploaded once, by finalize: the poses as added, which no kernel writes (the edge report of a graph whose solve failed numerically),
  // and the square-root information of the graphs that have it
  for (int a = 0; a < A; ++a) {
    const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
    o_in[(size_t)a * 10 + 8] = carve.take(sizeof(double) * 6 * G.N);
    put(o_in[(size_t)a * 10 + 8], G.x0.data(), sizeof(double) * 6 * G.N);
    o_in[(size_t)a * 10 + 9] = carve.take(sizeof(double) * G.winfo.size());
    put(o_in[(size_t)a * 10 + 9], G.winfo.data(), sizeof(double) * G.winfo.size());
  }
  b->init_bytes = carve.off;
  for (int a = 0; a < A; ++a) {
    const auto& G = b->graphs[(size_t)b->active[(size_t)a]];
    const PoSymbolic& S = G.sym;
    const size_t* o = &o_in[(size_t)a * 10];
    const size_t o_H = carve.take(sizeof(double) * (size_t)S.n * S.ld), o_g = carve.take(sizeof(double) * S.n), o_d2 = carve.take(sizeof(double) * S.n),
                 o_y = carve.take(sizeof(double) * S.n), o_linv = carve.take(sizeof(double) * kNB * kNB * (size_t)std::max(S.nblk_j, 1)),
                 o_Lf = carve.take(sizeof(double) * (size_t)std::max(S.nj, 1) * S.ld);
    if (!arena) continue;
    PoBatchGraph& D = desc[(size_t)a];
    std::memset(&D, 0, sizeof(D));
    PoPtrs& p = D.p;
    p.p1 = (const int*)(arena + o[0]); p.p2 = (const int*)(arena + o[1]); p.slot = (const int*)(arena + o[2]); p.cons = (const double*)(arena + o[3]);
    p.scale = (double*)(arena + o[4]); p.scal = (double*)(arena + o[6]); p.flags = (int*)(arena + o[7]);
    p.x = (double*)(arena + b->o_x[(size_t)a]); p.st = (LMState*)(arena + o_st) + a; p.trace = (IterRec*)(arena + b->o_trace) + (size_t)kMaxTrace * a;
    p.H = (double*)(arena + o_H); p.g = (double*)(arena + o_g); p.d2 = (double*)(arena + o_d2); p.y = (double*)(arena + o_y);
    p.N = G.N; p.E = G.E; p.n = S.n; p.ld = S.ld;
    p.huber = b->huber;
    p.winfo = G.weighted ? (const double*)(arena + o[9]) : nullptr;
    D.pj = p;                               // the junction block as a matrix of its own (same leading dimension)
    D.pj.n = S.nj; D.pj.H = p.H + (size_t)S.n_chain * S.ld + S.n_chain; D.pj.y = p.y + S.n_chain;
    D.chains = (const PoChain*)(arena + o[5]);
    D.Lf_j = (double*)(arena + o_Lf);
    D.linv = (double*)(arena + o_linv);
    D.n_l1 = S.n_l1;
    D.x0 = (const double*)(arena + o[8]);
    D.report = (double*)(arena + b->o_report[(size_t)a]);
  }
  put(o_graphs, desc.data(), sizeof(PoBatchGraph) * desc.size());
  if (arena) {
    b->h_desc = desc;
    b->d_graphs = (PoBatchGraph*)(arena + o_graphs); b->d_items = (PoItem*)(arena + o_items); b->d_jgraphs = (int*)(arena + o_jg);
  }
  *total_bytes = carve.off;
}
}  // namespace

extern "C" int slslam_po_batch_finalize(slslam_po_batch* b, const slslam_solver_options* opt_in) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (b->finalized) return SLSLAM_ERR_STATE;
  slslam_solver_options opt;
  if (!po_policy(opt_in, &opt, &b->pol)) return SLSLAM_ERR_INVALID_ARGUMENT;      // (slslam_po_solve's policy)
  if (opt.po_dense_factor || opt.po_factor_fp32) return SLSLAM_ERR_UNSUPPORTED;      // the structured fp64 factorisation only
  b->huber = opt.po_huber_delta;
  const int ndev = device_count();
  if (ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (b->device < 0) { if (hipGetDevice(&b->device) != hipSuccess) return SLSLAM_ERR_NO_DEVICE; }
  if (b->device >= ndev) return SLSLAM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(b->device));
  b->active.clear();
  b->weighted = false;
  for (size_t i = 0; i < b->graphs.size(); ++i) {
    b->graphs[i].active = b->graphs[i].E > 0 ? (int)b->active.size() : -1;
    if (b->graphs[i].E > 0) { b->active.push_back((int)i); b->weighted = b->weighted || b->graphs[i].weighted; }
  }
  if (!b->active.empty()) {
    size_t up = 0, down = 0, total = 0;
    po_batch_layout(b, nullptr, &up, &down, &total);
    hipError_t e = hipFuncSetAttribute((const void*)k_pob_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStepLds);
    if (e == hipSuccess) e = hipMalloc((void**)&b->arena, total);
    if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_up, b->init_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&b->h_down, down, hipHostMallocDefault);
    if (e == hipSuccess) {
      std::memset(b->h_up, 0, b->init_bytes);
      po_batch_layout(b, b->arena, &b->up_bytes, &b->down_bytes, &total);
      e = hipMemcpy(b->arena, b->h_up, b->init_bytes, hipMemcpyHostToDevice);
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
  b->cov_pending = b->cov_valid = false;    // (a covariance enqueued before this call is no longer the covariance at the batch's poses)
  if (b->active.empty()) return SLSLAM_OK;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpyAsync(b->arena, b->h_up, b->up_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_solve(slslam_po_batch* b, void* stream) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  b->have_results = false;
  b->cov_pending = b->cov_valid = false;    // (a covariance enqueued before this call is no longer the covariance at the batch's poses)
  const int A = (int)b->active.size();
  if (A == 0) return SLSLAM_OK;
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  const PoBatchGraph* gs = b->d_graphs;
  const PoItem* items = b->d_items;
  const Policy pol = b->pol;
  auto linearise = [&](int mode) {          // with the loss (po_huber_delta > 0) or, as before there was one, without; whitening only when a graph has weights
    const dim3 g_edges((unsigned)b->edge_cnt);
    const bool robust = b->huber > 0.0;
    if (b->weighted) {
      if (robust) hipLaunchKernelGGL((k_pob_linearise<true, true>), g_edges, dim3(64), 0, s, gs, items + b->edge_off, mode);
      else hipLaunchKernelGGL((k_pob_linearise<false, true>), g_edges, dim3(64), 0, s, gs, items + b->edge_off, mode);
    } else if (robust) hipLaunchKernelGGL((k_pob_linearise<true, false>), g_edges, dim3(64), 0, s, gs, items + b->edge_off, mode);
    else hipLaunchKernelGGL((k_pob_linearise<false, false>), g_edges, dim3(64), 0, s, gs, items + b->edge_off, mode);
  };
  auto zero_and_linearise = [&]() {
    hipLaunchKernelGGL(k_pob_zero, dim3((unsigned)b->zero_cnt), dim3(256), 0, s, gs, items + b->zero_off);
    linearise(0);
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
      HIP_TRY(hipMemcpyAsync(b->h_down, b->arena, sizeof(LMState) * (size_t)A, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
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
    linearise(1);
    hipLaunchKernelGGL(k_pob_update, dim3((unsigned)A), dim3(64), 0, s, gs, pol);
  }
  HIP_TRY(hipGetLastError());
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_download(slslam_po_batch* b, void* stream) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  const int A = (int)b->active.size();
  if (A > 0) {
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)stream;
    // every graph's edge report (slslam_po_batch_get_edge_report), at the batch's own po_huber_delta, in one launch ahead of the copy
    if (b->weighted) hipLaunchKernelGGL(k_pob_edge_report<true>, dim3((unsigned)b->edge_cnt), dim3(64), 0, s, (const PoBatchGraph*)b->d_graphs, (const PoItem*)(b->d_items + b->edge_off));
    else hipLaunchKernelGGL(k_pob_edge_report<false>, dim3((unsigned)b->edge_cnt), dim3(64), 0, s, (const PoBatchGraph*)b->d_graphs, (const PoItem*)(b->d_items + b->edge_off));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b->h_down, b->arena, b->down_bytes, hipMemcpyDeviceToHost, s));
    if (b->cov_pending) HIP_TRY(hipMemcpyAsync(b->cov_h_down, b->cov_dev + b->cov_plan.down_off, b->cov_plan.down_bytes, hipMemcpyDeviceToHost, s));
    if (b->cov_pending && b->gate_call && b->gate_plan.down_bytes > 0) HIP_TRY(hipMemcpyAsync(b->gate_h_down, b->cov_dev + b->gate_plan.down_off, b->gate_plan.down_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
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
      G.report.resize((size_t)2 * G.E);
      std::memcpy(G.report.data(), b->h_down + b->o_report[(size_t)a], sizeof(double) * 2 * (size_t)G.E);
      steps = std::max(steps, G.st.n_success + G.st.n_unsuccess);
      if (!b->cov_pending) continue;
      const PoCovPlan& P = b->cov_plan;      // the covariances enqueued since the last download come back with the other results
      std::memcpy(&G.cov_status, b->cov_h_down + P.o_status + sizeof(int) * (size_t)a, sizeof(int));
      G.cov_poses.resize((size_t)36 * G.N);
      std::memcpy(G.cov_poses.data(), b->cov_h_down + P.o_poses[(size_t)a], sizeof(double) * 36 * (size_t)G.N);
      G.cov_pairs.resize((size_t)36 * G.cov_pa.size());
      if (!G.cov_pa.empty()) std::memcpy(G.cov_pairs.data(), b->cov_h_down + P.o_pairs[(size_t)a], sizeof(double) * 36 * G.cov_pa.size());
      if (!b->gate_call || b->gate_plan.down_bytes == 0) continue;
      const size_t m = G.gate_pa.size();     // the gate's results, likewise
      G.gate_status.resize(m); G.gate_err.resize(6 * m); G.gate_cov.resize(36 * m); G.gate_W.resize(36 * m); G.gate_m2.resize(m);
      po_gate_read(b->gate_plan, b->gate_h_down, a, (int)m, nullptr, G.gate_status.data(), G.gate_err.data(), G.gate_cov.data(), G.gate_W.data(), G.gate_m2.data());
    }
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  if (A > 0) b->iter_hint = steps;
  if (b->cov_pending) { b->cov_pending = false; b->cov_valid = true; }
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
}  // namespace

extern "C" int slslam_po_batch_get_parameters(const slslam_po_batch* b, int index, double* parameters) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  if (G->N > 0 && !parameters) return SLSLAM_ERR_INVALID_ARGUMENT;
  // a numerical failure leaves the parameters untouched (slslam_po_solve)
  const bool solved = G->active >= 0 && po_termination(&G->st) != SLSLAM_NUMERICAL_FAILURE;
  if (G->N > 0) std::memcpy(parameters, solved ? G->x.data() : G->x0.data(), sizeof(double) * 6 * (size_t)G->N);
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_edge_report(const slslam_po_batch* b, int index, double* sq_norm, double* weight) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  const size_t E = (size_t)G->E;             // (a graph without edges: nothing to report)
  if (sq_norm && E) std::memcpy(sq_norm, G->report.data(), sizeof(double) * E);
  if (weight && E) std::memcpy(weight, G->report.data() + E, sizeof(double) * E);
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_summary(const slslam_po_batch* b, int index, slslam_summary* s) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  if (!s) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::memset(s, 0, sizeof(*s));
  s->termination_type = po_termination(G->active < 0 ? nullptr : &G->st);              // (no edges: nothing was solved)
  if (G->active >= 0) po_fill_summary(G->st, s->termination_type, G->sym, s);
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_trace(const slslam_po_batch* b, int index, slslam_iteration* trace, int cap, int* len) {
  const slslam_po_batch::Graph* G = nullptr;
  const int rc = po_batch_graph(b, index, &G);
  if (rc != SLSLAM_OK) return rc;
  po_export_trace(G->st, G->trace.data(), trace, cap, len);      // (a graph without edges: its state is all zero, no records)
  return SLSLAM_OK;
}

// ---- covariances of the batch's graphs (po_covariance.h: the kernels and the plan)
extern "C" int slslam_po_batch_set_covariance_pairs(slslam_po_batch* b, int index, int num_pairs, const int* pair_a, const int* pair_b) {
  if (!b || index < 0 || index >= (int)b->graphs.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_po_batch::Graph& G = b->graphs[(size_t)index];
  if (!po_cov_pairs_ok(G.N, num_pairs, pair_a, pair_b)) return SLSLAM_ERR_INVALID_ARGUMENT;
  try {
    std::vector<int> pa(pair_a, pair_a + num_pairs), pb(pair_b, pair_b + num_pairs);
    G.cov_pa.swap(pa); G.cov_pb.swap(pb);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  b->cov_dirty = true;
  b->cov_pending = b->cov_valid = false;    // (results of a call made with the previous list no longer match the list)
  return SLSLAM_OK;
}

namespace {
// slslam_po_batch_covariance and slslam_po_batch_gate: the covariance launch sequence and, for the gate, k_po_gate behind it
int po_batch_covariance_call(slslam_po_batch* b, void* stream, bool gate) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!b->finalized) return SLSLAM_ERR_STATE;
  const int A = (int)b->active.size();
  ++b->cov_calls;
  b->cov_valid = false;
  b->gate_call = gate;
  if (A == 0) { b->cov_pending = true; return SLSLAM_OK; }
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t s = (hipStream_t)stream;
  if (b->cov_dirty) {
    try {
      std::vector<PoCovInput> in((size_t)A);
      bool any_candidates = false;          // without any, the plan is slslam_po_batch_covariance's as it always was: no gate region
      for (int a = 0; a < A; ++a) any_candidates = any_candidates || !b->graphs[(size_t)b->active[(size_t)a]].gate_pa.empty();
      std::vector<PoGateInput> gin(any_candidates ? (size_t)A : 0);
      for (int a = 0; a < A; ++a) {
        auto& G = b->graphs[(size_t)b->active[(size_t)a]];
        G.plan_pa = G.cov_pa; G.plan_pa.insert(G.plan_pa.end(), G.gate_pa.begin(), G.gate_pa.end());
        G.plan_pb = G.cov_pb; G.plan_pb.insert(G.plan_pb.end(), G.gate_pb.begin(), G.gate_pb.end());
        const PoBatchGraph& D = b->h_desc[(size_t)a];
        PoCovInput& I = in[(size_t)a];
        I.N = G.N; I.E = G.E; I.n = G.sym.n; I.ld = G.sym.ld;
        I.d_p1 = D.p.p1; I.d_p2 = D.p.p2; I.d_slot = D.p.slot; I.d_cons = D.p.cons; I.d_winfo = D.p.winfo;      // the batch's own arrays: the chains-first slots do as well as any
        I.d_x_src = D.p.x; I.d_st_src = D.p.st; I.d_x0 = D.x0;
        I.pa = G.plan_pa.data(); I.pb = G.plan_pb.data(); I.P = (int)G.plan_pa.size();
        if (!any_candidates) continue;
        PoGateInput& Q = gin[(size_t)a];
        Q.num = (int)G.gate_pa.size(); Q.pair_off = (int)G.cov_pa.size(); Q.cons = G.gate_cons.data();
        Q.rmeas = G.gate_r.empty() ? nullptr : G.gate_r.data(); Q.sigma2 = G.gate_sigma2;
      }
      PoCovPlan plan;
      PoGatePlan gplan;
      PoCarve gcarve;
      gcarve.off = po_cov_layout(in, b->huber, PoCarve(), nullptr, nullptr, &plan);
      const size_t bytes = any_candidates ? po_gate_layout(gin, gcarve, nullptr, nullptr, &gplan) : gcarve.off;
      HIP_TRY(hipStreamSynchronize(s));     // (an earlier covariance call may still read the plan that is about to be replaced)
      if (bytes > b->cov_dev_bytes) {
        if (b->cov_dev) (void)hipFree(b->cov_dev);
        b->cov_dev = nullptr; b->cov_dev_bytes = 0;
        HIP_TRY(hipMalloc((void**)&b->cov_dev, bytes));
        b->cov_dev_bytes = bytes; ++b->cov_allocs;
      }
      if (plan.down_bytes > b->cov_down_cap) {
        if (b->cov_h_down) (void)hipHostFree(b->cov_h_down);
        b->cov_h_down = nullptr; b->cov_down_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&b->cov_h_down, plan.down_bytes, hipHostMallocDefault));
        b->cov_down_cap = plan.down_bytes; ++b->cov_allocs;
      }
      if (gplan.down_bytes > b->gate_down_cap) {
        if (b->gate_h_down) (void)hipHostFree(b->gate_h_down);
        b->gate_h_down = nullptr; b->gate_down_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&b->gate_h_down, gplan.down_bytes, hipHostMallocDefault));
        b->gate_down_cap = gplan.down_bytes; ++b->cov_allocs;
      }
      std::vector<char> img, gimg;
      po_cov_layout(in, b->huber, PoCarve(), b->cov_dev, &img, &plan);
      if (any_candidates) po_gate_layout(gin, gcarve, b->cov_dev, &gimg, &gplan);
      HIP_TRY(hipMemcpyAsync(b->cov_dev + plan.img_off, img.data(), plan.img_bytes, hipMemcpyHostToDevice, s));
      if (any_candidates) HIP_TRY(hipMemcpyAsync(b->cov_dev + gplan.img_off, gimg.data(), gplan.img_bytes, hipMemcpyHostToDevice, s));
      HIP_TRY(hipStreamSynchronize(s));     // (img leaves scope)
      HIP_TRY(po_cov_lds_attribute());
      b->cov_plan = std::move(plan);
      b->gate_plan = std::move(gplan);
      b->cov_dirty = false;
    } catch (const std::bad_alloc&) {
      return SLSLAM_ERR_NO_MEMORY;
    }
  }
  int rc = po_cov_enqueue(b->cov_plan, s);
  if (rc == SLSLAM_OK && gate) rc = po_gate_enqueue(b->cov_plan, b->gate_plan, s);
  if (rc == SLSLAM_OK) b->cov_pending = true;
  return rc;
}
}  // namespace

extern "C" int slslam_po_batch_covariance(slslam_po_batch* b, void* stream) { return po_batch_covariance_call(b, stream, false); }

// ---- the gate (po_gate.h): candidates per graph, judged behind a covariance call of the batch
extern "C" int slslam_po_batch_set_candidates(slslam_po_batch* b, int index, const slslam_po_candidates* c) {
  if (!b || index < 0 || index >= (int)b->graphs.size()) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_po_batch::Graph& G = b->graphs[(size_t)index];
  if (!po_candidates_ok(G.N, c)) return SLSLAM_ERR_INVALID_ARGUMENT;
  try {
    const size_t m = (size_t)c->num;
    std::vector<int> pa(c->pose_a, c->pose_a + m), pb(c->pose_b, c->pose_b + m);
    std::vector<double> cons(c->constraints, c->constraints + 6 * m), r;
    if (c->cov_meas && m) r.assign(c->cov_meas, c->cov_meas + 36 * m);
    G.gate_pa.swap(pa); G.gate_pb.swap(pb); G.gate_cons.swap(cons); G.gate_r.swap(r);
    G.gate_sigma2 = c->sigma2;
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  b->cov_dirty = true;
  b->cov_pending = b->cov_valid = false;    // (results of a call made with the previous list no longer match the list)
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_gate(slslam_po_batch* b, void* stream) {
  const int rc = po_batch_covariance_call(b, stream, true);
  if (rc != SLSLAM_OK) return rc;
  // a graph without edges is not on the device (no free pose: every Sigma block is zero, S = R): its candidates go through the primitive
  for (auto& G : b->graphs) {
    const int m = (int)G.gate_pa.size();
    if (G.active >= 0 || m == 0) continue;
    try {
      std::vector<double> xa((size_t)6 * m), xb((size_t)6 * m);
      for (int k = 0; k < m; ++k) {
        std::memcpy(&xa[(size_t)6 * k], &G.x0[(size_t)6 * G.gate_pa[(size_t)k]], sizeof(double) * 6);
        std::memcpy(&xb[(size_t)6 * k], &G.x0[(size_t)6 * G.gate_pb[(size_t)k]], sizeof(double) * 6);
      }
      G.gate_status.resize((size_t)m); G.gate_err.resize((size_t)6 * m); G.gate_cov.resize((size_t)36 * m); G.gate_W.resize((size_t)36 * m); G.gate_m2.resize((size_t)m);
      slslam_po_edge_items it = { m, xa.data(), xb.data(), G.gate_cons.data(), nullptr, nullptr, nullptr, G.gate_r.empty() ? nullptr : G.gate_r.data(), G.gate_sigma2 };
      const int re = slslam_po_edge_statistics(&it, G.gate_status.data(), G.gate_err.data(), G.gate_cov.data(), G.gate_W.data(), G.gate_m2.data());
      if (re != SLSLAM_OK) return re;
    } catch (const std::bad_alloc&) {
      return SLSLAM_ERR_NO_MEMORY;
    }
  }
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_gate(const slslam_po_batch* b, int index, int* status, double* error, double* cov, double* sqrt_information,
                                        double* mahalanobis2) {
  if (!b || index < 0 || index >= (int)b->graphs.size() || !b->cov_valid || !b->gate_call) return SLSLAM_ERR_INVALID_ARGUMENT;
  const slslam_po_batch::Graph& G = b->graphs[(size_t)index];
  const size_t m = G.gate_pa.size();
  if (m == 0) return SLSLAM_OK;
  if (status) std::memcpy(status, G.gate_status.data(), sizeof(int) * m);
  if (error) std::memcpy(error, G.gate_err.data(), sizeof(double) * 6 * m);
  if (cov) std::memcpy(cov, G.gate_cov.data(), sizeof(double) * 36 * m);
  if (sqrt_information) std::memcpy(sqrt_information, G.gate_W.data(), sizeof(double) * 36 * m);
  if (mahalanobis2) std::memcpy(mahalanobis2, G.gate_m2.data(), sizeof(double) * m);
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_get_covariance(const slslam_po_batch* b, int index, int* status, double* cov_poses, double* cov_pairs) {
  if (!b || index < 0 || index >= (int)b->graphs.size() || !b->cov_valid) return SLSLAM_ERR_INVALID_ARGUMENT;
  const slslam_po_batch::Graph& G = b->graphs[(size_t)index];
  const size_t np = 36 * (size_t)G.N, nq = 36 * G.cov_pa.size();
  const bool have = G.active >= 0;           // (a graph without edges has no free pose: zeros)
  if (status) *status = have ? G.cov_status : SLSLAM_COV_OK;
  if (cov_poses && np) { if (have) std::memcpy(cov_poses, G.cov_poses.data(), sizeof(double) * np); else std::memset(cov_poses, 0, sizeof(double) * np); }
  if (cov_pairs && nq) { if (have) std::memcpy(cov_pairs, G.cov_pairs.data(), sizeof(double) * nq); else std::memset(cov_pairs, 0, sizeof(double) * nq); }
  return SLSLAM_OK;
}

extern "C" int slslam_po_batch_covariance_stats(const slslam_po_batch* b, long long* calls, long long* allocations) {
  if (!b) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (calls) *calls = b->cov_calls;
  if (allocations) *allocations = b->cov_allocs;
  return SLSLAM_OK;
}

#endif  // SLSLAM_PO_BATCH_H_

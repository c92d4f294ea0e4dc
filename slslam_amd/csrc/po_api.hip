// slslam_amd/csrc/po_api.hip — C ABI of the pose-graph path: slslam_po_solve replaces
// POProblem::build + POProblem::set_options + ceres::Solve (reference src/slam.cpp:1283-1293).
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <type_traits>
#include <mutex>
#include <vector>

#include "../../include/slslam_hip.h"
#include "po_kernels.h"
#include "device_cache.h"
#include "call_block.h"

using namespace slslam;

namespace {

enum { kMaxChain = 32 };

// Symbolic analysis of the structured factorisation: junction = free pose with >= 3 distinct free
// neighbours (plus one pose per junction-free cycle); every other free pose lies on a chain.
// Output: slot[] (offset of each pose in the reduced vector: chains first, pose by pose along the
// path; junctions last), the chain descriptors, n_chain = unknowns before the junction block.
void order_chains_first(int N, int E, const int* p1, const int* p2, const std::vector<int>& used, int gauge,
                        std::vector<int>& slot, std::vector<PoChain>& chains, int* n_chain, int* n_total, std::vector<int>* level_counts) {
  std::vector<std::vector<int>> adj(N);
  auto add = [&](int a, int b) { for (int v : adj[a]) if (v == b) return; adj[a].push_back(b); };
  for (int e = 0; e < E; ++e) {
    const int a = p1[e], b = p2[e];
    if (a == gauge || b == gauge) continue;           // the constant pose only contributes to diagonals
    add(a, b); add(b, a);
  }
  std::vector<char> isfree(N, 0), junction(N, 0), done(N, 0);
  for (int k = 0; k < N; ++k) isfree[k] = used[k] && k != gauge;
  for (int k = 0; k < N; ++k) if (isfree[k] && adj[k].size() >= 3) junction[k] = 1;
  std::vector<std::vector<int>> paths;
  auto walk = [&](int start) {                        // start: a chain pose with at most one chain neighbour
    std::vector<int> path;
    int prev = -1, cur = start;
    while (cur >= 0) {
      path.push_back(cur); done[cur] = 1;
      int nxt = -1;
      for (int v : adj[cur]) if (v != prev && !junction[v] && !done[v]) { nxt = v; break; }
      prev = cur; cur = nxt;
    }
    paths.push_back(path);
  };
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = 0; k < N; ++k) {
      if (!isfree[k] || junction[k] || done[k]) continue;
      int chain_nb = 0;
      for (int v : adj[k]) if (!junction[v] && !done[v]) ++chain_nb;
      if (chain_nb <= 1) walk(k);
    }
    if (pass == 0)                                    // what is left are junction-free cycles: open each at one pose
      for (int k = 0; k < N; ++k)
        if (isfree[k] && !junction[k] && !done[k]) {
          bool alone = true;                          // still untouched after this loop's earlier promotions?
          for (int v : adj[k]) if (junction[v]) alone = false;
          if (alone) {                                // one pose per cycle: walk the rest of the cycle right away, so that no
            junction[k] = 1;                          // other pose of it is promoted (its poses are chain poses from here on)
            for (int v : adj[k]) if (isfree[v] && !junction[v] && !done[v]) { walk(v); break; }
          }
        }
  }
  // a chain whose two ends meet the same junction: move its last pose to the junctions
  for (auto& path : paths) {
    if (path.size() < 2) continue;
    int jl = -1, jr = -1;
    for (int v : adj[path.front()]) if (junction[v]) jl = v;
    for (int v : adj[path.back()]) if (junction[v]) jr = v;
    if (jl >= 0 && jl == jr) { junction[path.back()] = 1; path.pop_back(); }
  }
  // A chain is sequential (one 6 x 6 step after the other, ~2 us each), so long paths are cut - on several LEVELS since round 5: a path of L poses
  // becomes pieces of s poses separated by single CUT poses (level-1 chains: their ends are cut poses or the path's junctions), and the cut
  // poses of a path, in path order, are a chain of their own on the next level: eliminating the pieces leaves them coupled to each other and to
  // the path's two junctions exactly as the poses of a chain are (the pieces' Schur complements land on the blocks (c_i, c_i), (c_i+1, c_i),
  // (junction, c_1), (junction, c_m) - what k_po_chain_eliminate reads for a chain c_1 .. c_m) - so that chain is cut the same way, and so on.
  // The same two kernels run once per level, upwards for the elimination, downwards for the substitution; s ~ L^(1/levels) with up to three
  // levels, i.e. a sequential depth of ~3 L^(1/3) steps for a long path instead of min(L, 32), and the cut poses no longer enlarge the dense
  // junction block (until round 5 a path was cut every 32 poses and the cut poses joined the junctions: 26 junction poses instead of 10
  // for the 260-pose bench graph - a second 64-wide block step of the dense factorisation in every iteration).
  struct Piece { std::vector<int> poses; int left, right; };      // left / right: the POSE the piece ends at (-1: a free end)
  std::vector<std::vector<Piece>> levels;
  {
    auto piece_len = [](size_t L) -> size_t {
      const int m = L <= 8 ? 1 : (L <= 72 ? 2 : 3);                    // levels this chain is spread over
      if (m <= 1) return L;
      return (size_t)std::min((int)kMaxChain, std::max(2, (int)std::lround(std::pow((double)L, 1.0 / m))));
    };
    struct Job { std::vector<int> seq; int left, right, level; };
    std::vector<Job> jobs;
    for (auto& path : paths) {
      int jl_pose = -1, jr_pose = -1;
      for (int v : adj[path.front()]) if (junction[v]) jl_pose = v;
      for (int v : adj[path.back()]) if (junction[v] && (path.size() > 1 || v != jl_pose)) jr_pose = v;
      jobs.push_back(Job{ path, jl_pose, jr_pose, 0 });
    }
    for (size_t q = 0; q < jobs.size(); ++q) {                         // (jobs grows: a cut chain is the next level's job)
      const Job job = jobs[q];
      if (levels.size() <= (size_t)job.level) levels.resize((size_t)job.level + 1);
      const size_t sub = std::max<size_t>(1, piece_len(job.seq.size()));
      std::vector<int> cuts;
      size_t b = 0;
      int left = job.left;
      while (job.seq.size() - b > sub + 1 && job.level < 7) {            // (at least one pose is left behind the cut pose; eight levels at most)
        levels[(size_t)job.level].push_back(Piece{ std::vector<int>(job.seq.begin() + b, job.seq.begin() + b + sub), left, job.seq[b + sub] });
        left = job.seq[b + sub];
        cuts.push_back(left);
        b += sub + 1;
      }
      // (the rest of the chain; longer than kMaxChain only when the level cap above was reached - then it is simply a long chain)
      levels[(size_t)job.level].push_back(Piece{ std::vector<int>(job.seq.begin() + b, job.seq.end()), left, job.right });
      if (!cuts.empty()) jobs.push_back(Job{ cuts, job.left, job.right, job.level + 1 });
    }
  }
  int n = 0;
  for (const auto& lv : levels)
    for (const Piece& pc : lv) {
      PoChain c;
      c.start = n; c.len = (int)pc.poses.size(); c.jl = -1; c.jr = -1;
      for (int v : pc.poses) { slot[v] = n; n += 6; }
      chains.push_back(c);
    }
  if (level_counts) { level_counts->clear(); for (const auto& lv : levels) level_counts->push_back((int)lv.size()); }
  *n_chain = n;
  for (int k = 0; k < N; ++k) if (isfree[k] && junction[k]) { slot[k] = n; n += 6; }
  *n_total = n;
  {
    size_t q = 0;
    for (const auto& lv : levels)
      for (const Piece& pc : lv) {
        PoChain& c = chains[q++];
        c.jl = pc.left >= 0 ? slot[pc.left] : -1;
        c.jr = pc.right >= 0 ? slot[pc.right] : -1;
      }
  }
}

}  // namespace

// ---- what slslam_po_solve, slslam_po_batch_* and slslam_po_structure share on the host
namespace {

// The graph checks of slslam_po_solve and slslam_po_batch_add, in two steps (slslam_po_solve looks at its options in between).
// values = false: the index arrays only (slslam_po_structure reads neither constraints nor parameters).
bool po_graph_arrays_ok(const slslam_po_graph* g, bool values) {
  const int N = g->num_poses, E = g->num_edges;
  if (N < 0 || E < 0) return false;
  if (E > 0 && (!g->pose_index_1 || !g->pose_index_2 || (values && !g->constraints))) return false;
  return !(values && N > 0 && !g->parameters);
}
bool po_graph_entries_ok(const slslam_po_graph* g, bool values) {
  const int N = g->num_poses, E = g->num_edges;
  for (int e = 0; e < E; ++e) {
    const int a = g->pose_index_1[e], b = g->pose_index_2[e];
    if (a < 0 || a >= N || b < 0 || b >= N || a == b) return false;
    for (int q = 0; values && q < 6; ++q) if (!std::isfinite(g->constraints[6 * (size_t)e + q])) return false;
  }
  for (size_t i = 0; values && i < (size_t)6 * N; ++i) if (!std::isfinite(g->parameters[i])) return false;
  // the edges' square-root information matrices, when given: any finite values (an all-zero W_e removes its edge)
  for (size_t i = 0; values && g->sqrt_information && i < (size_t)36 * E; ++i) if (!std::isfinite(g->sqrt_information[i])) return false;
  return true;
}

// po_huber_delta as the C ABI takes it: 0 (no loss) or a finite positive scale.
bool po_huber_ok(double delta) { return std::isfinite(delta) && delta >= 0.0; }

// The caller's options (the defaults when there are none) and the numeric policy the kernels take.  false: max_num_iterations out of range
// or po_huber_delta negative / not finite.  (The edges' loss travels in PoPtrs.huber; Policy.huber_delta is the LBA path's and stays 0.)
bool po_policy(const slslam_solver_options* opt_in, slslam_solver_options* opt, Policy* pol) {
  if (opt_in) *opt = *opt_in; else slslam_default_options(opt);
  if (opt->max_num_iterations < 0 || opt->max_num_iterations > 100000) return false;
  if (!po_huber_ok(opt->po_huber_delta)) return false;
  std::memset(pol, 0, sizeof(*pol));
  pol->huber_delta = 0.0; pol->baseline = 0.0;
  pol->initial_radius = opt->initial_trust_region_radius; pol->max_radius = opt->max_trust_region_radius;
  pol->min_radius = opt->min_trust_region_radius; pol->min_relative_decrease = opt->min_relative_decrease;
  pol->min_lm_diagonal = opt->min_lm_diagonal; pol->max_lm_diagonal = opt->max_lm_diagonal;
  pol->function_tolerance = opt->function_tolerance; pol->gradient_tolerance = opt->gradient_tolerance;
  pol->parameter_tolerance = opt->parameter_tolerance; pol->max_num_iterations = opt->max_num_iterations;
  pol->max_invalid = opt->max_num_consecutive_invalid_steps; pol->jacobi_scaling = opt->jacobi_scaling; pol->keep_jacobian = 0;
  return true;
}

// Everything that follows from a graph's edge lists alone.
struct PoSymbolic {
  std::vector<int> slot;                 // [N] offset of each pose in the reduced vector; -1: the constant pose or a pose no edge references
  std::vector<PoChain> chains;           // level after level
  std::vector<int> level_counts;         // chains per level
  int n_chain = 0;                       // unknowns of the chain poses (ordered first: level-1 chains, then the chains of cut poses, level after level)
  int n = 0, kept = 0, ld = 0;           // unknowns, edges with a free pose, leading dimension of the normal matrix
  int nj = 0, nblk_j = 0;                // the junction block: unknowns, 64-wide blocks
  int n_l1 = 0;                          // unknowns of the level-1 chains
};

// chains_first: the ordering of the structured factorisation (order_chains_first); otherwise the free poses in index order, no chains and
// no junction block (the dense factorisations of slslam_po_solve).
void po_analyse(int N, int E, const int* p1, const int* p2, bool chains_first, PoSymbolic* S) {
  *S = PoSymbolic();
  S->slot.assign((size_t)N, -1);
  if (E == 0) return;
  // program reduction: pose1 of edge 0 is constant (po_problem.cpp:62-63); unreferenced poses are not in the problem
  std::vector<int> used((size_t)N, 0);
  for (int e = 0; e < E; ++e) { used[p1[e]] = 1; used[p2[e]] = 1; }
  const int gauge = p1[0];
  if (chains_first) order_chains_first(N, E, p1, p2, used, gauge, S->slot, S->chains, &S->n_chain, &S->n, &S->level_counts);
  else for (int k = 0; k < N; ++k) if (used[k] && k != gauge) { S->slot[k] = S->n; S->n += 6; }
  for (int e = 0; e < E; ++e) if (S->slot[p1[e]] >= 0 || S->slot[p2[e]] >= 0) ++S->kept;
  S->ld = ((S->n + 7) / 8) * 8 + 8;
  if (!chains_first) return;
  S->nj = S->n - S->n_chain;
  S->nblk_j = (S->nj + kNB - 1) / kNB;
  const int n_level1 = S->level_counts.empty() ? 0 : S->level_counts[0];
  S->n_l1 = n_level1 > 0 ? S->chains[(size_t)n_level1 - 1].start + 6 * S->chains[(size_t)n_level1 - 1].len : 0;
}

// Workgroups of k_po_zero_structured.  What the level-1 eliminations ADD into - the blocks of the cut poses and of the junctions, among
// themselves - starts at zero: the square behind the level-1 unknowns (the dense factorisation reads the junction block of it), beside
// the E blocks the linearisation adds into, the gradient and the cost.
long long po_zero_blocks(const PoSymbolic& S, int E) {
  const long long nz = S.n - S.n_l1, zero_items = (long long)E * 144 + nz * nz + S.n + 1;
  return (zero_items + 255) / 256;
}

// st == nullptr: nothing was solved (no edges, or no non-constant parameter block).
int po_termination(const LMState* st) {
  if (!st) return SLSLAM_FUNCTION_TOLERANCE;
  return st->status == kRunning ? SLSLAM_NO_CONVERGENCE : st->status;
}

void po_fill_summary(const LMState& st, int termination, const PoSymbolic& S, slslam_summary* s) {
  s->num_successful_steps = st.n_success; s->num_unsuccessful_steps = st.n_unsuccess;
  s->initial_cost = st.initial_cost;
  s->final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;
  s->fixed_cost = st.fixed_cost; s->termination_type = termination;
  s->num_free_parameters = S.n; s->num_residual_blocks = S.kept;
}

void po_export_trace(const LMState& st, const IterRec* recs, slslam_iteration* trace, int cap, int* len) {
  const int nt = st.ntrace < kMaxTrace ? st.ntrace : kMaxTrace;
  if (len) *len = nt;
  for (int i = 0; trace && i < nt && i < cap; ++i) {
    const IterRec& r = recs[i];
    slslam_iteration& o = trace[i];
    o.iteration = r.iteration; o.step_is_valid = r.step_is_valid; o.step_is_successful = r.step_is_successful;
    o.cost = r.cost; o.cost_change = r.cost_change; o.gradient_max_norm = r.gradient_max_norm;
    o.step_norm = r.step_norm; o.relative_decrease = r.relative_decrease;
    o.trust_region_radius = r.trust_region_radius; o.model_cost_change = r.model_cost_change;
  }
}

// Carves one allocation into 256-byte aligned pieces: take() returns the piece's offset, off is what has been handed out.
struct PoCarve {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

}  // namespace

namespace {
// Optional timing of slslam_po_solve (slslam_po_set_profiling): hipEvents on the solve's stream around the whole device
// part and around every factorisation + triangular solve; read back with slslam_po_last_timing.
struct PoTiming { bool enabled = false; double total_ms = 0, factor_ms = 0, factor_max_ms = 0; int factor_calls = 0, unknowns = 0, junction_unknowns = 0; };
thread_local PoTiming g_po_timing;
}  // namespace

extern "C" int slslam_po_set_profiling(int enable) { g_po_timing.enabled = enable != 0; return SLSLAM_OK; }
extern "C" int slslam_po_last_timing(double* total_ms, double* factor_ms, int* factor_calls, int* unknowns, int* junction_unknowns) {
  if (total_ms) *total_ms = g_po_timing.total_ms;
  if (factor_ms) *factor_ms = g_po_timing.factor_max_ms;
  if (factor_calls) *factor_calls = g_po_timing.factor_calls;
  if (unknowns) *unknowns = g_po_timing.unknowns;
  if (junction_unknowns) *junction_unknowns = g_po_timing.junction_unknowns;
  return SLSLAM_OK;
}

namespace {
// Blocked right-looking Cholesky of an nb-block matrix: the first diagonal block, then ONE launch per block step (k_po_step:
// panel solve + trailing update + the next diagonal block's factorisation; three launches per step until round 4).
template <typename T>
void po_factor_dense(PoPtrs& pp, T* A, T* Lf, T* linv, int nb) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_po_potrf_diag<T>, dim3(1), dim3(256), 0, 0, pp, A, linv, 0, Lf);
  for (int bk = 0; bk + 1 < nb; ++bk) {
    const int tb = nb - 1 - bk;
    hipLaunchKernelGGL(k_po_step<T>, dim3((unsigned)(tb * (tb + 1) / 2)), dim3(256), kPoStepLdsTiles * kNB * kLdT * sizeof(T), 0, pp, A, Lf, linv, bk);
  }
}
// (k_po_step keeps three 64 x 66 tiles in dynamic LDS: 101 KB of doubles - above the 64 KB a kernel gets without asking)
// HIP function attributes are per DEVICE and slslam_po_solve runs on whatever device is current: the limit is raised once per device
// (a bit per device id under a mutex; a process that solves on device 0 and then on device 1 raises it on both).
hipError_t po_step_lds_attributes() {
  static std::mutex mu;
  static unsigned long long done_mask = 0;          // devices 0..63; beyond that the attribute is set on every call (it is cheap)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lock(mu);
  if (dev >= 0 && dev < 64 && ((done_mask >> dev) & 1ull)) return hipSuccess;
  e = hipFuncSetAttribute((const void*)k_po_step<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPoStepLdsTiles * kNB * kLdT * sizeof(double)));
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_po_step<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kPoStepLdsTiles * kNB * kLdT * sizeof(float)));
  if (e == hipSuccess && dev >= 0 && dev < 64) done_mask |= 1ull << dev;
  return e;
}
}  // namespace

namespace {
thread_local int po_iter_hint = -1;      // LM iterations the calling thread's previous pose-graph solve took

// One slslam_po_solve call: what its stages share.  Leaving the call, on whatever path, destroys the profiling events that are still
// alive and hands the device block back.
struct PoSolve {
  const slslam_po_graph* g = nullptr;
  slslam_solver_options opt;
  Policy pol;
  bool f32 = false, structured = true;
  const bool timing = g_po_timing.enabled;
  const PoSymbolic* S = nullptr;         // the calling thread's cached analysis (structured) or dense_sym
  PoSymbolic dense_sym;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  int arena_device = 0;
  char* stage = nullptr;                 // the calling thread's pinned image: the upload, then what comes back
  size_t up_bytes = 0, down_bytes = 0;
  PoPtrs p, pj;                          // the whole system; the junction block as a matrix of its own
  PoChain* d_chains = nullptr;
  double *d_linv = nullptr, *d_Lf = nullptr;   // d_Lf: the Cholesky factor (k_po_step keeps it apart from the matrix it updates)
  float *d_Hf = nullptr, *d_linvf = nullptr, *d_Lff = nullptr;
  unsigned* d_tri_flags = nullptr;       // k_po_trisolve_wide: one progress word per 64-row block
  unsigned tri_epoch = 1;
  int nblk = 0;
  size_t nn = 1, hbytes = 0;             // entries of a vector of unknowns, bytes of the normal matrix (never empty)
  bool zero_small = false;               // k_po_zero_structured instead of whole-matrix memsets
  int wide_resident = 0;                 // workgroups of k_po_trisolve_wide the device keeps resident together (0: not known - the one-workgroup substitution runs)
  dim3 g_zero, g_edges;
  std::vector<hipEvent_t> tev;           // [0] start, [1] end, then (start, stop) per factorisation
  LMState hst;
  bool have_results = false;

  void stamp() {
    hipEvent_t e;
    if (timing && hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, 0); tev.push_back(e); }
  }
  // where the download put what lives at `dev` in the arena
  template <typename T> const T* landed(const T* dev) const { return (const T*)(stage + ((const char*)dev - arena)); }
  ~PoSolve() {
    for (hipEvent_t e : tev) (void)hipEventDestroy(e);
    DeviceBlockCache::give_back(arena, arena_bytes, arena_device);
  }
};

int po_solve_validate(const slslam_po_graph* g, const slslam_solver_options* opt_in, PoSolve& c) {
  if (!g || !po_graph_arrays_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!po_policy(opt_in, &c.opt, &c.pol)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!po_graph_entries_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  c.g = g;
  c.f32 = c.opt.po_factor_fp32 != 0;
  c.structured = !c.f32 && !c.opt.po_dense_factor;
  return SLSLAM_OK;
}

void po_solve_analyse(PoSolve& c) {
  const int N = c.g->num_poses, E = c.g->num_edges;
  const int *p1 = c.g->pose_index_1, *p2 = c.g->pose_index_2;
  if (!c.structured) { po_analyse(N, E, p1, p2, false, &c.dense_sym); c.S = &c.dense_sym; return; }
  // The symbolic analysis depends on the TOPOLOGY alone, and the reference's graph only changes when a loop closure adds an edge
  // (src/slam.cpp:1248-1280): the calling thread keeps the analysis of its last graph and reuses it when the edge lists are the same.
  struct Cached { int N = -1, E = -1; std::vector<int> p1, p2; PoSymbolic sym; };
  static thread_local Cached* last = nullptr;
  if (!last) last = new Cached();          // (never destroyed: no teardown order to get wrong at thread exit)
  const bool hit = last->N == N && last->E == E && std::memcmp(last->p1.data(), p1, sizeof(int) * (size_t)E) == 0 &&
                   std::memcmp(last->p2.data(), p2, sizeof(int) * (size_t)E) == 0;
  if (!hit) {
    last->N = -1;                          // (nothing to hit should the analysis throw half way)
    po_analyse(N, E, p1, p2, true, &last->sym);
    last->p1.assign(p1, p1 + E); last->p2.assign(p2, p2 + E);
    last->N = N; last->E = E;
  }
  c.S = &last->sym;
}

// k_po_trisolve_wide spin-waits across workgroups: all of its nblk workgroups have to be resident together.  Ask the runtime how
// many fit (a CU mask or a compute partition shows up here); when it cannot tell, the one-workgroup substitution runs instead.
int po_wide_resident(bool f32, int device) {
  int num_cus = 0, per_cu = 0;
  (void)hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device);
  const hipError_t eo = f32 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_po_trisolve_wide<float>, 256, 0)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_po_trisolve_wide<double>, 256, 0);
  if (eo == hipSuccess && per_cu > 0 && num_cus > 0) return num_cus;      // (one workgroup per CU is all that is counted on)
  (void)hipGetLastError();
  return 0;
}

// One device allocation carved into the work arrays (17 hipMalloc / hipFree pairs cost more than a small solve); what the host fills comes
// FIRST and contiguous - state | trace | poses (what comes back, in one copy) | indices, slots, constraints, scale, chains, the small zeroed
// words - so that it goes up in ONE copy from a pinned image the calling thread keeps (a dozen synchronous hipMemcpy / hipMemset calls were a
// quarter of a 260-pose solve's host clock)
int po_solve_upload(PoSolve& c) {
  const slslam_po_graph* g = c.g;
  const PoSymbolic& S = *c.S;
  const int N = g->num_poses, E = g->num_edges, n = S.n, ld = S.ld;
  const bool f32 = c.f32;
  c.nn = (size_t)(n > 0 ? n : 1);
  c.hbytes = c.nn * ld * sizeof(double);
  c.nblk = (n + kNB - 1) / kNB;
  c.zero_small = c.structured && n > 0;
  c.g_zero = dim3((unsigned)po_zero_blocks(S, E));
  c.g_edges = dim3((unsigned)((E + 4) / 5));
  const size_t nn = c.nn, nb2 = (size_t)kNB * kNB * (size_t)(c.nblk > 0 ? c.nblk : 1), fbytes = f32 ? sizeof(float) * nn * ld : 0;
  PoCarve a;
  const size_t o_st = a.take(sizeof(LMState)), o_trace = a.take(sizeof(IterRec) * kMaxTrace), o_x = a.take(sizeof(double) * 12 * (N > 0 ? N : 1));
  c.down_bytes = a.off;
  const size_t o_p1 = a.take(sizeof(int) * E), o_p2 = a.take(sizeof(int) * E), o_slot = a.take(sizeof(int) * (N > 0 ? N : 1)),
               o_cons = a.take(sizeof(double) * 6 * E), o_winfo = a.take(g->sqrt_information ? sizeof(double) * 36 * E : 0), o_scale = a.take(sizeof(double) * nn), o_chains = a.take(sizeof(PoChain) * (S.chains.size() + 1)),
               o_scal = a.take(sizeof(double) * 8), o_flags = a.take(sizeof(int) * 2), o_tri = a.take(sizeof(unsigned) * (size_t)(c.nblk + 1));
  c.up_bytes = a.off;
  const size_t o_H = a.take(c.hbytes), o_g = a.take(sizeof(double) * nn), o_d2 = a.take(sizeof(double) * nn), o_y = a.take(sizeof(double) * nn),
               o_linv = a.take(sizeof(double) * nb2), o_Hf = a.take(fbytes), o_Lf = a.take(f32 ? 0 : c.hbytes), o_Lff = a.take(fbytes),
               o_linvf = a.take(f32 ? sizeof(float) * nb2 : 0);
  c.arena_bytes = a.off;
  (void)hipGetDevice(&c.arena_device);
  HIP_TRY(DeviceBlockCache::acquire(a.off, c.arena_device, &c.arena));   // the block of the previous one-shot solve, if large enough
  char* arena = c.arena;
  PoPtrs& p = c.p;
  std::memset(&p, 0, sizeof(p));
  p.p1 = (int*)(arena + o_p1); p.p2 = (int*)(arena + o_p2); p.slot = (int*)(arena + o_slot); p.cons = (double*)(arena + o_cons);
  p.x = (double*)(arena + o_x); p.scale = (double*)(arena + o_scale); p.H = (double*)(arena + o_H); p.g = (double*)(arena + o_g);
  p.d2 = (double*)(arena + o_d2); p.y = (double*)(arena + o_y); c.d_linv = (double*)(arena + o_linv);
  if (f32) { c.d_Hf = (float*)(arena + o_Hf); c.d_linvf = (float*)(arena + o_linvf); c.d_Lff = (float*)(arena + o_Lff); }
  else c.d_Lf = (double*)(arena + o_Lf);
  c.d_tri_flags = (unsigned*)(arena + o_tri);
  p.scal = (double*)(arena + o_scal); p.flags = (int*)(arena + o_flags); p.st = (LMState*)(arena + o_st);
  p.trace = (IterRec*)(arena + o_trace); c.d_chains = (PoChain*)(arena + o_chains);
  p.N = N; p.E = E; p.n = n; p.ld = ld;
  p.huber = c.opt.po_huber_delta;
  p.winfo = g->sqrt_information ? (const double*)(arena + o_winfo) : nullptr;
  c.pj = p;                                // the junction block as a matrix of its own (same leading dimension)
  c.pj.n = S.nj; c.pj.H = p.H + (size_t)S.n_chain * ld + S.n_chain; c.pj.y = p.y + S.n_chain;
  // the pinned image (kept per calling thread, grown on demand)
  struct HostStage { char* p = nullptr; size_t bytes = 0; };
  static thread_local HostStage* hs = nullptr;
  if (!hs) hs = new HostStage();
  if (hs->bytes < c.up_bytes) {
    if (hs->p) (void)hipHostFree(hs->p);
    hs->p = nullptr; hs->bytes = 0;
    HIP_TRY(hipHostMalloc((void**)&hs->p, c.up_bytes + c.up_bytes / 4 + 4096, hipHostMallocDefault));
    hs->bytes = c.up_bytes + c.up_bytes / 4 + 4096;
  }
  char* stage = c.stage = hs->p;
  std::memset(stage, 0, c.up_bytes);
  c.hst = lm_initial_state(c.pol);
  std::memcpy(stage + o_st, &c.hst, sizeof(c.hst));
  std::memcpy(stage + o_x, g->parameters, sizeof(double) * 6 * N);
  std::memcpy(stage + o_x + sizeof(double) * 6 * N, g->parameters, sizeof(double) * 6 * N);
  std::memcpy(stage + o_p1, g->pose_index_1, sizeof(int) * E); std::memcpy(stage + o_p2, g->pose_index_2, sizeof(int) * E);
  std::memcpy(stage + o_slot, S.slot.data(), sizeof(int) * N); std::memcpy(stage + o_cons, g->constraints, sizeof(double) * 6 * E);
  if (g->sqrt_information) std::memcpy(stage + o_winfo, g->sqrt_information, sizeof(double) * 36 * E);
  std::fill_n((double*)(stage + o_scale), nn, 1.0);
  if (!S.chains.empty()) std::memcpy(stage + o_chains, S.chains.data(), sizeof(PoChain) * S.chains.size());
  HIP_TRY(hipMemcpyAsync(arena, stage, c.up_bytes, hipMemcpyHostToDevice, 0));
  c.wide_resident = po_wide_resident(f32, c.arena_device);
  return SLSLAM_OK;
}

// k_po_linearise with the loss (po_huber_delta > 0) or, as before there was one, without; whitening only for a graph that brings
// sqrt_information (without it: the two instantiations there were)
void po_launch_linearise(const PoSolve& c, int mode) {
  const bool robust = c.p.huber > 0.0;
  if (c.p.winfo) {
    if (robust) hipLaunchKernelGGL((k_po_linearise<true, true>), c.g_edges, dim3(64), 0, 0, c.p, mode);
    else hipLaunchKernelGGL((k_po_linearise<false, true>), c.g_edges, dim3(64), 0, 0, c.p, mode);
  } else if (robust) hipLaunchKernelGGL((k_po_linearise<true, false>), c.g_edges, dim3(64), 0, 0, c.p, mode);
  else hipLaunchKernelGGL((k_po_linearise<false, false>), c.g_edges, dim3(64), 0, 0, c.p, mode);
}

// ---- initial evaluation: cost, gradient, column norms -> Jacobi scale
int po_solve_enqueue_initial(PoSolve& c) {
  if (po_step_lds_attributes() != hipSuccess) { HIP_TRY(hipErrorInvalidValue); }
  c.stamp(); c.stamp();                   // [1] is re-recorded at the end
  const PoPtrs& p = c.p;
  // (structured: only what the linearisation adds into and the junction block are zeroed, by one small launch: k_po_zero_structured)
  if (c.zero_small) {
    HIP_TRY(hipMemsetAsync(p.g, 0, sizeof(double) * c.nn, 0));             // (once: the padding behind the n gradient entries)
    hipLaunchKernelGGL(k_po_zero_structured, c.g_zero, dim3(256), 0, 0, p, c.S->n_l1);
  } else {
    HIP_TRY(hipMemsetAsync(p.H, 0, c.hbytes, 0));
    HIP_TRY(hipMemsetAsync(p.g, 0, sizeof(double) * c.nn, 0));
  }
  po_launch_linearise(c, 0);
  hipLaunchKernelGGL(k_po_prepare, dim3(1), dim3(256), 0, 0, p, c.pol, 1);
  return SLSLAM_OK;
}

// The dense factorisations (fp64 or fp32 factor): the blocked Cholesky of the whole matrix, then the substitutions.
template <typename T>
void po_factor_solve_dense(PoSolve& c, T* A, T* Lf, T* linv) {
  po_factor_dense<T>(c.p, A, Lf, linv, c.nblk);
  if (c.nblk >= 4 && c.nblk <= c.wide_resident) {
    // one workgroup per 64-row block, all resident: the substitutions spread over the chip (k_po_trisolve_wide)
    hipLaunchKernelGGL(k_po_trisolve_wide<T>, dim3((unsigned)c.nblk), dim3(256), 0, 0, c.p, (const T*)Lf, (const T*)linv, c.d_tri_flags, c.tri_epoch);
    c.tri_epoch += 2u;
  } else {
    hipLaunchKernelGGL(k_po_trisolve<T>, dim3(1), dim3(1024), 0, 0, c.p, (const T*)Lf, (const T*)linv);
  }
}

// ---- one LM iteration, enqueued without host synchronisation; a finished solve early-outs on the device
int po_solve_enqueue_iteration(PoSolve& c) {
  PoPtrs& p = c.p;
  const PoSymbolic& S = *c.S;
  if (c.zero_small) hipLaunchKernelGGL(k_po_zero_structured, c.g_zero, dim3(256), 0, 0, p, S.n_l1);
  else {
    HIP_TRY(hipMemsetAsync(p.H, 0, c.hbytes, 0));
    HIP_TRY(hipMemsetAsync(p.g, 0, sizeof(double) * c.nn, 0));
    HIP_TRY(hipMemsetAsync(p.scal, 0, sizeof(double), 0));            // kPoCost
  }
  po_launch_linearise(c, 0);
  hipLaunchKernelGGL(k_po_prepare, dim3(1), dim3(256), 0, 0, p, c.pol, 0);
  if (c.f32) hipLaunchKernelGGL(k_po_to_f32, dim3(256), dim3(256), 0, 0, p, c.d_Hf);
  c.stamp();
  if (c.structured) {
    // chains eliminated concurrently, then the dense MFMA Cholesky of the junction block only
    size_t off = 0;                                                  // level after level: the pieces, then the chains of their cut poses, ...
    for (int cnt : S.level_counts) {
      if (cnt > 0) hipLaunchKernelGGL(k_po_chain_eliminate, dim3((unsigned)cnt), dim3(64), 0, 0, p, (const PoChain*)(c.d_chains + off));
      off += (size_t)cnt;
    }
    double* Lf_j = c.d_Lf + (size_t)S.n_chain * S.ld + S.n_chain;    // the junction block's factor (same leading dimension)
    po_factor_dense<double>(c.pj, c.pj.H, Lf_j, c.d_linv, S.nblk_j);
    if (S.nj > 0) hipLaunchKernelGGL(k_po_trisolve<double>, dim3(1), dim3(1024), 0, 0, c.pj, (const double*)Lf_j, (const double*)c.d_linv);
    for (size_t lv = S.level_counts.size(); lv-- > 0;) {             // ... and back down
      off -= (size_t)S.level_counts[lv];
      if (S.level_counts[lv] > 0) hipLaunchKernelGGL(k_po_chain_backsub, dim3((unsigned)S.level_counts[lv]), dim3(64), 0, 0, p, (const PoChain*)(c.d_chains + off));
    }
  } else if (c.f32) {
    po_factor_solve_dense<float>(c, c.d_Hf, c.d_Lff, c.d_linvf);
  } else {
    po_factor_solve_dense<double>(c, p.H, c.d_Lf, c.d_linv);
  }
  c.stamp();
  hipLaunchKernelGGL(k_po_candidate, dim3(1), dim3(256), 0, 0, p);
  po_launch_linearise(c, 1);
  hipLaunchKernelGGL(k_po_update, dim3(1), dim3(64), 0, 0, p, c.pol);
  return SLSLAM_OK;
}

// Asks the device whether the solve has finished (state | trace | poses in one copy: when it has, this IS the download).
int po_solve_poll(PoSolve& c) {
  HIP_TRY(hipMemcpyAsync(c.stage, c.arena, c.down_bytes, hipMemcpyDeviceToHost, 0));
  HIP_TRY(hipStreamSynchronize(0));
  std::memcpy(&c.hst, c.landed(c.p.st), sizeof(c.hst));
  c.have_results = c.hst.status != kRunning;
  return SLSLAM_OK;
}

// slslam_po_last_timing's figures, from the events of a finished solve.
void po_solve_read_timing(PoSolve& c) {
  PoTiming& T = g_po_timing;
  T.total_ms = 0; T.factor_ms = 0; T.factor_max_ms = 0; T.factor_calls = 0; T.unknowns = c.S->n; T.junction_unknowns = c.S->nj;
  float ms = 0.f;
  if (c.tev.size() >= 2 && hipEventElapsedTime(&ms, c.tev[0], c.tev[1]) == hipSuccess) T.total_ms = ms;
  for (size_t i = 2; i + 1 < c.tev.size(); i += 2)
    if (hipEventElapsedTime(&ms, c.tev[i], c.tev[i + 1]) == hipSuccess) { T.factor_ms += ms; T.factor_calls++; if (ms > T.factor_max_ms) T.factor_max_ms = ms; }
}

int po_solve_report(PoSolve& c, slslam_summary* summary, slslam_iteration* trace, int trace_cap, int* trace_len) {
  HIP_TRY(hipGetLastError());
  if (c.timing && c.tev.size() >= 2) (void)hipEventRecord(c.tev[1], 0);
  if (!c.have_results || c.timing) HIP_TRY(hipDeviceSynchronize());
  if (c.timing) po_solve_read_timing(c);
  // state | trace | poses come back in ONE copy (they are the first bytes of the block)
  if (!c.have_results) HIP_TRY(hipMemcpy(c.stage, c.arena, c.down_bytes, hipMemcpyDeviceToHost));
  std::memcpy(&c.hst, c.landed(c.p.st), sizeof(c.hst));
  const LMState& st = c.hst;
  const int N = c.g->num_poses;
  const int term = po_termination(c.S->n > 0 ? &st : nullptr);      // (n == 0: no non-constant parameter blocks)
  po_iter_hint = st.n_success + st.n_unsuccess;
  if (term != SLSLAM_NUMERICAL_FAILURE)
    std::memcpy(c.g->parameters, c.landed(c.p.x) + (size_t)st.cur * 6 * N, sizeof(double) * 6 * N);
  if (summary) po_fill_summary(st, term, *c.S, summary);
  po_export_trace(st, c.landed(c.p.trace), trace, trace_cap, trace_len);
  return SLSLAM_OK;
}
}  // namespace

extern "C" int slslam_po_solve(const slslam_po_graph* g, const slslam_solver_options* opt_in,
                               slslam_summary* summary, slslam_iteration* trace, int trace_cap, int* trace_len) {
  PoSolve c;
  int rc = po_solve_validate(g, opt_in, c);
  if (rc != SLSLAM_OK) return rc;
  if (trace_len) *trace_len = 0;
  if (summary) std::memset(summary, 0, sizeof(*summary));
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (g->num_edges == 0) { if (summary) summary->termination_type = po_termination(nullptr); return SLSLAM_OK; }
  po_solve_analyse(c);
  if ((rc = po_solve_upload(c)) != SLSLAM_OK) return rc;
  if ((rc = po_solve_enqueue_initial(c)) != SLSLAM_OK) return rc;
  // An iteration enqueued behind a finished solve early-outs on the device, but its ~14 launches still cost ~45 us: the host asks the device
  // whether it is done after one iteration more than this thread's PREVIOUS solve took steps (the terminating test runs at the head of the next one; consecutive pose graphs of a session are alike;
  // 8 when there is no history), then every 4.  The answer replaces the wait at the end, it is not an extra one.
  int next_check = po_iter_hint >= 0 ? std::min(po_iter_hint + 1, 8) : 8;
  for (int it = 0; it < c.pol.max_num_iterations && c.S->n > 0; ++it) {
    if (it == next_check) {               // stop enqueueing once the device reports termination
      if ((rc = po_solve_poll(c)) != SLSLAM_OK) return rc;
      if (c.have_results) break;
      next_check += 4;
    }
    if ((rc = po_solve_enqueue_iteration(c)) != SLSLAM_OK) return rc;
  }
  return po_solve_report(c, summary, trace, trace_cap, trace_len);
}


// Per-edge report at graph->parameters (what a solve has just updated in place): sq_norm[e] = |W_e Te|^2 (W_e = I without
// graph->sqrt_information), weight[e] = rho'(s) under
// HuberLoss(po_huber_delta) - the switch of reference src/po_problem.cpp:27,55.  One launch, one lane per edge.
extern "C" int slslam_po_edge_report(const slslam_po_graph* g, double po_huber_delta, double* sq_norm, double* weight) {
  if (!g || !po_graph_arrays_ok(g, true) || !po_huber_ok(po_huber_delta) || !po_graph_entries_ok(g, true)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  const int N = g->num_poses, E = g->num_edges;
  if (E == 0 || (!sq_norm && !weight)) return SLSLAM_OK;
  PoCarve a;
  const size_t o_p1 = a.take(sizeof(int) * E), o_p2 = a.take(sizeof(int) * E), o_cons = a.take(sizeof(double) * 6 * E),
               o_x = a.take(sizeof(double) * 6 * N), o_winfo = a.take(g->sqrt_information ? sizeof(double) * 36 * E : 0), up_bytes = a.off,
               o_out = a.take(sizeof(double) * 2 * E);
  struct Block {                          // the calling thread's cached device block, handed back on every path
    char* p = nullptr; size_t bytes = 0; int device = 0;
    ~Block() { DeviceBlockCache::give_back(p, bytes, device); }
  } blk;
  blk.bytes = a.off;
  HIP_TRY(hipGetDevice(&blk.device));
  HIP_TRY(DeviceBlockCache::acquire(blk.bytes, blk.device, &blk.p));
  std::vector<char> img(up_bytes > sizeof(double) * 2 * E ? up_bytes : sizeof(double) * 2 * E);
  std::memcpy(img.data() + o_p1, g->pose_index_1, sizeof(int) * E); std::memcpy(img.data() + o_p2, g->pose_index_2, sizeof(int) * E);
  std::memcpy(img.data() + o_cons, g->constraints, sizeof(double) * 6 * E); std::memcpy(img.data() + o_x, g->parameters, sizeof(double) * 6 * N);
  if (g->sqrt_information) std::memcpy(img.data() + o_winfo, g->sqrt_information, sizeof(double) * 36 * E);
  HIP_TRY(hipMemcpy(blk.p, img.data(), up_bytes, hipMemcpyHostToDevice));
  PoPtrs p;
  std::memset(&p, 0, sizeof(p));
  p.p1 = (const int*)(blk.p + o_p1); p.p2 = (const int*)(blk.p + o_p2); p.cons = (const double*)(blk.p + o_cons);
  p.N = N; p.E = E; p.huber = po_huber_delta;
  p.winfo = g->sqrt_information ? (const double*)(blk.p + o_winfo) : nullptr;
  double* d_out = (double*)(blk.p + o_out);
  const dim3 grid((unsigned)((E + 63) / 64));
  if (p.winfo) hipLaunchKernelGGL(k_po_edge_report<true>, grid, dim3(64), 0, 0, p, (const double*)(blk.p + o_x), d_out, d_out + E);
  else hipLaunchKernelGGL(k_po_edge_report<false>, grid, dim3(64), 0, 0, p, (const double*)(blk.p + o_x), d_out, d_out + E);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(img.data(), d_out, sizeof(double) * 2 * E, hipMemcpyDeviceToHost));
  if (sq_norm) std::memcpy(sq_norm, img.data(), sizeof(double) * E);
  if (weight) std::memcpy(weight, img.data() + sizeof(double) * E, sizeof(double) * E);
  return SLSLAM_OK;
}

// W = L^-1 for cov = L L^T, after scaling to unit diagonal (C = D cov D = Lc Lc^T, L = D^-1 Lc, W = Lc^-1 D): host only.
extern "C" int slslam_po_sqrt_information(const double* cov, double* W, int* status) {
  if (!cov || !W) return SLSLAM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 36; ++i) if (!std::isfinite(cov[i])) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::fill_n(W, 36, 0.0);
  if (status) *status = SLSLAM_COV_SINGULAR;
  double d[6], Lc[36] = {}, Li[36] = {};
  for (int i = 0; i < 6; ++i) {
    if (!(cov[7 * i] > 0.0)) return SLSLAM_OK;
    d[i] = 1.0 / std::sqrt(cov[7 * i]);
  }
  for (int j = 0; j < 6; ++j) {
    double piv = 1.0;                                        // the unit diagonal
    for (int k = 0; k < j; ++k) piv -= Lc[6 * j + k] * Lc[6 * j + k];
    if (!(piv > 1e-10)) return SLSLAM_OK;                    // (a scaled pivot at or below 1e-10: singular, as po_covariance.h rules)
    const double ljj = std::sqrt(piv);
    Lc[7 * j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double v = d[i] * cov[6 * i + j] * d[j];
      for (int k = 0; k < j; ++k) v -= Lc[6 * i + k] * Lc[6 * j + k];
      Lc[6 * i + j] = v / ljj;
    }
  }
  for (int j = 0; j < 6; ++j) {                              // Li = Lc^-1, column by column
    Li[7 * j] = 1.0 / Lc[7 * j];
    for (int i = j + 1; i < 6; ++i) {
      double v = 0.0;
      for (int k = j; k < i; ++k) v -= Lc[6 * i + k] * Li[6 * k + j];
      Li[6 * i + j] = v / Lc[7 * i];
    }
  }
  for (int i = 0; i < 6; ++i) for (int j = 0; j <= i; ++j) W[6 * i + j] = Li[6 * i + j] * d[j];
  if (status) *status = SLSLAM_COV_OK;
  return SLSLAM_OK;
}

namespace { thread_local int g_last_level1 = 0; }
/* (inspection, beside slslam_po_structure: how many of the chains it listed - the first ones - are level-1 chains; the rest are the chains
 * of cut poses of the higher levels, up to eight in all) */
extern "C" int slslam_po_structure_level1(void) { return g_last_level1; }

extern "C" int slslam_po_structure(const slslam_po_graph* g, int* slot_out, int max_chains, int* num_chains, int* chain_start,
                                   int* chain_len, int* chain_left, int* chain_right, int* num_chain_unknowns, int* num_unknowns) {
  if (!g || !slot_out || !num_chains || !po_graph_arrays_ok(g, false) || !po_graph_entries_ok(g, false)) return SLSLAM_ERR_INVALID_ARGUMENT;
  PoSymbolic S;
  po_analyse(g->num_poses, g->num_edges, g->pose_index_1, g->pose_index_2, true, &S);
  g_last_level1 = S.level_counts.empty() ? 0 : S.level_counts[0];
  for (int k = 0; k < g->num_poses; ++k) slot_out[k] = S.slot[k];
  *num_chains = (int)S.chains.size();
  if (num_chain_unknowns) *num_chain_unknowns = S.n_chain;
  if (num_unknowns) *num_unknowns = S.n;
  if ((int)S.chains.size() > max_chains) return SLSLAM_ERR_UNSUPPORTED;
  for (size_t c = 0; c < S.chains.size(); ++c) {
    if (chain_start) chain_start[c] = S.chains[c].start;
    if (chain_len) chain_len[c] = S.chains[c].len;
    if (chain_left) chain_left[c] = S.chains[c].jl;
    if (chain_right) chain_right[c] = S.chains[c].jr;
  }
  return SLSLAM_OK;
}

// posterior covariances of one graph or of a batch's graphs: the kernels, the plan, slslam_po_covariance
#include "po_covariance.h"
// edge statistics under those covariances: slslam_po_edge_statistics, slslam_po_gate and the gate's plan
#include "po_gate.h"
// a constraint's covariance in the edge error's coordinates (the gate's R): slslam_po_constraint_covariance
#include "po_constraint_cov.h"
// many graphs per call: slslam_po_batch_* (the same kernels' bodies, the same symbolic analysis)
#include "po_batch.h"

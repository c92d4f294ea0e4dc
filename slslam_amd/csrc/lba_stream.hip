// slslam_amd/csrc/lba_stream.hip — the stream object of the LBA path (include/slslam_hip.h: slslam_lba_stream_*): host orchestration of
// refillable batches.  No kernel: what it launches, it launches through the batch's entry points and lba_batch.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "../../include/slslam_hip.h"
#include "lba_batch.h"
#include "call_block.h"

// ------------------------------------------------------------------------------------------
// A STREAM of windows (BASELINE config 4 taken literally: every window arrives as the five host arrays the reference builds per
// window, src/slam.cpp:899-921): `depth` refillable batches in flight, each on a HIP stream of its own - while the GPU solves batch k
// and its copy engine uploads batch k + 1, the host threads pack batch k + 2.
struct slslam_lba_stream {
  int device = 0;
  slslam_solver_options opt;
  int depth = 3;
  std::unique_ptr<HostPool> pool;
  struct Slot {
    slslam_lba_batch* batch = nullptr;
    hipStream_t stream = nullptr;
    int n = 0;                                  // windows of the batch in the slot
    long long ticket = -1;
    bool in_flight = false;
    std::vector<double*> out_params;            // the callers' parameter arrays (solved in place, written by collect)
  };
  std::vector<Slot> slots;
  hipStream_t ingest_stream = nullptr, solve_stream = nullptr;      // shared by the slots whose refills are built on the device (see refill_device)
  hipStream_t build_stream = nullptr;        // ... the build kernels of batch k + 1 run BESIDE the solve of batch k: they are latency-bound (one wave walks a window's lines) and
                                             // leave the chip mostly idle - and a chip that idles for 3 ms between two solves starts the next one at lower clocks (measured: the
                                             // first solve after a light-load gap 16.6 ms against 15.0 back to back, tools/first_solve_after_refill.py)
  hipStream_t result_stream = nullptr;       // ... and where their results leave: the export over the link and the state / trace copies of batch k
  hipEvent_t ev_solved = nullptr, ev_built = nullptr;
  long long next_ticket = 0;
  // host-side accounting (ms, wall clock of the calling thread)
  double ms_submit = 0, ms_collect_wait = 0, ms_collect_copy = 0;
  long long n_refills = 0, n_builds = 0, n_windows = 0, n_iterations = 0;
  long long n_device_builds = 0, n_zero_copy = 0, n_fallback_windows = 0;
};

namespace {
// A batch the stream's host threads were lent to
void destroy_lent(slslam_lba_batch* b) {
  b->ext_pool = nullptr;
  slslam_lba_batch_destroy(b);
}

// A new batch for a slot: the set packed by the stream's host threads, finalized with the stream's options
int make_slot_batch(slslam_lba_stream* st, const slslam_lba_window* ws, int n, slslam_lba_batch** out) {
  slslam_lba_batch* b = nullptr;
  int rc = slslam_lba_batch_create(st->device, &b);
  if (rc != SLSLAM_OK) return rc;
  b->ext_pool = st->pool.get();
  b->wins.resize((size_t)n);
  std::vector<int> ps((size_t)n, SLSLAM_OK);
  if (!st->pool->run(n, [&](int i) { ps[(size_t)i] = pack_window(&ws[i], &b->wins[(size_t)i]); })) rc = SLSLAM_ERR_NO_MEMORY;
  for (int r : ps) if (r != SLSLAM_OK) rc = r;
  if (rc == SLSLAM_OK) rc = slslam_lba_batch_finalize(b, &st->opt);
  if (rc != SLSLAM_OK) { destroy_lent(b); return rc; }
  *out = b;
  return SLSLAM_OK;
}

// The slot's batch destroyed, once every stream that may still use it has drained
int drop_slot_batch(slslam_lba_stream* st, slslam_lba_stream::Slot& sl) {
  if (sl.stream) HIP_TRY(hipStreamSynchronize(sl.stream));
  HIP_TRY(hipStreamSynchronize(st->solve_stream)); HIP_TRY(hipStreamSynchronize(st->build_stream)); HIP_TRY(hipStreamSynchronize(st->result_stream));
  destroy_lent(sl.batch);
  sl.batch = nullptr;
  return SLSLAM_OK;
}
}  // namespace

extern "C" int slslam_lba_stream_create(int device, const slslam_solver_options* opt, int depth, slslam_lba_stream** out) {
  if (!out) return SLSLAM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const int ndev = device_count();
  if (ndev <= 0) return SLSLAM_ERR_NO_DEVICE;
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return SLSLAM_ERR_NO_DEVICE; }
  if (device >= ndev || depth < 1 || depth > 8) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_lba_stream* st = new (std::nothrow) slslam_lba_stream();
  if (!st) return SLSLAM_ERR_HIP;
  st->device = device; st->depth = depth;
  if (opt) st->opt = *opt; else slslam_default_options(&st->opt);
  if (st->opt.refill_headroom_percent <= 0) st->opt.refill_headroom_percent = 10;
  st->opt.use_graph = 1;
  int threads = st->opt.host_threads;
  if (threads <= 0) threads = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
  st->opt.host_threads = threads;
  st->pool.reset(new HostPool(threads));
  st->slots.resize((size_t)depth);
  if (hipSetDevice(device) != hipSuccess) { delete st; return SLSLAM_ERR_NO_DEVICE; }
  // TWO streams serve every slot whose batches are built on the device: ingest (the host link) and build + solve + results.  A process has
  // few hardware queues (4 unless GPU_MAX_HW_QUEUES says otherwise) and streams that share one run one behind the other: the slots' own
  // streams - what the host-packer path overlaps its uploads with - are made when that path is first taken, not before.
  // The ingest stream gets the highest priority: its few workgroups must find wave slots while a solve's thousands are queued.
  int pr_lo = 0, pr_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
  if (hipStreamCreateWithPriority(&st->ingest_stream, hipStreamNonBlocking, pr_hi) != hipSuccess || hipStreamCreateWithFlags(&st->solve_stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithPriority(&st->build_stream, hipStreamNonBlocking, 0) != hipSuccess ||
      hipStreamCreateWithFlags(&st->result_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&st->ev_solved, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&st->ev_built, hipEventDisableTiming) != hipSuccess) {
    slslam_lba_stream_destroy(st);
    return SLSLAM_ERR_HIP;
  }
  *out = st;
  return SLSLAM_OK;
}

extern "C" void slslam_lba_stream_destroy(slslam_lba_stream* st) {
  if (!st) return;
  (void)hipSetDevice(st->device);
  const hipStream_t shared[] = { st->ingest_stream, st->solve_stream, st->build_stream, st->result_stream };
  for (hipStream_t q : shared) if (q) (void)hipStreamSynchronize(q);
  for (auto& sl : st->slots) {
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    if (sl.batch) destroy_lent(sl.batch);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
  for (hipStream_t q : shared) if (q) (void)hipStreamDestroy(q);
  if (st->ev_solved) (void)hipEventDestroy(st->ev_solved);
  if (st->ev_built) (void)hipEventDestroy(st->ev_built);
  delete st;
}

namespace {
int stream_submit_impl(slslam_lba_stream* st, const slslam_lba_window* windows, const unsigned int* const* packed, int n, int* ticket);
}
extern "C" int slslam_lba_stream_submit(slslam_lba_stream* st, const slslam_lba_window* windows, int n, int* ticket) {
  return stream_submit_impl(st, windows, nullptr, n, ticket);
}
extern "C" int slslam_lba_stream_submit_packed(slslam_lba_stream* st, const slslam_lba_window* windows, const unsigned int* const* packed_index, int n, int* ticket) {
  return stream_submit_impl(st, windows, packed_index, n, ticket);
}
namespace {
int stream_submit_impl(slslam_lba_stream* st, const slslam_lba_window* windows, const unsigned int* const* packed, int n, int* ticket) {
  if (!st || !windows || n <= 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  const auto t0 = std::chrono::steady_clock::now();
  // windows whose indices came narrowed and that end up on the host packer (the slot's first batch, a refill the device build does not take)
  // get their three index arrays back first
  std::vector<slslam_lba_window> expanded;
  std::vector<std::vector<int>> exp_idx;
  auto expand = [&]() -> const slslam_lba_window* {
    if (!packed) return windows;
    if (!expanded.empty()) return expanded.data();
    expanded.assign(windows, windows + n);
    exp_idx.resize((size_t)n);
    for (int i = 0; i < n; ++i)
      if (packed[i]) expand_indices(packed[i], (size_t)std::max(0, windows[i].num_observations), exp_idx[(size_t)i], &expanded[(size_t)i]);
    return expanded.data();
  };
  auto& sl = st->slots[(size_t)(st->next_ticket % st->depth)];
  if (sl.in_flight) return SLSLAM_ERR_STATE;             // its results have not been collected
  HIP_TRY(hipSetDevice(st->device));
  int rc = SLSLAM_ERR_UNSUPPORTED;
  hipStream_t run = st->solve_stream;                     // where this ticket's solve and download go
  if (sl.batch && sl.n == n) {
    slslam_lba_batch* b = sl.batch;
    // the build stage on the device: ingest on the stream's ONE ingest stream, build + solve + results on its ONE solve stream
    if (refillable_as_is(b, n) && fits_batch_path(b, windows, packed, n)) {
      rc = refill_device(b, windows, n, st->build_stream, st->ingest_stream, packed);
      if (rc == SLSLAM_OK) {
        run = st->solve_stream;
        HIP_TRY(hipEventRecord(st->ev_built, st->build_stream));
        HIP_TRY(hipStreamWaitEvent(run, st->ev_built, 0));
      }
    }
    if (rc == SLSLAM_ERR_UNSUPPORTED) {
      // the host packer (or refused: a new batch below): its uploads overlap the other slots' solves on a stream of the slot's own
      if (!sl.stream) HIP_TRY(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
      rc = slslam_lba_batch_refill(b, expand(), n, (void*)sl.stream);
      if (rc == SLSLAM_OK) run = sl.stream;
    }
  }
  if (rc == SLSLAM_OK) { ++st->n_refills; if (sl.batch->device_built) { ++st->n_device_builds; if (sl.batch->ingest_pinned) ++st->n_zero_copy; } }
  else if (rc == SLSLAM_ERR_UNSUPPORTED) {
    // the first batch of the slot, another number of windows, or windows that do not fit the room the slot's arrays have: a new batch
    if (sl.batch && (rc = drop_slot_batch(st, sl)) != SLSLAM_OK) return rc;
    slslam_lba_batch* b = nullptr;
    if ((rc = make_slot_batch(st, expand(), n, &b)) != SLSLAM_OK) return rc;
    sl.batch = b; sl.n = n;
    ++st->n_builds;
  } else return rc;
  if ((rc = slslam_lba_batch_solve(sl.batch, (void*)run)) != SLSLAM_OK) return rc;
  if (run == st->solve_stream) {
    // the results leave on a stream of their own, behind the solve: the next batch's build does not wait for this batch's export
    HIP_TRY(hipEventRecord(st->ev_solved, run));
    HIP_TRY(hipStreamWaitEvent(st->result_stream, st->ev_solved, 0));
    run = st->result_stream;
  }
  if ((rc = download_async_impl(sl.batch, (void*)run, /*allow_inplace=*/true)) != SLSLAM_OK) return rc;
  sl.out_params.resize((size_t)n);
  for (int i = 0; i < n; ++i) sl.out_params[(size_t)i] = windows[i].parameters;
  sl.ticket = st->next_ticket; sl.in_flight = true;
  if (ticket) *ticket = (int)st->next_ticket;
  ++st->next_ticket; st->n_windows += n;
  st->ms_submit += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SLSLAM_OK;
}
}  // namespace

extern "C" int slslam_lba_stream_collect(slslam_lba_stream* st, int ticket, slslam_summary* summaries) {
  if (!st || ticket < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  auto& sl = st->slots[(size_t)(ticket % st->depth)];
  if (!sl.in_flight || sl.ticket != ticket) return SLSLAM_ERR_STATE;
  HIP_TRY(hipSetDevice(st->device));
  const auto t0 = std::chrono::steady_clock::now();
  int rc = slslam_lba_batch_wait(sl.batch);
  if (rc != SLSLAM_OK) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  std::vector<int> rs((size_t)sl.n, SLSLAM_OK);
  // (the step counts through get_summary, which routes a window of a MIXED batch - oversize windows among ordinary ones - to the part
  // that solved it: the top-level batch of such a slot holds no LM states of its own)
  std::vector<int> steps((size_t)sl.n, 0);
  slslam_lba_batch* bt = sl.batch;
  bool dev = bt->device_built && !bt->part[0];
  std::vector<int> flagged;
  if (dev) for (int i = 0; i < sl.n; ++i) if (bt->build_status[(size_t)i] != SLSLAM_OK) flagged.push_back(i);
  // A window as submit() handed it over, from what the device read (bt->host_src: the staging copy of pageable arrays, or the caller's
  // page-locked ones), its initial parameters put back into the caller's `parameters` first: results depend only on what the caller's arrays
  // held at submit time - a pageable array may have been reused or freed since, and `parameters` is written here, never read.
  std::vector<std::vector<int>> idx((size_t)sl.n);
  auto as_submitted = [&](int i) -> slslam_lba_window {
    const RawWin& r = bt->host_src[(size_t)i];
    slslam_lba_window w{};
    w.num_cameras = r.C; w.num_lines = r.L; w.num_observations = r.M; w.observations = r.obs; w.parameters = sl.out_params[(size_t)i];
    const size_t np = (size_t)6 * r.C + (size_t)4 * r.L;
    if (np && r.params_in != w.parameters) std::memcpy(w.parameters, r.params_in, np * sizeof(double));
    if (r.packed) expand_indices(r.packed, (size_t)r.M, idx[(size_t)i], &w);
    else { w.camera_index = r.cam; w.line_index = r.line; w.fixed_index = r.fixed; }
    return w;
  };
  // A refill that did not fit the room the slot's arrays have (only the device knows the tiles a set needs: k_build_layout flags the refill as
  // a whole) is what submit answers with a new batch when the HOST can see it: the same here, late - the set is packed by the host threads into
  // a batch of its own size (plus the stream's headroom), solved as ONE batch, and that batch takes the slot, so that the sets that follow fit.
  // (Solving 1024 flagged windows one by one would take a second, and the next set of that shape would be flagged again.)  The layout's fit flag
  // decides, whatever else the windows were flagged for: the host packer takes a window for the host path (a camera that sees a line twice)
  // in its stride - only a window with bad input, which the packer refuses, keeps the set on the per-window path below.
  bool whole_nofit = dev && sl.n > 0 && !bt->h_buildwin.empty() && !bt->h_totals.empty() && bt->h_totals[3] == 0 && (int)bt->host_src.size() == sl.n;
  for (int i = 0; whole_nofit && i < sl.n; ++i) if (bt->h_buildwin[i].status & kBuildInvalid) whole_nofit = false;
  if (whole_nofit) {
    const int n = sl.n;
    std::vector<slslam_lba_window> ws((size_t)n);
    for (int i = 0; i < n; ++i) ws[(size_t)i] = as_submitted(i);
    slslam_lba_batch* nb = nullptr;
    if ((rc = make_slot_batch(st, ws.data(), n, &nb)) != SLSLAM_OK) return rc;
    rc = slslam_lba_batch_solve(nb, (void*)st->solve_stream);
    if (rc == SLSLAM_OK) rc = download_async_impl(nb, (void*)st->solve_stream, /*allow_inplace=*/false);
    if (rc == SLSLAM_OK) rc = slslam_lba_batch_wait(nb);
    if (rc != SLSLAM_OK) { destroy_lent(nb); return rc; }
    if ((rc = drop_slot_batch(st, sl)) != SLSLAM_OK) return rc;
    sl.batch = bt = nb;
    ++st->n_builds; st->n_fallback_windows += n;
    dev = false; flagged.clear();
  }
  auto one = [&](int i) {
    if (dev && bt->build_status[(size_t)i] != SLSLAM_OK) return;                 // below
    int r = SLSLAM_OK;
    if (!(dev && bt->results_inplace)) r = slslam_lba_batch_get_parameters(bt, i, sl.out_params[(size_t)i]);     // (in place: the device wrote them there)
    slslam_summary sm;
    if (r == SLSLAM_OK) r = slslam_lba_batch_get_summary(bt, i, &sm);
    if (r == SLSLAM_OK) { steps[(size_t)i] = sm.num_successful_steps + sm.num_unsuccessful_steps; if (summaries) summaries[i] = sm; }
    rs[(size_t)i] = r;
  };
  if (dev && bt->results_inplace) { for (int i = 0; i < sl.n; ++i) one(i); }      // (summaries only: not worth waking the pool)
  else st->pool->run(sl.n, one);
  // windows the device build flagged (a camera that sees a line twice, a line with more than 64 observations, more than 20 free cameras,
  // no room in the slot's arrays, bad input): solved here through the host path, one by one, from what the device read - their status is
  // whatever that path says
  for (int i : flagged) {
    slslam_lba_window w = as_submitted(i);
    slslam_solver_options o = st->opt;
    o.refill_headroom_percent = 0; o.host_threads = 1; o.device_build = -1;
    slslam_summary sm;
    const int fr = slslam_lba_solve(&w, &o, &sm, nullptr, 0, nullptr);
    if (fr == SLSLAM_OK) { steps[(size_t)i] = sm.num_successful_steps + sm.num_unsuccessful_steps; if (summaries) summaries[i] = sm; }
    rs[(size_t)i] = fr;
    ++st->n_fallback_windows;
  }
  for (int r : rs) if (r != SLSLAM_OK) rc = r;
  for (int i = 0; i < sl.n; ++i) st->n_iterations += steps[(size_t)i];   // reference src/slam.cpp:949-950
  sl.in_flight = false;
  const auto t2 = std::chrono::steady_clock::now();
  st->ms_collect_wait += std::chrono::duration<double, std::milli>(t1 - t0).count();
  st->ms_collect_copy += std::chrono::duration<double, std::milli>(t2 - t1).count();
  return rc;
}

extern "C" int slslam_lba_stream_build_stats(const slslam_lba_stream* st, long long* device_builds, long long* zero_copy, long long* fallback_windows) {
  if (!st) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (device_builds) *device_builds = st->n_device_builds;
  if (zero_copy) *zero_copy = st->n_zero_copy;
  if (fallback_windows) *fallback_windows = st->n_fallback_windows;
  return SLSLAM_OK;
}

extern "C" int slslam_lba_stream_batch(slslam_lba_stream* st, int ticket, slslam_lba_batch** batch) {
  if (!st || !batch || ticket < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  auto& sl = st->slots[(size_t)(ticket % st->depth)];
  if (sl.ticket != ticket || !sl.batch) return SLSLAM_ERR_STATE;
  *batch = sl.batch;
  return SLSLAM_OK;
}

extern "C" int slslam_lba_stream_stats(const slslam_lba_stream* st, double* ms_submit, double* ms_collect_wait, double* ms_collect_copy,
                                       long long* refills, long long* builds, long long* windows, long long* lm_iterations, int* host_threads) {
  if (!st) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (ms_submit) *ms_submit = st->ms_submit;
  if (ms_collect_wait) *ms_collect_wait = st->ms_collect_wait;
  if (ms_collect_copy) *ms_collect_copy = st->ms_collect_copy;
  if (refills) *refills = st->n_refills;
  if (builds) *builds = st->n_builds;
  if (windows) *windows = st->n_windows;
  if (lm_iterations) *lm_iterations = st->n_iterations;
  if (host_threads) *host_threads = st->pool ? st->pool->threads() : 1;
  return SLSLAM_OK;
}

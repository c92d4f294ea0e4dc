// slslam_amd/csrc/lba_batch.h — the LBA batch as its host code sees it: the owners of device and host memory, struct slslam_lba_batch,
// and the functions of lba_api.hip that the stream object (lba_stream.hip) and the host utilities (lba_host_util.hip) call.
// Host only: no kernel and no kernel header - the batch's device code lives in lba_api.hip alone.  Internal: not part of the C ABI.
#ifndef SLSLAM_LBA_BATCH_H_
#define SLSLAM_LBA_BATCH_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/slslam_hip.h"
#include "lba_types.h"
#include "lba_pack.h"
#include "device_cache.h"
#include "hip_status.h"
#include "host_pool.h"

namespace slslam {

// The owners below free what they hold when they go; they are not copied (a copy would free it twice) and not moved (a DeviceArena
// keeps the addresses of the DevBufs it fills in).
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

template <typename T>
struct DevBuf : NoCopy {
  T* p = nullptr;
  size_t n = 0;
  bool in_arena = false;            // carved out of a DeviceArena: the arena frees it
  ~DevBuf() { release(); }
  int alloc(size_t count) {
    release();
    if (count > 0) HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
    return SLSLAM_OK;
  }
  void release() { if (p && !in_arena) (void)hipFree(p); p = nullptr; n = 0; in_arena = false; }
};

// Results on the host: pageable, or pinned for a batch that is refilled (its downloads are asynchronous copies).
template <typename T>
struct HostArr : NoCopy {
  T* p = nullptr;
  size_t n = 0;
  bool pinned = false;
  std::vector<T> v;
  ~HostArr() { release(); }
  int alloc(size_t count, bool pin, bool zero = true) {        // (zero = false: a staging block, written before it is read)
    release();
    if (pin && count > 0) { HIP_TRY(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault)); pinned = true; if (zero) std::memset((void*)p, 0, count * sizeof(T)); }
    else { v.assign(count, T()); p = v.data(); }
    n = count;
    return SLSLAM_OK;
  }
  void release() { if (pinned && p) (void)hipHostFree(p); p = nullptr; n = 0; pinned = false; std::vector<T>().swap(v); }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
};

// A derived result of a resident batch (its posterior covariances, its report, its segments): device arrays that kernels of its own
// fill at the batch's current parameters, and their copies on the host.  ONE protocol: the first call makes the buffers and they are
// kept; a call leaves its result ENQUEUED on the device, the next download copies it with the other results (COPYING), its arrival
// makes it READY for the getter; a refill replaces the windows and with them the result (NONE).
struct DerivedResult : NoCopy {
  enum State { NONE, ENQUEUED, COPYING, READY };
  struct Mirror {                    // bytes on the device and, where the host reads them, as many on the host
    DevBuf<char> d; HostArr<char> h;
    bool active = true;              // part of the last call's result: a download copies it
    template <typename T> T* dev() const { return reinterpret_cast<T*>(d.p); }
    template <typename T> const T* host() const { return reinterpret_cast<const T*>(h.p); }
  };
  struct Shape { size_t bytes; bool zeroed, mirrored; };
  Mirror m[4];
  State state = NONE;                // where the result of the LAST call is
  long long calls = 0, allocations = 0;
  bool allocated(int first = 0) const { return m[first].d.p != nullptr; }
  // Makes m[first ...] (the host side pinned when the downloads are asynchronous copies) and zeroes on `s` what is to read as zeros where
  // no launch writes.  A failure leaves them unallocated: the next call tries again.
  int allocate(int first, std::initializer_list<Shape> shapes, bool pin, hipStream_t s) {
    int rc = SLSLAM_OK, k = first;
    long long made = 0;
    for (const Shape& sh : shapes) {
      Mirror& x = m[k++];
      if ((rc = x.d.alloc(sh.bytes)) || (sh.mirrored && (rc = x.h.alloc(sh.bytes, pin)))) break;
      made += sh.mirrored ? 2 : 1;
    }
    if (rc != SLSLAM_OK) {
      for (int q = first; q < k; ++q) { m[q].d.release(); m[q].h.release(); }
      return rc;
    }
    allocations += made;
    k = first;
    for (const Shape& sh : shapes) {
      if (sh.zeroed) HIP_TRY(hipMemsetAsync(m[k].d.p, 0, sh.bytes, s));
      ++k;
    }
    return SLSLAM_OK;
  }
  int launched() { HIP_TRY(hipGetLastError()); state = ENQUEUED; return SLSLAM_OK; }      // behind a call's launches
  // what was enqueued since the last download comes back with it
  int download(hipStream_t s) {
    if (state != ENQUEUED) return SLSLAM_OK;
    for (Mirror& x : m)
      if (x.active && x.h.size() > 0) HIP_TRY(hipMemcpyAsync(x.h.data(), x.d.p, x.h.size(), hipMemcpyDeviceToHost, s));
    state = COPYING;
    return SLSLAM_OK;
  }
  void arrive() { if (state == COPYING) state = READY; }
  void invalidate() { state = NONE; }
};

// All device arrays of a batch in ONE allocation, everything the host fills in ONE host-to-device copy: the build of
// a single window (slslam_lba_solve, the per-keyframe call of the reference) is dominated by per-call driver overheads
// otherwise (~35 hipMalloc + ~20 synchronous hipMemcpy).
// The uploaded arrays have a host IMAGE with the same offsets (`stage`): the batch build writes every window's slices straight into
// it (fill_window, one window per host thread) and the image goes up in one copy.  A batch that is to be refilled
// (slslam_solver_options.refill_headroom_percent > 0) keeps the image, in pinned memory: slslam_lba_batch_refill packs the next set of
// windows into it and uploads the arrays with asynchronous copies on the caller's stream.
struct DeviceArena : NoCopy {
  struct Item { void** pp; size_t bytes; const void* host; size_t host_bytes; int group; size_t off; };   // group 0 uploaded, 1 scratch, 2 zeroed
  std::vector<Item> items;
  char* base = nullptr;
  size_t bytes = 0;
  int device = 0;
  bool cached = false;              // one-shot solves: the block comes from / returns to the thread's DeviceBlockCache
  char* stage = nullptr;            // host image of the uploaded arrays (offsets as on the device)
  bool stage_pinned = false;        // hipHostMalloc'ed and kept for refills; otherwise a vector that lives until push()
  bool keep_stage = false;
  std::vector<char> stage_vec;
  ~DeviceArena() { release(); }
  template <typename T>
  void add(DevBuf<T>& d, size_t count, const T* host, size_t host_count, int group) {
    d.n = count; d.in_arena = true; d.p = nullptr;
    items.push_back(Item{ (void**)&d.p, count * sizeof(T), host, host_count * sizeof(T), group, 0 });
  }
  template <typename T> void upload(DevBuf<T>& d, const std::vector<T>& h) { add(d, h.size(), h.data(), h.size(), 0); }
  // uploaded, `count` elements of room; the caller writes host_of(d) between layout() and push()
  template <typename T> void staged(DevBuf<T>& d, size_t count) { add(d, count, (const T*)nullptr, 0, 0); }
  template <typename T> void scratch(DevBuf<T>& d, size_t count) { add(d, count, (const T*)nullptr, 0, 1); }
  template <typename T> void zeroed(DevBuf<T>& d, size_t count) { add(d, count, (const T*)nullptr, 0, 2); }
  template <typename T> T* host_of(const DevBuf<T>& d) const { return reinterpret_cast<T*>(stage + ((char*)d.p - base)); }
  size_t upload_end = 0, zero_begin = 0;
  int layout() {
    size_t off = 0;
    upload_end = 0; zero_begin = 0;
    for (int group = 0; group < 3; ++group) {        // uploaded arrays first, then scratch, then the zero-initialised ones
      if (group == 2) zero_begin = off;
      for (Item& it : items) {
        if (it.group != group) continue;
        it.off = off;
        off += (it.bytes + 255) & ~(size_t)255;
      }
      if (group == 0) upload_end = off;
    }
    bytes = off;
    if (off == 0) { items.clear(); return SLSLAM_OK; }
    if (cached) HIP_TRY(DeviceBlockCache::acquire(off, device, &base));
    else HIP_TRY(hipMalloc((void**)&base, off));
    if (keep_stage) {
      HIP_TRY(hipHostMalloc((void**)&stage, std::max<size_t>(upload_end, 256), hipHostMallocDefault));
      stage_pinned = true;
      std::memset(stage, 0, upload_end);
    } else {
      stage_vec.assign(upload_end, 0);
      stage = stage_vec.data();
    }
    for (const Item& it : items) {
      *it.pp = base + it.off;
      if (it.host && it.host_bytes) std::memcpy(stage + it.off, it.host, it.host_bytes);
    }
    items.clear();
    return SLSLAM_OK;
  }
  int push() {
    if (bytes == 0) return SLSLAM_OK;
    if (upload_end) HIP_TRY(hipMemcpy(base, stage, upload_end, hipMemcpyHostToDevice));
    if (bytes > zero_begin) HIP_TRY(hipMemset(base + zero_begin, 0, bytes - zero_begin));
    if (!stage_pinned) { std::vector<char>().swap(stage_vec); stage = nullptr; }
    return SLSLAM_OK;
  }
  int commit() { const int rc = layout(); return rc != SLSLAM_OK ? rc : push(); }
  void release() {
    if (base) { if (cached) DeviceBlockCache::give_back(base, bytes, device); else (void)hipFree(base); }
    if (stage_pinned && stage) (void)hipHostFree(stage);
    stage = nullptr; stage_pinned = false; std::vector<char>().swap(stage_vec);
    base = nullptr; items.clear();
  }
};

enum { FAM_LIN = 0, FAM_SOLVE = 1, FAM_BACKSUB = 2, FAM_TRIG = 3, FAM_COST = 4, FAM_UPDATE = 5, FAM_INIT = 6, FAM_N = 8 };

// The mirrors (DerivedResult::m) of a batch's derived results
enum { COV_M_HDR, COV_M_CAMS, COV_M_LINES };                  // posterior covariances (lba_covariance.h): int [B][kCovHdr], double [B][stride], and -
                                                              // made by the first call that asks for them, active when the last one did - the lines' blocks, double [lines][16]
enum { REP_M_OBS, REP_M_LINES, REP_M_CAMS, REP_M_CAM_PART };  // the report (lba_report.h): double [2 obs], RepLine [lines], RepCam [cams]; double, device only
enum { SEG_M_STATUS, SEG_M_RANGE, SEG_M_LINES };              // the 3-D segments (lba_segments.h): int [obs], double [2 obs], SegLine [lines]

}  // namespace slslam

using namespace slslam;      // (the batch names its members' types as lba_api.hip does)

struct slslam_lba_batch {
  int device = 0;
  bool finalized = false;
  std::vector<PackedWindow> wins;
  slslam_solver_options opt;
  Policy pol;
  // host mirrors
  std::vector<WinDesc> h_wins;
  std::vector<long long> h_param_off;     // per window offset into the exported parameter vector
  long long total_params = 0;
  std::vector<LMState> h_state0;
  HostArr<LMState> h_state;
  HostArr<IterRec> h_trace;
  HostArr<double> h_params;
  // refills (slslam_lba_batch_refill): the device arrays have room for `refill_headroom_percent` more than the first windows needed; the
  // kernels' view of the batch (BatchPtrs: pointers, strides, counts) and with it the captured graph never change
  bool refillable = false;
  long long used_ncam = 0, used_nline = 0, used_nobs = 0, used_tiles = 0, used_items = 0;   // of the room the device arrays have
  int cap_maxC = 0, cap_maxn = 0;            // the LDS sizes of the launches were made for these
  int auto_rounds = 0, auto_cpw = 0;         // the automatic chunk policy as finalize resolved it: a refill cuts its windows the same way
  std::vector<int> sys_map_off_of_cf;        // per free-camera count: its table in d_sys_map, or -1
  hipEvent_t ev_stage_free = nullptr;        // recorded behind the uploads of a refill: the host image may be written again
  hipEvent_t ev_results = nullptr;           // recorded behind the copies of an asynchronous download
  bool results_pending = false;
  HostPool* ext_pool = nullptr;              // host threads lent by a stream object; else own_pool, made on demand
  std::unique_ptr<HostPool> own_pool;
  std::vector<PackedWindow> wins_spare;      // what a refill packs into; swapped with `wins` when the refill is accepted
  std::vector<int> h_ob_orig_off;          // per window offset into d_ob_orig
  bool downloaded = false;
  // device
  DeviceArena arena;
  DevBuf<uint16_t> d_sys_map;
  DevBuf<WinDesc> d_wins; DevBuf<Tile> d_tiles; DevBuf<Chunk> d_chunks; DevBuf<uint8_t> d_items; DevBuf<uint16_t> d_lane_map; DevBuf<int32_t> d_lane_ctx;
  DevBuf<uint32_t> d_line_desc;
  DevBuf<unsigned long long> d_dbg_cycles;
  int elim_mode = 0, elim_waves = 1;     // see BatchPtrs
  bool elim_mixed = false;               // ... its steady sweeps in mixed precision (lba_precision = 1: k_eliminate_grouped<false, false, true>)
  bool elim_grouped = false;             // elim_mode 1 with group-local accumulators (lba_eliminate_grouped.h); the windows are packed with grouping = 1
  size_t lds_elim = 0;
  DevBuf<unsigned long long> d_iter_counter;
  DevBuf<unsigned int> d_active;
  DevBuf<double> d_cam_x, d_cam_x0, d_cam_scale, d_cam_tab; DevBuf<int> d_cam_cf, d_cam_win;
  DevBuf<double> d_line_x, d_line_x0, d_line_scale; DevBuf<int> d_line_ptr, d_line_flags, d_line_win, d_line_orig;
  DevBuf<double> d_ob; DevBuf<int> d_ob_cam, d_ob_orig;
  DevBuf<double> d_ob_raw;                   // refillable batches: a refill's observations as the caller holds them, permuted into d_ob on the device (k_permute_obs)
  // the build stage on the device (lba_device_build.h): a refill whose windows go up as the caller holds them
  DevBuf<RawWin> d_rawwin; DevBuf<BuildWin> d_buildwin; DevBuf<uint32_t> d_raw_idx, d_fmask; DevBuf<double> d_line_raw; DevBuf<uint8_t> d_lflags;
  DevBuf<int> d_item_base, d_totals, d_line_pos;
  DevBuf<uint32_t> d_mid_keys; DevBuf<BuildLine> d_mid_li; DevBuf<uint4> d_mid_rows; DevBuf<uint16_t> d_mid_next, d_mid_trows, d_mid_tptr; DevBuf<BuildMid> d_mid;
  HostArr<RawWin> h_rawwin;                  // pinned [B]: what the device reads of every window (uploaded per refill)
  HostArr<BuildWin> h_buildwin;              // pinned [B]: what came of every window (downloaded with the results)
  HostArr<WinDesc> h_wins_dl;                // pinned [B]: the descriptors the device made
  HostArr<int> h_totals;                     // pinned [8]
  HostArr<char> h_raw_stage;                 // pinned, made on demand: pageable inputs are copied here (indices narrowed on the way)
  DevBuf<char> d_stage_in;                   // device, made on demand: where the copy engine puts a refill's arrays (k_ingest reads them from here)
  std::vector<RawWin> host_src;              // per window: host-readable pointers to what the device was given (the callers' page-locked arrays, or the staging copy)
  bool ingest_pinned = false;                // ... its observations and parameters were read where the caller holds them (page-locked), no staging copy
  bool device_built = false;                 // the batch's present windows were built on the device
  bool inplace_export = false;               // ... and their `parameters` arrays are pinned: results can be written straight into them
  bool results_inplace = false;              // the last download wrote them there
  std::vector<slslam_lba_window> src_windows;   // the callers' descriptors of a device-built refill (the in-place export's parameter arrays)
  std::vector<int> build_status;             // per window, after wait(): 0 or the SLSLAM_ERR_* a flagged window is reported with
  long long n_device_builds = 0, n_zero_copy = 0;
  // windows beyond the tiled sweeps (lba_big.h)
  bool big_mode = false;
  BigPtrs big;
  std::vector<long long> h_big_sys_off, h_big_linv_off;
  DevBuf<int> d_big_ob_line, d_big_cam_ptr, d_big_cam_obs, d_big_pair_ptr, d_big_pair_row, d_big_pair_col, d_big_pair_desc, d_big_flags;
  DevBuf<double> d_big_J, d_big_F, d_big_cost, d_big_camtab, d_big_line_acc, d_big_sys, d_big_scal, d_big_linv;
  DevBuf<long long> d_big_sys_off;
  DevBuf<double> d_slab_sum;
  long long slab_sum_stride = 0;           // > 0: k_slab_reduce runs ahead of the reduced solve
  bool slab_sum_image = false;             // ... and writes the LDS image of the reduced solve (BatchPtrs.slab_sum_image)
  int line_elim_stride = kLineElim;
  DevBuf<double> d_slab, d_bs_part, d_cost_part, d_ysys, d_params_out, d_fstore, d_line_elim, d_line_h;
  DevBuf<LMState> d_state; DevBuf<IterRec> d_trace; DevBuf<long long> d_param_off;
  BatchPtrs ptrs;
  int nchunk = 0, nline = 0, ncam = 0;
  long long nobs = 0;
  int num_cus = 256;
  bool fused_motion_only = false;
  bool share_cam_tab = false;            // the sweeps read the camera tables of a window from d_cam_tab (BatchPtrs.cam_tab)
  size_t lds_motion_only = 0;
  size_t lds_lin = 0, lds_solve = 0, lds_bs = 0, lds_bs_stream = 0, lds_cost = 0;
  // graph
  hipGraphExec_t graph_exec = nullptr;
  hipStream_t capture_stream = nullptr;
  // A batch that mixes oversize windows with ordinary ones is solved as TWO batches side by side: part[0] holds the ordinary
  // windows (tiled sweeps), part[1] the oversize ones (lba_big.h), the second on a stream of its own between a fork and a join on
  // the caller's.  This object then only routes: window i of the caller is window route[i].second of part[route[i].first].
  slslam_lba_batch* part[2] = { nullptr, nullptr };
  std::vector<std::pair<int, int>> route;
  std::vector<int> h_win_graded;             // per window: 0, or the number of slot rounds its graded chunk sizes were made for (finalize)
  std::vector<long long> part_param_off[2];  // per window of a part: where its parameters go in the caller's export layout
  DevBuf<long long> d_part_off[2];           // [3 nwin] per window of a part: offset in the part's export | offset in the caller's | length (k_scatter_windows)
  hipStream_t part_stream = nullptr;
  hipEvent_t part_fork = nullptr, part_join = nullptr;
  DevBuf<double> d_part_out[2];
  int num_windows() const { return part[0] ? (int)route.size() : (int)wins.size(); }
  size_t dbg_words() const { return std::max((size_t)32 * std::max(1, nchunk), (size_t)16 * std::max<size_t>(1, wins.size())); }   // d_dbg_cycles (timing builds)
  // the derived results (DerivedResult) and their mirrors.  A new one: a member, a place in `derived`, its enqueue function and its getter
  DerivedResult cov, rep, seg;
  DerivedResult* const derived[3] = { &cov, &rep, &seg };      // what downloads and refills go through
  long long cov_cam_stride = 0;                               // cov.m[COV_M_CAMS] = double [B][cov_cam_stride]
  size_t rep_cap_obs = 0;                                     // rep.m[REP_M_OBS] = double sq_norm [rep_cap_obs] | weight [rep_cap_obs]
  // profiling
  bool profiling = false;
  double fam_ms[FAM_N] = { 0 };
  int fam_launches[FAM_N] = { 0 };
  std::vector<hipEvent_t> ev_pool;            // created once, reused by every profiled solve
  std::vector<std::pair<int, int>> ev_used;   // (family, index of start event); stop = start + 1
  size_t ev_next = 0;                         // first unused event of the pool
  // folds the recorded event pairs into fam_ms / fam_launches and frees them for reuse (waits for the last one)
  void harvest_events() {
    if (ev_used.empty()) { ev_next = 0; return; }
    (void)hipEventSynchronize(ev_pool[ev_used.back().second + 1]);
    for (const auto& u : ev_used) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev_pool[u.second], ev_pool[u.second + 1]) == hipSuccess) { fam_ms[u.first] += ms; fam_launches[u.first]++; }
    }
    ev_used.clear(); ev_next = 0;
  }

  // what the batch owns (the DevBufs of the arena only point into it; the parts of a mixed batch: drop_parts)
  void release() {
    arena.release();
    d_stage_in.release();
    h_state.release(); h_trace.release(); h_params.release();
    h_rawwin.release(); h_buildwin.release(); h_wins_dl.release(); h_totals.release(); h_raw_stage.release();
    if (ev_stage_free) { (void)hipEventDestroy(ev_stage_free); ev_stage_free = nullptr; }
    if (ev_results) { (void)hipEventDestroy(ev_results); ev_results = nullptr; }
    if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
    if (capture_stream) { (void)hipStreamDestroy(capture_stream); capture_stream = nullptr; }
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    ev_pool.clear();
  }
};

namespace slslam {

// ---- what lba_api.hip lends the stream object and the host utilities (defined there, beside the kernels they launch)

// The LBAProblem::build stage of a refill on the device; SLSLAM_ERR_UNSUPPORTED: nothing touched, the caller goes on with the host packer
int refill_device(slslam_lba_batch* b, const slslam_lba_window* windows, int B, hipStream_t s, hipStream_t s_in, const unsigned int* const* packed = nullptr);
// Whether the batch can be refilled with n windows as it is, and whether these windows fit the solve it was captured for
bool refillable_as_is(const slslam_lba_batch* b, int n);
bool fits_batch_path(const slslam_lba_batch* b, const slslam_lba_window* windows, const unsigned int* const* packed, int n);
// slslam_lba_batch_download_async; allow_inplace: a device-built refill's results may go straight into the callers' page-locked arrays
int download_async_impl(slslam_lba_batch* b, void* stream, bool allow_inplace);
// A window's three index arrays <-> one word per observation (index_word.h)
unsigned narrow_indices(size_t M, const int* cam, const int* line, const int* fixed, const uint32_t* packed, int C, int L, uint32_t* out);
void expand_indices(const uint32_t* words, size_t M, std::vector<int>& store, slslam_lba_window* w);

}  // namespace slslam

#endif  // SLSLAM_LBA_BATCH_H_

// slslam_amd/csrc/lba_refine_api.h — host side of the structure-only refinement (include/slslam_hip.h: slslam_line_refiner_*,
// slslam_lba_refine_lines): validation, the lane-interleaved layout (lba_refine_layout.h), one upload, one launch of k_refine_lines
// (lba_refine_lines.h), one download, results back under the caller's line numbering.  Included by lba_api.hip alone, after its
// make_policy: the kernel shares lba_kernels.h, whose kernels one translation unit of the library defines.
#ifndef SLSLAM_LBA_REFINE_API_H_
#define SLSLAM_LBA_REFINE_API_H_

#include <cmath>

#include "call_block.h"
#include "lba_refine_layout.h"
#include "lba_refine_lines.h"

struct slslam_line_refiner {
  int device = -1;
  slslam_solver_options opt;
  long long cap_lines = 0, cap_obs = 0;
  GrowBuf d_in{Mem::kDevice}, d_out{Mem::kDevice}, h_in{Mem::kPinned}, h_out{Mem::kPinned};
  long long calls = 0, allocations = 0;
  // host work arrays, kept for their capacity
  std::vector<RefineWindowLayout> lay;
  std::vector<unsigned char> refine, cam_bad;
  std::vector<int> status;
  std::vector<long long> line_off, slot_off, row_off, cam_off;
};

namespace {

bool finite_n(const double* v, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

extern "C" int slslam_line_refiner_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations,
                                          slslam_line_refiner** out) {
  if (!out || max_lines < 0 || max_observations < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_refiner* r = new (std::nothrow) slslam_line_refiner();
  if (!r) return SLSLAM_ERR_NO_MEMORY;
  if (opt) r->opt = *opt; else slslam_default_options(&r->opt);
  r->device = device;
  r->cap_lines = max_lines; r->cap_obs = max_observations;
  *out = r;
  return SLSLAM_OK;
}

extern "C" void slslam_line_refiner_destroy(slslam_line_refiner* r) { delete r; }

extern "C" int slslam_line_refiner_stats(const slslam_line_refiner* r, long long* calls, long long* allocations) {
  return handle_stats(r, calls, allocations);
}

extern "C" int slslam_line_refiner_run(slslam_line_refiner* r, int n, const slslam_lba_window* windows,
                                       slslam_line_result* const* results, slslam_summary* totals) {
  // ---- every argument before anything is written or the device is asked
  if (!r || n < 0 || (n > 0 && !windows)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int maxC = 0;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const int C = w.num_cameras, L = w.num_lines, M = w.num_observations;
    if (C < 0 || L < 0 || M < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
    if (M > 0 && (!w.camera_index || !w.line_index || !w.fixed_index || !w.observations)) return SLSLAM_ERR_INVALID_ARGUMENT;
    if ((C > 0 || L > 0) && !w.parameters) return SLSLAM_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < M; ++k)
      if (w.camera_index[k] < 0 || w.camera_index[k] >= C || w.line_index[k] < 0 || w.line_index[k] >= L) return SLSLAM_ERR_INVALID_ARGUMENT;
    maxC = std::max(maxC, C);
  }
  const size_t lds_bytes = (size_t)lds_doubles_refine(maxC) * sizeof(double);
  if (lds_bytes > 64 * 1024) return SLSLAM_ERR_UNSUPPORTED;          // the camera table of a window lives in LDS (630 cameras)

  try {
    // ---- what becomes of every line, the layout of every window
    r->lay.resize((size_t)n);
    r->line_off.assign((size_t)n + 1, 0); r->slot_off.assign((size_t)n + 1, 0);
    r->row_off.assign((size_t)n + 1, 0); r->cam_off.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) r->line_off[(size_t)i + 1] = r->line_off[(size_t)i] + windows[i].num_lines;
    r->status.assign((size_t)r->line_off[(size_t)n], SLSLAM_LINE_NO_OBSERVATIONS);
    long long ngroups = 0;
    for (int i = 0; i < n; ++i) {
      const slslam_lba_window& w = windows[i];
      const int C = w.num_cameras, L = w.num_lines, M = w.num_observations;
      int* st = r->status.data() + r->line_off[(size_t)i];
      r->cam_bad.assign((size_t)C, 0);
      for (int c = 0; c < C; ++c) r->cam_bad[(size_t)c] = finite_n(w.parameters + 6 * (size_t)c, 6) ? 0 : 1;
      // one flagged observation makes the line constant (the packer's rule: reference src/lba_problem.cpp:88-91); the camera flags are ignored
      for (int k = 0; k < M; ++k) {
        const int l = w.line_index[k];
        if (w.fixed_index[2 * (size_t)k + 1]) st[l] = SLSLAM_LINE_CONSTANT;
        else if (st[l] == SLSLAM_LINE_NO_OBSERVATIONS) st[l] = SLSLAM_LINE_REFINED;
      }
      for (int k = 0; k < M; ++k) {
        const int l = w.line_index[k];
        if (st[l] == SLSLAM_LINE_REFINED && (r->cam_bad[(size_t)w.camera_index[k]] || !finite_n(w.observations + 8 * (size_t)k, 8)))
          st[l] = SLSLAM_LINE_INVALID;
      }
      r->refine.assign((size_t)L, 0);
      for (int l = 0; l < L; ++l) {
        if (st[l] == SLSLAM_LINE_REFINED && !finite_n(w.parameters + 6 * (size_t)C + 4 * (size_t)l, 4)) st[l] = SLSLAM_LINE_INVALID;
        r->refine[(size_t)l] = st[l] == SLSLAM_LINE_REFINED;
      }
      RefineWindowLayout& W = r->lay[(size_t)i];
      refine_layout_build(L, M, w.line_index, r->refine.data(), &W);
      ngroups += (long long)W.group_depth.size();
      r->slot_off[(size_t)i + 1] = ngroups * kRefineLanes;
      r->row_off[(size_t)i + 1] = r->row_off[(size_t)i] + W.rows;
      r->cam_off[(size_t)i + 1] = r->cam_off[(size_t)i] + C;
    }
    const long long nslot = ngroups * kRefineLanes, nrow = r->row_off[(size_t)n], nelem = nrow * kRefineLanes, ncam = r->cam_off[(size_t)n];
    if (ngroups > 0x7fffffffLL) return SLSLAM_ERR_UNSUPPORTED;
    ++r->calls;

    if (ngroups > 0) {
      const int rc = use_device(r->device);
      if (rc != SLSLAM_OK) return rc;

      // ---- the upload image: groups | cameras | line parameters | counts | observation cameras | observations (4 planes)
      const size_t o_grp = 0;
      const size_t o_cam = align256(o_grp + (size_t)ngroups * sizeof(RefineGroup));
      const size_t o_u = align256(o_cam + (size_t)ncam * 6 * sizeof(double));
      const size_t o_cnt = align256(o_u + (size_t)nslot * 4 * sizeof(double));
      const size_t o_oc = align256(o_cnt + (size_t)nslot * sizeof(int));
      const size_t o_ob = align256(o_oc + (size_t)nelem * sizeof(int));
      const size_t in_bytes = o_ob + (size_t)nelem * 64;
      const size_t out_bytes = (size_t)nslot * sizeof(RefineOut);
      // the buffers are made for the capacities of create (whole waves per window, rows padded to a group's longest line) or for
      // this call, whichever is larger
      const size_t cap_slot = (size_t)((r->cap_lines + kRefineLanes - 1) / kRefineLanes * kRefineLanes);
      const size_t cap_elem = (size_t)((r->cap_obs + kRefineLanes - 1) / kRefineLanes * kRefineLanes);
      const size_t cap_in = 5 * 256 + (cap_slot / kRefineLanes) * sizeof(RefineGroup) + cap_slot * 36 + cap_elem * 68;
      const size_t want_in = std::max(in_bytes, cap_in), want_out = std::max(out_bytes, cap_slot * sizeof(RefineOut));
      HIP_TRY(r->h_in.need(want_in, &r->allocations));
      HIP_TRY(r->d_in.need(want_in, &r->allocations));
      HIP_TRY(r->h_out.need(want_out, &r->allocations));
      HIP_TRY(r->d_out.need(want_out, &r->allocations));

      char* h = r->h_in.p;
      std::memset(h, 0, in_bytes);
      RefineGroup* hg = reinterpret_cast<RefineGroup*>(h + o_grp);
      double* hc = reinterpret_cast<double*>(h + o_cam);
      double* hu = reinterpret_cast<double*>(h + o_u);
      int* hn = reinterpret_cast<int*>(h + o_cnt);
      int* hoc = reinterpret_cast<int*>(h + o_oc);
      double* hob = reinterpret_cast<double*>(h + o_ob);
      long long g0 = 0;
      for (int i = 0; i < n; ++i) {
        const slslam_lba_window& w = windows[i];
        const RefineWindowLayout& W = r->lay[(size_t)i];
        const int C = w.num_cameras, M = w.num_observations;
        for (int c = 0; c < C; ++c)
          for (int a = 0; a < 6; ++a) {
            const double v = w.parameters[6 * (size_t)c + a];
            hc[(r->cam_off[(size_t)i] + c) * 6 + a] = std::isfinite(v) ? v : 0.0;      // (no refined line reads such a camera)
          }
        for (size_t g = 0; g < W.group_depth.size(); ++g) {
          RefineGroup& G = hg[g0 + (long long)g];
          G.row_base = r->row_off[(size_t)i] + W.group_row[g];
          G.cam_off = (int)r->cam_off[(size_t)i]; G.C = C; G.depth = W.group_depth[g]; G.pad = 0;
        }
        const long long s0 = r->slot_off[(size_t)i];
        for (size_t s = 0; s < W.order.size(); ++s) {
          const int l = W.order[s];
          hn[s0 + (long long)s] = W.count[(size_t)l];
          for (int a = 0; a < 4; ++a) hu[(s0 + (long long)s) * 4 + a] = w.parameters[6 * (size_t)C + 4 * (size_t)l + a];
        }
        const long long e0 = r->row_off[(size_t)i] * kRefineLanes;
        for (int k = 0; k < M; ++k) {
          const long long d = W.dest[(size_t)k];
          if (d < 0) continue;
          const long long e = e0 + d;
          hoc[e] = w.camera_index[k];
          for (int q = 0; q < 4; ++q) {
            hob[((long long)q * nelem + e) * 2] = w.observations[8 * (size_t)k + 2 * q];
            hob[((long long)q * nelem + e) * 2 + 1] = w.observations[8 * (size_t)k + 2 * q + 1];
          }
        }
        g0 += (long long)W.group_depth.size();
      }
      if (r->cam_off[(size_t)n] > 0x7fffffffLL) return SLSLAM_ERR_UNSUPPORTED;

      // ---- one upload, one launch, one download
      HIP_TRY(hipMemcpy(r->d_in.p, h, in_bytes, hipMemcpyHostToDevice));
      RefinePtrs p;
      p.groups = r->d_in.at<RefineGroup>(o_grp);
      p.cam_x = r->d_in.at<double>(o_cam);
      p.u = r->d_in.at<double>(o_u);
      p.cnt = r->d_in.at<int>(o_cnt);
      p.ob_cam = r->d_in.at<int>(o_oc);
      p.ob = r->d_in.at<double>(o_ob);
      p.ob_stride = nelem;
      p.out = r->d_out.at<RefineOut>(0);
      const Policy pol = make_policy(r->opt);
      hipLaunchKernelGGL(k_refine_lines, dim3((unsigned)ngroups), dim3(64), lds_bytes, 0, p, pol);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(r->h_out.p, r->d_out.p, out_bytes, hipMemcpyDeviceToHost));
    }

    // ---- results under the caller's line numbering; only a refined line's four doubles are written
    const RefineOut* ho = reinterpret_cast<const RefineOut*>(r->h_out.p);
    for (int i = 0; i < n; ++i) {
      const slslam_lba_window& w = windows[i];
      const RefineWindowLayout& W = r->lay[(size_t)i];
      const int C = w.num_cameras, L = w.num_lines;
      const int* st = r->status.data() + r->line_off[(size_t)i];
      slslam_line_result* res = results ? results[i] : nullptr;
      slslam_summary tot;
      std::memset(&tot, 0, sizeof tot);
      bool failed = false, capped = false;
      int term = SLSLAM_FUNCTION_TOLERANCE, nrefined = 0;
      if (res) std::memset(res, 0, sizeof(slslam_line_result) * (size_t)L);
      // (observations per line, whatever became of it)
      if (res) for (int k = 0; k < w.num_observations; ++k) res[w.line_index[k]].num_observations++;
      for (int l = 0; l < L; ++l) {
        if (res) res[l].status = st[l];
        if (st[l] != SLSLAM_LINE_REFINED) continue;
        const RefineOut& o = ho[r->slot_off[(size_t)i] + W.slot[(size_t)l]];
        for (int a = 0; a < 4; ++a) w.parameters[6 * (size_t)C + 4 * (size_t)l + a] = o.u[a];
        if (res) {
          res[l].termination_type = o.termination;
          res[l].num_successful_steps = o.n_success; res[l].num_unsuccessful_steps = o.n_unsuccess;
          res[l].initial_cost = o.initial_cost; res[l].final_cost = o.final_cost;
        }
        tot.num_successful_steps += o.n_success; tot.num_unsuccessful_steps += o.n_unsuccess;
        tot.initial_cost += o.initial_cost; tot.final_cost += o.final_cost;
        tot.num_residual_blocks += W.count[(size_t)l];
        failed = failed || o.termination == SLSLAM_NUMERICAL_FAILURE;
        capped = capped || o.termination == SLSLAM_NO_CONVERGENCE;
        term = nrefined ? std::max(term, o.termination) : o.termination;
        ++nrefined;
      }
      tot.num_free_parameters = 4 * nrefined;
      tot.termination_type = failed ? SLSLAM_NUMERICAL_FAILURE : capped ? SLSLAM_NO_CONVERGENCE : term;
      if (totals) totals[i] = tot;
    }
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

extern "C" int slslam_lba_refine_lines(const slslam_lba_window* window, const slslam_solver_options* opt, slslam_line_result* results,
                                       slslam_summary* total) {
  if (!window) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_refiner* r = nullptr;
  int rc = slslam_line_refiner_create(-1, opt, 0, 0, &r);
  if (rc != SLSLAM_OK) return rc;
  slslam_line_result* res[1] = { results };
  rc = slslam_line_refiner_run(r, 1, window, results ? res : nullptr, total);
  slslam_line_refiner_destroy(r);
  return rc;
}

#endif

// slslam_amd/csrc/lba_refine_host.h — host side of the structure-only refinement (include/slslam_hip.h: slslam_line_refiner_*,
// slslam_lba_refine_lines) without the device: what the refiner asks of the shared plan (line_call_plan.h), the upload image
// k_refine_lines reads (lba_refine_lines.h) and the scatter of its records back under the caller's line numbering, with the totals of
// every window.
//
// Plain C++: no HIP here, so that this side is checked on its own (tests/host_cxx/refine_host_check.cpp, under the sanitizers).
// lba_refine_api.h adds the buffers, the copies and the launch.
#ifndef SLSLAM_LBA_REFINE_HOST_H_
#define SLSLAM_LBA_REFINE_HOST_H_

#include <algorithm>

#include "line_call_plan.h"

namespace slslam {

struct RefineOut {         // per line slot
  double u[4];             // the refined line (the start values after a numerical failure, as every solve here)
  double initial_cost, final_cost;
  int termination, n_success, n_unsuccess, pad;
};

// cam_tab: kCandTab of lba_kernels.h, which plain C++ cannot include
inline LineCall refine_call(int cam_tab) {
  return { { SLSLAM_LINE_REFINED, SLSLAM_LINE_CONSTANT, SLSLAM_LINE_NO_OBSERVATIONS, SLSLAM_LINE_INVALID }, true, true, cam_tab, 6,
           sizeof(RefineOut) };
}

// The upload image, h[plan.in_bytes]: cameras as (w, t), start values per line slot.
inline void refine_fill_image(const LinePlan& P, int n, const slslam_lba_window* windows, char* h) {
  line_fill_common(P, n, windows, h);
  double* hc = reinterpret_cast<double*>(h + P.o_cam);
  double* hu = reinterpret_cast<double*>(h + P.o_u);
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const int C = w.num_cameras;
    for (int c = 0; c < C; ++c)
      for (int a = 0; a < 6; ++a) {
        const double v = w.parameters[6 * (size_t)c + a];
        hc[(P.cam_off[(size_t)i] + c) * 6 + a] = std::isfinite(v) ? v : 0.0;      // (no refined line reads such a camera)
      }
    const long long s0 = P.slot_off[(size_t)i];
    for (size_t s = 0; s < W.order.size(); ++s)
      for (int a = 0; a < 4; ++a) hu[(s0 + (long long)s) * 4 + a] = w.parameters[6 * (size_t)C + 4 * (size_t)W.order[s] + a];
  }
}

// The records back under the caller's line numbering; only a refined line's four doubles are written.  totals[i]: the sums over the
// refined lines of window i; its termination is failure first, then no-convergence, then the largest of the lines'.
inline void refine_scatter(const LinePlan& P, int n, const slslam_lba_window* windows, const RefineOut* ho, slslam_line_result* const* results,
                           slslam_summary* totals) {
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const int C = w.num_cameras, L = w.num_lines;
    const int* st = P.status.data() + P.line_off[(size_t)i];
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
      const RefineOut& o = ho[P.slot_off[(size_t)i] + W.slot[(size_t)l]];
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
}

}  // namespace slslam
#endif

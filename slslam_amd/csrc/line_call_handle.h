// slslam_amd/csrc/line_call_handle.h — what the handles of the line refiner and of the line triangulator hold and do alike: create,
// the four buffers made for create's capacities or for the call (line_call_plan.h has the rule).  A one-shot call runs a handle of
// its own that lives for the call: device -1, no capacity.  Both calls copy on the null stream and block.  Internal: not part of the C ABI.
#ifndef SLSLAM_LINE_CALL_HANDLE_H_
#define SLSLAM_LINE_CALL_HANDLE_H_

#include <algorithm>
#include <new>

#include "call_block.h"
#include "line_call_plan.h"

namespace slslam {

struct LineHandle {
  int device = -1;
  slslam_solver_options opt;
  long long cap_lines = 0, cap_obs = 0;
  GrowBuf d_in{Mem::kDevice}, d_out{Mem::kDevice}, h_in{Mem::kPinned}, h_out{Mem::kPinned};
  long long calls = 0, allocations = 0;
  LinePlan plan;             // host work arrays, kept for their capacity

  void init(int dev, const slslam_solver_options* o, long long max_lines, long long max_observations) {
    if (o) opt = *o; else slslam_default_options(&opt);
    device = dev;
    cap_lines = max_lines; cap_obs = max_observations;
  }
  // The buffers for the capacities of create or for this call's plan, whichever is larger; every buffer that grows is counted
  int fit(const LineCall& call) {
    size_t cap_in, cap_out;
    line_capacity_bytes(call, cap_lines, cap_obs, &cap_in, &cap_out);
    const size_t want_in = std::max(plan.in_bytes, cap_in), want_out = std::max(plan.out_bytes, cap_out);
    HIP_TRY(h_in.need(want_in, &allocations));
    HIP_TRY(d_in.need(want_in, &allocations));
    HIP_TRY(h_out.need(want_out, &allocations));
    HIP_TRY(d_out.need(want_out, &allocations));
    return SLSLAM_OK;
  }
};

template <typename H>
int line_handle_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations, H** out) {
  if (!out || max_lines < 0 || max_observations < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
  H* h = new (std::nothrow) H();
  if (!h) return SLSLAM_ERR_NO_MEMORY;
  h->init(device, opt, max_lines, max_observations);
  *out = h;
  return SLSLAM_OK;
}

}  // namespace slslam
#endif

// slslam_amd/csrc/lm_policy.h — the trust-region bookkeeping of every LM loop of the library, stated once.
//
// A restatement of Ceres 1.7 TrustRegionMinimizer::Minimize + LevenbergMarquardtStrategy (policy table: DESIGN.md §5): what a state
// looks like before its first evaluation, the initial evaluation with the tests that can end a solve before its first step, one
// step's accept / reject + radius update + stopping rules, and the gradient test after an accepted step.  Scalar C++ with no GPU in
// it: the kernels call it from the one thread that keeps a window's (graph's, line's) books, and a host compiler takes it as it is
// (tests/host_cxx/lm_policy_check.cpp runs it against the oracle's lm_core.c).  What differs from path to path stays with the
// callers: how cost, |g|_inf and |x|^2 are reduced, how the status reaches the other lanes, where the trace records go (the
// `record` / `patch_last_record` callables) and what is counted (`step_counted` / `still_running`).
#ifndef SLSLAM_LM_POLICY_H_
#define SLSLAM_LM_POLICY_H_

#include <cmath>

#include "lba_types.h"

#if defined(__HIPCC__)
#define SLSLAM_LM_FN __host__ __device__ __forceinline__
#else
#define SLSLAM_LM_FN inline
#endif

namespace slslam {

// The state before the first evaluation (Ceres: the LevenbergMarquardtStrategy constructor and the minimizer's zeroed locals).
SLSLAM_LM_FN LMState lm_initial_state(const Policy& pol) {
  LMState st = {};
  st.radius = pol.initial_radius;
  st.decrease_factor = 2.0;
  st.status = kRunning;
  st.fresh = 1;
  return st;
}

// Ceres' initial evaluation, given the cost of the reduced program and of the constant blocks, |g|_inf and |x|^2 at the start values
// and the number of free parameters: fills the state, ends the solve where it cannot start (nothing free: 2, a cost that is not
// finite: 4, a gradient within tolerance: 1 - none of them leaves a record), else hands trace record 0 to `record` and ends the
// solve with 0 if it may not iterate.  Returns the status it has set (kRunning: the solve goes on).
template <typename Record>
SLSLAM_LM_FN int lm_initial_evaluation(const Policy& pol, LMState* st, double cost, double fixed, double gmax, double xn2,
                                       int nfree_params, Record&& record) {
  st->cost = cost; st->fixed_cost = fixed; st->initial_cost = cost + fixed; st->min_cost = cost + fixed;
  st->x_norm = sqrt(xn2);
  st->grad_max = gmax;
  st->abs_grad_tol = pol.gradient_tolerance * (gmax > 1e-12 ? gmax : 1e-12);
  st->need_grad_check = 0;
  st->fresh = 0;
  int status = kRunning;
  if (nfree_params == 0) status = 2;                    // FUNCTION_TOLERANCE: no free blocks
  else if (!std::isfinite(cost)) status = kNumericalFailure;
  else if (gmax <= st->abs_grad_tol) status = 1;
  if (status == kRunning) {
    IterRec rec;
    rec.pad = 0;
    rec.iteration = 0; rec.step_is_valid = 0; rec.step_is_successful = 0;
    rec.cost = cost + fixed; rec.cost_change = 0; rec.gradient_max_norm = gmax; rec.step_norm = 0;
    rec.relative_decrease = 0; rec.trust_region_radius = st->radius; rec.model_cost_change = 0;
    record(rec);
    if (st->iter >= pol.max_num_iterations) status = 0;
  }
  st->status = status;
  return status;
}

// The gradient max-norm at a newly accepted point (Ceres tests it right after accepting a step; here the next linearisation
// supplies it): `patch_last_record(gm)` puts it into the record of the step that led there.
template <typename PatchLastRecord>
SLSLAM_LM_FN void lm_gradient_check(LMState* st, double gm, PatchLastRecord&& patch_last_record) {
  st->grad_max = gm;
  st->need_grad_check = 0;
  patch_last_record(gm);
  if (gm <= st->abs_grad_tol) st->status = 1 /* SLSLAM_GRADIENT_TOLERANCE */;
}

// One trust-region step's bookkeeping: given the cost at the candidate point and the step statistics, accept or reject, move the
// radius, record the iteration, test the stopping rules.  `record(rec)` is called with every recorded iteration, `step_counted()`
// once it is counted, `still_running()` when the solve goes on.
template <typename Record, typename StepCounted, typename StillRunning>
SLSLAM_LM_FN void lm_step_policy(const Policy& pol, LMState* st, double new_cost, double model, double dn2, double xn2,
                                 Record&& record, StepCounted&& step_counted, StillRunning&& still_running) {
  IterRec rec;
  rec.pad = 0;
  const double cost = st->cost;
  rec.iteration = st->iter + 1;
  rec.step_is_valid = 0; rec.step_is_successful = 0;
  rec.model_cost_change = model;
  rec.cost_change = 0; rec.step_norm = 0; rec.relative_decrease = 0;
  rec.gradient_max_norm = st->grad_max;
  bool valid = !st->solve_failed && !(model < 0.0);
  if (!std::isfinite(new_cost)) new_cost = 1.7976931348623157e308;
  if (!valid) {
    if (++st->n_invalid >= pol.max_invalid) { st->status = kNumericalFailure; return; }
  } else {
    st->n_invalid = 0;
    rec.step_is_valid = 1;
    rec.step_norm = sqrt(dn2);
    if (rec.step_norm <= pol.parameter_tolerance * (st->x_norm + pol.parameter_tolerance)) { st->status = 3; return; }
    rec.cost_change = cost - new_cost;
    if (fabs(rec.cost_change) < pol.function_tolerance * cost) { st->status = 2; return; }
    rec.relative_decrease = rec.cost_change / model;
    rec.step_is_successful = rec.relative_decrease > pol.min_relative_decrease;
  }
  if (rec.step_is_successful) {
    st->n_success++;
    const double q = 2.0 * rec.relative_decrease - 1.0;
    double f = 1.0 - q * q * q;
    if (f < 1.0 / 3.0) f = 1.0 / 3.0;
    st->radius = fmin(st->radius / f, pol.max_radius);
    st->decrease_factor = 2.0;
    st->cur = 1 - st->cur;
    st->cost = new_cost;
    st->x_norm = sqrt(xn2);
    st->need_grad_check = 1;      // the next linearisation supplies the gradient at the new point
    st->same_point = 0;
  } else {
    // only the radius changes: gradient and column norms stay valid - except after the very first sweep of an LBA solve, whose
    // camera entries are in unscaled coordinates (it doubled as the initial evaluation)
    st->same_point = st->iter > 0 ? 1 : 0;
    st->n_unsuccess++;
    if (rec.step_is_valid) { st->radius = st->radius / st->decrease_factor; st->decrease_factor *= 2.0; }
    else st->radius *= 0.5;
  }
  rec.cost = st->cost + st->fixed_cost;
  rec.trust_region_radius = st->radius;
  if (rec.cost < st->min_cost) st->min_cost = rec.cost;
  record(rec);
  st->iter = rec.iteration;
  step_counted();
  if (st->radius < pol.min_radius) { st->status = 5; return; }
  if (st->iter >= pol.max_num_iterations) { st->status = 0; return; }
  still_running();
}

}  // namespace slslam
#endif  // SLSLAM_LM_POLICY_H_

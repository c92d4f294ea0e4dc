// tests/host_cxx/lm_policy_check.cpp — csrc/lm_policy.h on the host against the oracle's trust-region driver (oracle/lm_core.c).
//
// One small dense problem, r_i(x) = x0 exp(x1 t_i) + x2 - y_i with t_i = i / 5, i = 0..5, y from x* = (2, -1, 0.5), as oracle_nlls
// callbacks.  Every case runs it twice: through oracle_lm_minimize, and through the loop below, which is what every device LM loop
// is once the sweeps and reductions are taken away - lm_initial_state, lm_initial_evaluation, D^2 = clamp(diag) / radius,
// lm_step_policy, lm_gradient_check - around the same callbacks in the same order.  Decisions, counts and the termination type must
// be equal, the doubles of the trace agree to 1e-12 relative: both sides do the heavy arithmetic in the same callbacks, only the
// policy's handful of scalar operations per iteration can differ.  Build with -fsanitize=address,undefined.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
#include "../../oracle/lm_core.h"
}
#include "../../slslam_amd/csrc/lm_policy.h"

using namespace slslam;

namespace {

enum { kM = 6, kN = 3 };
struct Problem {
  double t[kM], y[kM];
  double r[kM], J[kM][kN];      // residuals and Jacobian held since the last evaluate(want_jac = 1); the Jacobian possibly scaled
  int solve_fails;              // the `solve` callback always fails
};

void residuals(const Problem* P, const double* x, double* r, double (*J)[kN]) {
  for (int i = 0; i < kM; ++i) {
    const double e = std::exp(x[1] * P->t[i]);
    r[i] = x[0] * e + x[2] - P->y[i];
    if (J) { J[i][0] = e; J[i][1] = x[0] * P->t[i] * e; J[i][2] = 1.0; }
  }
}
int cb_evaluate(void* ctx, const double* x, double* cost, int want_jac, double* gradient) {
  Problem* P = (Problem*)ctx;
  double rl[kM];
  double* r = want_jac ? P->r : rl;
  residuals(P, x, r, want_jac ? P->J : nullptr);
  double c = 0.0;
  for (int i = 0; i < kM; ++i) c += r[i] * r[i];
  *cost = 0.5 * c;
  if (want_jac)
    for (int j = 0; j < kN; ++j) {
      double g = 0.0;
      for (int i = 0; i < kM; ++i) g += P->J[i][j] * P->r[i];
      gradient[j] = g;
    }
  return 1;
}
void cb_sq_col_norm(void* ctx, double* out) {
  Problem* P = (Problem*)ctx;
  for (int j = 0; j < kN; ++j) {
    double s = 0.0;
    for (int i = 0; i < kM; ++i) s += P->J[i][j] * P->J[i][j];
    out[j] = s;
  }
}
void cb_scale_cols(void* ctx, const double* scale) {
  Problem* P = (Problem*)ctx;
  for (int i = 0; i < kM; ++i)
    for (int j = 0; j < kN; ++j) P->J[i][j] *= scale[j];
}
int cb_solve(void* ctx, const double* lm_diag, double* y) {
  Problem* P = (Problem*)ctx;
  if (P->solve_fails) return 1;
  double A[kN * kN];
  for (int a = 0; a < kN; ++a) {
    for (int b = 0; b < kN; ++b) {
      double s = 0.0;
      for (int i = 0; i < kM; ++i) s += P->J[i][a] * P->J[i][b];
      A[a * kN + b] = s;
    }
    A[a * kN + a] += lm_diag[a] * lm_diag[a];
    double g = 0.0;
    for (int i = 0; i < kM; ++i) g += P->J[i][a] * P->r[i];
    y[a] = g;
  }
  if (oracle_dense_cholesky(A, kN)) return 1;
  oracle_dense_cholesky_solve(A, kN, y);
  return 0;
}
double cb_model_cost_change(void* ctx, const double* step) {
  Problem* P = (Problem*)ctx;
  double m = 0.0;
  for (int i = 0; i < kM; ++i) {
    double js = 0.0;
    for (int j = 0; j < kN; ++j) js += P->J[i][j] * step[j];
    m -= js * (P->r[i] + 0.5 * js);
  }
  return m;
}

Problem make_problem(int solve_fails) {
  Problem P;
  std::memset(&P, 0, sizeof(P));
  const double xs[kN] = { 2.0, -1.0, 0.5 };
  for (int i = 0; i < kM; ++i) { P.t[i] = i / 5.0; P.y[i] = xs[0] * std::exp(xs[1] * P.t[i]) + xs[2]; }
  P.solve_fails = solve_fails;
  return P;
}
oracle_nlls callbacks(Problem* P) {
  oracle_nlls f;
  f.n = kN; f.ctx = P; f.evaluate = cb_evaluate; f.sq_col_norm = cb_sq_col_norm; f.scale_cols = cb_scale_cols; f.solve = cb_solve;
  f.model_cost_change = cb_model_cost_change;
  return f;
}

Policy policy_of(const oracle_lm_options& o) {      // as the two host files that fill Policy do
  Policy p;
  std::memset(&p, 0, sizeof(p));
  p.initial_radius = o.initial_trust_region_radius; p.max_radius = o.max_trust_region_radius; p.min_radius = o.min_trust_region_radius;
  p.min_relative_decrease = o.min_relative_decrease; p.min_lm_diagonal = o.min_lm_diagonal; p.max_lm_diagonal = o.max_lm_diagonal;
  p.function_tolerance = o.function_tolerance; p.gradient_tolerance = o.gradient_tolerance; p.parameter_tolerance = o.parameter_tolerance;
  p.max_num_iterations = o.max_num_iterations; p.max_invalid = o.max_num_consecutive_invalid_steps; p.jacobi_scaling = o.jacobi_scaling;
  return p;
}

struct Result {
  int termination, n_success, n_unsuccess;
  double initial_cost, final_cost;
  std::vector<IterRec> trace;
};

// the loop of the device paths, on the host
Result minimize_with_policy(oracle_nlls* f, const Policy& pol, const double* x0) {
  Result R;
  double x[kN], xc[kN], gradient[kN], scale[kN], diag[kN], lm_diag[kN], step[kN];
  for (int i = 0; i < kN; ++i) { x[i] = x0[i]; scale[i] = 1.0; }
  LMState st = lm_initial_state(pol);
  auto record = [&](const IterRec& rec) { R.trace.push_back(rec); st.ntrace++; };
  auto max_abs = [&]() { double m = 0.0; for (int i = 0; i < kN; ++i) m = std::fmax(m, std::fabs(gradient[i])); return m; };
  double cost = 0.0, xn2 = 0.0;
  f->evaluate(f->ctx, x, &cost, 1, gradient);
  for (int i = 0; i < kN; ++i) xn2 += x[i] * x[i];
  if (lm_initial_evaluation(pol, &st, cost, 0.0, max_abs(), xn2, kN, record) == kRunning && pol.jacobi_scaling) {
    f->sq_col_norm(f->ctx, scale);
    for (int i = 0; i < kN; ++i) scale[i] = 1.0 / (1.0 + std::sqrt(scale[i]));
    f->scale_cols(f->ctx, scale);
  }
  bool have_diag = false;
  while (st.status == kRunning) {
    if (!have_diag) { f->sq_col_norm(f->ctx, diag); have_diag = true; }
    for (int i = 0; i < kN; ++i) lm_diag[i] = std::sqrt(std::fmin(std::fmax(diag[i], pol.min_lm_diagonal), pol.max_lm_diagonal) / st.radius);
    int failed = f->solve(f->ctx, lm_diag, step);
    for (int i = 0; i < kN && !failed; ++i) if (!std::isfinite(step[i])) failed = 1;
    double model = 0.0, new_cost = DBL_MAX, dn2 = 0.0, xn2c = 0.0;
    if (!failed) {
      for (int i = 0; i < kN; ++i) step[i] = -step[i];
      model = f->model_cost_change(f->ctx, step);
    }
    if (!failed && !(model < 0.0)) {
      for (int i = 0; i < kN; ++i) xc[i] = x[i] + step[i] * scale[i];
      f->evaluate(f->ctx, xc, &new_cost, 0, nullptr);
      for (int i = 0; i < kN; ++i) { const double d = x[i] - xc[i]; dn2 += d * d; xn2c += xc[i] * xc[i]; }
    }
    st.solve_failed = failed;
    const int n_success_before = st.n_success;
    lm_step_policy(pol, &st, new_cost, model, dn2, xn2c, record, []() {}, []() {});
    if (st.n_success != n_success_before) {
      for (int i = 0; i < kN; ++i) x[i] = xc[i];
      f->evaluate(f->ctx, x, &cost, 1, gradient);
      have_diag = false;
      lm_gradient_check(&st, max_abs(), [&](double gm) { R.trace.back().gradient_max_norm = gm; });
      if (st.status == kRunning && pol.jacobi_scaling) f->scale_cols(f->ctx, scale);
    }
  }
  R.termination = st.status; R.n_success = st.n_success; R.n_unsuccess = st.n_unsuccess;
  R.initial_cost = st.initial_cost; R.final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;
  return R;
}

int failures = 0;
void expect(bool ok, const char* name, const char* what, double a, double b, int k) {
  if (ok) return;
  std::printf("FAIL %s: %s differs at record %d: oracle %.17g, lm_policy.h %.17g\n", name, what, k, a, b);
  ++failures;
}
bool close_rel(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fmax(std::fabs(a), std::fabs(b)); }

struct Seen { int termination[6] = { 0, 0, 0, 0, 0, 0 }; int accepted = 0, rejected = 0, invalid = 0; } seen;

void run_case(const char* name, const oracle_lm_options& opt, const double* x0, int solve_fails, int want_a, int want_b, int min_rejected) {
  Problem Po = make_problem(solve_fails), Pd = make_problem(solve_fails);
  oracle_nlls fo = callbacks(&Po), fd = callbacks(&Pd);
  double xo[kN] = { x0[0], x0[1], x0[2] };
  oracle_summary s;
  std::memset(&s, 0, sizeof(s));
  oracle_iteration tr[kMaxTrace];
  int n = 0;
  oracle_lm_minimize(&fo, &opt, xo, &s, tr, kMaxTrace, &n);
  const Result R = minimize_with_policy(&fd, policy_of(opt), x0);
  int rejected = 0;
  for (int k = 1; k < n && k < kMaxTrace; ++k) {
    if (tr[k].step_is_successful) seen.accepted++;
    else if (tr[k].step_is_valid) { seen.rejected++; rejected++; }
    else seen.invalid++;
  }
  if (s.termination_type >= 0 && s.termination_type < 6) seen.termination[s.termination_type]++;
  std::printf("%-28s oracle: termination %d, %d records, %d + %d steps | lm_policy.h: termination %d, %d records, %d + %d steps\n", name,
              s.termination_type, n, s.num_successful_steps, s.num_unsuccessful_steps, R.termination, (int)R.trace.size(), R.n_success, R.n_unsuccess);
  if (want_a >= 0 && s.termination_type != want_a && s.termination_type != want_b) {
    std::printf("FAIL %s: the oracle ends with %d, the case is meant to end with %d\n", name, s.termination_type, want_a);
    ++failures;
  }
  if (rejected < min_rejected) { std::printf("FAIL %s: the oracle's trace has no rejected step\n", name); ++failures; }
  expect(s.termination_type == R.termination, name, "termination", s.termination_type, R.termination, -1);
  // The oracle, as Ceres, leaves a solve that an accepted step brought within the gradient tolerance before it records that step; the
  // library records every counted step and writes the new gradient norm into the record (lm_gradient_check).  That one record apart,
  // the traces have the same length; the steps counted are the same in either case.
  const int unrecorded = s.termination_type == 1 && n > 0 && s.num_successful_steps + s.num_unsuccessful_steps == n ? 1 : 0;
  expect(n + unrecorded == (int)R.trace.size(), name, "record count", n + unrecorded, (double)R.trace.size(), -1);
  if (unrecorded && !R.trace.empty())
    expect(R.trace.back().step_is_successful == 1 && R.trace.back().iteration == n, name, "the record of the last accepted step", n, R.trace.back().iteration, n);
  expect(s.num_successful_steps == R.n_success, name, "successful steps", s.num_successful_steps, R.n_success, -1);
  expect(s.num_unsuccessful_steps == R.n_unsuccess, name, "unsuccessful steps", s.num_unsuccessful_steps, R.n_unsuccess, -1);
  expect(close_rel(s.initial_cost, R.initial_cost), name, "initial cost", s.initial_cost, R.initial_cost, -1);
  expect(close_rel(s.final_cost, R.final_cost), name, "final cost", s.final_cost, R.final_cost, -1);
  for (int k = 0; k < n && k < (int)R.trace.size() && k < kMaxTrace; ++k) {
    const oracle_iteration& a = tr[k];
    const IterRec& b = R.trace[k];
    expect(a.iteration == b.iteration, name, "iteration", a.iteration, b.iteration, k);
    expect(a.step_is_valid == b.step_is_valid, name, "step_is_valid", a.step_is_valid, b.step_is_valid, k);
    expect(a.step_is_successful == b.step_is_successful, name, "step_is_successful", a.step_is_successful, b.step_is_successful, k);
    expect(close_rel(a.trust_region_radius, b.trust_region_radius), name, "radius", a.trust_region_radius, b.trust_region_radius, k);
    expect(close_rel(a.cost, b.cost), name, "cost", a.cost, b.cost, k);
    expect(close_rel(a.cost_change, b.cost_change), name, "cost change", a.cost_change, b.cost_change, k);
    expect(close_rel(a.relative_decrease, b.relative_decrease), name, "relative decrease", a.relative_decrease, b.relative_decrease, k);
    expect(close_rel(a.step_norm, b.step_norm), name, "step norm", a.step_norm, b.step_norm, k);
    expect(close_rel(a.gradient_max_norm, b.gradient_max_norm), name, "gradient max-norm", a.gradient_max_norm, b.gradient_max_norm, k);
  }
}

}  // namespace

int main() {
  const double start[kN] = { 1.0, 0.0, 0.0 };
  oracle_lm_options d;
  oracle_lm_default_options(&d);
  { oracle_lm_options o = d; run_case("near-default", o, start, 0, 1, 2, 0); }
  { oracle_lm_options o = d; o.max_num_iterations = 2; run_case("max_num_iterations = 2", o, start, 0, 0, 0, 0); }
  { oracle_lm_options o = d; o.gradient_tolerance = 1.0; run_case("gradient_tolerance = 1", o, start, 0, 1, 1, 0); }
  { oracle_lm_options o = d; o.parameter_tolerance = 1e3; run_case("parameter_tolerance = 1e3", o, start, 0, 3, 3, 0); }
  { oracle_lm_options o = d; o.function_tolerance = 0.9; run_case("function_tolerance = 0.9", o, start, 0, 2, 2, 0); }   // (0.5: every step from this start more than halves the cost)
  { oracle_lm_options o = d; o.initial_trust_region_radius = 1e4; o.min_trust_region_radius = 1e9; run_case("min_radius = 1e9", o, start, 0, 5, 5, 0); }
  { oracle_lm_options o = d; run_case("solve always fails", o, start, 1, 4, 4, 0); }
  { oracle_lm_options o = d; const double far[kN] = { 1.0, 3.0, 0.0 }; run_case("start (1, 3, 0): rejected steps", o, far, 0, -1, -1, 1); }
  for (int t = 0; t < 6; ++t)
    if (!seen.termination[t]) { std::printf("FAIL: no case ends with termination %d in the oracle\n", t); ++failures; }
  if (!seen.accepted || !seen.rejected || !seen.invalid) {
    std::printf("FAIL: the oracle's traces hold %d accepted, %d rejected valid and %d invalid steps: each must occur\n", seen.accepted, seen.rejected, seen.invalid);
    ++failures;
  }
  if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
  std::printf("lm policy ok\n");
  return 0;
}

// slslam_amd/csrc/lba_refine_lines.h — structure-only refinement: every camera constant, every line its own 4-unknown LM problem,
// the whole solve of every line of every window in ONE launch, lane <-> line.
//
// The mirror image of lba_motion_only.h.  With the cameras fixed the normal matrix is block diagonal: nothing couples two lines, so
// each gets its OWN trust region (the general path runs one for the window) and no reduced camera system exists.  A workgroup is one
// wave = 64 lines of one window (sorted by observation count, observations lane-interleaved: lba_refine_layout.h); it builds the
// window's camera table (R, t per camera: the cameras never move, no J_L) in LDS once; then every lane loops
//   linearise its observations at the accepted point (lba_math.h, Huber corrector folded in) -> J^T J (10 values), J^T r (4) in registers
//   | Jacobi scale from the first linearisation | D^2 = clamp(diag) / radius | 4 x 4 Cholesky (chol4_inverse, as the sweeps) | candidate
//   line | second pass over the observations for the candidate cost | lm_step_policy() - lm_policy.h, the policy every path runs, one
//   LMState per lane in registers.
// The row loops are wave-uniform (a group's rows), the lanes predicated: a lane whose line has stopped idles, a lane whose step was
// rejected skips the linearisation pass (the point has not moved), the wave leaves when all its lanes have stopped.  fp64 throughout,
// no atomics, nothing shared between lanes but the read-only camera table: a line's bytes cannot depend on its company.
#ifndef SLSLAM_LBA_REFINE_LINES_H_
#define SLSLAM_LBA_REFINE_LINES_H_

#include "lba_kernels.h"
#include "lba_refine_host.h"

namespace slslam {

struct RefinePtrs {
  const RefineGroup* groups; // (LineGroup, line_call_plan.h; RefineOut: lba_refine_host.h)
  const double* cam_x;     // [ncam][6] (w, t)
  const double* u;         // [nslot][4], slot = 64 group + lane
  const int* cnt;          // [nslot] observations of the slot's line; 0: an unused slot
  const int* ob_cam;       // [nrow * 64] window-local camera of observation (row, lane)
  const double* ob;        // [4][ob_stride] double2: the four observed endpoints, as BatchPtrs.ob
  long long ob_stride;     // = nrow * 64
  RefineOut* out;          // [nslot]
};

__host__ __device__ inline int lds_doubles_refine(int C) { return C * kCandTab; }

__global__ __launch_bounds__(64) void k_refine_lines(RefinePtrs p, Policy pol) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const RefineGroup gr = p.groups[blockIdx.x];
  for (int c = lane; c < gr.C; c += 64) {
    const double* x = p.cam_x + (long long)(gr.cam_off + c) * kCamRec;
    const double w[3] = { x[0], x[1], x[2] };
    double R[9];
    cam_rotation<double>(w, R);
    double* ct = smem + c * kCandTab;
#pragma unroll
    for (int q = 0; q < 9; ++q) ct[q] = R[q];
    ct[9] = x[3]; ct[10] = x[4]; ct[11] = x[5];
  }
  __syncthreads();

  const long long slot = (long long)blockIdx.x * 64 + lane;
  const int cnt = p.cnt[slot];
  const long long e0 = gr.row_base * 64 + lane;            // the lane's observation j is element e0 + 64 j
  double u[4], sc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { u[a] = p.u[slot * 4 + a]; sc[a] = 1.0; }
  LMState st = lm_initial_state(pol);

  // observation j of this lane and its camera's table entry
  auto load_obs = [&](int j, double (&ob)[8], double (&R)[9], double (&t)[3]) {
    const long long e = e0 + (long long)j * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double2 v = reinterpret_cast<const double2*>(p.ob)[(long long)q * p.ob_stride + e];
      ob[2 * q] = v.x; ob[2 * q + 1] = v.y;
    }
    const double* ct = smem + p.ob_cam[e] * kCandTab;
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = ct[q];
    t[0] = ct[9]; t[1] = ct[10]; t[2] = ct[11];
  };

  double H[10], g[4];                // J^T J (lower triangle, packed as chol4_inverse reads it) and J^T r at the accepted point, scaled
#pragma unroll
  for (int q = 0; q < 10; ++q) H[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) g[q] = 0.0;
  bool running = cnt > 0, have_lin = false;
  while (__any(running)) {
    const bool lin = running && !have_lin;
    if (__any(lin)) {
      // ---- pass 1: linearise the lane's observations at the accepted point (Jacobi scale: 1 in the first pass of a solve)
      double cost = 0.0, trig[7];
      if (lin) {
#pragma unroll
        for (int q = 0; q < 10; ++q) H[q] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = 0.0;
      }
      line_trig<double>(u, trig);
      for (int j = 0; j < gr.depth; ++j) {
        if (lin && j < cnt) {
          double ob[8], R[9], t[3], rs[4], Jl[16], c;
          load_obs(j, ob, R, t);
          obs_linearise_raw<double>(R, t, trig, sc, ob, pol.baseline, pol.huber_delta, rs, Jl, &c, [](int, const double*) {});
          cost += c;
          int q = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) g[a] += Jl[4 * r + a] * rs[r];
#pragma unroll
            for (int b = 0; b <= a; ++b, ++q) {
#pragma unroll
              for (int r = 0; r < 4; ++r) H[q] += Jl[4 * r + a] * Jl[4 * r + b];
            }
          }
        }
      }
      if (lin) {
        have_lin = true;
        if (st.fresh) {
          // ---- Ceres' initial evaluation: cost, gradient max-norm, |x|, Jacobi scale from diag(J^T J) at the start values
          double gmax = 0.0, xn2 = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            gmax = fmax(gmax, fabs(g[a]));
            xn2 += u[a] * u[a];
            sc[a] = pol.jacobi_scaling ? 1.0 / (1.0 + sqrt(H[tri_index(a, a)])) : 1.0;
          }
          lm_initial_evaluation(pol, &st, cost, 0.0, gmax, xn2, 4 /* a lane with a line has its four unknowns */, [](const IterRec&) {});
          // the system to scaled coordinates (a congruence with diag(scale)), as the other paths do
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            g[a] *= sc[a];
#pragma unroll
            for (int b = 0; b <= a; ++b) H[tri_index(a, b)] *= sc[a] * sc[b];
          }
        } else if (st.need_grad_check) {
          // ---- gradient max-norm at the newly accepted point (g is the scaled gradient)
          double gm = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) gm = fmax(gm, fabs(g[a] / sc[a]));
          lm_gradient_check(&st, gm, [](double) {});
        }
        running = st.status == kRunning;
      }
    }

    // ---- damped normal equations, step, candidate line
    double D2[4], K[10], z[4], y[4], uc[4], model = 0.0, dn2 = 0.0, xn2 = 0.0;
    lm_diag4(H, pol, 1.0 / st.radius, D2);
    const bool ok = chol4_inverse(H, D2, K);
    chol4_apply(K, g, z);
    chol4_apply_t(K, z, y);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      model += 0.5 * y[a] * (g[a] + D2[a] * y[a]);
      uc[a] = u[a] - y[a] * sc[a];
      const double dd = u[a] - uc[a];
      dn2 += dd * dd;
      xn2 += uc[a] * uc[a];
    }

    // ---- pass 2: cost at the candidate line (residuals only)
    if (__any(running)) {
      double ccost = 0.0, trig[7], cp[3], dv[3];
      line_trig<double>(uc, trig);
      line_points<double>(trig, cp, dv);
      for (int j = 0; j < gr.depth; ++j) {
        if (running && j < cnt) {
          double ob[8], R[9], t[3], r[4], c;
          load_obs(j, ob, R, t);
          obs_residual<double>(R, t, cp, dv, ob, pol.baseline, r);
          huber_scale<double>(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3], pol.huber_delta, &c);
          ccost += c;
        }
      }

      // ---- accept / reject, radius, stopping rules
      if (running) {
        const int n_success_before = st.n_success;
        st.solve_failed = (ok && isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]) && isfinite(y[3])) ? 0 : 1;
        lm_step_policy(pol, &st, ccost, model, dn2, xn2, [](const IterRec&) {}, []() {}, []() {});
        if (st.n_success != n_success_before) {
#pragma unroll
          for (int a = 0; a < 4; ++a) u[a] = uc[a];
          have_lin = false;
        }
        running = st.status == kRunning;
      }
    }
  }

  RefineOut o;
  const bool failed = st.status == kNumericalFailure;
#pragma unroll
  for (int a = 0; a < 4; ++a) o.u[a] = failed ? p.u[slot * 4 + a] : u[a];
  o.initial_cost = st.initial_cost;
  o.final_cost = st.min_cost < st.initial_cost ? st.min_cost : st.initial_cost;
  o.termination = st.status == kRunning ? 0 : st.status;
  o.n_success = st.n_success; o.n_unsuccess = st.n_unsuccess; o.pad = 0;
  p.out[slot] = o;
}

}  // namespace slslam
#endif

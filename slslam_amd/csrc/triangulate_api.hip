// slslam_amd/csrc/triangulate_api.hip — the line triangulator (include/slslam_hip.h: slslam_line_triangulator_*,
// slslam_lba_triangulate_lines): making a landmark, the link between the matcher / pose estimator and the refiner or the window solve.
// Per call, whatever the number of windows:
//   host     validation, the plan shared with the refiner (line_call_plan.h), the camera tables (lba_triangulate_host.h)
//   upload   one block [groups | cameras (R, t) | counts | observation cameras | observations]
//   launch   k_triangulate_lines (lba_triangulate.h): one wave per 64 lines of one window
//   download one block [TriOut per line slot], scattered back under the caller's line numbering
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <chrono>
#include <new>

#include "../../include/slslam_hip.h"
#include "lba_triangulate.h"
#include "line_call_handle.h"

using namespace slslam;

struct slslam_line_triangulator : LineHandle {
  double last_ms[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };   // the last run: host layout, upload, kernel, download, scatter
};

extern "C" int slslam_line_triangulator_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations,
                                               slslam_line_triangulator** out) {
  return line_handle_create(device, opt, max_lines, max_observations, out);
}

extern "C" void slslam_line_triangulator_destroy(slslam_line_triangulator* t) { delete t; }

extern "C" int slslam_line_triangulator_stats(const slslam_line_triangulator* t, long long* calls, long long* allocations) {
  return handle_stats(t, calls, allocations);
}

extern "C" int slslam_line_triangulator_run(slslam_line_triangulator* t, int n, const slslam_lba_window* windows, int method,
                                            double inverse_depth, double min_parallax, slslam_triangulated_line* const* results,
                                            double* const* lines_av) {
  // ---- every argument before anything is written or the device is asked
  if (!t) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = tri_validate(n, windows, method, inverse_depth, min_parallax);
  if (rc != SLSLAM_OK) return rc;
  using clk = std::chrono::steady_clock;
  const auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  try {
    TriPlan& P = t->plan;
    const clk::time_point t0 = clk::now();
    clk::time_point t1 = t0, t2 = t0, t3 = t0, t4 = t0;
    rc = tri_plan_build(n, windows, &P);
    if (rc != SLSLAM_OK) return rc;
    ++t->calls;

    if (P.ngroups > 0) {
      if ((rc = use_device(t->device)) != SLSLAM_OK) return rc;

      if ((rc = t->fit(tri_call())) != SLSLAM_OK) return rc;
      tri_fill_image(P, n, windows, [](const double* wt, double* T) { slslam_gc::wt_to_Rt(wt, T); }, t->h_in.p);

      // ---- one upload, one launch, one download
      t1 = clk::now();
      HIP_TRY(hipMemcpy(t->d_in.p, t->h_in.p, P.in_bytes, hipMemcpyHostToDevice));
      t2 = clk::now();
      TriPtrs p;
      p.groups = t->d_in.at<TriGroup>(P.o_grp);
      p.cam = t->d_in.at<double>(P.o_cam);
      p.cnt = t->d_in.at<int>(P.o_cnt);
      p.ob_cam = t->d_in.at<int>(P.o_oc);
      p.ob = t->d_in.at<double>(P.o_ob);
      p.ob_stride = P.nelem;
      p.out = t->d_out.at<TriOut>(0);
      const size_t lds_bytes = (size_t)lds_doubles_triangulate(P.maxC) * sizeof(double);
      hipLaunchKernelGGL(k_triangulate_lines, dim3((unsigned)P.ngroups), dim3(64), lds_bytes, 0, p, t->opt.baseline, inverse_depth,
                         min_parallax, method);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipStreamSynchronize(0));              // (the download would wait as well: this only splits the two times)
      t3 = clk::now();
      HIP_TRY(hipMemcpy(t->h_out.p, t->d_out.p, P.out_bytes, hipMemcpyDeviceToHost));
      t4 = clk::now();
    } else {
      t1 = t2 = t3 = t4 = clk::now();
    }
    tri_scatter(P, n, windows, reinterpret_cast<const TriOut*>(t->h_out.p), results, lines_av);
    const double m[5] = { ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, clk::now()) };
    for (int a = 0; a < 5; ++a) t->last_ms[a] = m[a];
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

extern "C" int slslam_line_triangulator_timing(const slslam_line_triangulator* t, double* ms) {
  if (!t || !ms) return SLSLAM_ERR_INVALID_ARGUMENT;
  for (int a = 0; a < 5; ++a) ms[a] = t->last_ms[a];
  return SLSLAM_OK;
}

extern "C" int slslam_lba_triangulate_lines(const slslam_lba_window* window, const slslam_solver_options* opt, int method,
                                            double inverse_depth, double min_parallax, slslam_triangulated_line* results, double* lines_av) {
  if (!window) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_triangulator t;
  t.init(-1, opt, 0, 0);
  slslam_triangulated_line* res[1] = { results };
  double* av[1] = { lines_av };
  return slslam_line_triangulator_run(&t, 1, window, method, inverse_depth, min_parallax, results ? res : nullptr, lines_av ? av : nullptr);
}

// Test hook: ONE line through the functions of lba_triangulate.h on the host, in the kernel's order.
extern "C" int slslam_debug_triangulate_host(int num_observations, const double* observations, const double* cameras, double baseline,
                                             int method, double inverse_depth, double min_parallax, double* line_av, double* eigenvalues,
                                             int* status, int* num_planes, int* clamped, double* offdiagonal) {
  if (num_observations < 1 || !observations || !cameras || (method != 0 && method != 1)) return SLSLAM_ERR_INVALID_ARGUMENT;
  double T[12], cp[3], v[3], lam[4] = { 0.0, 0.0, 0.0, 0.0 }, off = 0.0;
  int cl = 0, planes = 0, st = SLSLAM_TRI_STEREO;
  slslam_gc::wt_to_Rt(cameras, T);
  const bool have = tri_stereo_first(observations, T, baseline, inverse_depth, cp, v, &cl);
  if (have && method == 1) {
    double G[10] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, cpm[3], vm[3], l4[4];
    for (int j = 0; j < num_observations; ++j) {
      double pl[4], pr[4];
      slslam_gc::wt_to_Rt(cameras + 6 * (size_t)j, T);
      tri_camera_planes(observations + 8 * (size_t)j, baseline, pl, pr);
      planes += tri_gram_add(pl, T, G) ? 1 : 0;
      planes += tri_gram_add(pr, T, G) ? 1 : 0;
    }
    tri_multiview_line(G, l4, cpm, vm, &off);
    if (vm[0] * v[0] + vm[1] * v[1] + vm[2] * v[2] < 0.0) { vm[0] = -vm[0]; vm[1] = -vm[1]; vm[2] = -vm[2]; }
    if (tri_take_multiview(num_observations, l4, cpm, vm, min_parallax)) {
      st = SLSLAM_TRI_MULTIVIEW;
      for (int a = 0; a < 3; ++a) { cp[a] = cpm[a]; v[a] = vm[a]; }
      for (int a = 0; a < 4; ++a) lam[a] = l4[a];
    }
  }
  if (status) *status = have ? st : SLSLAM_TRI_INVALID;
  if (num_planes) *num_planes = have ? planes : 0;
  if (clamped) *clamped = (have && st == SLSLAM_TRI_STEREO) ? cl : 0;
  if (offdiagonal) *offdiagonal = off;
  if (eigenvalues) for (int a = 0; a < 4; ++a) eigenvalues[a] = lam[a];
  if (line_av && have) for (int a = 0; a < 3; ++a) { line_av[a] = cp[a]; line_av[3 + a] = v[a]; }
  return SLSLAM_OK;
}

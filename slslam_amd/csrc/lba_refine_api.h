// slslam_amd/csrc/lba_refine_api.h — the structure-only refinement's handle and C entry points (include/slslam_hip.h:
// slslam_line_refiner_*, slslam_lba_refine_lines): the buffers, one upload, one launch of k_refine_lines (lba_refine_lines.h), one
// download.  The plan, the image and the scatter are plain C++ (line_call_plan.h, lba_refine_host.h).  Included by lba_api.hip alone,
// after its make_policy: the kernel shares lba_kernels.h, whose kernels one translation unit of the library defines.
#ifndef SLSLAM_LBA_REFINE_API_H_
#define SLSLAM_LBA_REFINE_API_H_

#include "lba_refine_lines.h"
#include "line_call_handle.h"

struct slslam_line_refiner : LineHandle {};

extern "C" int slslam_line_refiner_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations,
                                          slslam_line_refiner** out) {
  return line_handle_create(device, opt, max_lines, max_observations, out);
}

extern "C" void slslam_line_refiner_destroy(slslam_line_refiner* r) { delete r; }

extern "C" int slslam_line_refiner_stats(const slslam_line_refiner* r, long long* calls, long long* allocations) {
  return handle_stats(r, calls, allocations);
}

extern "C" int slslam_line_refiner_run(slslam_line_refiner* r, int n, const slslam_lba_window* windows,
                                       slslam_line_result* const* results, slslam_summary* totals) {
  // ---- every argument before anything is written or the device is asked
  if (!r) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = line_validate_windows(n, windows);
  if (rc != SLSLAM_OK) return rc;
  try {
    const LineCall call = refine_call(kCandTab);
    LinePlan& P = r->plan;
    if ((rc = line_plan_build(call, n, windows, &P)) != SLSLAM_OK) return rc;
    ++r->calls;

    if (P.ngroups > 0) {
      if ((rc = use_device(r->device)) != SLSLAM_OK) return rc;
      if ((rc = r->fit(call)) != SLSLAM_OK) return rc;
      refine_fill_image(P, n, windows, r->h_in.p);

      // ---- one upload, one launch, one download
      HIP_TRY(hipMemcpy(r->d_in.p, r->h_in.p, P.in_bytes, hipMemcpyHostToDevice));
      RefinePtrs p;
      p.groups = r->d_in.at<RefineGroup>(P.o_grp);
      p.cam_x = r->d_in.at<double>(P.o_cam);
      p.u = r->d_in.at<double>(P.o_u);
      p.cnt = r->d_in.at<int>(P.o_cnt);
      p.ob_cam = r->d_in.at<int>(P.o_oc);
      p.ob = r->d_in.at<double>(P.o_ob);
      p.ob_stride = P.nelem;
      p.out = r->d_out.at<RefineOut>(0);
      const Policy pol = make_policy(r->opt);
      hipLaunchKernelGGL(k_refine_lines, dim3((unsigned)P.ngroups), dim3(64), (size_t)lds_doubles_refine(P.maxC) * sizeof(double), 0, p, pol);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(r->h_out.p, r->d_out.p, P.out_bytes, hipMemcpyDeviceToHost));
    }
    refine_scatter(P, n, windows, reinterpret_cast<const RefineOut*>(r->h_out.p), results, totals);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

extern "C" int slslam_lba_refine_lines(const slslam_lba_window* window, const slslam_solver_options* opt, slslam_line_result* results,
                                       slslam_summary* total) {
  if (!window) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_line_refiner r;
  r.init(-1, opt, 0, 0);
  slslam_line_result* res[1] = { results };
  return slslam_line_refiner_run(&r, 1, window, results ? res : nullptr, total);
}

#endif

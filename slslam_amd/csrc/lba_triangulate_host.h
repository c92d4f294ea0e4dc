// slslam_amd/csrc/lba_triangulate_host.h — host side of the line triangulator (include/slslam_hip.h: slslam_line_triangulator_*,
// slslam_lba_triangulate_lines) without the device: the validation of a call, what the triangulator asks of the plan it shares with
// the refiner (line_call_plan.h: what becomes of every line, the lane-interleaved layout, the offsets), the upload image
// k_triangulate_lines reads (lba_triangulate.h) and the scatter of its records back under the caller's line numbering.
//
// Plain C++: no HIP here, so that this side is checked on its own (tests/host_cxx/triangulate_host_check.cpp, under the sanitizers).
// triangulate_api.hip adds the buffers, the copies and the launch.
#ifndef SLSLAM_LBA_TRIANGULATE_HOST_H_
#define SLSLAM_LBA_TRIANGULATE_HOST_H_

#include "line_call_plan.h"

namespace slslam {

enum { kTriCamTab = 13 };  // doubles per camera of the LDS table: R[9] t[3]; odd stride in 8-byte units, as the refiner's (kCandTab)
enum { kTriCamRec = 12 };  // doubles per camera in the upload: R[9] row-major | t[3]

struct TriOut {            // per line slot, written by the slot's lane
  double u[4];             // av_to_orth of the chosen line
  double av[6];            // the chosen line: closest point | direction
  double eig[4];           // descending; zeros unless status is SLSLAM_TRI_MULTIVIEW
  int status;              // SLSLAM_TRI_MULTIVIEW / _STEREO / _INVALID (a stereo-first line with v = 0 or a non-finite number)
  int num_planes;          // planes that entered the Gram matrix (method 1)
  int clamped;             // the stereo-first line was taken and its depth clamp fired
  int pad;
};

using TriPlan = LinePlan;

// A line that runs is SLSLAM_TRI_STEREO "for the device"; the kernel says which it became
inline LineCall tri_call() {
  return { { SLSLAM_TRI_STEREO, SLSLAM_TRI_CONSTANT, SLSLAM_TRI_NO_OBSERVATIONS, SLSLAM_TRI_INVALID }, false, false, kTriCamTab, kTriCamRec,
           sizeof(TriOut) };
}

// Every argument of a run, before anything is written or the device is asked.
inline int tri_validate(int n, const slslam_lba_window* windows, int method, double inverse_depth, double min_parallax) {
  if (method != 0 && method != 1) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!(min_parallax >= 0.0)) return SLSLAM_ERR_INVALID_ARGUMENT;                          // NaN or negative
  if (!std::isfinite(inverse_depth) || !(inverse_depth > 0.0)) return SLSLAM_ERR_INVALID_ARGUMENT;
  return line_validate_windows(n, windows);
}

inline int tri_plan_build(int n, const slslam_lba_window* windows, TriPlan* plan) { return line_plan_build(tri_call(), n, windows, plan); }

// The upload image, h[plan.in_bytes].  pose_to_Rt: (w, t)[6] -> R row-major | t [12] (slslam_gc::wt_to_Rt in the library).
inline void tri_fill_image(const TriPlan& P, int n, const slslam_lba_window* windows, void (*pose_to_Rt)(const double*, double*), char* h) {
  line_fill_common(P, n, windows, h);
  double* hc = reinterpret_cast<double*>(h + P.o_cam);
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    if (P.lay[(size_t)i].group_depth.empty()) continue;
    for (int c = 0; c < w.num_cameras; ++c) {
      const double* x = w.parameters + 6 * (size_t)c;
      if (finite_n(x, 6)) pose_to_Rt(x, hc + (P.cam_off[(size_t)i] + c) * kTriCamRec);      // (no line of the launch reads another)
    }
  }
}

// The records back under the caller's line numbering: only a MULTIVIEW / STEREO line's four doubles (and six of lines_av) are written.
inline void tri_scatter(const TriPlan& P, int n, const slslam_lba_window* windows, const TriOut* ho, slslam_triangulated_line* const* results,
                        double* const* lines_av) {
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const int C = w.num_cameras, L = w.num_lines;
    const int* st = P.status.data() + P.line_off[(size_t)i];
    slslam_triangulated_line* res = results ? results[i] : nullptr;
    double* av = lines_av ? lines_av[i] : nullptr;
    if (res) {
      std::memset(res, 0, sizeof(slslam_triangulated_line) * (size_t)L);
      for (int l = 0; l < L; ++l) res[l].first_camera = -1;
      for (int k = 0; k < w.num_observations; ++k) {
        slslam_triangulated_line& r = res[w.line_index[k]];
        if (r.num_observations++ == 0) r.first_camera = w.camera_index[k];
      }
    }
    for (int l = 0; l < L; ++l) {
      if (res) res[l].status = st[l];
      if (st[l] != SLSLAM_TRI_STEREO) continue;
      const TriOut& o = ho[P.slot_off[(size_t)i] + W.slot[(size_t)l]];
      if (res) res[l].status = o.status;
      if (o.status != SLSLAM_TRI_MULTIVIEW && o.status != SLSLAM_TRI_STEREO) continue;
      for (int a = 0; a < 4; ++a) w.parameters[6 * (size_t)C + 4 * (size_t)l + a] = o.u[a];
      if (av) for (int a = 0; a < 6; ++a) av[6 * (size_t)l + a] = o.av[a];
      if (res) {
        res[l].num_planes = o.num_planes;
        res[l].clamped = o.clamped;
        for (int a = 0; a < 4; ++a) res[l].eigenvalues[a] = o.eig[a];
      }
    }
  }
}

}  // namespace slslam
#endif

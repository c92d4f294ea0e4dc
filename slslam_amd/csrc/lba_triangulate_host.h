// slslam_amd/csrc/lba_triangulate_host.h — host side of the line triangulator (include/slslam_hip.h: slslam_line_triangulator_*,
// slslam_lba_triangulate_lines) without the device: the validation of a call, what becomes of every line (slslam::tri_plan_build - the
// lane-interleaved layout is the refiner's, lba_refine_layout.h, reused as it is), the upload image k_triangulate_lines reads
// (lba_triangulate.h) and the scatter of its records back under the caller's line numbering.
//
// Plain C++: no HIP here, so that this side is checked on its own (tests/host_cxx/triangulate_host_check.cpp, under the sanitizers).
// triangulate_api.hip adds the buffers, the copies and the launch.
#ifndef SLSLAM_LBA_TRIANGULATE_HOST_H_
#define SLSLAM_LBA_TRIANGULATE_HOST_H_

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/slslam_hip.h"
#include "lba_refine_layout.h"

namespace slslam {

enum { kTriCamTab = 13 };  // doubles per camera of the LDS table: R[9] t[3]; odd stride in 8-byte units, as the refiner's (kCandTab)
enum { kTriCamRec = 12 };  // doubles per camera in the upload: R[9] row-major | t[3]

struct TriGroup {          // one wave's work
  long long row_base;      // first row (64 observation slots) of the group
  int cam_off, C;          // the window's cameras in TriPtrs.cam
  int depth;               // rows of the group = observations of its longest line
  int pad;
};
struct TriOut {            // per line slot, written by the slot's lane
  double u[4];             // av_to_orth of the chosen line
  double av[6];            // the chosen line: closest point | direction
  double eig[4];           // descending; zeros unless status is SLSLAM_TRI_MULTIVIEW
  int status;              // SLSLAM_TRI_MULTIVIEW / _STEREO / _INVALID (a stereo-first line with v = 0 or a non-finite number)
  int num_planes;          // planes that entered the Gram matrix (method 1)
  int clamped;             // the stereo-first line was taken and its depth clamp fired
  int pad;
};

// Where everything of a call lies.  Upload: groups | cameras | counts | observation cameras | observations (4 planes of double2).
struct TriPlan {
  std::vector<RefineWindowLayout> lay;
  std::vector<unsigned char> run, cam_bad;          // work arrays of one window
  std::vector<int> status;                          // per line of the call: what the host knows before the device is asked
  std::vector<long long> line_off, slot_off, row_off, cam_off;
  long long ngroups = 0, nslot = 0, nrow = 0, nelem = 0, ncam = 0;
  int maxC = 0;
  size_t o_grp = 0, o_cam = 0, o_cnt = 0, o_oc = 0, o_ob = 0, in_bytes = 0, out_bytes = 0;
};

inline size_t tri_align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline bool tri_finite_n(const double* v, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

// Every argument of a run, before anything is written or the device is asked.
inline int tri_validate(int n, const slslam_lba_window* windows, int method, double inverse_depth, double min_parallax) {
  if (n < 0 || (n > 0 && !windows)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (method != 0 && method != 1) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!(min_parallax >= 0.0)) return SLSLAM_ERR_INVALID_ARGUMENT;                          // NaN or negative
  if (!std::isfinite(inverse_depth) || !(inverse_depth > 0.0)) return SLSLAM_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const int C = w.num_cameras, L = w.num_lines, M = w.num_observations;
    if (C < 0 || L < 0 || M < 0) return SLSLAM_ERR_INVALID_ARGUMENT;
    if (M > 0 && (!w.camera_index || !w.line_index || !w.fixed_index || !w.observations)) return SLSLAM_ERR_INVALID_ARGUMENT;
    if ((C > 0 || L > 0) && !w.parameters) return SLSLAM_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < M; ++k)
      if (w.camera_index[k] < 0 || w.camera_index[k] >= C || w.line_index[k] < 0 || w.line_index[k] >= L) return SLSLAM_ERR_INVALID_ARGUMENT;
  }
  return SLSLAM_OK;
}

// What becomes of every line (the refiner's rules: one flagged observation makes the line constant, reference src/lba_problem.cpp:88-91;
// the camera flags are ignored; a non-finite observation or camera makes the lines that see it invalid), the layout of every window and
// the offsets of the upload.  SLSLAM_ERR_UNSUPPORTED beyond the refiner's limits.  The windows have passed tri_validate.
inline int tri_plan_build(int n, const slslam_lba_window* windows, TriPlan* plan) {
  TriPlan& P = *plan;
  P.lay.resize((size_t)n);
  P.line_off.assign((size_t)n + 1, 0); P.slot_off.assign((size_t)n + 1, 0);
  P.row_off.assign((size_t)n + 1, 0); P.cam_off.assign((size_t)n + 1, 0);
  P.maxC = 0;
  for (int i = 0; i < n; ++i) {
    P.line_off[(size_t)i + 1] = P.line_off[(size_t)i] + windows[i].num_lines;
    if (windows[i].num_cameras > P.maxC) P.maxC = windows[i].num_cameras;
  }
  if ((size_t)P.maxC * kTriCamTab * sizeof(double) > 64 * 1024) return SLSLAM_ERR_UNSUPPORTED;   // a window's camera table lives in LDS (630 cameras)
  P.status.assign((size_t)P.line_off[(size_t)n], SLSLAM_TRI_NO_OBSERVATIONS);
  P.ngroups = 0;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const int C = w.num_cameras, L = w.num_lines, M = w.num_observations;
    int* st = P.status.data() + P.line_off[(size_t)i];
    P.cam_bad.assign((size_t)C, 0);
    for (int c = 0; c < C; ++c) P.cam_bad[(size_t)c] = tri_finite_n(w.parameters + 6 * (size_t)c, 6) ? 0 : 1;
    for (int k = 0; k < M; ++k) {
      const int l = w.line_index[k];
      if (w.fixed_index[2 * (size_t)k + 1]) st[l] = SLSLAM_TRI_CONSTANT;
      else if (st[l] == SLSLAM_TRI_NO_OBSERVATIONS) st[l] = SLSLAM_TRI_STEREO;              // "for the device"; the kernel says which
    }
    for (int k = 0; k < M; ++k) {
      const int l = w.line_index[k];
      if (st[l] == SLSLAM_TRI_STEREO && (P.cam_bad[(size_t)w.camera_index[k]] || !tri_finite_n(w.observations + 8 * (size_t)k, 8)))
        st[l] = SLSLAM_TRI_INVALID;
    }
    P.run.assign((size_t)L, 0);
    for (int l = 0; l < L; ++l) P.run[(size_t)l] = st[l] == SLSLAM_TRI_STEREO;
    RefineWindowLayout& W = P.lay[(size_t)i];
    refine_layout_build(L, M, w.line_index, P.run.data(), &W);
    P.ngroups += (long long)W.group_depth.size();
    P.slot_off[(size_t)i + 1] = P.ngroups * kRefineLanes;
    P.row_off[(size_t)i + 1] = P.row_off[(size_t)i] + W.rows;
    P.cam_off[(size_t)i + 1] = P.cam_off[(size_t)i] + C;
  }
  P.nslot = P.ngroups * kRefineLanes; P.nrow = P.row_off[(size_t)n]; P.nelem = P.nrow * kRefineLanes; P.ncam = P.cam_off[(size_t)n];
  if (P.ngroups > 0x7fffffffLL || P.ncam > 0x7fffffffLL) return SLSLAM_ERR_UNSUPPORTED;
  P.o_grp = 0;
  P.o_cam = tri_align256(P.o_grp + (size_t)P.ngroups * sizeof(TriGroup));
  P.o_cnt = tri_align256(P.o_cam + (size_t)P.ncam * kTriCamRec * sizeof(double));
  P.o_oc = tri_align256(P.o_cnt + (size_t)P.nslot * sizeof(int));
  P.o_ob = tri_align256(P.o_oc + (size_t)P.nelem * sizeof(int));
  P.in_bytes = P.o_ob + (size_t)P.nelem * 64;
  P.out_bytes = (size_t)P.nslot * sizeof(TriOut);
  return SLSLAM_OK;
}

// The upload image, h[plan.in_bytes].  pose_to_Rt: (w, t)[6] -> R row-major | t [12] (slslam_gc::wt_to_Rt in the library).
inline void tri_fill_image(const TriPlan& P, int n, const slslam_lba_window* windows, void (*pose_to_Rt)(const double*, double*), char* h) {
  std::memset(h, 0, P.in_bytes);
  TriGroup* hg = reinterpret_cast<TriGroup*>(h + P.o_grp);
  double* hc = reinterpret_cast<double*>(h + P.o_cam);
  int* hn = reinterpret_cast<int*>(h + P.o_cnt);
  int* hoc = reinterpret_cast<int*>(h + P.o_oc);
  double* hob = reinterpret_cast<double*>(h + P.o_ob);
  long long g0 = 0;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const int C = w.num_cameras, M = w.num_observations;
    if (!W.group_depth.empty())
      for (int c = 0; c < C; ++c) {
        const double* x = w.parameters + 6 * (size_t)c;
        if (tri_finite_n(x, 6)) pose_to_Rt(x, hc + (P.cam_off[(size_t)i] + c) * kTriCamRec);      // (no line of the launch reads another)
      }
    for (size_t g = 0; g < W.group_depth.size(); ++g) {
      TriGroup& G = hg[g0 + (long long)g];
      G.row_base = P.row_off[(size_t)i] + W.group_row[g];
      G.cam_off = (int)P.cam_off[(size_t)i]; G.C = C; G.depth = W.group_depth[g]; G.pad = 0;
    }
    const long long s0 = P.slot_off[(size_t)i];
    for (size_t s = 0; s < W.order.size(); ++s) hn[s0 + (long long)s] = W.count[(size_t)W.order[s]];
    const long long e0 = P.row_off[(size_t)i] * kRefineLanes;
    for (int k = 0; k < M; ++k) {
      const long long d = W.dest[(size_t)k];
      if (d < 0) continue;
      const long long e = e0 + d;
      hoc[e] = w.camera_index[k];
      for (int q = 0; q < 4; ++q) {
        hob[((long long)q * P.nelem + e) * 2] = w.observations[8 * (size_t)k + 2 * q];
        hob[((long long)q * P.nelem + e) * 2 + 1] = w.observations[8 * (size_t)k + 2 * q + 1];
      }
    }
    g0 += (long long)W.group_depth.size();
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

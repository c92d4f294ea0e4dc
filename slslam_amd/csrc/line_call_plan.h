// slslam_amd/csrc/line_call_plan.h — the host plan the line refiner (lba_refine_host.h) and the line triangulator
// (lba_triangulate_host.h) share: the window checks, the one classification of a line, the waves of 64 (lba_refine_layout.h), the
// prefix arrays over the windows, the offsets of the upload image, the part of the image both kernels read alike and the capacity
// rule of the handles.  What differs between the two calls is a LineCall; each keeps its own camera fill, records and scatter.
// Plain C++, no HIP: checked on the host under the sanitizers (tests/host_cxx/refine_host_check.cpp, triangulate_host_check.cpp).
#ifndef SLSLAM_LINE_CALL_PLAN_H_
#define SLSLAM_LINE_CALL_PLAN_H_

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_layout.h"
#include "lba_refine_layout.h"

namespace slslam {

struct LineGroup {         // one wave's work
  long long row_base;      // first row (64 observation slots) of the group
  int cam_off, C;          // the window's cameras in the call's camera array
  int depth;               // rows of the group = observations of its longest line
  int pad;
};
using RefineGroup = LineGroup;   // (the names the two kernels read it under)
using TriGroup = LineGroup;

enum LineFate { kLineRun = 0, kLineConstant, kLineNoObservations, kLineInvalid };

// What differs between the two calls
struct LineCall {
  int name[4];             // the ABI constant of each LineFate: SLSLAM_LINE_* or SLSLAM_TRI_*
  bool finite_start;       // a line that runs also needs four finite start values
  bool has_u;              // the image has the start values u [nslot][4]
  int cam_tab;             // doubles per camera of the kernel's LDS table (the 64 KiB limit)
  int cam_rec;             // doubles per camera in the image
  size_t out_rec;          // bytes of the record a line slot downloads
};

// Where everything of a call lies.  Upload: groups | cameras | u (if the call has it) | counts | observation cameras | observations (4
// planes of double2).
struct LinePlan {
  std::vector<RefineWindowLayout> lay;
  std::vector<unsigned char> run, cam_bad;          // work arrays of one window
  std::vector<int> status;                          // per line of the call, in the call's ABI constants: what the host knows before the device is asked
  std::vector<long long> line_off, slot_off, row_off, cam_off;
  long long ngroups = 0, nslot = 0, nrow = 0, nelem = 0, ncam = 0;
  int maxC = 0;
  size_t o_grp = 0, o_cam = 0, o_u = 0, o_cnt = 0, o_oc = 0, o_ob = 0, in_bytes = 0, out_bytes = 0;
};

inline bool finite_n(const double* v, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

// The windows of a run, before anything is written or the device is asked.
inline int line_validate_windows(int n, const slslam_lba_window* windows) {
  if (n < 0 || (n > 0 && !windows)) return SLSLAM_ERR_INVALID_ARGUMENT;
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

// What becomes of every line (one flagged observation makes the line constant: the packer's rule, reference src/lba_problem.cpp:88-91;
// the camera flags are ignored; a non-finite observation or camera makes the lines that see it invalid, and so do non-finite start
// values where the call reads them), the layout of every window and the offsets of the upload.  SLSLAM_ERR_UNSUPPORTED beyond the
// limits: a window's camera table lives in LDS (630 cameras), groups and cameras are counted in ints.  The windows have passed
// line_validate_windows.
inline int line_plan_build(const LineCall& call, int n, const slslam_lba_window* windows, LinePlan* plan) {
  LinePlan& P = *plan;
  const int run = call.name[kLineRun];
  P.lay.resize((size_t)n);
  P.line_off.assign((size_t)n + 1, 0); P.slot_off.assign((size_t)n + 1, 0);
  P.row_off.assign((size_t)n + 1, 0); P.cam_off.assign((size_t)n + 1, 0);
  P.maxC = 0;
  for (int i = 0; i < n; ++i) {
    P.line_off[(size_t)i + 1] = P.line_off[(size_t)i] + windows[i].num_lines;
    if (windows[i].num_cameras > P.maxC) P.maxC = windows[i].num_cameras;
  }
  if ((size_t)P.maxC * (size_t)call.cam_tab * sizeof(double) > 64 * 1024) return SLSLAM_ERR_UNSUPPORTED;
  P.status.assign((size_t)P.line_off[(size_t)n], call.name[kLineNoObservations]);
  P.ngroups = 0;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const int C = w.num_cameras, L = w.num_lines, M = w.num_observations;
    int* st = P.status.data() + P.line_off[(size_t)i];
    P.cam_bad.assign((size_t)C, 0);
    for (int c = 0; c < C; ++c) P.cam_bad[(size_t)c] = finite_n(w.parameters + 6 * (size_t)c, 6) ? 0 : 1;
    for (int k = 0; k < M; ++k) {
      const int l = w.line_index[k];
      if (w.fixed_index[2 * (size_t)k + 1]) st[l] = call.name[kLineConstant];
      else if (st[l] == call.name[kLineNoObservations]) st[l] = run;
    }
    for (int k = 0; k < M; ++k) {
      const int l = w.line_index[k];
      if (st[l] == run && (P.cam_bad[(size_t)w.camera_index[k]] || !finite_n(w.observations + 8 * (size_t)k, 8)))
        st[l] = call.name[kLineInvalid];
    }
    P.run.assign((size_t)L, 0);
    for (int l = 0; l < L; ++l) {
      if (call.finite_start && st[l] == run && !finite_n(w.parameters + 6 * (size_t)C + 4 * (size_t)l, 4)) st[l] = call.name[kLineInvalid];
      P.run[(size_t)l] = st[l] == run;
    }
    RefineWindowLayout& W = P.lay[(size_t)i];
    refine_layout_build(L, M, w.line_index, P.run.data(), &W);
    P.ngroups += (long long)W.group_depth.size();
    P.slot_off[(size_t)i + 1] = P.ngroups * kRefineLanes;
    P.row_off[(size_t)i + 1] = P.row_off[(size_t)i] + W.rows;
    P.cam_off[(size_t)i + 1] = P.cam_off[(size_t)i] + C;
  }
  P.nslot = P.ngroups * kRefineLanes; P.nrow = P.row_off[(size_t)n]; P.nelem = P.nrow * kRefineLanes; P.ncam = P.cam_off[(size_t)n];
  if (P.ngroups > 0x7fffffffLL || P.ncam > 0x7fffffffLL) return SLSLAM_ERR_UNSUPPORTED;
  Carve c;
  P.o_grp = c.take((size_t)P.ngroups * sizeof(LineGroup));
  P.o_cam = c.take((size_t)P.ncam * (size_t)call.cam_rec * sizeof(double));
  P.o_u = c.take(call.has_u ? (size_t)P.nslot * 4 * sizeof(double) : 0);
  P.o_cnt = c.take((size_t)P.nslot * sizeof(int));
  P.o_oc = c.take((size_t)P.nelem * sizeof(int));
  P.o_ob = c.take((size_t)P.nelem * 64);
  P.in_bytes = c.at;                                // (an element's 64 bytes x 64 lanes per row: the last region ends on a multiple of 256)
  P.out_bytes = (size_t)P.nslot * call.out_rec;
  return SLSLAM_OK;
}

// The image h[plan.in_bytes], zeroed, with what both kernels read alike: groups, counts, observation cameras and the four observation
// planes.  The cameras (and u) are the caller's to add.
inline void line_fill_common(const LinePlan& P, int n, const slslam_lba_window* windows, char* h) {
  std::memset(h, 0, P.in_bytes);
  LineGroup* hg = reinterpret_cast<LineGroup*>(h + P.o_grp);
  int* hn = reinterpret_cast<int*>(h + P.o_cnt);
  int* hoc = reinterpret_cast<int*>(h + P.o_oc);
  double* hob = reinterpret_cast<double*>(h + P.o_ob);
  long long g0 = 0;
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = windows[i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    for (size_t g = 0; g < W.group_depth.size(); ++g) {
      LineGroup& G = hg[g0 + (long long)g];
      G.row_base = P.row_off[(size_t)i] + W.group_row[g];
      G.cam_off = (int)P.cam_off[(size_t)i]; G.C = w.num_cameras; G.depth = W.group_depth[g]; G.pad = 0;
    }
    const long long s0 = P.slot_off[(size_t)i];
    for (size_t s = 0; s < W.order.size(); ++s) hn[s0 + (long long)s] = W.count[(size_t)W.order[s]];
    const long long e0 = P.row_off[(size_t)i] * kRefineLanes;
    for (int k = 0; k < w.num_observations; ++k) {
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

// What a handle made for max_lines and max_observations holds from its first run: whole waves per window, rows padded to a group's
// longest line (the cameras of a call are not known at create and are not counted)
inline void line_capacity_bytes(const LineCall& call, long long max_lines, long long max_observations, size_t* cap_in, size_t* cap_out) {
  const size_t cap_slot = (size_t)((max_lines + kRefineLanes - 1) / kRefineLanes * kRefineLanes);
  const size_t cap_elem = (size_t)((max_observations + kRefineLanes - 1) / kRefineLanes * kRefineLanes);
  *cap_in = 5 * 256 + (cap_slot / kRefineLanes) * sizeof(LineGroup) + cap_slot * (call.has_u ? 36 : 4) + cap_elem * 68;
  *cap_out = cap_slot * call.out_rec;
}

}  // namespace slslam
#endif

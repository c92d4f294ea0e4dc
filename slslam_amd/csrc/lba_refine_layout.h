// slslam_amd/csrc/lba_refine_layout.h — where the lines and observations of a window go for k_refine_lines (lba_refine_lines.h).
//
// The kernel runs lane <-> line: a wave takes 64 lines of one window and every lane walks its own line's observations.  A CSR list
// per line would make "observation j of every lane" 64 scattered reads, so the observations of a group of 64 lines are stored
// lane-interleaved: observation j of the line in lane i sits at element (group_row + j) * 64 + i of every observation array - one
// contiguous row per j.  A group is padded to its longest line, so the lines are first sorted by observation count (descending, stable:
// a counting sort) - the lanes of a wave then have similar trip counts and the padding of a window is bounded by 126 x its longest line.
// A line's observations keep the caller's order (the sum over them is then the sum a one-line problem makes).
//
// Plain C++: no HIP here, so that the host side is checked on its own (tests/host_cxx/refine_layout_check.cpp, under the sanitizers).
#ifndef SLSLAM_LBA_REFINE_LAYOUT_H_
#define SLSLAM_LBA_REFINE_LAYOUT_H_

#include <cstddef>
#include <vector>

namespace slslam {

enum { kRefineLanes = 64 };

struct RefineWindowLayout {
  std::vector<int> count;            // [L] observations of a refined line; 0 for a line that is not refined
  std::vector<int> order;            // the refined lines, most observations first (ties: the caller's order)
  std::vector<int> slot;             // [L] position in `order` (group = slot / 64, lane = slot % 64), -1: not refined
  std::vector<int> group_depth;      // per group: observations of its longest line = rows of the group
  std::vector<long long> group_row;  // per group: its first row, relative to the window's first row
  std::vector<long long> dest;       // [M] element (row * 64 + lane, relative to the window's first row) of observation i; -1: its line is not refined
  long long rows = 0;                // rows of the window (64 elements each)
  std::vector<int> fill, bucket;     // work arrays (kept for their capacity)
};

// line_index[M] must lie in [0, L) (the caller has checked); refine[L]: 1 = the line is refined.
inline void refine_layout_build(int L, int M, const int* line_index, const unsigned char* refine, RefineWindowLayout* out) {
  RefineWindowLayout& W = *out;
  W.count.assign((size_t)L, 0);
  W.slot.assign((size_t)L, -1);
  W.order.clear(); W.group_depth.clear(); W.group_row.clear();
  W.dest.assign((size_t)M, -1);
  W.rows = 0;
  int longest = 0, nref = 0;
  for (int i = 0; i < M; ++i) {
    const int l = line_index[i];
    if (refine[l]) { const int c = ++W.count[(size_t)l]; if (c > longest) longest = c; }
  }
  // counting sort by descending count; a refined line has at least one observation
  W.bucket.assign((size_t)longest + 2, 0);
  for (int l = 0; l < L; ++l) if (W.count[(size_t)l] > 0) { ++W.bucket[(size_t)(longest - W.count[(size_t)l]) + 1]; ++nref; }
  for (int k = 0; k <= longest; ++k) W.bucket[(size_t)k + 1] += W.bucket[(size_t)k];
  W.order.assign((size_t)nref, -1);
  for (int l = 0; l < L; ++l) {
    if (W.count[(size_t)l] == 0) continue;
    const int s = W.bucket[(size_t)(longest - W.count[(size_t)l])]++;
    W.order[(size_t)s] = l;
    W.slot[(size_t)l] = s;
  }
  const int ngroups = (nref + kRefineLanes - 1) / kRefineLanes;
  for (int g = 0; g < ngroups; ++g) {
    const int depth = W.count[(size_t)W.order[(size_t)g * kRefineLanes]];     // the group's first line is its longest
    W.group_depth.push_back(depth);
    W.group_row.push_back(W.rows);
    W.rows += depth;
  }
  W.fill.assign((size_t)L, 0);
  for (int i = 0; i < M; ++i) {
    const int l = line_index[i], s = W.slot[(size_t)l];
    if (s < 0) continue;
    const int j = W.fill[(size_t)l]++;
    W.dest[(size_t)i] = (W.group_row[(size_t)(s / kRefineLanes)] + j) * kRefineLanes + s % kRefineLanes;
  }
}

}  // namespace slslam
#endif

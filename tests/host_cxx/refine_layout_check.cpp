// tests/host_cxx/refine_layout_check.cpp — the lane-interleaved layout of the structure-only refinement (slslam_amd/csrc/lba_refine_layout.h)
// on a few hand-made windows: every observation of a refined line lands exactly once, in its line's lane, in the caller's order; lines
// are sorted by observation count; a group has the rows of its longest line.  Built with -fsanitize=address,undefined and run by
// tests/test_refine_lines_cpu.py.  Prints "refine layout ok" and exits 0, or says what is wrong and exits 1.
#include <cstdio>
#include <vector>

#include "../../slslam_amd/csrc/lba_refine_layout.h"

using slslam::RefineWindowLayout;
using slslam::kRefineLanes;

static int check(const char* name, int L, const std::vector<int>& line_index, const std::vector<unsigned char>& refine) {
  const int M = (int)line_index.size();
  RefineWindowLayout W;
  slslam::refine_layout_build(L, M, line_index.data(), refine.data(), &W);
#define FAIL(...) do { std::printf("%s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)
  std::vector<int> want(L, 0);
  for (int i = 0; i < M; ++i) if (refine[line_index[i]]) ++want[line_index[i]];
  int nref = 0;
  for (int l = 0; l < L; ++l) {
    if (W.count[l] != want[l]) FAIL("line %d count %d, expected %d", l, W.count[l], want[l]);
    if ((want[l] > 0) != (W.slot[l] >= 0)) FAIL("line %d slot %d with %d observations", l, W.slot[l], want[l]);
    if (want[l] > 0) ++nref;
  }
  if ((int)W.order.size() != nref) FAIL("%zu lines in order, expected %d", W.order.size(), nref);
  for (int s = 0; s < nref; ++s) {
    if (W.slot[W.order[s]] != s) FAIL("slot of order[%d]", s);
    if (s > 0 && W.count[W.order[s]] > W.count[W.order[s - 1]]) FAIL("order not by descending count at %d", s);
    if (s > 0 && W.count[W.order[s]] == W.count[W.order[s - 1]] && W.order[s] < W.order[s - 1]) FAIL("sort not stable at %d", s);
  }
  const int ngroups = (nref + kRefineLanes - 1) / kRefineLanes;
  if ((int)W.group_depth.size() != ngroups || (int)W.group_row.size() != ngroups) FAIL("%zu groups, expected %d", W.group_depth.size(), ngroups);
  long long rows = 0;
  for (int g = 0; g < ngroups; ++g) {
    if (W.group_row[g] != rows) FAIL("group %d starts at row %lld, expected %lld", g, W.group_row[g], rows);
    int longest = 0;
    for (int s = g * kRefineLanes; s < nref && s < (g + 1) * kRefineLanes; ++s) if (W.count[W.order[s]] > longest) longest = W.count[W.order[s]];
    if (W.group_depth[g] != longest) FAIL("group %d depth %d, longest line %d", g, W.group_depth[g], longest);
    rows += longest;
  }
  if (W.rows != rows) FAIL("rows %lld, expected %lld", W.rows, rows);
  std::vector<int> hits((size_t)rows * kRefineLanes, 0), seen(L, 0);
  for (int i = 0; i < M; ++i) {
    const int l = line_index[i];
    const long long d = W.dest[i];
    if (!refine[l]) { if (d != -1) FAIL("observation %d of a line that is not refined has a place", i); continue; }
    if (d < 0 || d >= rows * kRefineLanes) FAIL("observation %d out of range: %lld", i, d);
    const int s = W.slot[l], g = s / kRefineLanes;
    if (d % kRefineLanes != s % kRefineLanes) FAIL("observation %d in lane %lld, line's lane %d", i, d % kRefineLanes, s % kRefineLanes);
    if (d / kRefineLanes != W.group_row[g] + seen[l]) FAIL("observation %d in row %lld, expected %lld", i, d / kRefineLanes, W.group_row[g] + seen[l]);
    ++seen[l];
    if (++hits[(size_t)d] != 1) FAIL("element %lld taken twice", d);
  }
  long long placed = 0, expect = 0;
  for (int v : hits) placed += v;
  for (int l = 0; l < L; ++l) expect += want[l];
  if (placed != expect) FAIL("%lld observations placed, expected %lld", placed, expect);
  return 0;
#undef FAIL
}

int main() {
  int bad = 0;
  {  // nothing at all
    bad += check("empty", 0, {}, {});
  }
  {  // lines without observations, a line that is not refined
    std::vector<int> li = { 4, 1, 4, 4, 1, 6 };
    std::vector<unsigned char> rf = { 1, 1, 1, 1, 1, 1, 0, 1 };
    bad += check("empty lines", 8, li, rf);
  }
  {  // 65 lines: a second group of one line; counts 1 .. 5, interleaved
    std::vector<int> li;
    for (int rep = 0; rep < 5; ++rep)
      for (int l = 64; l >= 0; --l) if (rep <= l % 5) li.push_back(l);
    bad += check("65 lines", 65, li, std::vector<unsigned char>(65, 1));
  }
  {  // a line with 64 observations among short ones
    std::vector<int> li;
    for (int k = 0; k < 64; ++k) { li.push_back(2); if (k % 9 == 0) li.push_back(k % 4); }
    bad += check("64 observations", 5, li, std::vector<unsigned char>(5, 1));
  }
  {  // 200 lines, every third one not refined
    std::vector<int> li;
    std::vector<unsigned char> rf(200);
    for (int l = 0; l < 200; ++l) { rf[l] = l % 3 != 0; for (int k = 0; k < 1 + (l * 7) % 11; ++k) li.push_back(l); }
    bad += check("200 lines", 200, li, rf);
  }
  if (bad) return 1;
  std::printf("refine layout ok\n");
  return 0;
}

// tests/host_cxx/refine_host_check.cpp — the host side of the structure-only refinement (slslam_amd/csrc/lba_refine_host.h over
// line_call_plan.h) without a device: what becomes of every line, the upload image (every observation of a line that runs lands once,
// in its line's lane, in the caller's order; counts, groups, cameras as (w, t) with non-finite numbers as 0, the caller's four start
// values per slot) and the scatter of hand-made records back under the caller's numbering with the totals of every window -
// untouched bytes stay untouched.  Built with -fsanitize=address,undefined and run by tests/test_refine_lines_cpu.py.  Prints
// "refine host ok" and exits 0, or says what is wrong and exits 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/lba_refine_host.h"

using namespace slslam;

#define FAIL(...) do { std::printf("%s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const LineCall kCall = refine_call(13);

struct Window {
  int C = 0, L = 0;
  std::vector<int> cam, line, fixed;
  std::vector<double> obs, prm;
  slslam_lba_window c() {
    slslam_lba_window w;
    w.num_cameras = C; w.num_lines = L; w.num_observations = (int)cam.size();
    w.camera_index = cam.data(); w.line_index = line.data(); w.fixed_index = fixed.data();
    w.observations = obs.data(); w.parameters = prm.data();
    return w;
  }
};

// line l gets 1 + (l * 7) % 5 observations, cameras round robin, the lines interleaved; observation k holds 100 k + q in its q-th
// double, parameter i is 0.001 i
Window make(int C, int L) {
  Window w;
  w.C = C; w.L = L;
  for (int rep = 0; rep < 5; ++rep)
    for (int l = 0; l < L; ++l)
      if (rep < 1 + (l * 7) % 5) {
        const int k = (int)w.cam.size();
        w.cam.push_back((l + rep) % C); w.line.push_back(l); w.fixed.push_back(0); w.fixed.push_back(0);
        for (int q = 0; q < 8; ++q) w.obs.push_back(100.0 * k + q);
      }
  for (int i = 0; i < 6 * C + 4 * L; ++i) w.prm.push_back(0.001 * i);
  return w;
}

bool same_bytes(const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }

// The termination of a hand-made record: mostly FUNCTION_TOLERANCE; `flavour` decides which lines cap or fail
int termination_of(int flavour, int l) {
  if (flavour >= 1 && l % 5 == 1) return SLSLAM_NO_CONVERGENCE;
  if (flavour == 2 && l % 9 == 4) return SLSLAM_NUMERICAL_FAILURE;
  return l % 3 == 0 ? SLSLAM_PARAMETER_TOLERANCE : SLSLAM_FUNCTION_TOLERANCE;
}

// want[i]: the status the call must give line by line (hand-written by the caller of this check), or empty: derived by the rules
int check_call(const char* name, std::vector<Window>& ws, const std::vector<std::vector<int>>& want = {}) {
  const int n = (int)ws.size();
  std::vector<slslam_lba_window> cw;
  for (Window& w : ws) cw.push_back(w.c());
  if (line_validate_windows(n, cw.data()) != SLSLAM_OK) FAIL("refused");
  LinePlan P;
  if (line_plan_build(kCall, n, cw.data(), &P) != SLSLAM_OK) FAIL("no plan");
  if (P.out_bytes != (size_t)P.nslot * sizeof(RefineOut)) FAIL("out_bytes");
  std::vector<char> img(P.in_bytes + 1, 0x5a);
  refine_fill_image(P, n, cw.data(), img.data());
  if (img[P.in_bytes] != 0x5a) FAIL("the image was overrun");
  const LineGroup* hg = reinterpret_cast<const LineGroup*>(img.data() + P.o_grp);
  const double* hc = reinterpret_cast<const double*>(img.data() + P.o_cam);
  const double* hu = reinterpret_cast<const double*>(img.data() + P.o_u);
  const int* hn = reinterpret_cast<const int*>(img.data() + P.o_cnt);
  const int* hoc = reinterpret_cast<const int*>(img.data() + P.o_oc);
  const double* hob = reinterpret_cast<const double*>(img.data() + P.o_ob);
  if (P.o_grp != 0 || P.o_cam % 256 || P.o_u % 256 || P.o_cnt % 256 || P.o_oc % 256 || P.o_ob % 256) FAIL("a block of the image is not 256-byte aligned");
  if (!(P.o_cam <= P.o_u && P.o_u <= P.o_cnt && P.o_cnt <= P.o_oc && P.o_oc <= P.o_ob && P.o_ob <= P.in_bytes)) FAIL("the blocks are out of order");
  if (P.o_u + (size_t)P.nslot * 32 > P.o_cnt || P.o_cam + (size_t)P.ncam * 48 > P.o_u) FAIL("two blocks overlap");

  std::vector<RefineOut> out((size_t)P.nslot);
  std::vector<std::vector<int>> nobs((size_t)n);
  std::vector<int> used((size_t)P.nelem, 0);
  long long g = 0;
  for (int i = 0; i < n; ++i) {
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const slslam_lba_window& w = cw[(size_t)i];
    std::vector<int> expect((size_t)w.num_lines, SLSLAM_LINE_NO_OBSERVATIONS);
    nobs[(size_t)i].assign((size_t)w.num_lines, 0);
    for (int k = 0; k < w.num_observations; ++k) {
      const int l = w.line_index[k];
      ++nobs[(size_t)i][(size_t)l];
      bool bad = false;
      for (int q = 0; q < 8; ++q) bad = bad || !std::isfinite(w.observations[8 * k + q]);
      for (int q = 0; q < 6; ++q) bad = bad || !std::isfinite(w.parameters[6 * w.camera_index[k] + q]);
      for (int q = 0; q < 4; ++q) bad = bad || !std::isfinite(w.parameters[6 * w.num_cameras + 4 * l + q]);
      int& s = expect[(size_t)l];
      if (w.fixed_index[2 * k + 1]) s = SLSLAM_LINE_CONSTANT;
      else if (s == SLSLAM_LINE_NO_OBSERVATIONS) s = bad ? SLSLAM_LINE_INVALID : SLSLAM_LINE_REFINED;
      else if (s == SLSLAM_LINE_REFINED && bad) s = SLSLAM_LINE_INVALID;
    }
    if (!want.empty() && want[(size_t)i] != expect) FAIL("window %d: the check's own rules do not give the hand-written fates", i);
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = P.status[(size_t)(P.line_off[(size_t)i] + l)];
      if (s != expect[(size_t)l]) FAIL("window %d line %d: status %d, expected %d", i, l, s, expect[(size_t)l]);
      if ((s == SLSLAM_LINE_REFINED) != (W.slot[(size_t)l] >= 0)) FAIL("window %d line %d: slot %d with status %d", i, l, W.slot[(size_t)l], s);
    }
    for (size_t q = 0; q < W.group_depth.size(); ++q, ++g) {
      const LineGroup& G = hg[g];
      if (G.row_base != P.row_off[(size_t)i] + W.group_row[q] || G.depth != W.group_depth[q] || G.C != w.num_cameras ||
          G.cam_off != (int)P.cam_off[(size_t)i] || G.pad != 0) FAIL("window %d group %zu", i, q);
      if ((G.row_base + G.depth) * kRefineLanes > P.nelem) FAIL("window %d group %zu reads beyond the observations", i, q);
      if ((long long)G.cam_off + G.C > P.ncam) FAIL("window %d group %zu reads beyond the cameras", i, q);
    }
    // cameras: (w, t) as the caller has them, a non-finite number as 0
    for (int c = 0; c < 6 * w.num_cameras; ++c) {
      const double v = w.parameters[c], got = hc[P.cam_off[(size_t)i] * 6 + c];
      if (got != (std::isfinite(v) ? v : 0.0)) FAIL("window %d camera double %d: %g", i, c, got);
    }
    std::vector<int> seen((size_t)w.num_lines, 0);
    for (int k = 0; k < w.num_observations; ++k) {
      const int l = w.line_index[k], s = W.slot[(size_t)l];
      if (s < 0) continue;
      const long long slot = P.slot_off[(size_t)i] + s;
      const LineGroup& G = hg[slot / kRefineLanes];
      if (seen[(size_t)l] >= G.depth) FAIL("window %d line %d is longer than its group", i, l);
      const long long e = (G.row_base + seen[(size_t)l]++) * kRefineLanes + slot % kRefineLanes;
      if (used[(size_t)e]++) FAIL("window %d observation %d: its element is taken twice", i, k);
      if (hoc[e] != w.camera_index[k]) FAIL("window %d observation %d: camera", i, k);
      for (int q = 0; q < 8; ++q)
        if (hob[((long long)(q / 2) * P.nelem + e) * 2 + q % 2] != w.observations[8 * k + q]) FAIL("window %d observation %d: double %d", i, k, q);
    }
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = W.slot[(size_t)l];
      if (s < 0) continue;
      const long long slot = P.slot_off[(size_t)i] + s;
      if (hn[slot] != nobs[(size_t)i][(size_t)l] || seen[(size_t)l] != hn[slot]) FAIL("window %d line %d: count %d, expected %d", i, l, hn[slot], nobs[(size_t)i][(size_t)l]);
      for (int a = 0; a < 4; ++a)
        if (hu[slot * 4 + a] != w.parameters[6 * w.num_cameras + 4 * l + a]) FAIL("window %d line %d: start value %d", i, l, a);
      RefineOut& o = out[(size_t)slot];
      o.termination = termination_of(i % 3, l);
      o.n_success = 1 + l % 4; o.n_unsuccess = l % 3; o.pad = 0;
      o.initial_cost = 2.0 + l; o.final_cost = 0.5 + 0.25 * l;
      for (int a = 0; a < 4; ++a) o.u[a] = 1000.0 * (i + 1) + l + 0.125 * a;
    }
  }
  if (g != P.ngroups) FAIL("%lld groups, expected %lld", g, P.ngroups);
  // what no line owns is zero: unused slots (count 0, u 0) and the padding of the observation rows
  long long nused = 0;
  for (int i = 0; i < n; ++i) {
    nused += (long long)P.lay[(size_t)i].order.size();
    for (long long s = P.slot_off[(size_t)i] + (long long)P.lay[(size_t)i].order.size(); s < P.slot_off[(size_t)i + 1]; ++s)
      if (hn[s] != 0 || hu[4 * s] != 0.0 || hu[4 * s + 3] != 0.0) FAIL("window %d: an unused slot is not zero", i);
  }
  for (long long e = 0; e < P.nelem; ++e)
    if (!used[(size_t)e] && (hoc[e] != 0 || hob[2 * e] != 0.0 || hob[(3 * P.nelem + e) * 2 + 1] != 0.0)) FAIL("padding element %lld is not zero", e);

  // ---- the scatter: results of window 0 are not asked for (when there is more than one window); totals always
  std::vector<std::vector<slslam_line_result>> res((size_t)n);
  std::vector<std::vector<double>> before((size_t)n);
  std::vector<slslam_line_result*> rp((size_t)n, nullptr);
  std::vector<slslam_summary> tot((size_t)n + 1);
  std::memset(tot.data(), 0x5a, sizeof(slslam_summary) * tot.size());
  const slslam_summary guard = tot[(size_t)n];
  for (int i = 0; i < n; ++i) {
    res[(size_t)i].resize((size_t)cw[(size_t)i].num_lines);
    before[(size_t)i] = ws[(size_t)i].prm;
    if (i > 0 || n == 1) rp[(size_t)i] = res[(size_t)i].data();
  }
  const std::vector<Window> inputs = ws;
  refine_scatter(P, n, cw.data(), out.data(), rp.data(), tot.data());
  if (!same_bytes(&tot[(size_t)n], &guard, sizeof guard)) FAIL("the totals were overrun");
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = cw[(size_t)i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const Window& in = inputs[(size_t)i];
    if (ws[(size_t)i].cam != in.cam || ws[(size_t)i].line != in.line || ws[(size_t)i].fixed != in.fixed ||
        !same_bytes(ws[(size_t)i].obs.data(), in.obs.data(), 8 * in.obs.size())) FAIL("window %d: an input array was written", i);
    if (!same_bytes(ws[(size_t)i].prm.data(), before[(size_t)i].data(), 8 * 6 * (size_t)w.num_cameras)) FAIL("window %d: a camera parameter moved", i);
    slslam_summary t;
    std::memset(&t, 0, sizeof t);
    bool failed = false, capped = false;
    int term = SLSLAM_FUNCTION_TOLERANCE, nref = 0;
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = W.slot[(size_t)l];
      const RefineOut* o = s >= 0 ? &out[(size_t)(P.slot_off[(size_t)i] + s)] : nullptr;
      const double* got = ws[(size_t)i].prm.data() + 6 * (size_t)w.num_cameras + 4 * (size_t)l;
      if (!same_bytes(got, o ? o->u : before[(size_t)i].data() + 6 * (size_t)w.num_cameras + 4 * (size_t)l, 32)) FAIL("window %d line %d: parameters", i, l);
      if (o) {
        t.num_successful_steps += o->n_success; t.num_unsuccessful_steps += o->n_unsuccess;
        t.initial_cost += o->initial_cost; t.final_cost += o->final_cost;
        t.num_residual_blocks += nobs[(size_t)i][(size_t)l];
        failed = failed || o->termination == SLSLAM_NUMERICAL_FAILURE;
        capped = capped || o->termination == SLSLAM_NO_CONVERGENCE;
        term = nref++ ? (o->termination > term ? o->termination : term) : o->termination;
      }
      if (rp[(size_t)i]) {
        const slslam_line_result& r = res[(size_t)i][(size_t)l];
        if (r.status != P.status[(size_t)(P.line_off[(size_t)i] + l)] || r.num_observations != nobs[(size_t)i][(size_t)l]) FAIL("window %d line %d: status / observations", i, l);
        if (r.termination_type != (o ? o->termination : 0) || r.num_successful_steps != (o ? o->n_success : 0) ||
            r.num_unsuccessful_steps != (o ? o->n_unsuccess : 0) || r.initial_cost != (o ? o->initial_cost : 0.0) ||
            r.final_cost != (o ? o->final_cost : 0.0)) FAIL("window %d line %d: record", i, l);
      }
    }
    t.num_free_parameters = 4 * nref;
    t.termination_type = failed ? SLSLAM_NUMERICAL_FAILURE : capped ? SLSLAM_NO_CONVERGENCE : term;
    const slslam_summary& got = tot[(size_t)i];
    if (got.num_successful_steps != t.num_successful_steps || got.num_unsuccessful_steps != t.num_unsuccessful_steps ||
        got.initial_cost != t.initial_cost || got.final_cost != t.final_cost || got.fixed_cost != 0.0 ||
        got.num_residual_blocks != t.num_residual_blocks || got.num_free_parameters != t.num_free_parameters ||
        got.termination_type != t.termination_type) FAIL("window %d: totals (termination %d, expected %d)", i, got.termination_type, t.termination_type);
  }
  // neither results nor totals asked for: only the refined lines' parameters are written, to the same bytes
  std::vector<Window> again = inputs;
  std::vector<slslam_lba_window> cw2;
  for (Window& w : again) cw2.push_back(w.c());
  refine_scatter(P, n, cw2.data(), out.data(), nullptr, nullptr);
  for (int i = 0; i < n; ++i)
    if (!same_bytes(again[(size_t)i].prm.data(), ws[(size_t)i].prm.data(), 8 * ws[(size_t)i].prm.size())) FAIL("window %d: the scatter without results differs", i);
  if (nused == 0 && P.ngroups != 0) FAIL("groups without lines");
  return 0;
}

int check_limits() {
  const char* name = "limits";
  Window big = make(631, 2);
  slslam_lba_window w = big.c();
  LinePlan P;
  if (line_validate_windows(1, &w) != SLSLAM_OK || line_plan_build(kCall, 1, &w, &P) != SLSLAM_ERR_UNSUPPORTED) FAIL("631 cameras were taken");
  Window ok = make(630, 2);
  w = ok.c();
  if (line_plan_build(kCall, 1, &w, &P) != SLSLAM_OK) FAIL("630 cameras were refused");
  Window bad = make(3, 10);
  bad.cam[4] = 3;
  w = bad.c();
  if (line_validate_windows(1, &w) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("camera index out of range");
  // the capacity rule: whole waves, five alignment gaps, 24 bytes per group, 36 per slot (count + u), 68 per element
  size_t in = 0, out = 0;
  line_capacity_bytes(kCall, 0, 0, &in, &out);
  if (in != 5 * 256 || out != 0) FAIL("capacity of an empty handle: %zu, %zu", in, out);
  line_capacity_bytes(kCall, 65, 129, &in, &out);
  if (in != 5 * 256 + 2 * 24 + 128 * 36 + 192 * 68 || out != 128 * sizeof(RefineOut)) FAIL("capacity of 65 lines, 129 observations: %zu, %zu", in, out);
  return 0;
}

}  // namespace

int main() {
  int bad = check_limits();
  {
    std::vector<Window> ws;
    bad += check_call("an empty call", ws);
  }
  {  // every observation lands in a lane of its own line
    std::vector<Window> ws = { make(3, 10) };
    bad += check_call("3 cameras x 10 lines", ws);
  }
  {  // two waves, the second with 6 lines
    std::vector<Window> ws = { make(8, 70) };
    bad += check_call("70 running lines", ws);
    LinePlan P;
    slslam_lba_window w = ws[0].c();
    if (line_plan_build(kCall, 1, &w, &P) != SLSLAM_OK || P.ngroups != 2 || P.lay[0].order.size() != 70 || P.nslot != 128) {
      std::printf("70 running lines: not two waves\n");
      ++bad;
    }
  }
  {
    std::vector<Window> ws = { make(3, 10) };
    for (size_t k = 0; k < ws[0].line.size(); ++k) ws[0].fixed[2 * k + 1] = 1;
    bad += check_call("every line constant", ws, { std::vector<int>(10, SLSLAM_LINE_CONSTANT) });
    LinePlan P;
    slslam_lba_window w = ws[0].c();
    if (line_plan_build(kCall, 1, &w, &P) != SLSLAM_OK || P.ngroups != 0 || P.nslot != 0 || P.nelem != 0 || P.out_bytes != 0) {
      std::printf("every line constant: something is left for the device\n");
      ++bad;
    }
  }
  {  // the fates, hand-written.  Line l of make(4, 14) has 1 + (7 l) % 5 = 1 3 5 2 4 1 3 5 2 4 1 3 5 2 observations and sees cameras
     // l % 4 .. (l + count - 1) % 4: lines 0, 5, 8, 10 and 13 do not see camera 3, which is not finite.  Of those, line 13 has the first
     // of its two observations flagged, line 5 a NaN observation, line 8 a NaN start value; lines 14 and 15 (beyond the last observed
     // line) have no observations
    std::vector<Window> ws = { make(4, 14) };
    Window& a = ws[0];
    a.L = 16; a.prm.resize(6 * 4 + 4 * 16, 0.25);
    for (size_t k = 0; k < a.line.size(); ++k) {
      if (a.line[k] == 13) { a.fixed[2 * k + 1] = 1; break; }
    }
    for (size_t k = 0; k < a.line.size(); ++k) a.fixed[2 * k] = 1;                      // the camera flags are ignored
    for (size_t k = 0; k < a.line.size(); ++k) if (a.line[k] == 5) a.obs[8 * k + 3] = kNaN;
    a.prm[6 * 3 + 1] = std::numeric_limits<double>::infinity();
    a.prm[6 * 4 + 4 * 8 + 2] = kNaN;
    const int R = SLSLAM_LINE_REFINED, K = SLSLAM_LINE_CONSTANT, N = SLSLAM_LINE_NO_OBSERVATIONS, X = SLSLAM_LINE_INVALID;
    bad += check_call("the fates", ws, { { R, X, X, X, X, X, X, X, X, X, R, X, X, K, N, N } });
  }
  {  // three windows: a window with flagged and broken lines between two that run; totals with a capped and a failed line
    std::vector<Window> ws = { make(3, 150), make(7, 65), make(2, 9), make(4, 0) };
    for (size_t k = 0; k < ws[0].line.size(); ++k) if (ws[0].line[k] % 11 == 2 && k % 3 == 0) ws[0].fixed[2 * k + 1] = 1;
    ws[0].obs[8 * 17 + 5] = kNaN;
    ws[1].prm[6 * 3 + 1] = kNaN;
    ws[2].prm[6 * 2 + 4 * 3] = kNaN;
    bad += check_call("four windows", ws);
  }
  if (bad) return 1;
  std::printf("refine host ok\n");
  return 0;
}

// tests/host_cxx/triangulate_host_check.cpp — the host side of the line triangulator (slslam_amd/csrc/lba_triangulate_host.h over the
// plan it shares with the refiner, line_call_plan.h) without a device: the validation of a call, what becomes of every line, the upload image (every observation of a line that runs lands once, in
// its line's lane, in the caller's order; counts, groups and camera tables where the kernel reads them) and the scatter of hand-made
// records back under the caller's numbering - untouched outputs stay untouched.  Built with -fsanitize=address,undefined and run by
// tests/test_lba_triangulate_cpu.py.  Prints "triangulate host ok" and exits 0, or says what is wrong and exits 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../slslam_amd/csrc/lba_triangulate_host.h"

using namespace slslam;

#define FAIL(...) do { std::printf("%s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

namespace {

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

// line l gets 1 + (l * 7) % 5 observations, cameras round robin; observation k holds 100 k + q in its q-th double
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

void fake_pose(const double* wt, double* T) { for (int q = 0; q < 12; ++q) T[q] = wt[q % 6] + q; }

int check_validation() {
  const char* name = "validation";
  Window a = make(3, 10);
  slslam_lba_window w = a.c();
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  if (tri_validate(1, &w, 1, 0.1, 0.0) != SLSLAM_OK) FAIL("a good call was refused");
  if (tri_validate(0, nullptr, 0, 0.1, 0.0) != SLSLAM_OK) FAIL("an empty call was refused");
  if (tri_validate(-1, &w, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("n < 0");
  if (tri_validate(1, nullptr, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("no windows");
  if (tri_validate(1, &w, 2, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT || tri_validate(1, &w, -1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("method");
  if (tri_validate(1, &w, 1, 0.1, nan) != SLSLAM_ERR_INVALID_ARGUMENT || tri_validate(1, &w, 1, 0.1, -1e-9) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("min_parallax");
  if (tri_validate(1, &w, 1, 0.1, inf) != SLSLAM_OK) FAIL("min_parallax = inf (always fall back) was refused");
  for (double d : { 0.0, -0.1, nan, inf })
    if (tri_validate(1, &w, 1, d, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("inverse_depth %g", d);
  Window b = make(3, 10);
  b.line[4] = 10;
  slslam_lba_window wb = b.c();
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("line index out of range");
  b = make(3, 10); b.cam[7] = -1; wb = b.c();
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("camera index out of range");
  wb = a.c(); wb.num_lines = -1;
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("negative count");
  wb = a.c(); wb.observations = nullptr;
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("missing observations");
  wb = a.c(); wb.parameters = nullptr;
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_ERR_INVALID_ARGUMENT) FAIL("missing parameters");
  Window big = make(631, 2);
  wb = big.c();
  TriPlan P;
  if (tri_validate(1, &wb, 1, 0.1, 0.0) != SLSLAM_OK || tri_plan_build(1, &wb, &P) != SLSLAM_ERR_UNSUPPORTED) FAIL("631 cameras were taken");
  return 0;
}

int check_call(const char* name, std::vector<Window>& ws) {
  const int n = (int)ws.size();
  std::vector<slslam_lba_window> cw;
  for (Window& w : ws) cw.push_back(w.c());
  if (tri_validate(n, cw.data(), 1, 0.1, 0.0) != SLSLAM_OK) FAIL("refused");
  TriPlan P;
  if (tri_plan_build(n, cw.data(), &P) != SLSLAM_OK) FAIL("no plan");
  std::vector<char> img(P.in_bytes + 1, 0x5a);
  tri_fill_image(P, n, cw.data(), fake_pose, img.data());
  if (img[P.in_bytes] != 0x5a) FAIL("the image was overrun");
  const TriGroup* hg = reinterpret_cast<const TriGroup*>(img.data() + P.o_grp);
  const double* hc = reinterpret_cast<const double*>(img.data() + P.o_cam);
  const int* hn = reinterpret_cast<const int*>(img.data() + P.o_cnt);
  const int* hoc = reinterpret_cast<const int*>(img.data() + P.o_oc);
  const double* hob = reinterpret_cast<const double*>(img.data() + P.o_ob);
  if (P.o_cam % 256 || P.o_cnt % 256 || P.o_oc % 256 || P.o_ob % 256) FAIL("a block of the image is not 256-byte aligned");

  // hand-made device records: slot s says which line it holds
  std::vector<TriOut> out((size_t)P.nslot);
  long long g = 0;
  for (int i = 0; i < n; ++i) {
    const RefineWindowLayout& W = P.lay[(size_t)i];
    const slslam_lba_window& w = cw[(size_t)i];
    std::vector<int> expect_status((size_t)w.num_lines, SLSLAM_TRI_NO_OBSERVATIONS), nobs((size_t)w.num_lines, 0);
    for (int k = 0; k < w.num_observations; ++k) {
      const int l = w.line_index[k];
      ++nobs[(size_t)l];
      bool bad = false;
      for (int q = 0; q < 8; ++q) bad = bad || !std::isfinite(w.observations[8 * k + q]);
      for (int q = 0; q < 6; ++q) bad = bad || !std::isfinite(w.parameters[6 * w.camera_index[k] + q]);
      int& s = expect_status[(size_t)l];
      if (w.fixed_index[2 * k + 1]) s = SLSLAM_TRI_CONSTANT;
      else if (s == SLSLAM_TRI_NO_OBSERVATIONS) s = bad ? SLSLAM_TRI_INVALID : SLSLAM_TRI_STEREO;
      else if (s == SLSLAM_TRI_STEREO && bad) s = SLSLAM_TRI_INVALID;
    }
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = P.status[(size_t)(P.line_off[(size_t)i] + l)];
      if (s != expect_status[(size_t)l]) FAIL("window %d line %d: status %d, expected %d", i, l, s, expect_status[(size_t)l]);
      if ((s == SLSLAM_TRI_STEREO) != (W.slot[(size_t)l] >= 0)) FAIL("window %d line %d: slot %d with status %d", i, l, W.slot[(size_t)l], s);
    }
    for (size_t q = 0; q < W.group_depth.size(); ++q, ++g) {
      const TriGroup& G = hg[g];
      if (G.row_base != P.row_off[(size_t)i] + W.group_row[q] || G.depth != W.group_depth[q] || G.C != w.num_cameras ||
          G.cam_off != (int)P.cam_off[(size_t)i]) FAIL("window %d group %zu", i, q);
      if ((G.row_base + G.depth) * kRefineLanes > P.nelem) FAIL("window %d group %zu reads beyond the observations", i, q);
      if ((long long)G.cam_off + G.C > P.ncam) FAIL("window %d group %zu reads beyond the cameras", i, q);
    }
    if (!W.group_depth.empty())
      for (int c = 0; c < w.num_cameras; ++c) {
        double T[12];
        bool fin = true;
        for (int q = 0; q < 6; ++q) fin = fin && std::isfinite(w.parameters[6 * c + q]);
        fake_pose(w.parameters + 6 * c, T);
        for (int q = 0; q < 12; ++q)
          if (hc[(P.cam_off[(size_t)i] + c) * kTriCamRec + q] != (fin ? T[q] : 0.0)) FAIL("window %d camera %d", i, c);
      }
    std::vector<int> seen((size_t)w.num_lines, 0);
    for (int k = 0; k < w.num_observations; ++k) {
      const int l = w.line_index[k], s = W.slot[(size_t)l];
      if (s < 0) continue;
      const long long slot = P.slot_off[(size_t)i] + s;
      const TriGroup& G = hg[slot / kRefineLanes];
      if (hn[slot] != nobs[(size_t)l]) FAIL("window %d line %d: count %d, expected %d", i, l, hn[slot], nobs[(size_t)l]);
      if (seen[(size_t)l] >= G.depth) FAIL("window %d line %d is longer than its group", i, l);
      const long long e = (G.row_base + seen[(size_t)l]++) * kRefineLanes + slot % kRefineLanes;
      if (hoc[e] != w.camera_index[k]) FAIL("window %d observation %d: camera", i, k);
      for (int q = 0; q < 8; ++q)
        if (hob[((long long)(q / 2) * P.nelem + e) * 2 + q % 2] != w.observations[8 * k + q]) FAIL("window %d observation %d: double %d", i, k, q);
    }
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = W.slot[(size_t)l];
      if (s < 0) continue;
      TriOut& o = out[(size_t)(P.slot_off[(size_t)i] + s)];
      o.status = l % 7 == 3 ? SLSLAM_TRI_INVALID : l % 2 ? SLSLAM_TRI_MULTIVIEW : SLSLAM_TRI_STEREO;
      o.num_planes = 2 * nobs[(size_t)l]; o.clamped = l % 2 ? 0 : 1; o.pad = 0;
      for (int a = 0; a < 4; ++a) { o.u[a] = 1000.0 * i + l + 0.1 * a; o.eig[a] = l % 2 ? 4.0 - a : 0.0; }
      for (int a = 0; a < 6; ++a) o.av[a] = -(1000.0 * i + l + 0.1 * a);
    }
  }
  if (g != P.ngroups) FAIL("%lld groups, expected %lld", g, P.ngroups);

  // the scatter: results of window 0 and lines_av of the last window are not asked for
  std::vector<std::vector<slslam_triangulated_line>> res((size_t)n);
  std::vector<std::vector<double>> av((size_t)n), before((size_t)n);
  std::vector<slslam_triangulated_line*> rp((size_t)n, nullptr);
  std::vector<double*> ap((size_t)n, nullptr);
  for (int i = 0; i < n; ++i) {
    res[(size_t)i].resize((size_t)cw[(size_t)i].num_lines);
    av[(size_t)i].assign(6 * (size_t)cw[(size_t)i].num_lines, 7.5);
    before[(size_t)i] = ws[(size_t)i].prm;
    if (i > 0) rp[(size_t)i] = res[(size_t)i].data();
    if (i + 1 < n || n == 1) ap[(size_t)i] = av[(size_t)i].data();
  }
  tri_scatter(P, n, cw.data(), out.data(), rp.data(), ap.data());
  for (int i = 0; i < n; ++i) {
    const slslam_lba_window& w = cw[(size_t)i];
    const RefineWindowLayout& W = P.lay[(size_t)i];
    for (int c = 0; c < 6 * w.num_cameras; ++c)
      if (!(ws[(size_t)i].prm[(size_t)c] == before[(size_t)i][(size_t)c]) && std::isfinite(before[(size_t)i][(size_t)c])) FAIL("window %d: a camera parameter moved", i);
    for (int l = 0; l < w.num_lines; ++l) {
      const int s = W.slot[(size_t)l];
      const TriOut* o = s >= 0 ? &out[(size_t)(P.slot_off[(size_t)i] + s)] : nullptr;
      const bool made = o && o->status != SLSLAM_TRI_INVALID;
      for (int a = 0; a < 4; ++a) {
        const double got = ws[(size_t)i].prm[6 * (size_t)w.num_cameras + 4 * (size_t)l + a];
        if (got != (made ? o->u[a] : before[(size_t)i][6 * (size_t)w.num_cameras + 4 * (size_t)l + a])) FAIL("window %d line %d: parameter %d", i, l, a);
      }
      if (ap[(size_t)i])
        for (int a = 0; a < 6; ++a)
          if (av[(size_t)i][6 * (size_t)l + a] != (made ? o->av[a] : 7.5)) FAIL("window %d line %d: lines_av %d", i, l, a);
      if (rp[(size_t)i]) {
        const slslam_triangulated_line& r = res[(size_t)i][(size_t)l];
        int nob = 0, first = -1;
        for (int k = 0; k < w.num_observations; ++k) if (w.line_index[k] == l) { if (!nob++) first = w.camera_index[k]; }
        if (r.num_observations != nob || r.first_camera != first) FAIL("window %d line %d: %d observations, first camera %d", i, l, r.num_observations, r.first_camera);
        const int want = o ? o->status : P.status[(size_t)(P.line_off[(size_t)i] + l)];
        if (r.status != want) FAIL("window %d line %d: status %d, expected %d", i, l, r.status, want);
        if (r.num_planes != (made ? o->num_planes : 0) || r.clamped != (made ? o->clamped : 0)) FAIL("window %d line %d: planes / clamped", i, l);
        for (int a = 0; a < 4; ++a) if (r.eigenvalues[a] != (made ? o->eig[a] : 0.0)) FAIL("window %d line %d: eigenvalue %d", i, l, a);
      }
    }
  }
  return 0;
}

}  // namespace

int main() {
  int bad = check_validation();
  {
    std::vector<Window> ws;
    bad += check_call("no windows", ws);
  }
  {
    std::vector<Window> ws = { make(4, 0), make(0, 0) };
    bad += check_call("empty windows", ws);
  }
  {
    std::vector<Window> ws = { make(5, 60) };
    bad += check_call("one wave", ws);
  }
  {  // three windows; constant lines, a NaN observation, a NaN camera, a line nobody observes behind the last observed one
    std::vector<Window> ws = { make(3, 150), make(7, 65), make(2, 9) };
    for (size_t k = 0; k < ws[0].line.size(); ++k) if (ws[0].line[k] % 11 == 2 && k % 3 == 0) ws[0].fixed[2 * k + 1] = 1;
    ws[0].obs[8 * 17 + 5] = std::numeric_limits<double>::quiet_NaN();
    ws[1].prm[6 * 3 + 1] = std::numeric_limits<double>::infinity();
    ws[2].L = 12; ws[2].prm.resize(6 * 2 + 4 * 12, 0.25);
    for (size_t k = 0; k < ws[2].fixed.size(); ++k) ws[2].fixed[k] = k % 2 == 0;        // the camera flags are ignored
    bad += check_call("three windows", ws);
  }
  if (bad) return 1;
  std::printf("triangulate host ok\n");
  return 0;
}

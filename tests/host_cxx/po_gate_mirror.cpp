// tests/host_cxx/po_gate_mirror.cpp — POProblem::gate (slslam_amd/host/po_problem.h; an extension the reference does not have) against
// slslam_po_gate called directly with the same arrays.  Needs a device.
//   po_gate_mirror <file.txt>   reads "N E weighted robust M", E x (i1 i2), 6E constraints, 6N parameters, 36E weights when weighted,
//                               M x (a b), 6M candidate constraints, 36M measurement covariances, sigma2; exits 0 when the member
//                               function returns (to 1e-9) what the C ABI returns for the graph it should have forwarded,
//                               and prints the M squared Mahalanobis distances, %.17g
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/slslam_hip.h"
#include "po_problem.h"

struct Out {
  int cov_status;
  std::vector<int> status;
  std::vector<double> error, cov, w, m2;
  explicit Out(int M) : cov_status(-1), status(M, -1), error(6 * M), cov(36 * M), w(36 * M), m2(M) {}
  // (two covariance runs differ by the order of the linearisation's atomic sums: equal to 1e-9 of the largest entry, not bit for bit)
  static bool close(const std::vector<double>& a, const std::vector<double>& b) {
    double top = 0.0, d = 0.0;
    for (size_t i = 0; i < a.size(); ++i) { top = std::max(top, std::fabs(b[i])); d = std::max(d, std::fabs(a[i] - b[i])); }
    return d <= 1e-9 * top;
  }
  bool same(const Out& o) const {
    return cov_status == o.cov_status && status == o.status && close(error, o.error) && close(cov, o.cov) && close(w, o.w) && close(m2, o.m2);
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int N = 0, E = 0, weighted = 0, robust = 0, M = 0;
  if (std::fscanf(f, "%d %d %d %d %d", &N, &E, &weighted, &robust, &M) != 5 || N < 0 || E < 0 || M < 0) return 2;
  ceres::POProblem po(E, 10);
  int* i1 = new int[E]; int* i2 = new int[E];
  double* cons = new double[6 * E]; double* x = new double[6 * N];
  po.set_pose_index_1(i1); po.set_pose_index_2(i2); po.set_constraints(cons); po.set_parameters(x);
  po.set_num_poses(N);
  po.set_robustify(robust != 0);
  int ok = 1;
  for (int e = 0; e < E; ++e) ok &= std::fscanf(f, "%d %d", &i1[e], &i2[e]) == 2;
  for (int q = 0; q < 6 * E; ++q) ok &= std::fscanf(f, "%lf", &cons[q]) == 1;
  for (int q = 0; q < 6 * N; ++q) ok &= std::fscanf(f, "%lf", &x[q]) == 1;
  if (weighted) {
    double* w = new double[36 * E];
    po.set_sqrt_information(w);
    for (int q = 0; q < 36 * E; ++q) ok &= std::fscanf(f, "%lf", &w[q]) == 1;
  }
  std::vector<int> ca(M), cb(M);
  std::vector<double> cc(6 * M), cr(36 * M);
  double sigma2 = 0.0;
  for (int k = 0; k < M; ++k) ok &= std::fscanf(f, "%d %d", &ca[k], &cb[k]) == 2;
  for (int q = 0; q < 6 * M; ++q) ok &= std::fscanf(f, "%lf", &cc[q]) == 1;
  for (int q = 0; q < 36 * M; ++q) ok &= std::fscanf(f, "%lf", &cr[q]) == 1;
  ok &= std::fscanf(f, "%lf", &sigma2) == 1;
  std::fclose(f);
  if (!ok) return 2;
  slslam_po_candidates cand = slslam_po_candidates();
  cand.num = M; cand.pose_a = ca.data(); cand.pose_b = cb.data(); cand.constraints = cc.data(); cand.cov_meas = cr.data(); cand.sigma2 = sigma2;
  Out mine(M), direct(M);
  const int rc = po.gate(cand, &mine.cov_status, mine.status.data(), mine.error.data(), mine.cov.data(), mine.w.data(), mine.m2.data());
  if (rc != SLSLAM_OK) { std::fprintf(stderr, "POProblem::gate: %s\n", slslam_status_string(rc)); return 1; }
  slslam_po_graph g = slslam_po_graph();
  g.num_poses = N; g.num_edges = E; g.pose_index_1 = i1; g.pose_index_2 = i2; g.constraints = cons; g.parameters = x;
  g.sqrt_information = po.sqrt_information();
  const int rd = slslam_po_gate(&g, robust ? 0.001 : 0.0, &cand, &direct.cov_status, direct.status.data(), direct.error.data(), direct.cov.data(),
                                direct.w.data(), direct.m2.data());
  if (rd != SLSLAM_OK) return 1;
  for (int k = 0; k < M; ++k) std::printf("%.17g\n", mine.m2[k]);
  if (!mine.same(direct)) { std::fprintf(stderr, "POProblem::gate differs from slslam_po_gate\n"); return 1; }
  cand.sigma2 = 0.0;                               // the C ABI's refusal comes through
  return po.gate(cand, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == SLSLAM_ERR_INVALID_ARGUMENT ? 0 : 1;
}

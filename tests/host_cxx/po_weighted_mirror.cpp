// tests/host_cxx/po_weighted_mirror.cpp — POProblem::set_sqrt_information (slslam_amd/host/po_problem.h; an extension the reference
// does not have) through the facade's ceres::Solve.
//   po_weighted_mirror                 (built with -DPO_WEIGHTED_SEAM: the program defines slslam_po_solve itself, as
//                                       po_robustify_seam.cpp does, so no device is needed)  a fresh POProblem forwards NULL, one with
//                                       set_sqrt_information forwards the array it was given; then a POProblem that owns weights goes out
//                                       of scope WITHOUT a solve (the destructor delete[]s them once)
//   po_weighted_mirror <graph.txt>     (built without the seam; needs a device)  reads "N E weighted", E x (i1 i2), 6E constraints,
//                                       6N parameters, 36E weights when weighted; solves through ceres::Solve and prints the 6N
//                                       parameters, one per line, %.17g
#include <cstdio>
#include <cstdlib>

#include "../../include/slslam_hip.h"
#include "po_problem.h"

#ifdef PO_WEIGHTED_SEAM
static const double* seen_w = nullptr;
static int calls = 0;
extern "C" int slslam_po_solve(const slslam_po_graph* graph, const slslam_solver_options*, slslam_summary* summary, slslam_iteration*, int,
                               int* trace_len) {
  ++calls;
  seen_w = graph->sqrt_information;
  if (summary) { *summary = slslam_summary(); summary->num_residual_blocks = graph->num_edges; }
  if (trace_len) *trace_len = 0;
  return SLSLAM_OK;
}
#endif

static int solve(ceres::POProblem& po) {
  ceres::Problem problem;
  po.build(&problem);
  ceres::Solver::Options options;
  po.set_options(&options);
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);
  return summary.backend_status;
}

#ifdef PO_WEIGHTED_SEAM
static void fill(ceres::POProblem& po, int E) {
  int* i1 = new int[E]; int* i2 = new int[E];
  for (int e = 0; e < E; ++e) { i1[e] = e; i2[e] = e + 1; }
  po.set_pose_index_1(i1); po.set_pose_index_2(i2);
  po.set_constraints(new double[6 * E]());
  po.set_parameters(new double[6 * (E + 1)]());
}
#endif

int main(int argc, char** argv) {
#ifdef PO_WEIGHTED_SEAM
  (void)argc; (void)argv;
  const int E = 3;
  int rc = 0;
  {
    ceres::POProblem po(E, 10);
    fill(po, E);
    std::printf("fresh null %d\n", po.sqrt_information() == nullptr ? 1 : 0);
    rc |= solve(po);
    std::printf("forwarded null %d\n", seen_w == nullptr ? 1 : 0);
    double* w = new double[36 * E]();
    for (int e = 0; e < E; ++e) for (int q = 0; q < 6; ++q) w[36 * e + 7 * q] = 2.0;
    po.set_sqrt_information(w);
    rc |= solve(po);
    std::printf("forwarded same %d getter same %d\n", seen_w == w ? 1 : 0, po.sqrt_information() == w ? 1 : 0);
  }
  {
    ceres::POProblem po(E, 10);                  // owns its weights and is never solved
    fill(po, E);
    po.set_sqrt_information(new double[36 * E]());
  }
  std::printf("calls %d\n", calls);
  return rc;
#else
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int N = 0, E = 0, weighted = 0;
  if (std::fscanf(f, "%d %d %d", &N, &E, &weighted) != 3 || N < 0 || E < 0) return 2;
  ceres::POProblem po(E, 10);
  int* i1 = new int[E]; int* i2 = new int[E];
  double* cons = new double[6 * E]; double* x = new double[6 * N];
  po.set_pose_index_1(i1); po.set_pose_index_2(i2); po.set_constraints(cons); po.set_parameters(x);
  po.set_num_poses(N);
  int ok = 1;
  for (int e = 0; e < E; ++e) ok &= std::fscanf(f, "%d %d", &i1[e], &i2[e]) == 2;
  for (int q = 0; q < 6 * E; ++q) ok &= std::fscanf(f, "%lf", &cons[q]) == 1;
  for (int q = 0; q < 6 * N; ++q) ok &= std::fscanf(f, "%lf", &x[q]) == 1;
  if (weighted) {
    double* w = new double[36 * E];
    po.set_sqrt_information(w);
    for (int q = 0; q < 36 * E; ++q) ok &= std::fscanf(f, "%lf", &w[q]) == 1;
  }
  std::fclose(f);
  if (!ok) return 2;
  const int rc = solve(po);
  for (int q = 0; q < 6 * N; ++q) std::printf("%.17g\n", po.parameters()[q]);
  return rc;
#endif
}

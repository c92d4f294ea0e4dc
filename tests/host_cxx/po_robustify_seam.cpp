// tests/host_cxx/po_robustify_seam.cpp — what POProblem::set_robustify hands the C ABI.
// The facade's ceres::Solve (slslam_amd/host/problems.cpp) marshals a POProblem into slslam_po_solve.  This program defines
// slslam_po_solve itself: the dynamic linker resolves the host library's call to the executable's definition first, so the options
// the facade built are observed here, with no device and no solve.  Prints the po_huber_delta of three calls - a fresh POProblem
// (the reference's constructor constant: robustify = false, src/po_problem.cpp:27), set_robustify(true) (HuberLoss(0.001), :55),
// set_robustify(false) - and what robust() answered each time.
#include <cstdio>

#include "../../include/slslam_hip.h"
#include "po_problem.h"

static double seen_delta = -1.0, seen_lba_delta = -1.0;
static int calls = 0;

extern "C" int slslam_po_solve(const slslam_po_graph* graph, const slslam_solver_options* opt, slslam_summary* summary,
                               slslam_iteration*, int, int* trace_len) {
  ++calls;
  seen_delta = opt ? opt->po_huber_delta : -2.0;
  seen_lba_delta = opt ? opt->huber_delta : -2.0;
  if (summary) { *summary = slslam_summary(); summary->num_residual_blocks = graph->num_edges; }
  if (trace_len) *trace_len = 0;
  return SLSLAM_OK;
}

static int solve_once(ceres::POProblem& po) {
  ceres::Problem problem;
  po.build(&problem);
  ceres::Solver::Options options;
  po.set_options(&options);
  ceres::Solver::Summary summary;
  seen_delta = -1.0;
  ceres::Solve(options, &problem, &summary);
  std::printf("robust %d po_huber_delta %.17g huber_delta %.17g backend %d blocks %d\n", po.robust() ? 1 : 0, seen_delta, seen_lba_delta,
              summary.backend_status, summary.num_residual_blocks_reduced);
  return summary.backend_status;
}

int main() {
  const int E = 2;
  ceres::POProblem po(E, 10);                    // (takes ownership of the four arrays)
  po.set_pose_index_1(new int[E]{ 0, 1 });
  po.set_pose_index_2(new int[E]{ 1, 2 });
  po.set_constraints(new double[6 * E]());
  po.set_parameters(new double[6 * 3]());
  int rc = solve_once(po);
  po.set_robustify(true);
  rc |= solve_once(po);
  po.set_robustify(false);
  rc |= solve_once(po);
  std::printf("calls %d\n", calls);
  return rc;
}

/* tests/host_cxx/refine_abi_probe.c — sizeof / offsetof of the structs of the structure-only refinement as a C compiler sees
 * include/slslam_hip.h, one "name value" per line; tests/test_refine_lines_cpu.py compares them with the ctypes mirror. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/slslam_hip.h"

#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("slslam_line_result %zu\n", sizeof(slslam_line_result));
  OFF(slslam_line_result, status); OFF(slslam_line_result, termination_type); OFF(slslam_line_result, num_successful_steps);
  OFF(slslam_line_result, num_unsuccessful_steps); OFF(slslam_line_result, num_observations); OFF(slslam_line_result, initial_cost);
  OFF(slslam_line_result, final_cost);
  printf("slslam_summary %zu\n", sizeof(slslam_summary));
  OFF(slslam_summary, num_successful_steps); OFF(slslam_summary, num_unsuccessful_steps); OFF(slslam_summary, initial_cost);
  OFF(slslam_summary, final_cost); OFF(slslam_summary, fixed_cost); OFF(slslam_summary, termination_type);
  OFF(slslam_summary, num_free_parameters); OFF(slslam_summary, num_residual_blocks);
  printf("slslam_lba_window %zu\n", sizeof(slslam_lba_window));
  OFF(slslam_lba_window, num_cameras); OFF(slslam_lba_window, num_lines); OFF(slslam_lba_window, num_observations);
  OFF(slslam_lba_window, camera_index); OFF(slslam_lba_window, line_index); OFF(slslam_lba_window, fixed_index);
  OFF(slslam_lba_window, observations); OFF(slslam_lba_window, parameters);
  printf("SLSLAM_LINE_REFINED %d\nSLSLAM_LINE_CONSTANT %d\nSLSLAM_LINE_NO_OBSERVATIONS %d\nSLSLAM_LINE_INVALID %d\n",
         SLSLAM_LINE_REFINED, SLSLAM_LINE_CONSTANT, SLSLAM_LINE_NO_OBSERVATIONS, SLSLAM_LINE_INVALID);
  return 0;
}

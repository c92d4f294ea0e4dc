/* tests/host_cxx/triangulate_abi_probe.c — sizeof / offsetof of slslam_triangulated_line and the SLSLAM_TRI_* values as a C compiler
 * sees include/slslam_hip.h, one "name value" per line; tests/test_lba_triangulate_cpu.py compares them with the ctypes mirror. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/slslam_hip.h"

#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))

int main(void) {
  printf("slslam_triangulated_line %zu\n", sizeof(slslam_triangulated_line));
  OFF(slslam_triangulated_line, status); OFF(slslam_triangulated_line, num_observations); OFF(slslam_triangulated_line, num_planes);
  OFF(slslam_triangulated_line, first_camera); OFF(slslam_triangulated_line, eigenvalues); OFF(slslam_triangulated_line, clamped);
  OFF(slslam_triangulated_line, reserved);
  printf("SLSLAM_TRI_MULTIVIEW %d\nSLSLAM_TRI_STEREO %d\nSLSLAM_TRI_CONSTANT %d\nSLSLAM_TRI_NO_OBSERVATIONS %d\nSLSLAM_TRI_INVALID %d\n",
         SLSLAM_TRI_MULTIVIEW, SLSLAM_TRI_STEREO, SLSLAM_TRI_CONSTANT, SLSLAM_TRI_NO_OBSERVATIONS, SLSLAM_TRI_INVALID);
  return 0;
}

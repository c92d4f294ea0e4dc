"""ctypes binding of the C ABI in include/slslam_hip.h (libslslam_hip.so, built in-tree).

The Python layer is plumbing for tests, benches and multi-GPU fan-out; the product is the HIP
library.  There is no CPU fallback here: if the library is missing or no HIP device is usable
the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libslslam_hip.so")

OK = 0
STATUS = {0: "ok", 1: "invalid argument", 2: "no usable HIP device", 3: "HIP runtime error",
          4: "unsupported problem shape", 5: "invalid call sequence", 6: "host allocation failed"}
TERMINATION = {0: "NO_CONVERGENCE", 1: "GRADIENT_TOLERANCE", 2: "FUNCTION_TOLERANCE",
               3: "PARAMETER_TOLERANCE", 4: "NUMERICAL_FAILURE", 5: "MIN_RADIUS"}
KERNEL_FAMILIES = ["linearise_schur", "reduced_solve", "backsub", "line_trig", "candidate_cost",
                   "lm_update", "init_linearise", "unused"]


class SlslamError(RuntimeError):
    def __init__(self, status, where):
        super().__init__("%s: %s (status %d)" % (where, STATUS.get(status, "?"), status))
        self.status = status


class SolverOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("huber_delta", C.c_double), ("baseline", C.c_double),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_num_consecutive_invalid_steps", C.c_int), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("jacobi_scaling", C.c_int), ("use_graph", C.c_int), ("chunks_per_window", C.c_int),
                ("reuse_elimination", C.c_int), ("po_factor_fp32", C.c_int), ("po_dense_factor", C.c_int), ("lba_fused_motion_only", C.c_int),
                ("lba_elimination", C.c_int), ("lba_keep_jacobian", C.c_int), ("refill_headroom_percent", C.c_int),
                ("host_threads", C.c_int), ("reproducible", C.c_int), ("lba_precision", C.c_int), ("device_build", C.c_int),
                ("po_huber_delta", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("fixed_cost", C.c_double),
                ("termination_type", C.c_int), ("num_free_parameters", C.c_int),
                ("num_residual_blocks", C.c_int)]


class Iteration(C.Structure):
    _fields_ = [("iteration", C.c_int), ("step_is_valid", C.c_int), ("step_is_successful", C.c_int),
                ("cost", C.c_double), ("cost_change", C.c_double), ("gradient_max_norm", C.c_double),
                ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("trust_region_radius", C.c_double), ("model_cost_change", C.c_double)]


class LBAWindow(C.Structure):
    _fields_ = [("num_cameras", C.c_int), ("num_lines", C.c_int), ("num_observations", C.c_int),
                ("camera_index", C.POINTER(C.c_int)), ("line_index", C.POINTER(C.c_int)),
                ("fixed_index", C.POINTER(C.c_int)), ("observations", C.POINTER(C.c_double)),
                ("parameters", C.POINTER(C.c_double))]


class RansacTrials(C.Structure):
    _fields_ = [("num_trials", C.c_int), ("sample_size", C.c_int), ("num_lines", C.c_int), ("samples", C.POINTER(C.c_int)),
                ("observations0", C.POINTER(C.c_double)), ("observations1", C.POINTER(C.c_double))]


class RansacFrame(C.Structure):
    _fields_ = [("num_hypotheses", C.c_int), ("num_lines", C.c_int), ("poses", C.POINTER(C.c_double)),
                ("observations", C.POINTER(C.c_double)), ("lines", C.POINTER(C.c_double))]


class PoseEstimate(C.Structure):
    _fields_ = [("status", C.c_int), ("trial_cnt", C.c_int), ("ransac_score", C.c_int), ("ransac_pose", C.c_double * 12),
                ("ransac_inlier_bits", C.POINTER(C.c_ulonglong)), ("summary", Summary), ("pose", C.c_double * 12),
                ("num_inliers", C.c_int), ("inlier_bits", C.POINTER(C.c_ulonglong))]


class MatchFrame(C.Structure):
    _fields_ = [("num_observations", C.c_int), ("num_lines", C.c_int), ("pose", C.POINTER(C.c_double)),
                ("observations", C.POINTER(C.c_double)), ("lines", C.POINTER(C.c_double)), ("extents", C.POINTER(C.c_double))]


class MatchResult(C.Structure):
    _fields_ = [("status", C.c_int), ("num_matched", C.c_int), ("match", C.POINTER(C.c_int)), ("best_line", C.POINTER(C.c_int)),
                ("best_error", C.POINTER(C.c_float)), ("second_error", C.POINTER(C.c_float)), ("num_admissible", C.POINTER(C.c_int)),
                ("best_observation", C.POINTER(C.c_int))]


class LineResult(C.Structure):
    _fields_ = [("status", C.c_int), ("termination_type", C.c_int), ("num_successful_steps", C.c_int),
                ("num_unsuccessful_steps", C.c_int), ("num_observations", C.c_int), ("initial_cost", C.c_double),
                ("final_cost", C.c_double)]


class TriangulatedLine(C.Structure):
    _fields_ = [("status", C.c_int), ("num_observations", C.c_int), ("num_planes", C.c_int), ("first_camera", C.c_int),
                ("eigenvalues", C.c_double * 4), ("clamped", C.c_int), ("reserved", C.c_int)]


class PlaceFrame(C.Structure):
    _fields_ = [("num_descriptors", C.c_int), ("descriptors", C.POINTER(C.c_float))]


class PlaceResult(C.Structure):
    _fields_ = [("status", C.c_int), ("num_states", C.c_int), ("has_virtual", C.c_int), ("words", C.POINTER(C.c_int)),
                ("score", C.POINTER(C.c_float)), ("touched", C.POINTER(C.c_ubyte)), ("likelihood", C.POINTER(C.c_float)),
                ("top_id", C.POINTER(C.c_int)), ("top_score", C.POINTER(C.c_float))]


class DescriptorQuery(C.Structure):
    _fields_ = [("num_descriptors", C.c_int), ("descriptors", C.POINTER(C.c_float)), ("num_candidates", C.c_int),
                ("candidates", C.POINTER(C.c_int))]


class DescriptorResult(C.Structure):
    _fields_ = [("status", C.c_int), ("num_matched", C.c_int), ("num_keyframe_descriptors", C.c_int), ("match", C.POINTER(C.c_int)),
                ("best", C.POINTER(C.c_int)), ("best_distance", C.POINTER(C.c_float)), ("second_distance", C.POINTER(C.c_float)),
                ("num_admissible", C.POINTER(C.c_int)), ("best_query", C.POINTER(C.c_int))]


class VocTreeTrainOptions(C.Structure):
    _fields_ = [("K", C.c_int), ("L", C.c_int), ("D", C.c_int), ("max_iterations", C.c_int), ("seed", C.c_ulonglong)]


class VocTreeTrainReport(C.Structure):
    _fields_ = [("levels", C.c_int), ("iterations", C.c_int * 4), ("changed", C.c_longlong * 4), ("empty_children", C.c_longlong * 4),
                ("distortion", C.c_double * 4), ("setup_ms", C.c_double * 4), ("kernel_ms", C.c_double * 4), ("download_ms", C.c_double * 4),
                ("centre_ms", C.c_double * 4), ("upload_ms", C.c_double * 4), ("total_ms", C.c_double)]


class MsldOptions(C.Structure):
    _fields_ = [("bands", C.c_int), ("band_width", C.c_int), ("orient", C.c_int)]


class MsldFrame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_longlong), ("image", C.POINTER(C.c_ubyte)),
                ("num_segments", C.c_int), ("segments", C.POINTER(C.c_float))]


class MsldResult(C.Structure):
    _fields_ = [("descriptors", C.POINTER(C.c_float)), ("status", C.POINTER(C.c_int)), ("num_samples", C.POINTER(C.c_int)),
                ("polarity", C.POINTER(C.c_float))]


class LineDetectOptions(C.Structure):
    _fields_ = [("grad_threshold", C.c_int), ("tol_num", C.c_int), ("tol_den", C.c_int), ("min_pixels", C.c_int),
                ("min_length", C.c_double), ("max_thickness", C.c_double), ("max_segments", C.c_int)]


class LineDetectFrame(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("stride", C.c_longlong), ("image", C.POINTER(C.c_ubyte))]


class LineDetectResult(C.Structure):
    _fields_ = [("segments", C.POINTER(C.c_float)), ("length", C.POINTER(C.c_double)), ("thickness", C.POINTER(C.c_double)),
                ("strength", C.POINTER(C.c_double)), ("pixels", C.POINTER(C.c_int)), ("label", C.POINTER(C.c_int)),
                ("num_components", C.POINTER(C.c_int)), ("num_ok", C.POINTER(C.c_int)), ("num_written", C.POINTER(C.c_int)),
                ("status_counts", C.POINTER(C.c_int)), ("labels", C.POINTER(C.c_int))]


class StereoMatchOptions(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("min_disparity", "max_disparity", "max_tan2", "min_rows", "min_overlap", "ratio",
                                          "max_distance", "fx", "fy", "cx", "cy")]


class StereoFrame(C.Structure):
    _fields_ = [("num_left", C.c_int), ("left_segments", C.POINTER(C.c_float)), ("left_descriptors", C.POINTER(C.c_float)),
                ("num_right", C.c_int), ("right_segments", C.POINTER(C.c_float)), ("right_descriptors", C.POINTER(C.c_float))]


class StereoResult(C.Structure):
    _fields_ = [("status", C.c_int), ("num_matched", C.c_int), ("match", C.POINTER(C.c_int)), ("best", C.POINTER(C.c_int)),
                ("best_distance", C.POINTER(C.c_float)), ("second_distance", C.POINTER(C.c_float)),
                ("num_admissible", C.POINTER(C.c_int)), ("best_left", C.POINTER(C.c_int)), ("segment_status", C.POINTER(C.c_int)),
                ("observations", C.POINTER(C.c_double)), ("disparity", C.POINTER(C.c_double))]


class LineTrackOptions(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("max_tan2", "max_shift", "max_offset", "min_overlap", "min_length", "ratio", "max_distance")]


class LineTrackFrame(C.Structure):
    _fields_ = [("num_segments", C.c_int), ("segments", C.POINTER(C.c_float)), ("descriptors", C.POINTER(C.c_float)),
                ("predict", C.POINTER(C.c_double))]


class LineTrackResult(C.Structure):
    _fields_ = [("status", C.c_int), ("num_continued", C.c_int), ("num_new", C.c_int), ("id", C.POINTER(C.c_int)),
                ("age", C.POINTER(C.c_int)), ("segment_status", C.POINTER(C.c_int)), ("match", C.POINTER(C.c_int)),
                ("best", C.POINTER(C.c_int)), ("best_distance", C.POINTER(C.c_float)), ("second_distance", C.POINTER(C.c_float)),
                ("num_admissible", C.POINTER(C.c_int)), ("best_row", C.POINTER(C.c_int))]


class RectifyOptions(C.Structure):
    _fields_ = [("border_mode", C.c_int), ("border_value", C.c_int), ("smooth_sigma", C.c_double)]


class RectifyCamera(C.Structure):
    """slslam_rectify_camera.  RectifyCamera.make(...) takes keywords with an identity default for everything but the sizes."""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")] + [("R", C.c_double * 9)] + \
               [(k, C.c_double) for k in ("fx2", "fy2", "cx2", "cy2")] + \
               [(k, C.c_int) for k in ("src_width", "src_height", "dst_width", "dst_height")]

    @classmethod
    def make(cls, src_width, src_height, dst_width=None, dst_height=None, fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0,
             k3=0.0, R=None, fx2=None, fy2=None, cx2=None, cy2=None):
        c = cls()
        c.fx, c.fy, c.cx, c.cy = float(fx), float(fy), float(cx), float(cy)
        c.k1, c.k2, c.p1, c.p2, c.k3 = float(k1), float(k2), float(p1), float(p2), float(k3)
        c.R[:] = np.asarray(np.eye(3) if R is None else R, dtype=np.float64).reshape(9).tolist()
        c.fx2, c.fy2 = float(fx if fx2 is None else fx2), float(fy if fy2 is None else fy2)
        c.cx2, c.cy2 = float(cx if cx2 is None else cx2), float(cy if cy2 is None else cy2)
        c.src_width, c.src_height = int(src_width), int(src_height)
        c.dst_width, c.dst_height = int(src_width if dst_width is None else dst_width), int(src_height if dst_height is None else dst_height)
        return c

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "R"}
        d["R"] = np.array(list(self.R)).reshape(3, 3)
        return d


class RectifyFrame(C.Structure):
    _fields_ = [("camera", C.c_int), ("stride", C.c_longlong), ("image", C.POINTER(C.c_ubyte))]


class RectifyResult(C.Structure):
    _fields_ = [("image", C.POINTER(C.c_ubyte)), ("stride", C.c_longlong), ("valid", C.POINTER(C.c_ubyte)), ("num_valid", C.POINTER(C.c_int))]


class StereoRig(C.Structure):
    _fields_ = [("left_k", C.c_double * 4), ("left_dist", C.c_double * 5), ("right_k", C.c_double * 4), ("right_dist", C.c_double * 5),
                ("R", C.c_double * 9), ("t", C.c_double * 3)] + \
               [(k, C.c_int) for k in ("left_width", "left_height", "right_width", "right_height", "dst_width", "dst_height",
                                       "has_principal", "reserved")] + [("cx2", C.c_double), ("cy2", C.c_double)]


RECTIFY_BORDER = {"constant": 0, "replicate": 1}
RECTIFY_SUBPIXEL_BITS = 8                               # SLSLAM_RECTIFY_SUBPIXEL_BITS
RECTIFY_NO_COORD = -2 ** 31                             # SLSLAM_RECTIFY_NO_COORD
RECTIFY_TILE = (64, 16)                                 # SLSLAM_RECTIFY_TILE_WIDTH, _HEIGHT: the smoothing kernel's tile
STEREO_STATUS = {0: "OK", 1: "EMPTY"}
TRACK_STATUS = {0: "OK", 1: "EMPTY"}
TRACK_SEGMENT_STATUS = {0: "CONTINUED", 1: "NEW", 2: "SHORT", 3: "INVALID"}
STEREO_SEGMENT_STATUS = {0: "MATCHED", 1: "UNMATCHED", 2: "FLAT", 3: "INVALID"}
MSLD_STATUS = {0: "OK", 1: "FLAT", 2: "TOO_SHORT", 3: "OUTSIDE", 4: "INVALID"}
LSD_STATUS = {0: "OK", 1: "SMALL", 2: "ISOTROPIC", 3: "SHORT", 4: "THICK"}
LSD_TILE = 32                                           # SLSLAM_LSD_TILE: the side of the detector's labelling tiles
PLACE_STATUS = {0: "OK", 1: "EMPTY", 2: "INVALID_DESCRIPTOR"}
DESC_STATUS = {0: "OK", 1: "EMPTY", 2: "INVALID_DESCRIPTOR"}
TRI_MULTIVIEW, TRI_STEREO, TRI_CONSTANT, TRI_NO_OBSERVATIONS, TRI_INVALID = 0, 1, 2, 3, 4
TRI_STATUS = {0: "MULTIVIEW", 1: "STEREO", 2: "CONSTANT", 3: "NO_OBSERVATIONS", 4: "INVALID"}
LINE_REFINED, LINE_CONSTANT, LINE_NO_OBSERVATIONS, LINE_INVALID = 0, 1, 2, 3
LINE_STATUS = {0: "REFINED", 1: "CONSTANT", 2: "NO_OBSERVATIONS", 3: "INVALID"}
POSE_STATUS = {0: "OK", 1: "TOO_FEW_FEATURES", 2: "RANSAC_FAILED"}
MATCH_STATUS = {0: "OK", 1: "EMPTY", 2: "INVALID_POSE"}
COV_OK, COV_SINGULAR = 0, 1


class POGraph(C.Structure):
    _fields_ = [("num_poses", C.c_int), ("num_edges", C.c_int),
                ("pose_index_1", C.POINTER(C.c_int)), ("pose_index_2", C.POINTER(C.c_int)),
                ("constraints", C.POINTER(C.c_double)), ("parameters", C.POINTER(C.c_double)),
                ("sqrt_information", C.POINTER(C.c_double))]      # [36E] row-major W_e; NULL (the default): identity


class POEdgeItems(C.Structure):
    _fields_ = [("n", C.c_int), ("pose_a", C.POINTER(C.c_double)), ("pose_b", C.POINTER(C.c_double)), ("constraints", C.POINTER(C.c_double)),
                ("cov_aa", C.POINTER(C.c_double)), ("cov_bb", C.POINTER(C.c_double)), ("cov_ab", C.POINTER(C.c_double)),
                ("cov_meas", C.POINTER(C.c_double)), ("sigma2", C.c_double)]


class POCandidates(C.Structure):
    _fields_ = [("num", C.c_int), ("pose_a", C.POINTER(C.c_int)), ("pose_b", C.POINTER(C.c_int)), ("constraints", C.POINTER(C.c_double)),
                ("cov_meas", C.POINTER(C.c_double)), ("sigma2", C.c_double)]


class POConstraintItems(C.Structure):
    _fields_ = [("n", C.c_int), ("pose_a", C.POINTER(C.c_double)), ("pose_b", C.POINTER(C.c_double)), ("constraints", C.POINTER(C.c_double)),
                ("cov_constraint", C.POINTER(C.c_double)), ("sigma2", C.c_double)]


# every symbol include/slslam_hip.h declares (checked by the CPU test-suite)
EXPORTS = [
    "slslam_default_options", "slslam_lba_solve", "slslam_lba_batch_create", "slslam_lba_batch_destroy",
    "slslam_lba_batch_add", "slslam_lba_batch_finalize", "slslam_lba_batch_solve", "slslam_lba_batch_reset",
    "slslam_lba_batch_download", "slslam_lba_batch_download_async", "slslam_lba_batch_wait", "slslam_lba_batch_refill",
    "slslam_lba_stream_create", "slslam_lba_stream_destroy", "slslam_lba_stream_submit", "slslam_lba_stream_collect", "slslam_lba_stream_stats",
    "slslam_lba_stream_build_stats", "slslam_lba_stream_batch", "slslam_lba_stream_submit_packed", "slslam_pinned_alloc", "slslam_pinned_free", "slslam_pinned_register", "slslam_pinned_unregister",
    "slslam_pinned_contains", "slslam_pack_indices", "slslam_debug_device_pack", "slslam_debug_device_pack_timed",
    "slslam_lba_batch_get_parameters", "slslam_lba_batch_get_summary",
    "slslam_lba_batch_get_trace", "slslam_lba_batch_export_device", "slslam_lba_batch_counts", "slslam_lba_batch_window_chunks", "slslam_lba_batch_path", "slslam_lba_batch_elimination",
    "slslam_lba_batch_iterations", "slslam_lba_batch_set_profiling", "slslam_lba_batch_kernel_times", "slslam_lba_batch_linearise",
    "slslam_lba_batch_covariance", "slslam_lba_batch_get_covariance", "slslam_lba_batch_covariance_stats", "slslam_lba_covariance",
    "slslam_lba_batch_report", "slslam_lba_batch_get_report", "slslam_lba_batch_report_stats", "slslam_lba_report",
    "slslam_lba_batch_segments", "slslam_lba_batch_get_segments", "slslam_lba_batch_segments_stats", "slslam_lba_segments",
    "slslam_po_solve", "slslam_po_edge_report", "slslam_po_batch_get_edge_report", "slslam_po_structure", "slslam_po_structure_level1", "slslam_po_batch_create", "slslam_po_batch_destroy", "slslam_po_batch_add", "slslam_po_batch_finalize", "slslam_po_batch_solve", "slslam_po_batch_reset", "slslam_po_batch_download", "slslam_po_batch_get_parameters", "slslam_po_batch_get_summary", "slslam_po_batch_get_trace", "slslam_po_covariance", "slslam_po_sqrt_information", "slslam_po_batch_set_covariance_pairs", "slslam_po_batch_covariance", "slslam_po_batch_get_covariance", "slslam_po_batch_covariance_stats", "slslam_po_edge_statistics", "slslam_po_gate", "slslam_po_batch_set_candidates", "slslam_po_batch_gate", "slslam_po_batch_get_gate", "slslam_po_constraint_covariance", "slslam_po_set_profiling", "slslam_po_last_timing", "slslam_debug_phase_cycles", "slslam_debug_read_cycles", "slslam_ransac_score", "slslam_ransac_generate", "slslam_ransac_motion", "slslam_ransac_motion_batch", "slslam_pose_estimator_create", "slslam_pose_estimator_destroy", "slslam_pose_estimator_run", "slslam_pose_estimator_stats", "slslam_pose_estimator_window", "slslam_pose_estimator_set_covariance", "slslam_pose_estimator_get_covariance", "slslam_line_matcher_create", "slslam_line_matcher_destroy", "slslam_line_matcher_run", "slslam_line_matcher_stats", "slslam_match_lines", "slslam_line_refiner_create", "slslam_line_refiner_destroy", "slslam_line_refiner_run", "slslam_line_refiner_stats", "slslam_lba_refine_lines", "slslam_line_triangulator_create", "slslam_line_triangulator_destroy", "slslam_line_triangulator_run", "slslam_line_triangulator_stats", "slslam_line_triangulator_timing", "slslam_lba_triangulate_lines", "slslam_debug_triangulate_host",
    "slslam_voctree_create", "slslam_voctree_load", "slslam_voctree_destroy", "slslam_place_db_create", "slslam_place_db_destroy",
    "slslam_place_db_insert", "slslam_place_db_run", "slslam_place_db_size", "slslam_place_db_virtual", "slslam_place_db_stats",
    "slslam_place_filter_create", "slslam_place_filter_destroy", "slslam_place_filter_update",
    "slslam_descriptor_matcher_create", "slslam_descriptor_matcher_destroy", "slslam_descriptor_matcher_insert",
    "slslam_descriptor_matcher_run", "slslam_descriptor_matcher_size", "slslam_descriptor_matcher_stats", "slslam_match_descriptors",
    "slslam_msld_default_options", "slslam_line_descriptor_create", "slslam_line_descriptor_destroy", "slslam_line_descriptor_run",
    "slslam_line_descriptor_stats", "slslam_line_descriptor_timing", "slslam_describe_lines",
    "slslam_line_detect_default_options", "slslam_line_detector_create", "slslam_line_detector_destroy", "slslam_line_detector_run",
    "slslam_line_detector_stats", "slslam_line_detector_timing", "slslam_detect_lines",
    "slslam_stereo_match_default_options", "slslam_stereo_matcher_create", "slslam_stereo_matcher_destroy", "slslam_stereo_matcher_run",
    "slslam_stereo_matcher_stats", "slslam_stereo_matcher_timing", "slslam_match_stereo",
    "slslam_line_track_default_options", "slslam_line_tracker_create", "slslam_line_tracker_destroy", "slslam_line_tracker_run",
    "slslam_line_tracker_reset", "slslam_line_tracker_state", "slslam_line_tracker_stats", "slslam_line_tracker_timing",
    "slslam_track_lines",
    "slslam_rectify_default_options", "slslam_rectify_smooth_taps", "slslam_stereo_rectify", "slslam_image_rectifier_create",
    "slslam_image_rectifier_destroy", "slslam_image_rectifier_run", "slslam_image_rectifier_get_map", "slslam_image_rectifier_stats",
    "slslam_image_rectifier_timing", "slslam_rectify_images",
    "slslam_voctree_train", "slslam_voctree_save", "slslam_voctree_centres", "slslam_voctree_key", "slslam_debug_voctree_step", "slslam_device_count", "slslam_release_cached_memory", "slslam_version", "slslam_status_string",
]

_lib = None


def lib():
    """Load the in-tree HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # SLSLAM_HIP_LIBRARY: a variant build of the same library (kernel experiments); still a HIP library - no fallback
    path = os.environ.get("SLSLAM_HIP_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise SlslamError(2, "libslslam_hip.so not built (run __graft_entry__.build()): " + path)
    L = C.CDLL(path)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.slslam_default_options.argtypes = [C.POINTER(SolverOptions)]
    L.slslam_default_options.restype = None
    L.slslam_lba_solve.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), C.POINTER(Summary),
                                   C.POINTER(Iteration), C.c_int, ip]
    L.slslam_lba_batch_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.slslam_lba_batch_destroy.argtypes = [vp]
    L.slslam_lba_batch_destroy.restype = None
    L.slslam_lba_batch_add.argtypes = [vp, C.POINTER(LBAWindow), ip]
    L.slslam_lba_batch_finalize.argtypes = [vp, C.POINTER(SolverOptions)]
    L.slslam_lba_batch_solve.argtypes = [vp, vp]
    L.slslam_lba_batch_reset.argtypes = [vp, vp]
    L.slslam_lba_batch_download.argtypes = [vp, vp]
    L.slslam_lba_batch_download_async.argtypes = [vp, vp]
    L.slslam_lba_batch_wait.argtypes = [vp]
    L.slslam_lba_batch_refill.argtypes = [vp, C.POINTER(LBAWindow), C.c_int, vp]
    L.slslam_lba_stream_create.argtypes = [C.c_int, C.POINTER(SolverOptions), C.c_int, C.POINTER(vp)]
    L.slslam_lba_stream_destroy.argtypes = [vp]
    L.slslam_lba_stream_destroy.restype = None
    L.slslam_lba_stream_submit.argtypes = [vp, C.POINTER(LBAWindow), C.c_int, ip]
    L.slslam_lba_stream_collect.argtypes = [vp, C.c_int, C.POINTER(Summary)]
    L.slslam_lba_stream_stats.argtypes = [vp, dp, dp, dp] + [C.POINTER(C.c_longlong)] * 4 + [ip]
    L.slslam_lba_stream_build_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 3
    L.slslam_lba_stream_submit_packed.argtypes = [vp, C.POINTER(LBAWindow), C.POINTER(C.POINTER(C.c_uint)), C.c_int, ip]
    L.slslam_lba_stream_batch.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.slslam_pinned_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.slslam_pinned_free.argtypes = [vp]
    L.slslam_pinned_register.argtypes = [vp, C.c_size_t]
    L.slslam_pinned_unregister.argtypes = [vp]
    L.slslam_pinned_contains.argtypes = [vp, C.c_size_t]
    L.slslam_pack_indices.argtypes = [C.c_int, ip, ip, ip, C.POINTER(C.c_uint)]
    L.slslam_debug_device_pack.argtypes = [C.POINTER(LBAWindow), C.c_int, ip, ip, ip, ip, ip, ip, C.POINTER(C.c_ubyte), ip, C.c_int, C.c_int,
                                           C.POINTER(C.c_ushort), C.POINTER(C.c_uint), ip]
    L.slslam_debug_device_pack_timed.argtypes = L.slslam_debug_device_pack.argtypes + [C.POINTER(C.c_ulonglong)]
    L.slslam_lba_batch_get_parameters.argtypes = [vp, C.c_int, dp]
    L.slslam_lba_batch_get_summary.argtypes = [vp, C.c_int, C.POINTER(Summary)]
    L.slslam_lba_batch_get_trace.argtypes = [vp, C.c_int, C.POINTER(Iteration), C.c_int, ip]
    L.slslam_lba_batch_export_device.argtypes = [vp, vp, vp]
    L.slslam_lba_batch_counts.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 5
    L.slslam_lba_batch_window_chunks.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.slslam_lba_batch_path.argtypes = [vp, C.POINTER(C.c_int)]
    L.slslam_lba_batch_elimination.argtypes = [vp, C.POINTER(C.c_int)]
    L.slslam_lba_batch_iterations.argtypes = [vp, vp, C.POINTER(C.c_longlong), C.c_int]
    L.slslam_lba_batch_set_profiling.argtypes = [vp, C.c_int]
    L.slslam_lba_batch_kernel_times.argtypes = [vp, dp, ip]
    L.slslam_lba_batch_linearise.argtypes = [vp, C.c_int, dp, dp, dp, dp]
    L.slslam_lba_batch_covariance.argtypes = [vp, vp, C.c_int]
    L.slslam_lba_batch_get_covariance.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp]
    L.slslam_lba_batch_covariance_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    L.slslam_lba_covariance.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), ip, ip, ip, dp, dp]
    L.slslam_lba_batch_report.argtypes = [vp, vp]
    L.slslam_lba_batch_get_report.argtypes = [vp, C.c_int, dp, dp, vp, vp]
    L.slslam_lba_batch_report_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    L.slslam_lba_report.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), dp, dp, vp, vp]
    L.slslam_lba_batch_segments.argtypes = [vp, vp, C.c_double]
    L.slslam_lba_batch_get_segments.argtypes = [vp, C.c_int, ip, dp, vp]
    L.slslam_lba_batch_segments_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    L.slslam_lba_segments.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), C.c_double, ip, dp, vp]
    L.slslam_po_solve.argtypes = [C.POINTER(POGraph), C.POINTER(SolverOptions), C.POINTER(Summary),
                                  C.POINTER(Iteration), C.c_int, ip]
    L.slslam_po_batch_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.slslam_po_batch_destroy.argtypes = [vp]
    L.slslam_po_batch_destroy.restype = None
    L.slslam_po_batch_add.argtypes = [vp, C.POINTER(POGraph), ip]
    L.slslam_po_batch_finalize.argtypes = [vp, C.POINTER(SolverOptions)]
    L.slslam_po_batch_solve.argtypes = [vp, vp]
    L.slslam_po_batch_reset.argtypes = [vp, vp]
    L.slslam_po_batch_download.argtypes = [vp, vp]
    L.slslam_po_batch_get_parameters.argtypes = [vp, C.c_int, dp]
    L.slslam_po_batch_get_summary.argtypes = [vp, C.c_int, C.POINTER(Summary)]
    L.slslam_po_batch_get_trace.argtypes = [vp, C.c_int, C.POINTER(Iteration), C.c_int, ip]
    L.slslam_po_edge_report.argtypes = [C.POINTER(POGraph), C.c_double, dp, dp]
    L.slslam_po_sqrt_information.argtypes = [dp, dp, ip]
    L.slslam_po_batch_get_edge_report.argtypes = [vp, C.c_int, dp, dp]
    L.slslam_po_covariance.argtypes = [C.POINTER(POGraph), C.c_double, C.c_int, ip, ip, ip, dp, dp]
    L.slslam_po_batch_set_covariance_pairs.argtypes = [vp, C.c_int, C.c_int, ip, ip]
    L.slslam_po_batch_covariance.argtypes = [vp, vp]
    L.slslam_po_batch_get_covariance.argtypes = [vp, C.c_int, ip, dp, dp]
    L.slslam_po_batch_covariance_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    if hasattr(L, "slslam_po_gate"):         # (a SLSLAM_HIP_LIBRARY built before the edge statistics existed still loads: tools time it)
        L.slslam_po_edge_statistics.argtypes = [C.POINTER(POEdgeItems), ip, dp, dp, dp, dp]
        L.slslam_po_gate.argtypes = [C.POINTER(POGraph), C.c_double, C.POINTER(POCandidates), ip, ip, dp, dp, dp, dp]
        L.slslam_po_batch_set_candidates.argtypes = [vp, C.c_int, C.POINTER(POCandidates)]
        L.slslam_po_batch_gate.argtypes = [vp, vp]
        L.slslam_po_batch_get_gate.argtypes = [vp, C.c_int, ip, dp, dp, dp, dp]
    if hasattr(L, "slslam_po_constraint_covariance"):      # (likewise: a library built before the motion covariances existed)
        L.slslam_po_constraint_covariance.argtypes = [C.POINTER(POConstraintItems), dp, dp, dp]
        L.slslam_pose_estimator_set_covariance.argtypes = [vp, C.c_int]
        L.slslam_pose_estimator_get_covariance.argtypes = [vp, C.c_int, ip, dp, dp, dp, ip]
    L.slslam_ransac_score.argtypes = [C.POINTER(RansacFrame), C.c_double, C.c_double, ip, C.POINTER(C.c_ulonglong)]
    L.slslam_po_structure.argtypes = [C.POINTER(POGraph), ip, C.c_int, ip, ip, ip, ip, ip, ip, ip]
    L.slslam_ransac_generate.argtypes = [C.POINTER(RansacTrials), C.c_double, dp, ip]
    L.slslam_ransac_motion.argtypes = [C.POINTER(RansacTrials), dp, C.c_double, C.c_double, C.c_double, C.c_int, ip, ip, dp,
                                       C.POINTER(C.c_ulonglong)]
    L.slslam_ransac_motion_batch.argtypes = [C.c_int, C.POINTER(RansacTrials), C.POINTER(dp), C.c_double, C.c_double, C.c_double,
                                             C.c_int, ip, ip, dp, C.POINTER(C.POINTER(C.c_ulonglong))]
    L.slslam_pose_estimator_create.argtypes = [C.c_int, C.POINTER(SolverOptions), C.c_int, C.c_int, C.POINTER(vp)]
    L.slslam_pose_estimator_destroy.argtypes = [vp]
    L.slslam_pose_estimator_destroy.restype = None
    L.slslam_pose_estimator_run.argtypes = [vp, C.c_int, C.POINTER(RansacTrials), C.POINTER(dp), C.c_double, C.c_double, C.c_double, C.c_int,
                                            C.POINTER(PoseEstimate)]
    L.slslam_pose_estimator_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 4
    L.slslam_pose_estimator_window.argtypes = [vp, C.c_int, C.POINTER(C.c_uint), dp, dp, dp, ip]
    if hasattr(L, "slslam_match_lines"):         # (likewise: a library built before the line matcher existed)
        L.slslam_line_matcher_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.slslam_line_matcher_destroy.argtypes = [vp]
        L.slslam_line_matcher_destroy.restype = None
        L.slslam_line_matcher_run.argtypes = [vp, C.c_int, C.POINTER(MatchFrame), C.c_double, C.c_double, C.c_double, C.c_double,
                                              C.POINTER(MatchResult)]
        L.slslam_line_matcher_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_match_lines.argtypes = [C.POINTER(MatchFrame), C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(MatchResult)]
    L.slslam_line_refiner_create.argtypes = [C.c_int, C.POINTER(SolverOptions), C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.slslam_line_refiner_destroy.argtypes = [vp]
    L.slslam_line_refiner_destroy.restype = None
    L.slslam_line_refiner_run.argtypes = [vp, C.c_int, C.POINTER(LBAWindow), C.POINTER(C.POINTER(LineResult)), C.POINTER(Summary)]
    L.slslam_line_refiner_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    L.slslam_lba_refine_lines.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), C.POINTER(LineResult), C.POINTER(Summary)]
    L.slslam_line_triangulator_create.argtypes = [C.c_int, C.POINTER(SolverOptions), C.c_longlong, C.c_longlong, C.POINTER(vp)]
    L.slslam_line_triangulator_destroy.argtypes = [vp]
    L.slslam_line_triangulator_destroy.restype = None
    L.slslam_line_triangulator_run.argtypes = [vp, C.c_int, C.POINTER(LBAWindow), C.c_int, C.c_double, C.c_double,
                                               C.POINTER(C.POINTER(TriangulatedLine)), C.POINTER(dp)]
    L.slslam_line_triangulator_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
    L.slslam_line_triangulator_timing.argtypes = [vp, dp]
    L.slslam_lba_triangulate_lines.argtypes = [C.POINTER(LBAWindow), C.POINTER(SolverOptions), C.c_int, C.c_double, C.c_double,
                                               C.POINTER(TriangulatedLine), dp]
    L.slslam_debug_triangulate_host.argtypes = [C.c_int, dp, dp, C.c_double, C.c_int, C.c_double, C.c_double, dp, dp, ip, ip, ip, dp]
    if hasattr(L, "slslam_place_db_run"):        # (likewise: a library built before the place recogniser existed)
        fp = C.POINTER(C.c_float)
        L.slslam_voctree_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, fp, C.POINTER(vp)]
        L.slslam_voctree_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.slslam_voctree_destroy.argtypes = [vp]
        L.slslam_voctree_destroy.restype = None
        L.slslam_place_db_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.slslam_place_db_destroy.argtypes = [vp]
        L.slslam_place_db_destroy.restype = None
        L.slslam_place_db_insert.argtypes = [vp, C.POINTER(PlaceFrame), ip, ip]
        L.slslam_place_db_run.argtypes = [vp, C.c_int, C.POINTER(PlaceFrame), C.c_int, C.POINTER(PlaceResult)]
        L.slslam_place_db_size.argtypes = [vp, ip, ip, ip]
        L.slslam_place_db_virtual.argtypes = [vp, ip, ip]
        L.slslam_place_db_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_place_filter_create.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]
        L.slslam_place_filter_destroy.argtypes = [vp]
        L.slslam_place_filter_destroy.restype = None
        L.slslam_place_filter_update.argtypes = [vp, C.c_int, fp, fp, ip, ip]
    if hasattr(L, "slslam_match_descriptors"):   # (likewise: a library built before the descriptor matcher existed)
        fp = C.POINTER(C.c_float)
        L.slslam_descriptor_matcher_create.argtypes = [C.c_int] * 6 + [C.POINTER(vp)]
        L.slslam_descriptor_matcher_destroy.argtypes = [vp]
        L.slslam_descriptor_matcher_destroy.restype = None
        L.slslam_descriptor_matcher_insert.argtypes = [vp, C.c_int, fp, ip, ip]
        L.slslam_descriptor_matcher_run.argtypes = [vp, C.c_int, C.POINTER(DescriptorQuery), C.c_double, C.c_double, C.c_int,
                                                    C.POINTER(DescriptorResult)]
        L.slslam_descriptor_matcher_size.argtypes = [vp, ip]
        L.slslam_descriptor_matcher_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_match_descriptors.argtypes = [C.c_int, C.c_int, fp, C.c_int, fp, C.c_double, C.c_double, C.POINTER(DescriptorResult)]
    if hasattr(L, "slslam_voctree_train"):      # (likewise: a library built before the tree trainer existed)
        fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
        L.slslam_voctree_train.argtypes = [C.c_int, C.POINTER(VocTreeTrainOptions), C.c_longlong, fp, fp, ip, C.POINTER(VocTreeTrainReport)]
        L.slslam_voctree_save.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, fp]
        L.slslam_voctree_centres.argtypes = [C.c_longlong, C.c_int, lp, fp, fp]
        L.slslam_voctree_key.argtypes = [C.c_ulonglong, C.c_ulonglong]
        L.slslam_voctree_key.restype = C.c_ulonglong
        L.slslam_debug_voctree_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, fp, C.c_longlong, fp, ip, ip, lp, lp]
    if hasattr(L, "slslam_describe_lines"):     # (likewise: a library built before the line descriptor existed)
        L.slslam_msld_default_options.argtypes = [C.POINTER(MsldOptions)]
        L.slslam_msld_default_options.restype = None
        L.slslam_line_descriptor_create.argtypes = [C.c_int, C.POINTER(MsldOptions), C.c_int, C.c_longlong, C.c_int, C.POINTER(vp)]
        L.slslam_line_descriptor_destroy.argtypes = [vp]
        L.slslam_line_descriptor_destroy.restype = None
        L.slslam_line_descriptor_run.argtypes = [vp, C.c_int, C.POINTER(MsldFrame), C.POINTER(MsldResult)]
        L.slslam_line_descriptor_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_line_descriptor_timing.argtypes = [vp, C.c_int, dp]
        L.slslam_describe_lines.argtypes = [C.POINTER(MsldOptions), C.POINTER(MsldFrame), C.POINTER(MsldResult)]
    if hasattr(L, "slslam_detect_lines"):       # (likewise: a library built before the line detector existed)
        L.slslam_line_detect_default_options.argtypes = [C.POINTER(LineDetectOptions)]
        L.slslam_line_detect_default_options.restype = None
        L.slslam_line_detector_create.argtypes = [C.c_int, C.POINTER(LineDetectOptions), C.c_int, C.c_longlong, C.POINTER(vp)]
        L.slslam_line_detector_destroy.argtypes = [vp]
        L.slslam_line_detector_destroy.restype = None
        L.slslam_line_detector_run.argtypes = [vp, C.c_int, C.POINTER(LineDetectFrame), C.POINTER(LineDetectResult)]
        L.slslam_line_detector_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_line_detector_timing.argtypes = [vp, C.c_int, dp]
        L.slslam_detect_lines.argtypes = [C.POINTER(LineDetectOptions), C.POINTER(LineDetectFrame), C.POINTER(LineDetectResult)]
    if hasattr(L, "slslam_match_stereo"):       # (likewise: a library built before the stereo line matcher existed)
        fp = C.POINTER(C.c_float)
        L.slslam_stereo_match_default_options.argtypes = [C.POINTER(StereoMatchOptions)]
        L.slslam_stereo_match_default_options.restype = None
        L.slslam_stereo_matcher_create.argtypes = [C.c_int] * 4 + [C.POINTER(vp)]
        L.slslam_stereo_matcher_destroy.argtypes = [vp]
        L.slslam_stereo_matcher_destroy.restype = None
        L.slslam_stereo_matcher_run.argtypes = [vp, C.POINTER(StereoMatchOptions), C.c_int, C.POINTER(StereoFrame), C.POINTER(StereoResult)]
        L.slslam_stereo_matcher_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_stereo_matcher_timing.argtypes = [vp, C.c_int, dp]
        L.slslam_match_stereo.argtypes = [C.c_int, C.POINTER(StereoMatchOptions), C.POINTER(StereoFrame), C.POINTER(StereoResult)]
    if hasattr(L, "slslam_track_lines"):        # (likewise: a library built before the line tracker existed)
        L.slslam_line_track_default_options.argtypes = [C.POINTER(LineTrackOptions)]
        L.slslam_line_track_default_options.restype = None
        L.slslam_line_tracker_create.argtypes = [C.c_int] * 4 + [C.POINTER(vp)]
        L.slslam_line_tracker_destroy.argtypes = [vp]
        L.slslam_line_tracker_destroy.restype = None
        L.slslam_line_tracker_run.argtypes = [vp, C.POINTER(LineTrackOptions), C.c_int, C.POINTER(LineTrackFrame), C.POINTER(LineTrackResult)]
        L.slslam_line_tracker_reset.argtypes = [vp, C.c_int]
        L.slslam_line_tracker_state.argtypes = [vp, ip, ip]
        L.slslam_line_tracker_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_line_tracker_timing.argtypes = [vp, C.c_int, dp]
        L.slslam_track_lines.argtypes = [C.c_int, C.POINTER(LineTrackOptions), C.c_int, C.POINTER(LineTrackFrame), C.POINTER(LineTrackResult)]
    if hasattr(L, "slslam_rectify_images"):     # (likewise: a library built before the image rectifier existed)
        bp = C.POINTER(C.c_ubyte)
        L.slslam_rectify_default_options.argtypes = [C.POINTER(RectifyOptions)]
        L.slslam_rectify_default_options.restype = None
        L.slslam_rectify_smooth_taps.argtypes = [C.c_double, ip, ip]
        L.slslam_stereo_rectify.argtypes = [C.POINTER(StereoRig), C.POINTER(RectifyCamera), C.POINTER(RectifyCamera), dp, dp]
        L.slslam_image_rectifier_create.argtypes = [C.c_int, C.POINTER(RectifyOptions), C.c_int, C.POINTER(RectifyCamera), C.c_int, C.c_longlong,
                                                    C.POINTER(vp)]
        L.slslam_image_rectifier_destroy.argtypes = [vp]
        L.slslam_image_rectifier_destroy.restype = None
        L.slslam_image_rectifier_run.argtypes = [vp, C.c_int, C.POINTER(RectifyFrame), C.POINTER(RectifyResult)]
        L.slslam_image_rectifier_get_map.argtypes = [vp, C.c_int, ip, ip, bp, dp, dp]
        L.slslam_image_rectifier_stats.argtypes = [vp] + [C.POINTER(C.c_longlong)] * 2
        L.slslam_image_rectifier_timing.argtypes = [vp, C.c_int, dp]
        L.slslam_rectify_images.argtypes = [C.POINTER(RectifyOptions), C.c_int, C.POINTER(RectifyCamera), C.c_int, C.POINTER(RectifyFrame),
                                            C.POINTER(RectifyResult)]
    L.slslam_po_set_profiling.argtypes = [C.c_int]
    L.slslam_po_last_timing.argtypes = [dp, dp, ip, ip, ip]
    L.slslam_debug_phase_cycles.argtypes = [vp, dp]
    L.slslam_debug_read_cycles.argtypes = [vp, C.POINTER(C.c_ulonglong), C.c_longlong, C.POINTER(C.c_longlong)]
    L.slslam_device_count.restype = C.c_int
    L.slslam_release_cached_memory.restype = None
    L.slslam_version.restype = C.c_char_p
    L.slslam_status_string.argtypes = [C.c_int]
    L.slslam_status_string.restype = C.c_char_p
    _lib = L
    return L


def _check(status, where):
    if status != OK:
        raise SlslamError(status, where)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class _Handle:
    """An object of the library behind a pointer: close() destroys it once, and the end of the Python object closes it.  A class names
    the library's destroy (_DESTROY) and, where it is not _h, the attribute that holds the pointer (_H)."""
    _H, _DESTROY = "_h", None

    def close(self):
        if getattr(self, self._H):
            getattr(lib(), self._DESTROY)(getattr(self, self._H))
            setattr(self, self._H, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CountedHandle(_Handle):
    """A handle that counts its calls and the times it allocated (_STATS: the library's getter of the two)."""
    _STATS = None

    def stats(self):
        c, a = C.c_longlong(0), C.c_longlong(0)
        _check(getattr(lib(), self._STATS)(getattr(self, self._H), C.byref(c), C.byref(a)), self._STATS)
        return {"calls": c.value, "allocations": a.value}


class _TimedHandle(_CountedHandle):
    """A handle whose runs can time their launches by events (_TIMING: the library's switch and getter)."""
    _TIMING = None

    def set_timing(self, enable):
        _check(getattr(lib(), self._TIMING)(self._h, int(bool(enable)), None), self._TIMING)

    def kernel_ms(self):
        """The last timed run's launches by events (after set_timing(True))."""
        ms = C.c_double(0.0)
        _check(getattr(lib(), self._TIMING)(self._h, -1, C.byref(ms)), self._TIMING)      # (-1: the switch stays)
        return ms.value


def _float_options(o, default, what, options):
    """The library's defaults (default: the *_default_options symbol) in the struct o with the given float fields replaced."""
    getattr(lib(), default)(C.byref(o))
    for k, v in options.items():
        if not hasattr(o, k):
            raise TypeError("unknown %s option %r" % (what, k))
        setattr(o, k, float(v))
    return o


def _frame_arrays(Frame, Result, items, make):
    """(Frame[n], Result[n], keep) for a run over items: make(item) -> (frame, result, what both point to, ...)."""
    n = len(items)
    frs, outs, keep = (Frame * max(n, 1))(), (Result * max(n, 1))(), []
    for i, item in enumerate(items):
        made = make(item)
        frs[i], outs[i] = made[0], made[1]
        keep.append(made[2])
    return frs, outs, keep


def default_options(**kw):
    o = SolverOptions()
    lib().slslam_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("unknown solver option %r" % k)
        setattr(o, k, v)
    return o


def release_cached_memory():
    """Frees the device block the one-shot solves of this thread keep between calls."""
    lib().slslam_release_cached_memory()


def device_count():
    return lib().slslam_device_count()


def _summary_dict(s):
    d = {k: getattr(s, k) for k, _ in Summary._fields_}
    d["termination"] = TERMINATION.get(d["termination_type"], "?")
    return d


def _trace_list(tr, n):
    return [{k: getattr(tr[i], k) for k, _ in Iteration._fields_} for i in range(n)]


class PinnedArena:
    """One block of page-locked host memory (slslam_pinned_alloc) that numpy arrays are carved out of: what a caller that streams windows
    allocates its five arrays per window from (instead of `new[]`, reference src/slam.cpp:899-903), so that the GPU reads them in place."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes) + 64
        _check(lib().slslam_pinned_alloc(self.nbytes, C.byref(self.ptr)), "slslam_pinned_alloc")
        self._buf = (C.c_ubyte * self.nbytes).from_address(self.ptr.value)
        self._mem = np.frombuffer(self._buf, dtype=np.uint8)
        self._off = (-self.ptr.value) % 64

    def take(self, a):
        """A copy of array `a` inside the block (64-byte aligned)."""
        a = np.ascontiguousarray(a)
        n = a.nbytes
        if self._off + n > self.nbytes:
            raise MemoryError("PinnedArena exhausted")
        out = self._mem[self._off:self._off + n].view(a.dtype).reshape(a.shape)
        out[...] = a
        self._off += (n + 63) & ~63
        return out

    def close(self):
        if self.ptr:
            self._mem = None
            self._buf = None
            lib().slslam_pinned_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _WindowArrays:
    """Keeps the numpy buffers a slslam_lba_window points to alive."""

    def __init__(self, w, params=None, arena=None, params_arena=None, obs_arena=None):
        self.cam = np.ascontiguousarray(w["camera_index"], dtype=np.int32)
        self.line = np.ascontiguousarray(w["line_index"], dtype=np.int32)
        self.fixed = np.ascontiguousarray(w["fixed_index"], dtype=np.int32).reshape(-1)
        self.obs = np.ascontiguousarray(w["observations"], dtype=np.float64).reshape(-1)
        self.params = np.array(w["parameters"] if params is None else params, dtype=np.float64).reshape(-1).copy()
        if arena is not None:
            self.cam, self.line, self.fixed = (arena.take(x) for x in (self.cam, self.line, self.fixed))
            self.obs = (obs_arena or arena).take(self.obs)
        if params_arena is not None or arena is not None:
            self.params = (params_arena or arena).take(self.params)
        m = len(self.cam)
        if len(self.line) != m or len(self.fixed) != 2 * m or len(self.obs) != 8 * m:
            raise ValueError("inconsistent window arrays")
        if len(self.params) != 6 * int(w["num_cameras"]) + 4 * int(w["num_lines"]):
            raise ValueError("parameter vector has the wrong length")
        self.c = LBAWindow(int(w["num_cameras"]), int(w["num_lines"]), m, _ip(self.cam), _ip(self.line),
                           _ip(self.fixed), _dp(self.obs), _dp(self.params))


def _cov_result(fn, where, num_cameras, num_lines, with_lines):
    """Calls fn(status, F, free_camera, cov_cameras, cov_lines) and trims the outputs to the window's free cameras."""
    st, nf = C.c_int(-1), C.c_int(0)
    free = np.full(max(num_cameras, 1), -1, dtype=np.int32)
    cc = np.zeros(36 * num_cameras * num_cameras)
    cl = np.zeros((num_lines, 4, 4)) if with_lines else None
    _check(fn(C.byref(st), C.byref(nf), _ip(free), _dp(cc), _dp(cl) if with_lines else None), where)
    n = 6 * nf.value
    return st.value, free[:nf.value].copy(), cc[:n * n].reshape(n, n).copy(), cl


def lba_covariance(w, params=None, with_lines=True, **opt):
    """Posterior covariance of one window at its parameters, no solve (slslam_lba_covariance; Ceres: ceres::Covariance).
    Returns (status, free_camera, cov_cameras[6F, 6F], cov_lines[L, 4, 4] or None)."""
    arr = _WindowArrays(w, params)
    o = default_options(**opt)
    return _cov_result(lambda *a: lib().slslam_lba_covariance(C.byref(arr.c), C.byref(o), *a), "slslam_lba_covariance",
                       int(w["num_cameras"]), int(w["num_lines"]), with_lines)


# slslam_lba_line_report / slslam_lba_camera_report as numpy structured dtypes (include/slslam_hip.h)
LINE_REPORT_DTYPE = np.dtype([("status", np.int32), ("num_observations", np.int32), ("num_downweighted", np.int32), ("reserved", np.int32),
                              ("sq_norm_sum", np.float64), ("cost", np.float64), ("min_pivot", np.float64)])
CAMERA_REPORT_DTYPE = np.dtype([("status", np.int32), ("num_observations", np.int32), ("num_downweighted", np.int32), ("reserved", np.int32),
                                ("sq_norm_sum", np.float64), ("cost", np.float64)])
LBA_LINE_FREE, LBA_LINE_CONSTANT, LBA_LINE_NO_OBSERVATIONS = 0, 1, 2


def _report_result(fn, where, num_cameras, num_lines, num_observations):
    """Calls fn(sq_norm, weight, lines, cameras): dict(sq_norm[M], weight[M], lines[L], cameras[C]), the last two structured arrays."""
    sq, wt = np.zeros(num_observations), np.zeros(num_observations)
    ln, cm = np.zeros(num_lines, dtype=LINE_REPORT_DTYPE), np.zeros(num_cameras, dtype=CAMERA_REPORT_DTYPE)
    _check(fn(_dp(sq), _dp(wt), ln.ctypes.data_as(C.c_void_p), cm.ctypes.data_as(C.c_void_p)), where)
    return {"sq_norm": sq, "weight": wt, "lines": ln, "cameras": cm}


def lba_report(w, params=None, **opt):
    """Per-observation |r|^2 and Huber weights, per-line and per-camera sums and the lines' smallest scaled pivot of one window at its
    parameters, no solve (slslam_lba_report; Ceres: ceres::Problem::Evaluate).  Returns the dict LBABatch.get_report returns."""
    arr = _WindowArrays(w, params)
    o = default_options(**opt)
    return _report_result(lambda *a: lib().slslam_lba_report(C.byref(arr.c), C.byref(o), *a), "slslam_lba_report",
                          int(w["num_cameras"]), int(w["num_lines"]), len(arr.cam))


# slslam_lba_line_segment as a numpy structured dtype (include/slslam_hip.h)
LINE_SEGMENT_DTYPE = np.dtype([("status", np.int32), ("num_observations", np.int32), ("num_used", np.int32), ("num_clamped", np.int32),
                               ("t_min", np.float64), ("t_max", np.float64), ("p_min", np.float64, (3,)), ("p_max", np.float64, (3,))])
SEGMENT_OK, SEGMENT_NO_OBSERVATIONS, SEGMENT_NONE = 0, 1, 2
(SEGMENT_OBS_USED, SEGMENT_OBS_USED_CLAMPED, SEGMENT_OBS_DEGENERATE, SEGMENT_OBS_BEHIND, SEGMENT_OBS_OUT_OF_RANGE,
 SEGMENT_OBS_COLLAPSED) = range(6)


def _segments_result(fn, where, num_lines, num_observations):
    """Calls fn(obs_status, obs_range, lines): dict(obs_status[M], obs_range[M, 2], and the fields of slslam_lba_line_segment as arrays [L])."""
    st, rg = np.zeros(num_observations, dtype=np.int32), np.zeros((num_observations, 2))
    ln = np.zeros(num_lines, dtype=LINE_SEGMENT_DTYPE)
    _check(fn(_ip(st), _dp(rg), ln.ctypes.data_as(C.c_void_p)), where)
    out = {"obs_status": st, "obs_range": rg}
    out.update({k: np.ascontiguousarray(ln[k]) for k in LINE_SEGMENT_DTYPE.names})
    return out


def lba_segments(w, max_range=0.0, params=None, **opt):
    """The 3-D segments of the lines of one window at its parameters, no solve (slslam_lba_segments; the reference's
    SLAM::extend_end_points per observation).  max_range <= 0: no range clamp.  Returns the dict LBABatch.get_segments returns."""
    arr = _WindowArrays(w, params)
    o = default_options(**opt)
    return _segments_result(lambda *a: lib().slslam_lba_segments(C.byref(arr.c), C.byref(o), float(max_range), *a), "slslam_lba_segments",
                            int(w["num_lines"]), len(arr.cam))


def lba_solve(w, params=None, trace_cap=64, **opt):
    """One window through slslam_lba_solve (LBAProblem::build + set_options + ceres::Solve).
    Returns (solved parameters, summary dict, trace list)."""
    arr = _WindowArrays(w, params)
    o = default_options(**opt)
    s = Summary()
    tr = (Iteration * trace_cap)()
    n = C.c_int(0)
    _check(lib().slslam_lba_solve(C.byref(arr.c), C.byref(o), C.byref(s), tr, trace_cap, C.byref(n)), "slslam_lba_solve")
    return arr.params, _summary_dict(s), _trace_list(tr, min(n.value, trace_cap))


def _line_results(num_lines):
    """A numpy structured array laid out as slslam_line_result[num_lines]."""
    return np.zeros(max(int(num_lines), 0), dtype=np.dtype(LineResult))


def lba_refine_lines(w, params=None, **opt):
    """Every line of one window refined against its cameras, all held constant (slslam_lba_refine_lines).
    Returns (parameters with the refined lines, per-line results as a structured array, totals dict)."""
    arr = _WindowArrays(w, params)
    o = default_options(**opt)
    res = _line_results(w["num_lines"])
    tot = Summary()
    _check(lib().slslam_lba_refine_lines(C.byref(arr.c), C.byref(o), res.ctypes.data_as(C.POINTER(LineResult)), C.byref(tot)),
           "slslam_lba_refine_lines")
    return arr.params, res, _summary_dict(tot)


class _LineHandle(_CountedHandle):
    """What LineRefiner and LineTriangulator share: create (_CREATE) for a capacity; per run the slslam_lba_window array (_windows, with
    the _WindowArrays that keep it alive) and one pointer per window to its result array (_pointers)."""
    _H, _CREATE = "h", None

    def __init__(self, max_lines, max_observations, device=-1, **opt):
        self.h = C.c_void_p()
        o = default_options(**opt)
        _check(getattr(lib(), self._CREATE)(device, C.byref(o), int(max_lines), int(max_observations), C.byref(self.h)), self._CREATE)

    @staticmethod
    def _windows(windows, params=None):
        arrs = [_WindowArrays(w, None if params is None else params[i]) for i, w in enumerate(windows)]
        return arrs, (LBAWindow * max(len(arrs), 1))(*[a.c for a in arrs])

    @staticmethod
    def _pointers(arrays, ctype):
        return (C.POINTER(ctype) * max(len(arrays), 1))(*[a.ctypes.data_as(C.POINTER(ctype)) for a in arrays])


class LineRefiner(_LineHandle):
    """slslam_line_refiner: every line of every window of a run refined in one launch, buffers reused between runs."""
    _DESTROY, _STATS, _CREATE = "slslam_line_refiner_destroy", "slslam_line_refiner_stats", "slslam_line_refiner_create"

    def run(self, windows, params=None):
        """windows: dicts as for lba_solve (params: their start vectors, else each window's own).
        Returns (list of parameter vectors, list of per-line structured arrays, list of totals dicts)."""
        arrs, cw = self._windows(windows, params)
        n = len(arrs)
        res = [_line_results(w["num_lines"]) for w in windows]
        tot = (Summary * max(n, 1))()
        _check(lib().slslam_line_refiner_run(self.h, n, cw, self._pointers(res, LineResult), tot), "slslam_line_refiner_run")
        return [a.params for a in arrs], res, [_summary_dict(tot[i]) for i in range(n)]


def lba_triangulate_lines(w, method=1, inverse_depth=0.1, min_parallax=0.0, **opt):
    """Every line of one window made from its observations under the window's cameras (slslam_lba_triangulate_lines): method 0 the
    reference's stereo-first start, method 1 the multi-view line where it has parallax.  Returns (parameters with the new lines,
    per-line records as a structured array, lines_av[L, 6] - rows of lines that were not made are NaN)."""
    arr = _WindowArrays(w)
    o = default_options(**opt)
    res = np.zeros(max(int(w["num_lines"]), 0), dtype=np.dtype(TriangulatedLine))
    av = np.full((max(int(w["num_lines"]), 0), 6), np.nan)
    _check(lib().slslam_lba_triangulate_lines(C.byref(arr.c), C.byref(o), int(method), float(inverse_depth), float(min_parallax),
                                              res.ctypes.data_as(C.POINTER(TriangulatedLine)), _dp(av)), "slslam_lba_triangulate_lines")
    return arr.params, res, av


class LineTriangulator(_LineHandle):
    """slslam_line_triangulator: every line of every window of a run made in one launch, buffers reused between runs."""
    _DESTROY, _STATS, _CREATE = "slslam_line_triangulator_destroy", "slslam_line_triangulator_stats", "slslam_line_triangulator_create"

    def run(self, windows, method=1, inverse_depth=0.1, min_parallax=0.0):
        """windows: dicts as for lba_solve.  Returns (list of parameter vectors, list of per-line structured arrays, list of lines_av)."""
        arrs, cw = self._windows(windows)
        res = [np.zeros(max(int(w["num_lines"]), 0), dtype=np.dtype(TriangulatedLine)) for w in windows]
        avs = [np.full((max(int(w["num_lines"]), 0), 6), np.nan) for w in windows]
        _check(lib().slslam_line_triangulator_run(self.h, len(arrs), cw, int(method), float(inverse_depth), float(min_parallax),
                                                  self._pointers(res, TriangulatedLine), self._pointers(avs, C.c_double)),
               "slslam_line_triangulator_run")
        return [a.params for a in arrs], res, avs

    def timing(self):
        """Host wall-clock milliseconds of the last run: dict(layout, upload, kernel, download, scatter)."""
        ms = np.zeros(5)
        _check(lib().slslam_line_triangulator_timing(self.h, _dp(ms)), "slslam_line_triangulator_timing")
        return dict(zip(("layout", "upload", "kernel", "download", "scatter"), ms.tolist()))


def triangulate_host(observations, cameras, baseline=0.12, method=1, inverse_depth=0.1, min_parallax=0.0):
    """One line through the device's header functions on the host (slslam_debug_triangulate_host): observations[n, 8] in the caller's
    order, cameras[n, 6] the (w, t) of each observation's camera.  Returns dict(status, num_planes, clamped, eigenvalues[4], av[6],
    offdiagonal)."""
    ob = np.ascontiguousarray(observations, dtype=np.float64).reshape(-1, 8)
    cm = np.ascontiguousarray(cameras, dtype=np.float64).reshape(-1, 6)
    if len(ob) != len(cm):
        raise ValueError("one camera per observation")
    av, eig, off = np.full(6, np.nan), np.zeros(4), C.c_double(0.0)
    st, pl, cl = C.c_int(-1), C.c_int(0), C.c_int(0)
    _check(lib().slslam_debug_triangulate_host(len(ob), _dp(ob), _dp(cm), float(baseline), int(method), float(inverse_depth),
                                               float(min_parallax), _dp(av), _dp(eig), C.byref(st), C.byref(pl), C.byref(cl), C.byref(off)),
           "slslam_debug_triangulate_host")
    return {"status": st.value, "num_planes": pl.value, "clamped": cl.value, "eigenvalues": eig, "av": av, "offdiagonal": off.value}


class LBABatch(_Handle):
    """Many independent windows resident in HBM, solved in lock-step (slslam_lba_batch_*)."""
    _DESTROY = "slslam_lba_batch_destroy"

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        _check(lib().slslam_lba_batch_create(int(device), C.byref(self._h)), "slslam_lba_batch_create")
        self.sizes = []          # (num_cameras, num_lines) per window
        self.num_obs = []        # observations per window
        self.finalized = False

    def add(self, w, params=None):
        arr = _WindowArrays(w, params)
        idx = C.c_int(-1)
        _check(lib().slslam_lba_batch_add(self._h, C.byref(arr.c), C.byref(idx)), "slslam_lba_batch_add")
        self.sizes.append((int(w["num_cameras"]), int(w["num_lines"])))
        self.num_obs.append(len(arr.cam))
        return idx.value

    def finalize(self, **opt):
        o = default_options(**opt)
        _check(lib().slslam_lba_batch_finalize(self._h, C.byref(o)), "slslam_lba_batch_finalize")
        self.finalized = True
        self.options = o

    def solve(self, stream=None):
        _check(lib().slslam_lba_batch_solve(self._h, C.c_void_p(stream or 0)), "slslam_lba_batch_solve")

    def reset(self, stream=None):
        _check(lib().slslam_lba_batch_reset(self._h, C.c_void_p(stream or 0)), "slslam_lba_batch_reset")

    def download(self, stream=None):
        _check(lib().slslam_lba_batch_download(self._h, C.c_void_p(stream or 0)), "slslam_lba_batch_download")

    def download_async(self, stream=None):
        _check(lib().slslam_lba_batch_download_async(self._h, C.c_void_p(stream or 0)), "slslam_lba_batch_download_async")

    def wait(self):
        _check(lib().slslam_lba_batch_wait(self._h), "slslam_lba_batch_wait")

    def refill(self, windows, stream=None):
        """Replaces every window of the finalized batch (slslam_lba_batch_refill); `windows`: a WindowSet or a list of window dicts."""
        ws = windows if isinstance(windows, WindowSet) else WindowSet(windows)
        _check(lib().slslam_lba_batch_refill(self._h, ws.c, len(ws), C.c_void_p(stream or 0)), "slslam_lba_batch_refill")
        self.sizes = list(ws.sizes)
        self.num_obs = list(ws.num_obs)

    def export_device(self, device_ptr, stream=None):
        _check(lib().slslam_lba_batch_export_device(self._h, C.c_void_p(device_ptr), C.c_void_p(stream or 0)),
               "slslam_lba_batch_export_device")

    def parameters(self, i):
        c, l = self.sizes[i]
        out = np.empty(6 * c + 4 * l)
        _check(lib().slslam_lba_batch_get_parameters(self._h, i, _dp(out)), "slslam_lba_batch_get_parameters")
        return out

    def summary(self, i):
        s = Summary()
        _check(lib().slslam_lba_batch_get_summary(self._h, i, C.byref(s)), "slslam_lba_batch_get_summary")
        return _summary_dict(s)

    def trace(self, i, cap=64):
        tr = (Iteration * cap)()
        n = C.c_int(0)
        _check(lib().slslam_lba_batch_get_trace(self._h, i, tr, cap, C.byref(n)), "slslam_lba_batch_get_trace")
        return _trace_list(tr, min(n.value, cap))

    def counts(self):
        v = [C.c_longlong(0) for _ in range(5)]
        _check(lib().slslam_lba_batch_counts(self._h, *[C.byref(x) for x in v]), "slslam_lba_batch_counts")
        return dict(zip(["windows", "cameras", "free_cameras", "lines", "observations"], [x.value for x in v]))

    def path(self):
        v = C.c_int(-1)
        _check(lib().slslam_lba_batch_path(self._h, C.byref(v)), "slslam_lba_batch_path")
        return v.value

    def elimination(self):
        """The lba_elimination value that reproduces the sweep this batch runs (what the automatic choice resolved to)."""
        v = C.c_int(-1)
        _check(lib().slslam_lba_batch_elimination(self._h, C.byref(v)), "slslam_lba_batch_elimination")
        return v.value

    def window_chunks(self, i):
        v = C.c_int(0)
        _check(lib().slslam_lba_batch_window_chunks(self._h, int(i), C.byref(v)), "slslam_lba_batch_window_chunks")
        return v.value

    def iterations(self, stream=None, clear=False):
        v = C.c_longlong(0)
        _check(lib().slslam_lba_batch_iterations(self._h, C.c_void_p(stream or 0), C.byref(v), int(clear)),
               "slslam_lba_batch_iterations")
        return v.value

    def total_parameters(self):
        return sum(6 * c + 4 * l for c, l in self.sizes)

    def set_profiling(self, enable):
        _check(lib().slslam_lba_batch_set_profiling(self._h, int(bool(enable))), "slslam_lba_batch_set_profiling")

    def kernel_times(self):
        ms = np.zeros(8)
        n = np.zeros(8, dtype=np.int32)
        _check(lib().slslam_lba_batch_kernel_times(self._h, _dp(ms), _ip(n)), "slslam_lba_batch_kernel_times")
        return {KERNEL_FAMILIES[i]: (float(ms[i]), int(n[i])) for i in range(8)}

    def _derived_stats(self, symbol):
        """{"calls", "allocations"} of one derived result (covariance, report, segments: they share a protocol and the shape of this call)."""
        v = [C.c_longlong(0) for _ in range(2)]
        _check(getattr(lib(), symbol)(self._h, *[C.byref(x) for x in v]), symbol)
        return dict(zip(["calls", "allocations"], [x.value for x in v]))

    def covariance(self, stream=None, with_lines=True):
        """Enqueues the posterior covariances of every window at its current device parameters (slslam_lba_batch_covariance);
        download() brings them back."""
        _check(lib().slslam_lba_batch_covariance(self._h, C.c_void_p(stream or 0), int(bool(with_lines))), "slslam_lba_batch_covariance")
        self._cov_lines = bool(with_lines)

    def get_covariance(self, i):
        """(status, free_camera, cov_cameras[6F, 6F], cov_lines[L, 4, 4] or None) of window i, after download()."""
        c, l = self.sizes[i]
        return _cov_result(lambda *a: lib().slslam_lba_batch_get_covariance(self._h, int(i), *a), "slslam_lba_batch_get_covariance",
                           c, l, getattr(self, "_cov_lines", False))

    def covariance_stats(self):
        return self._derived_stats("slslam_lba_batch_covariance_stats")

    def report(self, stream=None):
        """Enqueues the report on every window at its current device parameters (slslam_lba_batch_report); download() brings it back."""
        _check(lib().slslam_lba_batch_report(self._h, C.c_void_p(stream or 0)), "slslam_lba_batch_report")

    def get_report(self, i):
        """dict(sq_norm[M], weight[M], lines[L] (LINE_REPORT_DTYPE), cameras[C] (CAMERA_REPORT_DTYPE)) of window i, after download()."""
        c, l = self.sizes[i]
        return _report_result(lambda *a: lib().slslam_lba_batch_get_report(self._h, int(i), *a), "slslam_lba_batch_get_report",
                              c, l, self.num_obs[i])

    def report_stats(self):
        return self._derived_stats("slslam_lba_batch_report_stats")

    def segments(self, max_range=0.0, stream=None):
        """Enqueues the 3-D segments of the lines of every window at its current device parameters (slslam_lba_batch_segments);
        download() brings them back, get_segments(i) reads window i.  max_range <= 0: no range clamp."""
        _check(lib().slslam_lba_batch_segments(self._h, C.c_void_p(stream or 0), float(max_range)), "slslam_lba_batch_segments")

    def get_segments(self, i):
        """dict(obs_status[M], obs_range[M, 2], status[L], num_observations[L], num_used[L], num_clamped[L], t_min[L], t_max[L],
        p_min[L, 3], p_max[L, 3]) of window i, after download()."""
        return _segments_result(lambda *a: lib().slslam_lba_batch_get_segments(self._h, int(i), *a), "slslam_lba_batch_get_segments",
                                self.sizes[i][1], self.num_obs[i])

    def segments_stats(self):
        return self._derived_stats("slslam_lba_batch_segments_stats")

    def linearise(self, i, num_observations):
        m = int(num_observations)
        r, jc, jl, c = np.zeros((m, 4)), np.zeros((m, 4, 6)), np.zeros((m, 4, 4)), np.zeros(1)
        _check(lib().slslam_lba_batch_linearise(self._h, i, _dp(r), _dp(jc), _dp(jl), _dp(c)), "slslam_lba_batch_linearise")
        return float(c[0]), r, jc, jl


class WindowSet:
    """A C array of slslam_lba_window over numpy buffers that stay alive with it (what a caller of the stream / refill entry points
    holds: the five arrays of every window, reference src/slam.cpp:899-921)."""

    def __init__(self, windows, pinned=False, packed=False):
        """pinned: the arrays live in page-locked blocks (slslam_pinned_alloc): the device build reads them in place and the solved
        parameters are written back into them by the GPU.  packed: the three index arrays of every window are ALSO held narrowed to one
        32-bit word per observation (slslam_pack_indices), and LBAStream.submit hands those over instead (slslam_lba_stream_submit_packed)."""
        self.arena = self.params_arena = self.obs_arena = None
        self.packed = None
        if pinned:
            # three blocks - the index arrays of all windows, their observation arrays, their parameter arrays (derive() gives a set parameter
            # arrays of its own over the same inputs): arrays that lie next to each other go up in a few large copies of the copy engine, and the
            # index arrays - which the host threads narrow on the way - do not sit between the observation arrays
            self.arena = PinnedArena(sum(16 * len(w["camera_index"]) + 3 * 64 for w in windows) + 4096)
            self.obs_arena = PinnedArena(sum(64 * len(w["camera_index"]) + 64 for w in windows) + 4096)
            self.params_arena = PinnedArena(sum(8 * (6 * int(w["num_cameras"]) + 4 * int(w["num_lines"])) + 64 for w in windows) + 4096)
        if pinned and packed:
            self.arena.close()
            self.arena = PinnedArena(sum(4 * len(w["camera_index"]) + 64 for w in windows) + 4096)
        self.arrays = [_WindowArrays(w, arena=None if packed else self.arena, params_arena=self.params_arena, obs_arena=self.obs_arena) for w in windows]
        if packed:
            self.packed_arrays = []
            for a in self.arrays:
                pk = np.zeros(len(a.cam), dtype=np.uint32)
                _check(lib().slslam_pack_indices(len(a.cam), _ip(a.cam), _ip(a.line), _ip(a.fixed), pk.ctypes.data_as(C.POINTER(C.c_uint))), "slslam_pack_indices")
                if self.arena is not None:
                    pk = self.arena.take(pk)
                    a.obs = self.obs_arena.take(a.obs)
                    a.c = LBAWindow(a.c.num_cameras, a.c.num_lines, a.c.num_observations, _ip(a.cam), _ip(a.line), _ip(a.fixed), _dp(a.obs), _dp(a.params))
                self.packed_arrays.append(pk)
            self.packed = (C.POINTER(C.c_uint) * max(len(self.arrays), 1))(*[p_.ctypes.data_as(C.POINTER(C.c_uint)) for p_ in self.packed_arrays])
        self.c = (LBAWindow * max(len(self.arrays), 1))(*[a.c for a in self.arrays])
        self.sizes = [(int(w["num_cameras"]), int(w["num_lines"])) for w in windows]
        self.num_obs = [int(a.c.num_observations) for a in self.arrays]

    def __len__(self):
        return len(self.arrays)

    def parameters(self, i):
        return self.arrays[i].params

    def derive(self, order):
        """Another set over the SAME input arrays (indices, observations: read only) in another window order, with parameter arrays of its
        own holding the present values of this set's - what a bench needs to submit many distinct sets without holding each set's gigabyte
        of observations once more.  Page-locked like this set."""
        import copy
        out = WindowSet.__new__(WindowSet)
        out.arena = out.params_arena = out.obs_arena = None
        out.packed = None
        if self.packed is not None:
            out.packed_arrays = [self.packed_arrays[j] for j in order]
            out.packed = (C.POINTER(C.c_uint) * max(len(order), 1))(*[p_.ctypes.data_as(C.POINTER(C.c_uint)) for p_ in out.packed_arrays])
        if self.arena is not None:
            out.params_arena = PinnedArena(sum(a.params.nbytes + 64 for a in self.arrays) + 4096)
        out.arrays = []
        for j in order:
            a = copy.copy(self.arrays[j])
            a.params = out.params_arena.take(a.params) if out.params_arena is not None else a.params.copy()
            a.c = LBAWindow(a.c.num_cameras, a.c.num_lines, a.c.num_observations, _ip(a.cam), _ip(a.line), _ip(a.fixed), _dp(a.obs), _dp(a.params))
            out.arrays.append(a)
        out.c = (LBAWindow * max(len(out.arrays), 1))(*[a.c for a in out.arrays])
        out.sizes = [self.sizes[j] for j in order]
        out.num_obs = [self.num_obs[j] for j in order]
        out._base = self                      # (the shared arrays live in the base set's block)
        return out

    def close(self):
        self.arrays = [] if (self.arena is not None or self.params_arena is not None) else self.arrays
        for name in ("arena", "params_arena", "obs_arena"):
            if getattr(self, name, None) is not None:
                getattr(self, name).close()
                setattr(self, name, None)


class _BatchView(LBABatch):
    """A batch owned by somebody else (a stream's slot): the getters of LBABatch, no destroy."""

    def __init__(self, handle, sizes, num_obs=()):
        self._h = handle
        self.sizes = list(sizes)
        self.num_obs = list(num_obs)
        self.finalized = True

    def close(self):
        self._h = C.c_void_p()


def debug_device_pack(w, grouping=0, clocks=None):
    """slslam_debug_device_pack: one window through the device build alone; returns (status bits, dict as tests/test_host_side.py::_pack).
    clocks: a numpy uint64[16] that receives the shader-clock stamps of k_build_window's phases."""
    arr = _WindowArrays(w)
    Cn, L, M = int(w["num_cameras"]), int(w["num_lines"]), len(arr.cam)
    counts = np.zeros(5, dtype=np.int32)
    lo, lp = np.zeros(max(L, 1), dtype=np.int32), np.zeros(L + 1, dtype=np.int32)
    oo, oc, cf = np.zeros(max(M, 1), dtype=np.int32), np.zeros(max(M, 1), dtype=np.int32), np.zeros(max(Cn, 1), dtype=np.int32)
    max_tiles, max_items = L + 8, 64 * M + 8
    tiles = np.zeros(4 * max_tiles, dtype=np.int32)
    items = np.zeros(2 * max_items, dtype=np.uint8)
    lane_map = np.zeros(64 * max_tiles, dtype=np.uint16)
    desc = np.zeros(max(L, 1), dtype=np.uint32)
    st = C.c_int(-1)
    _check(lib().slslam_debug_device_pack_timed(C.byref(arr.c), int(grouping), _ip(counts), _ip(lo), _ip(lp), _ip(oo), _ip(oc), _ip(tiles),
                                                items.ctypes.data_as(C.POINTER(C.c_ubyte)), _ip(cf), max_tiles, max_items,
                                                lane_map.ctypes.data_as(C.POINTER(C.c_ushort)), desc.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(st),
                                                clocks.ctypes.data_as(C.POINTER(C.c_ulonglong)) if clocks is not None else None),
           "slslam_debug_device_pack")
    return st.value, dict(desc=desc[:L], Cf=int(counts[0]), ntiles=int(counts[1]), nitems=int(counts[2]), nfree=int(counts[3]), nkept=int(counts[4]),
                          line_order=lo[:L], line_ptr=lp, ob_orig=oo[:M], ob_cam=oc[:M], cam_cf=cf[:Cn],
                          tiles=tiles[:4 * int(counts[1])].reshape(-1, 4), items=items[:2 * int(counts[2])].reshape(-1, 2),
                          lane_map=lane_map[:64 * int(counts[1])].reshape(-1, 64))


class LBAStream(_Handle):
    """slslam_lba_stream_*: `depth` refillable batches in flight; submit(WindowSet) -> ticket, collect(ticket) -> summaries, the solved
    parameters land in the WindowSet's parameter arrays."""
    _DESTROY = "slslam_lba_stream_destroy"

    def __init__(self, device=-1, depth=3, **opt):
        self._h = C.c_void_p()
        o = default_options(**opt)
        _check(lib().slslam_lba_stream_create(int(device), C.byref(o), int(depth), C.byref(self._h)), "slslam_lba_stream_create")
        self._live = {}

    def submit(self, ws):
        t = C.c_int(-1)
        if getattr(ws, "packed", None) is not None:
            _check(lib().slslam_lba_stream_submit_packed(self._h, ws.c, ws.packed, len(ws), C.byref(t)), "slslam_lba_stream_submit_packed")
        else:
            _check(lib().slslam_lba_stream_submit(self._h, ws.c, len(ws), C.byref(t)), "slslam_lba_stream_submit")
        self._live[t.value] = ws
        return t.value

    def collect(self, ticket, want_summaries=True):
        ws = self._live.pop(ticket, None)
        if ws is None:                                   # not a ticket in flight: the library says so
            _check(lib().slslam_lba_stream_collect(self._h, int(ticket), None), "slslam_lba_stream_collect")
            raise SlslamError(5, "slslam_lba_stream_collect")
        sm = (Summary * max(len(ws), 1))() if want_summaries else None
        _check(lib().slslam_lba_stream_collect(self._h, int(ticket), sm), "slslam_lba_stream_collect")
        return [_summary_dict(sm[i]) for i in range(len(ws))] if want_summaries else None

    def batch_of(self, ticket, ws):
        """The batch that served `ticket` (its traces, chunk cuts, sweep): valid until the slot is submitted to again."""
        h = C.c_void_p()
        _check(lib().slslam_lba_stream_batch(self._h, int(ticket), C.byref(h)), "slslam_lba_stream_batch")
        return _BatchView(h, ws.sizes, ws.num_obs)

    def build_stats(self):
        q = [C.c_longlong(0) for _ in range(3)]
        _check(lib().slslam_lba_stream_build_stats(self._h, *[C.byref(x) for x in q]), "slslam_lba_stream_build_stats")
        return {"device_builds": q[0].value, "zero_copy": q[1].value, "fallback_windows": q[2].value}

    def stats(self):
        d = [C.c_double(0) for _ in range(3)]
        q = [C.c_longlong(0) for _ in range(4)]
        t = C.c_int(0)
        _check(lib().slslam_lba_stream_stats(self._h, *[C.byref(x) for x in d], *[C.byref(x) for x in q], C.byref(t)), "slslam_lba_stream_stats")
        return {"ms_submit": d[0].value, "ms_collect_wait": d[1].value, "ms_collect_copy": d[2].value,
                "refills": q[0].value, "builds": q[1].value, "windows": q[2].value, "lm_iterations": q[3].value, "host_threads": t.value}


def po_solve(g, params=None, trace_cap=64, **opt):
    """One pose graph through slslam_po_solve (POProblem::build + set_options + ceres::Solve).  g["sqrt_information"] ([E, 6, 6] or
    [36E], optional): the edges' square-root information matrices W_e - blocks are whitened by them; absent or None: identity."""
    cg, (i1, i2, cons, x, _) = _po_graph(g, params)
    o = default_options(**opt)
    s = Summary()
    tr = (Iteration * trace_cap)()
    n = C.c_int(0)
    _check(lib().slslam_po_solve(C.byref(cg), C.byref(o), C.byref(s), tr, trace_cap, C.byref(n)), "slslam_po_solve")
    return x, _summary_dict(s), _trace_list(tr, min(n.value, trace_cap))


def po_edge_report(g, params=None, po_huber_delta=0.0):
    """Per-edge (sq_norm, weight) at the graph's parameters (slslam_po_edge_report): |Te|^2 of every edge - |W_e Te|^2 when the graph
    has g["sqrt_information"] - and the weight rho' that HuberLoss(po_huber_delta) gives it (1 for inliers and without a loss); the
    smallest weight marks the loop closure to drop."""
    cg, (i1, i2, cons, x, _) = _po_graph(g, params)
    sq, wt = np.zeros(len(i1)), np.zeros(len(i1))
    _check(lib().slslam_po_edge_report(C.byref(cg), float(po_huber_delta), _dp(sq), _dp(wt)), "slslam_po_edge_report")
    return sq, wt


def _po_pairs(pairs):
    pr = np.ascontiguousarray(np.asarray([] if pairs is None else pairs, dtype=np.int32).reshape(-1, 2))
    return np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])


def po_covariance(g, pairs=None, po_huber_delta=0.0, params=None):
    """Posterior covariance of one pose graph at its parameters (slslam_po_covariance; ceres::Covariance): (status,
    cov_poses[N, 6, 6] - the marginal of every pose, zeros for the constant pose and unreferenced ones -, cov_pairs[P, 6, 6] - the
    cross blocks Sigma_ab of `pairs` [(a, b), ...], rows of a, columns of b).  status COV_SINGULAR: all zeros."""
    cg, (i1, i2, cons, x, _) = _po_graph(g, params)
    pa, pb = _po_pairs(pairs)
    st = C.c_int(-1)
    cp, cq = np.zeros((int(g["num_poses"]), 6, 6)), np.zeros((len(pa), 6, 6))
    _check(lib().slslam_po_covariance(C.byref(cg), float(po_huber_delta), len(pa), _ip(pa), _ip(pb), C.byref(st), _dp(cp), _dp(cq)),
           "slslam_po_covariance")
    return st.value, cp, cq


def _po_arrays(g, params=None):
    i1 = np.ascontiguousarray(g["pose_index_1"], dtype=np.int32)
    i2 = np.ascontiguousarray(g["pose_index_2"], dtype=np.int32)
    cons = np.ascontiguousarray(g["constraints"], dtype=np.float64).reshape(-1)
    x = np.array(g["parameters"] if params is None else params, dtype=np.float64).reshape(-1).copy()
    if len(i2) != len(i1) or len(cons) != 6 * len(i1) or len(x) != 6 * int(g["num_poses"]):
        raise ValueError("inconsistent pose-graph arrays")
    return i1, i2, cons, x


def _po_weights(g, num_edges):
    """g["sqrt_information"] as the flat [36E] array the C ABI takes, or None (absent or None: identity on every edge)."""
    w = g.get("sqrt_information") if hasattr(g, "get") else None
    if w is None:
        return None
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if len(w) != 36 * num_edges:
        raise ValueError("sqrt_information must hold 36 doubles per edge")
    return w


def _po_graph(g, params=None):
    """The POGraph of a graph dict and the arrays it points into (keep them alive for as long as the struct is used)."""
    i1, i2, cons, x = _po_arrays(g, params)
    w = _po_weights(g, len(i1))
    return POGraph(int(g["num_poses"]), len(i1), _ip(i1), _ip(i2), _dp(cons), _dp(x), None if w is None else _dp(w)), (i1, i2, cons, x, w)


def po_sqrt_information(cov):
    """(status, W[6, 6]) from a symmetric positive-definite 6 x 6 covariance (slslam_po_sqrt_information; host only): W lower
    triangular with W^T W = cov^-1 - an edge's entry of g["sqrt_information"], e.g. from a block lba_covariance or po_covariance
    returned.  status COV_SINGULAR: zeros."""
    cv = np.ascontiguousarray(cov, dtype=np.float64).reshape(-1)
    if len(cv) != 36:
        raise ValueError("cov must be 6 x 6")
    out = np.zeros((6, 6))
    st = C.c_int(-1)
    _check(lib().slslam_po_sqrt_information(_dp(cv), _dp(out), C.byref(st)), "slslam_po_sqrt_information")
    return st.value, out


def _opt36(a, n):
    """An optional [n, 6, 6] array as the flat array the C ABI takes, or None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if len(a) != 36 * n:
        raise ValueError("a covariance array must hold 36 doubles per item")
    return a


def _edge_outputs(n):
    return np.full(n, -1, dtype=np.int32), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros(n)


def _edge_dict(st, err, cov, w, m2):
    return dict(status=st, error=err, cov=cov, sqrt_information=w, mahalanobis2=m2)


def po_edge_statistics(pose_a, pose_b, constraints, cov_aa=None, cov_bb=None, cov_ab=None, cov_meas=None, sigma2=1.0):
    """Statistics of n edges under the covariance of their poses (slslam_po_edge_statistics): dict(status[n], error[n, 6] = Te,
    cov[n, 6, 6] = S = sigma2 J Sigma J^T + R, sqrt_information[n, 6, 6] = W with W^T W = S^-1, mahalanobis2[n] = |W Te|^2).  Any
    covariance array may be None (zeros).  A COV_SINGULAR item has zeros but for its error."""
    xa = np.ascontiguousarray(pose_a, dtype=np.float64).reshape(-1)
    xb = np.ascontiguousarray(pose_b, dtype=np.float64).reshape(-1)
    cc = np.ascontiguousarray(constraints, dtype=np.float64).reshape(-1)
    n = len(xa) // 6
    if len(xa) != 6 * n or len(xb) != 6 * n or len(cc) != 6 * n:
        raise ValueError("inconsistent edge arrays")
    blocks = [_opt36(a, n) for a in (cov_aa, cov_bb, cov_ab, cov_meas)]
    it = POEdgeItems(n, _dp(xa), _dp(xb), _dp(cc), *[None if a is None else _dp(a) for a in blocks], float(sigma2))
    out = _edge_outputs(n)
    _check(lib().slslam_po_edge_statistics(C.byref(it), _ip(out[0]), *[_dp(a) for a in out[1:]]), "slslam_po_edge_statistics")
    return _edge_dict(*out)


def _po_candidates(candidates):
    """The POCandidates of dict(pose_a, pose_b, constraints, cov_meas (optional), sigma2 (default 1)) and the arrays it points into."""
    pa = np.ascontiguousarray(candidates["pose_a"], dtype=np.int32).reshape(-1)
    pb = np.ascontiguousarray(candidates["pose_b"], dtype=np.int32).reshape(-1)
    cc = np.ascontiguousarray(candidates["constraints"], dtype=np.float64).reshape(-1)
    if len(pb) != len(pa) or len(cc) != 6 * len(pa):
        raise ValueError("inconsistent candidate arrays")
    r = _opt36(candidates.get("cov_meas"), len(pa))
    return POCandidates(len(pa), _ip(pa), _ip(pb), _dp(cc), None if r is None else _dp(r), float(candidates.get("sigma2", 1.0))), (pa, pb, cc, r)


def po_gate(g, candidates, po_huber_delta=0.0, params=None):
    """Candidate edges against one graph at its parameters (slslam_po_gate): (cov_status, dict as po_edge_statistics returns).
    candidates: dict(pose_a[M], pose_b[M], constraints[M, 6], cov_meas[M, 6, 6] or absent, sigma2)."""
    cg, keep = _po_graph(g, params)
    cc, keep2 = _po_candidates(candidates)
    out = _edge_outputs(cc.num)
    st = C.c_int(-1)
    _check(lib().slslam_po_gate(C.byref(cg), float(po_huber_delta), C.byref(cc), C.byref(st), _ip(out[0]), *[_dp(a) for a in out[1:]]), "slslam_po_gate")
    return st.value, _edge_dict(*out)


def po_constraint_covariance(pose_a, pose_b, constraints, cov_constraint=None, sigma2=1.0):
    """The covariance of n constraints in the coordinates of their edges' errors (slslam_po_constraint_covariance): dict(error[n, 6] = Te,
    jacobian[n, 6, 6] = J_C = dTe/dC, cov_meas[n, 6, 6] = sigma2 J_C cov_constraint J_C^T) - cov_meas is the R po_edge_statistics,
    po_gate and POBatch.set_candidates take.  cov_constraint [n, 6, 6] over (w_C, t_C), e.g. PoseEstimator's; None: zeros."""
    xa = np.ascontiguousarray(pose_a, dtype=np.float64).reshape(-1)
    xb = np.ascontiguousarray(pose_b, dtype=np.float64).reshape(-1)
    cc = np.ascontiguousarray(constraints, dtype=np.float64).reshape(-1)
    n = len(xa) // 6
    if len(xa) != 6 * n or len(xb) != 6 * n or len(cc) != 6 * n:
        raise ValueError("inconsistent constraint arrays")
    sc = _opt36(cov_constraint, n)
    it = POConstraintItems(n, _dp(xa), _dp(xb), _dp(cc), None if sc is None else _dp(sc), float(sigma2))
    err, jac, cov = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    _check(lib().slslam_po_constraint_covariance(C.byref(it), _dp(err), _dp(jac), _dp(cov)), "slslam_po_constraint_covariance")
    return dict(error=err, jacobian=jac, cov_meas=cov)


def motion_candidates(estimates, pose_a, pose_b, x):
    """Loop-closure candidates from motion estimates: (candidates, skipped).  estimates: the dicts PoseEstimator(covariance=True).run
    returns, estimate k the motion from graph pose pose_a[k] to pose_b[k]; x: the graph's [N, 6] poses.  candidates is the dict po_gate /
    POBatch.set_candidates take - constraints = the estimates' `constraint`, cov_meas = J_C (sigma2 covariance) J_C^T by
    po_constraint_covariance - with the candidates' own sigma2 left out (the default 1): set it to the graph's noise variance.
    Estimates that are not OK, or whose covariance is singular, are left out; skipped lists their indices."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 6)
    pa, pb = np.asarray(pose_a, dtype=np.int32).reshape(-1), np.asarray(pose_b, dtype=np.int32).reshape(-1)
    if len(pa) != len(estimates) or len(pb) != len(estimates):
        raise ValueError("one pose pair per estimate")
    keep = [k for k, e in enumerate(estimates) if e.get("status") == "OK" and e.get("cov_status") == COV_OK]
    skipped = [k for k in range(len(estimates)) if k not in keep]
    cons = np.array([estimates[k]["constraint"] for k in keep], dtype=np.float64).reshape(-1, 6)
    sig = np.array([estimates[k]["sigma2"] * np.asarray(estimates[k]["covariance"], dtype=np.float64) for k in keep]).reshape(-1, 6, 6)
    r = po_constraint_covariance(x[pa[keep]], x[pb[keep]], cons, sig, 1.0)
    return dict(pose_a=pa[keep], pose_b=pb[keep], constraints=cons, cov_meas=r["cov_meas"]), skipped


def se3_inverse(p):
    """P^-1 of a pose [angle-axis | translation] (the reference's gc_T_inv)."""
    p = np.asarray(p, dtype=np.float64)
    return np.concatenate([-p[:3], -_aa_rotate(-p[:3], p[3:])])


def _aa_rotate(w, v):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return v + np.cross(w, v)
    k = w / th
    return v * np.cos(th) + np.cross(k, v) * np.sin(th) + k * np.dot(k, v) * (1.0 - np.cos(th))


def _aa_to_quat(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.array([1.0, 0.5 * w[0], 0.5 * w[1], 0.5 * w[2]])
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) / th * w])


def se3_compose(t21, t10):
    """T20 = T21 T10 on [angle-axis | translation] (the reference's gc_T_20)."""
    t21, t10 = np.asarray(t21, dtype=np.float64), np.asarray(t10, dtype=np.float64)
    a, b = _aa_to_quat(t21[:3]), _aa_to_quat(t10[:3])
    q = np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])
    s = np.linalg.norm(q[1:])
    w = 2.0 * q[1:] if s < 1e-300 else 2.0 * np.arctan2(s, q[0]) / s * q[1:] if q[0] >= 0 else 2.0 * np.arctan2(-s, -q[0]) / s * q[1:]
    return np.concatenate([w, _aa_rotate(t21[:3], t10[3:]) + t21[3:]])


def lba_odometry_edges(cov_result, cameras, pairs, sigma2=1.0):
    """Odometry edges between cameras of ONE solved LBA window, weighted by the window's posterior covariance.  cov_result: what
    lba_covariance / LBABatch.get_covariance returned for the window - (status, free_camera[F], cov_cameras[6F, 6F], cov_lines);
    cameras [C, 6]: the solved camera parameters; pairs [(a, b), ...].  Returns (constraints [P, 6] with
    C = T_b o T_a^-1, the reference's src/slam.cpp:1410-1412, dict as po_edge_statistics returns): sqrt_information[k] is edge k's W_e.
    A constant camera contributes zero blocks; a pair of two constant cameras is COV_SINGULAR."""
    cams = np.asarray(cameras, dtype=np.float64).reshape(-1, 6)
    free = [int(c) for c in cov_result[1]] if cov_result[0] == COV_OK else []
    F = len(free)
    sig = np.asarray(cov_result[2], dtype=np.float64)[:6 * F, :6 * F].reshape(F, 6, F, 6).transpose(0, 2, 1, 3)
    pos = {c: k for k, c in enumerate(free)}
    P = len(pairs)
    xa, xb, cc = np.zeros((P, 6)), np.zeros((P, 6)), np.zeros((P, 6))
    saa, sbb, sab = np.zeros((P, 6, 6)), np.zeros((P, 6, 6)), np.zeros((P, 6, 6))
    for k, (a, b) in enumerate(pairs):
        xa[k], xb[k] = cams[a], cams[b]
        cc[k] = se3_compose(cams[b], se3_inverse(cams[a]))
        ka, kb = pos.get(int(a)), pos.get(int(b))
        if ka is not None:
            saa[k] = sig[ka, ka]
        if kb is not None:
            sbb[k] = sig[kb, kb]
        if ka is not None and kb is not None:
            sab[k] = sig[ka, kb]
    return cc, po_edge_statistics(xa, xb, cc, saa, sbb, sab, None, sigma2)


class POBatch(_Handle):
    """Many pose graphs solved together (slslam_po_batch_*): each graph gets what po_solve gives it.  add() copies the graph,
    finalize() uploads (the first call that needs a device), solve() enqueues, download() waits and brings the results back."""
    _DESTROY = "slslam_po_batch_destroy"

    def __init__(self, device=-1):
        self._h = C.c_void_p()
        _check(lib().slslam_po_batch_create(int(device), C.byref(self._h)), "slslam_po_batch_create")
        self._n = []
        self._e = []
        self._pairs = {}
        self._cands = {}

    def add(self, g, params=None):
        cg, (i1, i2, cons, x, _) = _po_graph(g, params)
        idx = C.c_int(-1)
        _check(lib().slslam_po_batch_add(self._h, C.byref(cg), C.byref(idx)), "slslam_po_batch_add")
        self._n.append(int(g["num_poses"]))
        self._e.append(len(i1))
        return idx.value

    def __len__(self):
        return len(self._n)

    def finalize(self, **opt):
        o = default_options(**opt)
        _check(lib().slslam_po_batch_finalize(self._h, C.byref(o)), "slslam_po_batch_finalize")

    def solve(self, stream=None):
        _check(lib().slslam_po_batch_solve(self._h, C.c_void_p(stream or 0)), "slslam_po_batch_solve")

    def reset(self, stream=None):
        _check(lib().slslam_po_batch_reset(self._h, C.c_void_p(stream or 0)), "slslam_po_batch_reset")

    def download(self, stream=None):
        _check(lib().slslam_po_batch_download(self._h, C.c_void_p(stream or 0)), "slslam_po_batch_download")

    def parameters(self, i):
        out = np.zeros(6 * self._n[i])
        _check(lib().slslam_po_batch_get_parameters(self._h, int(i), _dp(out)), "slslam_po_batch_get_parameters")
        return out

    def edge_report(self, i):
        """(sq_norm, weight) of graph i's edges at its returned parameters, under the batch's po_huber_delta."""
        sq, wt = np.zeros(self._e[i]), np.zeros(self._e[i])
        _check(lib().slslam_po_batch_get_edge_report(self._h, int(i), _dp(sq), _dp(wt)), "slslam_po_batch_get_edge_report")
        return sq, wt

    def set_covariance_pairs(self, i, pairs):
        """The pairs [(a, b), ...] whose cross blocks covariance() reports for graph i (replaces the previous list)."""
        pa, pb = _po_pairs(pairs)
        _check(lib().slslam_po_batch_set_covariance_pairs(self._h, int(i), len(pa), _ip(pa), _ip(pb)), "slslam_po_batch_set_covariance_pairs")
        self._pairs[int(i)] = len(pa)

    def covariance(self, stream=None):
        """Enqueue the covariance of every graph at its current poses; download() brings the results back."""
        _check(lib().slslam_po_batch_covariance(self._h, C.c_void_p(stream or 0)), "slslam_po_batch_covariance")

    def get_covariance(self, i):
        """(status, cov_poses[N, 6, 6], cov_pairs[P, 6, 6]) of graph i, as po_covariance returns them."""
        st = C.c_int(-1)
        cp, cq = np.zeros((self._n[i], 6, 6)), np.zeros((self._pairs.get(int(i), 0), 6, 6))
        _check(lib().slslam_po_batch_get_covariance(self._h, int(i), C.byref(st), _dp(cp), _dp(cq)), "slslam_po_batch_get_covariance")
        return st.value, cp, cq

    def set_candidates(self, i, candidates):
        """The candidate edges gate() judges for graph i (replaces the previous list; None or an empty list clears it)."""
        if candidates is None:
            candidates = dict(pose_a=[], pose_b=[], constraints=[])
        cc, keep = _po_candidates(candidates)
        _check(lib().slslam_po_batch_set_candidates(self._h, int(i), C.byref(cc)), "slslam_po_batch_set_candidates")
        self._cands[int(i)] = cc.num

    def gate(self, stream=None):
        """covariance() plus the statistics of every graph's candidates; download() brings both back."""
        _check(lib().slslam_po_batch_gate(self._h, C.c_void_p(stream or 0)), "slslam_po_batch_gate")

    def get_gate(self, i):
        """dict as po_edge_statistics returns, for graph i's candidates."""
        out = _edge_outputs(self._cands.get(int(i), 0))
        _check(lib().slslam_po_batch_get_gate(self._h, int(i), _ip(out[0]), *[_dp(a) for a in out[1:]]), "slslam_po_batch_get_gate")
        return _edge_dict(*out)

    def covariance_stats(self):
        c, a = C.c_longlong(0), C.c_longlong(0)
        _check(lib().slslam_po_batch_covariance_stats(self._h, C.byref(c), C.byref(a)), "slslam_po_batch_covariance_stats")
        return dict(calls=c.value, allocations=a.value)

    def summary(self, i):
        s = Summary()
        _check(lib().slslam_po_batch_get_summary(self._h, int(i), C.byref(s)), "slslam_po_batch_get_summary")
        return _summary_dict(s)

    def trace(self, i, cap=64):
        tr = (Iteration * cap)()
        n = C.c_int(0)
        _check(lib().slslam_po_batch_get_trace(self._h, int(i), tr, cap, C.byref(n)), "slslam_po_batch_get_trace")
        return _trace_list(tr, min(n.value, cap))


def po_solve_batch(graphs, trace_cap=64, stream=None, **opt):
    """The graphs through one POBatch: a list of (x, summary, trace), as po_solve returns for each."""
    b = POBatch()
    try:
        for g in graphs:
            b.add(g)
        b.finalize(**opt)
        b.solve(stream)
        b.download(stream)
        return [(b.parameters(i), b.summary(i), b.trace(i, trace_cap)) for i in range(len(b))]
    finally:
        b.close()


def po_solve_timed(g, **opt):
    """po_solve with the device-side split: returns (x, summary, dict(total_ms, factor_ms = the slowest factorisation,
    factor_calls, unknowns, junction_unknowns))."""
    lib().slslam_po_set_profiling(1)
    try:
        x, s, _ = po_solve(g, **opt)
        tot, fac = C.c_double(0), C.c_double(0)
        nc, nu, nj = C.c_int(0), C.c_int(0), C.c_int(0)
        lib().slslam_po_last_timing(C.byref(tot), C.byref(fac), C.byref(nc), C.byref(nu), C.byref(nj))
    finally:
        lib().slslam_po_set_profiling(0)
    return x, s, dict(total_ms=tot.value, factor_ms=fac.value, factor_calls=nc.value, unknowns=nu.value, junction_unknowns=nj.value)


def ransac_score(poses, observations, lines, baseline=0.12, error_thr=5.0 / 406.05):
    """Scores motion hypotheses against the common lines (slslam_ransac_score).
    poses [H,12] (R row-major, t), observations [K,8], lines [K,6] -> (scores [H], inlier mask [H,K] bool)."""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
    obs = np.ascontiguousarray(observations, dtype=np.float64).reshape(-1, 8)
    ln = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 6)
    if len(ln) != len(obs):
        raise ValueError("observations and lines must have the same length")
    h, k = len(poses), len(obs)
    words = (k + 63) // 64
    scores = np.zeros(max(h, 1), dtype=np.int32)
    bits = np.zeros(max(h * words, 1), dtype=np.uint64)
    fr = RansacFrame(h, k, _dp(poses), _dp(obs), _dp(ln))
    _check(lib().slslam_ransac_score(C.byref(fr), float(baseline), float(error_thr), _ip(scores),
                                     bits.ctypes.data_as(C.POINTER(C.c_ulonglong))), "slslam_ransac_score")
    mask = np.zeros((h, k), dtype=bool)
    if h and k:
        b = bits[:h * words].reshape(h, words)
        for w in range(words):
            n = min(64, k - 64 * w)
            mask[:, 64 * w:64 * w + n] = ((b[:, w:w + 1] >> np.arange(n, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return scores[:h], mask


def _trials(obs0, obs1, samples):
    o0 = np.ascontiguousarray(obs0, dtype=np.float64).reshape(-1, 8)
    o1 = np.ascontiguousarray(obs1, dtype=np.float64).reshape(-1, 8)
    smp = np.ascontiguousarray(samples, dtype=np.int32)
    if smp.ndim != 2 or len(o0) != len(o1):
        raise ValueError("samples must be [trials, s]; obs0 and obs1 must have the same length")
    return RansacTrials(smp.shape[0], smp.shape[1], len(o0), _ip(smp), _dp(o0), _dp(o1)), (o0, o1, smp)


def ransac_generate(obs0, obs1, samples, baseline=-0.12):
    """SLAM::vo_angle_axis_approx for every pre-drawn trial (slslam_ransac_generate) -> (poses [H,12], valid [H])."""
    tr, keep = _trials(obs0, obs1, samples)
    h = tr.num_trials
    poses = np.zeros((max(h, 1), 12))
    valid = np.zeros(max(h, 1), dtype=np.int32)
    _check(lib().slslam_ransac_generate(C.byref(tr), float(baseline), _dp(poses), _ip(valid)), "slslam_ransac_generate")
    return poses[:h], valid[:h]


def ransac_motion(obs0, obs1, lines, samples, baseline=0.12, error_thr=5.0 / 406.05, prob_free_outliers=0.999,
                  max_trials=1000, best_score=0):
    """SLAM::ransac_motion over a pre-drawn sample sequence (slslam_ransac_motion)
    -> (trial_cnt, best_score, best_pose [12], inlier mask [K])."""
    tr, keep = _trials(obs0, obs1, samples)
    ln = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 6)
    k = tr.num_lines
    if len(ln) != k:
        raise ValueError("lines and observations must have the same length")
    words = (k + 63) // 64
    bs = np.array([best_score], dtype=np.int32)
    tc = np.zeros(1, dtype=np.int32)
    pose = np.zeros(12)
    bits = np.zeros(max(words, 1), dtype=np.uint64)
    _check(lib().slslam_ransac_motion(C.byref(tr), _dp(ln), float(baseline), float(error_thr), float(prob_free_outliers),
                                      int(max_trials), _ip(bs), _ip(tc), _dp(pose), bits.ctypes.data_as(C.POINTER(C.c_ulonglong))),
           "slslam_ransac_motion")
    mask = np.zeros(k, dtype=bool)
    for w in range(words):
        n = min(64, k - 64 * w)
        mask[64 * w:64 * w + n] = ((bits[w] >> np.arange(n, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return int(tc[0]), int(bs[0]), pose, mask


def po_structure(g, max_chains=4096):
    """Symbolic analysis of the structured pose-graph factorisation (slslam_po_structure; host only).
    Returns dict(slot [N], chains [(start, len, left, right)], num_chain_unknowns, num_unknowns)."""
    i1 = np.ascontiguousarray(g["pose_index_1"], dtype=np.int32)
    i2 = np.ascontiguousarray(g["pose_index_2"], dtype=np.int32)
    n = int(g["num_poses"])
    cg = POGraph(n, len(i1), _ip(i1), _ip(i2), None, None)
    slot = np.zeros(max(n, 1), dtype=np.int32)
    arr = [np.zeros(max_chains, dtype=np.int32) for _ in range(4)]
    nc, ncu, nu = (np.zeros(1, dtype=np.int32) for _ in range(3))
    _check(lib().slslam_po_structure(C.byref(cg), _ip(slot), max_chains, _ip(nc), _ip(arr[0]), _ip(arr[1]), _ip(arr[2]), _ip(arr[3]),
                                     _ip(ncu), _ip(nu)), "slslam_po_structure")
    k = int(nc[0])
    return {"slot": slot[:n], "chains": [tuple(int(a[c]) for a in arr) for c in range(k)],
            "num_chain_unknowns": int(ncu[0]), "num_unknowns": int(nu[0]), "level1_chains": int(lib().slslam_po_structure_level1())}


def ransac_motion_batch(frames, baseline=0.12, error_thr=5.0 / 406.05, prob_free_outliers=0.999, max_trials=1000, best_score=0):
    """slslam_ransac_motion_batch: frames = list of dicts with obs0, obs1, lines, samples (as make_ransac_pair returns).
    best_score: every frame's incoming running best (SLAM::pose_estimation starts at -1).
    Returns a list of (trial_cnt, best_score, best_pose [12], inlier mask [K]) per frame."""
    n = len(frames)
    keep, trs, lns, bitbufs = [], (RansacTrials * max(n, 1))(), (C.POINTER(C.c_double) * max(n, 1))(), []
    bitptrs = (C.POINTER(C.c_ulonglong) * max(n, 1))()
    for i, fr in enumerate(frames):
        tr, k = _trials(fr["obs0"], fr["obs1"], fr["samples"])
        ln = np.ascontiguousarray(fr["lines"], dtype=np.float64).reshape(-1, 6)
        keep.append((k, ln))
        trs[i] = tr
        lns[i] = _dp(ln)
        bits = np.zeros(max((tr.num_lines + 63) // 64, 1), dtype=np.uint64)
        bitbufs.append(bits)
        bitptrs[i] = bits.ctypes.data_as(C.POINTER(C.c_ulonglong))
    bs = np.full(max(n, 1), best_score, dtype=np.int32)
    tc = np.zeros(max(n, 1), dtype=np.int32)
    poses = np.zeros((max(n, 1), 12))
    _check(lib().slslam_ransac_motion_batch(n, trs, lns, float(baseline), float(error_thr), float(prob_free_outliers), int(max_trials),
                                            _ip(bs), _ip(tc), _dp(poses), bitptrs), "slslam_ransac_motion_batch")
    out = []
    for i in range(n):
        k = trs[i].num_lines
        mask = np.zeros(k, dtype=bool)
        for w in range((k + 63) // 64):
            m = min(64, k - 64 * w)
            mask[64 * w:64 * w + m] = ((bitbufs[i][w] >> np.arange(m, dtype=np.uint64)) & np.uint64(1)).astype(bool)
        out.append((int(tc[i]), int(bs[i]), poses[i].copy(), mask))
    return out


def _bits_to_mask(bits, k):
    mask = np.zeros(k, dtype=bool)
    for w in range((k + 63) // 64):
        m = min(64, k - 64 * w)
        mask[64 * w:64 * w + m] = ((bits[w] >> np.arange(m, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return mask


class PoseEstimator(_Handle):
    """SLAM::pose_estimation for many frames per call (slslam_pose_estimator_*): RANSAC, motion-only BA on its inliers, final inliers.
    Keeps its device buffers and its refillable motion-only batch between calls."""
    _DESTROY = "slslam_pose_estimator_destroy"

    def __init__(self, max_frames=16, max_lines=512, device=-1, covariance=False, **opt):
        self._h = C.c_void_p()
        o = default_options(**opt)
        _check(lib().slslam_pose_estimator_create(int(device), C.byref(o), int(max_frames), int(max_lines), C.byref(self._h)),
               "slslam_pose_estimator_create")
        self._covariance = bool(covariance)
        if self._covariance:
            self.set_covariance(True)

    def set_covariance(self, enable):
        """From the next run on, OK frames carry the covariance of their motion (slslam_pose_estimator_set_covariance)."""
        _check(lib().slslam_pose_estimator_set_covariance(self._h, int(bool(enable))), "slslam_pose_estimator_set_covariance")
        self._covariance = bool(enable)

    def get_covariance(self, frame):
        """dict(constraint [6], covariance [6, 6], cov_status, sigma2, dof) of an OK frame of the last run
        (slslam_pose_estimator_get_covariance)."""
        st, dof, s2 = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        cons, cov = np.zeros(6), np.zeros((6, 6))
        _check(lib().slslam_pose_estimator_get_covariance(self._h, int(frame), C.byref(st), _dp(cons), _dp(cov), C.byref(s2), C.byref(dof)),
               "slslam_pose_estimator_get_covariance")
        return {"constraint": cons, "covariance": cov, "cov_status": st.value, "sigma2": s2.value, "dof": dof.value}

    def run(self, frames, baseline=0.12, error_thr=5.0 / 406.05, prob_free_outliers=0.999, max_trials=1000):
        """frames = list of dicts with obs0, obs1, lines, samples (as make_ransac_pair returns).  Returns one dict per frame:
        status, trial_cnt, ransac_score, ransac_pose [12], ransac_mask [K], summary, pose [12], num_inliers, mask [K]
        (the RANSAC fields in the shape ransac_motion_batch returns them) - and, with covariance enabled, for every OK frame
        constraint [6], covariance [6, 6], cov_status, sigma2, dof (get_covariance)."""
        n = len(frames)
        keep, trs, lns = [], (RansacTrials * max(n, 1))(), (C.POINTER(C.c_double) * max(n, 1))()
        outs = (PoseEstimate * max(n, 1))()
        bitbufs = []
        for i, fr in enumerate(frames):
            tr, k = _trials(fr["obs0"], fr["obs1"], fr["samples"])
            ln = np.ascontiguousarray(fr["lines"], dtype=np.float64).reshape(-1, 6)
            keep.append((k, ln))
            trs[i] = tr
            lns[i] = _dp(ln)
            words = max((tr.num_lines + 63) // 64, 1)
            rb, fb = np.zeros(words, dtype=np.uint64), np.zeros(words, dtype=np.uint64)
            bitbufs.append((rb, fb))
            outs[i].ransac_inlier_bits = rb.ctypes.data_as(C.POINTER(C.c_ulonglong))
            outs[i].inlier_bits = fb.ctypes.data_as(C.POINTER(C.c_ulonglong))
        _check(lib().slslam_pose_estimator_run(self._h, n, trs, lns, float(baseline), float(error_thr), float(prob_free_outliers),
                                               int(max_trials), outs), "slslam_pose_estimator_run")
        res = []
        for i in range(n):
            o, k = outs[i], trs[i].num_lines
            res.append({"status": POSE_STATUS[o.status], "trial_cnt": o.trial_cnt, "ransac_score": o.ransac_score,
                        "ransac_pose": np.array(o.ransac_pose[:]), "ransac_mask": _bits_to_mask(bitbufs[i][0], k),
                        "summary": _summary_dict(o.summary), "pose": np.array(o.pose[:]), "num_inliers": o.num_inliers,
                        "mask": _bits_to_mask(bitbufs[i][1], k)})
            if self._covariance and o.status == 0:
                res[-1].update(self.get_covariance(i))
        return res

    def stats(self):
        v = [C.c_longlong() for _ in range(4)]
        _check(lib().slslam_pose_estimator_stats(self._h, *[C.byref(x) for x in v]), "slslam_pose_estimator_stats")
        return dict(zip(("calls", "allocations", "finalizes", "refills"), (x.value for x in v)))

    def window(self, frame):
        """The motion-only window the last run packed on the device for `frame` (test hook): dict of index_words [2n],
        observations [2n, 8], parameters [12 + 4n], solved_camera [6]."""
        nl = C.c_int()
        _check(lib().slslam_pose_estimator_window(self._h, int(frame), None, None, None, None, C.byref(nl)), "slslam_pose_estimator_window")
        n = nl.value
        words = np.zeros(max(2 * n, 1), dtype=np.uint32)
        obs = np.zeros(max(16 * n, 1))
        par = np.zeros(12 + 4 * n)
        cam = np.zeros(6)
        _check(lib().slslam_pose_estimator_window(self._h, int(frame), words.ctypes.data_as(C.POINTER(C.c_uint)), _dp(obs), _dp(par), _dp(cam),
                                                  C.byref(nl)), "slslam_pose_estimator_window")
        return {"index_words": words[:2 * n], "observations": obs[:16 * n].reshape(-1, 8), "parameters": par, "solved_camera": cam}


# ----------------------------------------------------------------------------- line matching (slslam_line_matcher_*)
def _match_frame(fr):
    """frame dict (pose [12], observations [K, 8], lines [L, 6], optionally extents [L, 2]) -> (MatchFrame, the arrays it points to)"""
    pose = np.ascontiguousarray(fr["pose"], dtype=np.float64).reshape(-1)
    obs = np.ascontiguousarray(fr["observations"], dtype=np.float64).reshape(-1, 8)
    ln = np.ascontiguousarray(fr["lines"], dtype=np.float64).reshape(-1, 6)
    ext = fr.get("extents")
    if ext is not None:
        ext = np.ascontiguousarray(ext, dtype=np.float64).reshape(-1, 2)
        if len(ext) != len(ln):
            raise ValueError("extents and lines must have the same length")
    if len(pose) != 12:
        raise ValueError("pose must hold 12 doubles (R row-major | t)")
    return MatchFrame(len(obs), len(ln), _dp(pose), _dp(obs), _dp(ln), _dp(ext) if ext is not None else None), (pose, obs, ln, ext)


def _mutual_buffers(result, keys, n, m):
    """What the two matchers' results share: the six caller-owned arrays under the result struct's names for them - match, best, best
    value, second value, number admissible [n] each, the best row of every column [m]; -2 in what holds indices, 0 elsewhere - and
    the struct pointing at them."""
    b = {k: np.full(max(m if i == 5 else n, 1), 0 if i in (2, 3, 4) else -2, dtype=np.float32 if i in (2, 3) else np.int32)
         for i, k in enumerate(keys)}
    r = result(status=-1, **{k: a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_int)) for k, a in b.items()})
    return r, b


def _mutual_dict(status, r, b, n, m, **extra):
    out = dict(status=status[r.status], num_matched=r.num_matched, **extra)
    out.update({k: a[:m if i == 5 else n] for i, (k, a) in enumerate(b.items())})
    return out


def _match_buffers(k, l):
    return _mutual_buffers(MatchResult, ("match", "best_line", "best_error", "second_error", "num_admissible", "best_observation"), k, l)


def _match_dict(r, b, k, l):
    return _mutual_dict(MATCH_STATUS, r, b, k, l)


def match_lines(frame, baseline=0.12, error_thr=5.0 / 406.05, ratio=1.5, margin=0.0):
    """One frame's observations against its map lines under its predicted pose (slslam_match_lines).  frame: dict of pose [12],
    observations [K, 8], lines [L, 6] and optionally extents [L, 2].  Returns dict(status, num_matched, match [K], best_line [K],
    best_error [K] float32, second_error [K] float32, num_admissible [K], best_observation [L])."""
    mf, keep = _match_frame(frame)
    r, b = _match_buffers(mf.num_observations, mf.num_lines)
    _check(lib().slslam_match_lines(C.byref(mf), float(baseline), float(error_thr), float(ratio), float(margin), C.byref(r)),
           "slslam_match_lines")
    return _match_dict(r, b, mf.num_observations, mf.num_lines)


class LineMatcher(_CountedHandle):
    """slslam_line_matcher: many frames per call, every observation of a frame against every line of its map; buffers kept between runs."""
    _DESTROY, _STATS = "slslam_line_matcher_destroy", "slslam_line_matcher_stats"

    def __init__(self, max_frames=16, max_observations=512, max_lines=4096, device=-1):
        self._h = C.c_void_p()
        _check(lib().slslam_line_matcher_create(int(device), int(max_frames), int(max_observations), int(max_lines), C.byref(self._h)),
               "slslam_line_matcher_create")

    def run(self, frames, baseline=0.12, error_thr=5.0 / 406.05, ratio=1.5, margin=0.0):
        """frames: dicts as match_lines takes.  Returns one dict per frame, as match_lines returns."""
        n = len(frames)
        mfs, outs, keep, bufs = (MatchFrame * max(n, 1))(), (MatchResult * max(n, 1))(), [], []
        for i, fr in enumerate(frames):
            mfs[i], k = _match_frame(fr)
            outs[i], b = _match_buffers(mfs[i].num_observations, mfs[i].num_lines)
            keep.append(k)
            bufs.append(b)
        _check(lib().slslam_line_matcher_run(self._h, n, mfs, float(baseline), float(error_thr), float(ratio), float(margin), outs),
               "slslam_line_matcher_run")
        return [_match_dict(outs[i], bufs[i], mfs[i].num_observations, mfs[i].num_lines) for i in range(n)]


def matched_trials(frame, result, map_observations, num_trials=1001, sample_size=5, seed=0):
    """From a match result to the inputs of PoseEstimator.run / ransac_motion: the matched observations of the frame in ascending order,
    each aligned with its map line and with that landmark's earlier observation.  map_observations [L, 8]: the observation of every map
    line in the frame the lines are expressed in (obs0).  Returns dict(obs0, obs1, lines, samples [num_trials, sample_size] - distinct
    indices per trial, drawn from `seed` -, observation_index, line_index)."""
    obs = np.ascontiguousarray(frame["observations"], dtype=np.float64).reshape(-1, 8)
    ln = np.ascontiguousarray(frame["lines"], dtype=np.float64).reshape(-1, 6)
    mo = np.ascontiguousarray(map_observations, dtype=np.float64).reshape(-1, 8)
    if len(mo) != len(ln):
        raise ValueError("map_observations and lines must have the same length")
    match = np.asarray(result["match"])
    k = np.nonzero(match >= 0)[0]
    l = match[k]
    n = len(k)
    rng = np.random.default_rng(np.random.SeedSequence([11, int(seed)]))
    if n >= sample_size:
        samples = np.stack([rng.choice(n, size=sample_size, replace=False) for _ in range(num_trials)]).astype(np.int32)
    else:                # (too few for a sample: the estimator reports TOO_FEW_FEATURES; the indices only have to be in range)
        samples = (np.arange(num_trials * sample_size, dtype=np.int32).reshape(num_trials, sample_size) % max(n, 1)).astype(np.int32)
    return {"obs0": mo[l], "obs1": obs[k], "lines": ln[l], "samples": samples, "observation_index": k.astype(np.int32),
            "line_index": l.astype(np.int32)}


# ----------------------------------------------------------------------------- place recognition (slslam_voctree_*, slslam_place_*)
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class VocTree(_Handle):
    """slslam_voctree: K children per node, L levels, descriptors of D floats.  nodes: the interior nodes [(K^L - 1) / (K - 1), K, D]
    breadth-first (any shape of that many floats), or path: a file of exactly those floats."""
    _DESTROY = "slslam_voctree_destroy"

    def __init__(self, K, L, D, nodes=None, path=None, device=-1):
        self.K, self.L, self.D = int(K), int(L), int(D)
        self.num_leaves = self.K ** self.L
        self._h = C.c_void_p()
        if (nodes is None) == (path is None):
            raise ValueError("give nodes or path")
        if path is not None:
            _check(lib().slslam_voctree_load(os.fsencode(path), int(device), self.K, self.L, self.D, C.byref(self._h)), "slslam_voctree_load")
            return
        nodes = np.ascontiguousarray(nodes, dtype=np.float32).reshape(-1)
        if 2 <= self.K and 1 <= self.L <= 8 and nodes.size != (self.K ** self.L - 1) // (self.K - 1) * self.K * self.D:
            raise ValueError("nodes must hold (K^L - 1) / (K - 1) * K * D floats")
        _check(lib().slslam_voctree_create(int(device), self.K, self.L, self.D, _fp(nodes), C.byref(self._h)), "slslam_voctree_create")
        self.nodes = nodes.reshape(-1, self.K, self.D)

    @classmethod
    def train(cls, descriptors, K, L, max_iterations=10, seed=0, device=-1):
        """Trains a tree on descriptors [N, D] (train_voctree).  Returns (tree, the dict train_voctree returns)."""
        rep = train_voctree(descriptors, K, L, max_iterations=max_iterations, seed=seed, device=device)
        return cls(K, L, rep["nodes"].shape[2], nodes=rep["nodes"], device=device), rep

    def save(self, path):
        """Writes the file VocTree(path=...) reads.  A tree made from a path has no nodes to write."""
        if getattr(self, "nodes", None) is None:
            raise ValueError("this tree was loaded from a file")
        save_voctree(path, self.nodes)


def train_voctree(descriptors, K, L, max_iterations=10, seed=0, device=-1, timing=False):
    """slslam_voctree_train: hierarchical spherical k-means over descriptors [N, D] on the device; nodes, words and the counts are a
    function of the arguments alone, bit for bit.  Returns dict(nodes [(K^L - 1) / (K - 1), K, D], words [N], and per level iterations,
    changed, empty_children, distortion); timing=True adds the call's wall-clock split (setup_ms, kernel_ms, download_ms, centre_ms,
    upload_ms per level, total_ms)."""
    d = np.ascontiguousarray(descriptors, dtype=np.float32)
    if d.ndim != 2:
        raise ValueError("descriptors must be [N, D]")
    K, L = int(K), int(L)
    n, D = d.shape
    opt = VocTreeTrainOptions(K, L, D, int(max_iterations), int(seed) & 0xFFFFFFFFFFFFFFFF)
    num_int = (K ** L - 1) // (K - 1) if K >= 2 and 1 <= L <= 8 else 1
    nodes = np.zeros((num_int, max(K, 1), max(D, 1)), dtype=np.float32)
    words, rep = np.zeros(max(n, 1), dtype=np.int32), VocTreeTrainReport()
    _check(lib().slslam_voctree_train(int(device), C.byref(opt), n, _fp(d), _fp(nodes), _ip(words), C.byref(rep)), "slslam_voctree_train")
    out = {"nodes": nodes, "words": words[:n], "iterations": list(rep.iterations[:L]), "changed": list(rep.changed[:L]),
           "empty_children": list(rep.empty_children[:L]), "distortion": list(rep.distortion[:L])}
    if timing:
        for k in ("setup_ms", "kernel_ms", "download_ms", "centre_ms", "upload_ms"):
            out[k] = list(getattr(rep, k)[:L])
        out["total_ms"] = rep.total_ms
    return out


def save_voctree(path, nodes):
    """slslam_voctree_save: nodes [(K^L - 1) / (K - 1), K, D] as the file slslam_voctree_load reads."""
    nodes = np.ascontiguousarray(nodes, dtype=np.float32)
    if nodes.ndim != 3:
        raise ValueError("nodes must be [(K^L - 1) / (K - 1), K, D]")
    num_int, K, D = nodes.shape
    L = next((l for l in range(1, 9) if K >= 2 and (K ** l - 1) // (K - 1) == num_int), 0)
    _check(lib().slslam_voctree_save(os.fsencode(path), K, L, D, _fp(nodes)), "slslam_voctree_save")


def _place_frame(tree, fr):
    d = np.ascontiguousarray(fr, dtype=np.float32).reshape(-1, tree.D)
    return PlaceFrame(len(d), _fp(d)), d


class PlaceDB(_CountedHandle):
    """slslam_place_db: the documents of the inserted keyframes and queries against the visible ones; buffers kept between calls.
    A frame is its descriptors [n, D] float32."""
    _DESTROY, _STATS = "slslam_place_db_destroy", "slslam_place_db_stats"

    def __init__(self, tree, max_docs=4096, max_words=512, max_frames=64, recent=40, num_avg_words=100):
        self.tree = tree                                           # (the database uses the tree: keep it alive)
        self._h = C.c_void_p()
        _check(lib().slslam_place_db_create(tree._h, int(max_docs), int(max_words), int(max_frames), int(recent), int(num_avg_words),
                                            C.byref(self._h)), "slslam_place_db_create")

    def insert(self, frame):
        """Returns dict(status, words [n])."""
        pf, keep = _place_frame(self.tree, frame)
        st, words = C.c_int(-1), np.full(max(pf.num_descriptors, 1), -2, dtype=np.int32)
        _check(lib().slslam_place_db_insert(self._h, C.byref(pf), C.byref(st), _ip(words)), "slslam_place_db_insert")
        return {"status": PLACE_STATUS[st.value], "words": words[:pf.num_descriptors]}

    def run(self, frames, top_k=0):
        """Returns one dict per frame: status, has_virtual, words [n], score / touched / likelihood [visible + 1] (index 0: state -1,
        index d + 1: visible document d), top_id / top_score [top_k]."""
        n, s = len(frames), self.size()["visible"] + 1
        pfs, outs, keep, bufs = (PlaceFrame * max(n, 1))(), (PlaceResult * max(n, 1))(), [], []
        for i, fr in enumerate(frames):
            pfs[i], k = _place_frame(self.tree, fr)
            b = {"words": np.full(max(pfs[i].num_descriptors, 1), -2, dtype=np.int32), "score": np.zeros(s, dtype=np.float32),
                 "touched": np.zeros(s, dtype=np.uint8), "likelihood": np.zeros(s, dtype=np.float32),
                 "top_id": np.full(max(top_k, 1), -2, dtype=np.int32), "top_score": np.zeros(max(top_k, 1), dtype=np.float32)}
            outs[i] = PlaceResult(-1, 0, 0, _ip(b["words"]), _fp(b["score"]), b["touched"].ctypes.data_as(C.POINTER(C.c_ubyte)),
                                  _fp(b["likelihood"]), _ip(b["top_id"]), _fp(b["top_score"]))
            keep.append(k)
            bufs.append(b)
        _check(lib().slslam_place_db_run(self._h, n, pfs, int(top_k), outs), "slslam_place_db_run")
        res = []
        for i in range(n):
            b = bufs[i]
            res.append({"status": PLACE_STATUS[outs[i].status], "has_virtual": bool(outs[i].has_virtual),
                        "words": b["words"][:pfs[i].num_descriptors], "score": b["score"], "touched": b["touched"],
                        "likelihood": b["likelihood"], "top_id": b["top_id"][:top_k], "top_score": b["top_score"][:top_k]})
        return res

    def size(self):
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(lib().slslam_place_db_size(self._h, C.byref(a), C.byref(b), C.byref(c)), "slslam_place_db_size")
        return {"inserted": a.value, "visible": b.value, "doc_size": c.value}

    def virtual_words(self):
        n = C.c_int(0)
        _check(lib().slslam_place_db_virtual(self._h, None, C.byref(n)), "slslam_place_db_virtual")
        w = np.zeros(max(n.value, 1), dtype=np.int32)
        _check(lib().slslam_place_db_virtual(self._h, _ip(w), None), "slslam_place_db_virtual")
        return w[:n.value]


class PlaceFilter(_Handle):
    """slslam_place_filter: the Bayes filter over (no place, visible documents) and the loop decision.  Defaults: the reference's indoor
    preset (with recent = min_docs = 40).  Needs no device."""
    _DESTROY = "slslam_place_filter_destroy"

    def __init__(self, sigma=1.0, threshold=0.7, seq_len=10, min_docs=40):
        self._h = C.c_void_p()
        _check(lib().slslam_place_filter_create(float(sigma), float(threshold), int(seq_len), int(min_docs), C.byref(self._h)),
               "slslam_place_filter_create")

    def update(self, likelihood):
        """likelihood [N + 1] as PlaceDB.run returns it.  Returns (loop, keyframe, posterior [N + 1])."""
        lik = np.ascontiguousarray(likelihood, dtype=np.float32).reshape(-1)
        if len(lik) < 1:
            raise ValueError("likelihood holds state -1 and the visible documents")
        post, loop, kf = np.zeros(len(lik), dtype=np.float32), C.c_int(0), C.c_int(-1)
        _check(lib().slslam_place_filter_update(self._h, len(lik) - 1, _fp(lik), _fp(post), C.byref(loop), C.byref(kf)),
               "slslam_place_filter_update")
        return bool(loop.value), kf.value, post


def place_candidates(db, filt, frame):
    """One keyframe through the recogniser: insert it, query it against the visible documents, one filter step.  Returns
    (loop, keyframe, posterior): keyframe is the visible document a closed loop reports (-1 without one).  A frame the database does not
    take (no descriptors, a non-finite one) is neither inserted nor filtered: (False, -1, None)."""
    if db.insert(frame)["status"] != "OK":
        return False, -1, None
    return filt.update(db.run([frame])[0]["likelihood"])


# ----------------------------------------------------------------------------- descriptor matching (slslam_descriptor_matcher_*)
def _desc_buffers(n, m):
    return _mutual_buffers(DescriptorResult, ("match", "best", "best_distance", "second_distance", "num_admissible", "best_query"), n, m)


def _desc_dict(r, b, n, candidate):
    return _mutual_dict(DESC_STATUS, r, b, n, r.num_keyframe_descriptors, candidate=candidate)


def match_descriptors(query, keyframe, ratio=1.5, max_distance=float("inf")):
    """One frame's descriptors [n, D] against one keyframe's [m, D] by the place recogniser's distance (slslam_match_descriptors).
    Returns dict(status, num_matched, candidate (0), match [n], best [n], best_distance [n] float32, second_distance [n] float32,
    num_admissible [n], best_query [m])."""
    q = np.ascontiguousarray(query, dtype=np.float32)
    k = np.ascontiguousarray(keyframe, dtype=np.float32)
    if q.ndim != 2 or k.ndim != 2 or q.shape[1] != k.shape[1]:
        raise ValueError("query and keyframe must be [n, D] and [m, D]")
    r, b = _desc_buffers(len(q), len(k))
    _check(lib().slslam_match_descriptors(q.shape[1], len(q), _fp(q), len(k), _fp(k), float(ratio), float(max_distance), C.byref(r)),
           "slslam_match_descriptors")
    return _desc_dict(r, b, len(q), 0)


class DescriptorMatcher(_CountedHandle):
    """slslam_descriptor_matcher: the descriptors of the inserted keyframes on the device, and many (frame, candidate keyframe) pairs
    matched per call; buffers kept between calls.  A frame is its descriptors [n, D] float32.  Fed the frames a PlaceDB is fed, a
    keyframe's id here is its document id there."""
    _DESTROY, _STATS = "slslam_descriptor_matcher_destroy", "slslam_descriptor_matcher_stats"

    def __init__(self, D, max_keyframes=4096, max_descriptors=512, max_frames=64, max_candidates=3, device=-1):
        self.D = int(D)
        self._h = C.c_void_p()
        _check(lib().slslam_descriptor_matcher_create(int(device), self.D, int(max_keyframes), int(max_descriptors), int(max_frames),
                                                      int(max_candidates), C.byref(self._h)), "slslam_descriptor_matcher_create")
        self._counts = []                                          # descriptors of every inserted keyframe

    def _frame(self, fr):
        return np.ascontiguousarray(fr, dtype=np.float32).reshape(-1, self.D)

    def insert(self, frame):
        """Returns dict(status, id): id is the keyframe's number in the store, -1 when the frame is refused."""
        d = self._frame(frame)
        st, kid = C.c_int(-1), C.c_int(-1)
        _check(lib().slslam_descriptor_matcher_insert(self._h, len(d), _fp(d), C.byref(st), C.byref(kid)), "slslam_descriptor_matcher_insert")
        if kid.value >= 0:
            self._counts.append(len(d))
        return {"status": DESC_STATUS[st.value], "id": kid.value}

    def run(self, queries, ratio=1.5, max_distance=float("inf")):
        """queries: (frame, candidates) per query frame, candidates a sequence of store ids (-1: none).  Returns per query the list of
        its pairs' results, each a dict as match_descriptors returns with `candidate` the store id."""
        n = len(queries)
        qs, keep, bufs, cand = (DescriptorQuery * max(n, 1))(), [], [], []
        for i, (fr, cs) in enumerate(queries):
            d, c = self._frame(fr), np.ascontiguousarray(cs, dtype=np.int32).reshape(-1)
            qs[i] = DescriptorQuery(len(d), _fp(d), len(c), _ip(c))
            keep.append((d, c))
            for kid in c.tolist():
                cand.append((i, len(d), kid))
        outs = (DescriptorResult * max(len(cand), 1))()
        for p, (i, nd, kid) in enumerate(cand):
            outs[p], b = _desc_buffers(nd, self._counts[kid] if 0 <= kid < len(self._counts) else 0)
            bufs.append(b)
        _check(lib().slslam_descriptor_matcher_run(self._h, n, qs, float(ratio), float(max_distance), len(cand), outs),
               "slslam_descriptor_matcher_run")
        res = [[] for _ in range(n)]
        for p, (i, nd, kid) in enumerate(cand):
            res[i].append(_desc_dict(outs[p], bufs[p], nd, kid))
        return res

    def size(self):
        a = C.c_int(0)
        _check(lib().slslam_descriptor_matcher_size(self._h, C.byref(a)), "slslam_descriptor_matcher_size")
        return a.value


def loop_matches(matcher, frame, candidates, ratio=1.5, max_distance=float("inf")):
    """The link between place_candidates and matched_trials: one frame against the candidate keyframes a closed loop names (say the
    reported document and its neighbours).  Returns (candidate, result): the candidate with the most matches, the lowest id on ties,
    and its result as DescriptorMatcher.run returns it; (-1, None) when no candidate gives an OK pair.  result["match"] is what
    matched_trials takes, with keyframe descriptor j standing for map line j."""
    best = None
    for r in matcher.run([(frame, candidates)], ratio=ratio, max_distance=max_distance)[0]:
        if r["status"] == "OK" and (best is None or (r["num_matched"], -r["candidate"]) > (best["num_matched"], -best["candidate"])):
            best = r
    return (best["candidate"], best) if best is not None else (-1, None)


# ----------------------------------------------------------------------------- line descriptors from images (slslam_line_descriptor_*)
def msld_options(bands=9, band_width=5, orient=True):
    return MsldOptions(int(bands), int(band_width), int(bool(orient)))


def _image_rows(image):
    """A uint8 [H, W] array whose rows the library can walk: an image whose rows are contiguous passes its stride, any other is copied."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("an image is uint8 [H, W]")
    if img.shape[0] > 0 and img.shape[1] > 0 and (img.strides[1] != 1 or img.strides[0] < img.shape[1]):
        img = np.ascontiguousarray(img)
    return img


def _msld_frame(image, segments, D):
    """(MsldFrame, MsldResult, the arrays both point to)."""
    img = _image_rows(image)
    seg = np.ascontiguousarray(segments, dtype=np.float32).reshape(-1, 4)
    n = len(seg)
    b = {"descriptors": np.zeros((max(n, 1), D), dtype=np.float32), "status": np.full(max(n, 1), -1, dtype=np.int32),
         "num_samples": np.zeros(max(n, 1), dtype=np.int32), "polarity": np.zeros(max(n, 1), dtype=np.float32)}
    fr = MsldFrame(img.shape[1], img.shape[0], img.strides[0] if img.shape[0] > 0 else 0, img.ctypes.data_as(C.POINTER(C.c_ubyte)), n,
                   _fp(seg))
    return fr, MsldResult(_fp(b["descriptors"]), _ip(b["status"]), _ip(b["num_samples"]), _fp(b["polarity"])), (img, seg, b)


def _msld_dict(keep):
    _, seg, b = keep
    n = len(seg)
    return {"descriptors": b["descriptors"][:n], "status": [MSLD_STATUS[s] for s in b["status"][:n].tolist()],
            "num_samples": b["num_samples"][:n], "polarity": b["polarity"][:n]}


def describe_lines(image, segments, **options):
    """slslam_describe_lines: the MSLD descriptors of the segments [n, 4] (x0, y0, x1, y1) of one uint8 image [H, W].  Returns
    dict(descriptors [n, 8 bands] float32, status [n] of MSLD_STATUS's names, num_samples [n], polarity [n] float32)."""
    opt = msld_options(**options)
    fr, res, keep = _msld_frame(image, segments, 8 * max(opt.bands, 1))
    _check(lib().slslam_describe_lines(C.byref(opt), C.byref(fr), C.byref(res)), "slslam_describe_lines")
    return _msld_dict(keep)


class LineDescriptor(_TimedHandle):
    """slslam_line_descriptor: MSLD descriptors for the segments of many frames per call; buffers kept between calls.  A frame is
    (image uint8 [H, W], segments [n, 4])."""
    _DESTROY, _STATS, _TIMING = "slslam_line_descriptor_destroy", "slslam_line_descriptor_stats", "slslam_line_descriptor_timing"

    def __init__(self, bands=9, band_width=5, orient=True, max_frames=2, max_pixels=752 * 480, max_segments=512, device=-1):
        self.opt = msld_options(bands, band_width, orient)
        self.D = 8 * self.opt.bands
        self._h = C.c_void_p()
        _check(lib().slslam_line_descriptor_create(int(device), C.byref(self.opt), int(max_frames), int(max_pixels), int(max_segments),
                                                   C.byref(self._h)), "slslam_line_descriptor_create")

    def run(self, frames):
        """Returns one dict per frame, as describe_lines returns it."""
        frs, outs, keep = _frame_arrays(MsldFrame, MsldResult, frames, lambda f: _msld_frame(f[0], f[1], self.D))
        _check(lib().slslam_line_descriptor_run(self._h, len(frames), frs, outs), "slslam_line_descriptor_run")
        return [_msld_dict(k) for k in keep]


# ----------------------------------------------------------------------------- line segments from images (slslam_line_detector_*)
def line_detect_options(grad_threshold=24, tol_num=11, tol_den=64, min_pixels=12, min_length=10.0, max_thickness=3.0, max_segments=512):
    return LineDetectOptions(int(grad_threshold), int(tol_num), int(tol_den), int(min_pixels), float(min_length), float(max_thickness),
                             int(max_segments))


def _detect_frame(image, max_segments, labels):
    """(LineDetectFrame, LineDetectResult, the arrays both point to)."""
    img = _image_rows(image)
    s = max(int(max_segments), 1)
    b = {"segments": np.zeros((s, 4), dtype=np.float32), "length": np.zeros(s), "thickness": np.zeros(s), "strength": np.zeros(s),
         "pixels": np.zeros(s, dtype=np.int32), "label": np.full(s, -1, dtype=np.int32), "counts": np.full(3, -1, dtype=np.int32),
         "status_counts": np.zeros(5, dtype=np.int32), "labels": np.full(img.shape, -1, dtype=np.int32) if labels else None}
    fr = LineDetectFrame(img.shape[1], img.shape[0], img.strides[0] if img.shape[0] > 0 else 0, img.ctypes.data_as(C.POINTER(C.c_ubyte)))
    c = b["counts"].ctypes.data
    res = LineDetectResult(_fp(b["segments"]), _dp(b["length"]), _dp(b["thickness"]), _dp(b["strength"]), _ip(b["pixels"]), _ip(b["label"]),
                           C.cast(c, C.POINTER(C.c_int)), C.cast(c + 4, C.POINTER(C.c_int)), C.cast(c + 8, C.POINTER(C.c_int)),
                           _ip(b["status_counts"]), _ip(b["labels"]) if labels else None)
    return fr, res, (img, b)


def _detect_dict(keep):
    _, b = keep
    n = max(int(b["counts"][2]), 0)
    out = {k: b[k][:n] for k in ("segments", "length", "thickness", "strength", "pixels", "label")}
    out.update(num_components=int(b["counts"][0]), num_ok=int(b["counts"][1]), num_written=int(b["counts"][2]),
               status_counts={LSD_STATUS[i]: int(v) for i, v in enumerate(b["status_counts"])})
    if b["labels"] is not None:
        out["labels"] = b["labels"]
    return out


def detect_lines(image, labels=False, **options):
    """slslam_detect_lines: the line segments of one uint8 image [H, W].  Returns dict(segments [n, 4] float32 (x0, y0, x1, y1), length,
    thickness, strength [n] float64, pixels, label [n] int32, num_components, num_ok, num_written = n, status_counts: a dict over
    LSD_STATUS's names; with labels=True also labels [H, W] int32, -1 where a pixel is not strong)."""
    opt = line_detect_options(**options)
    fr, res, keep = _detect_frame(image, opt.max_segments, labels)
    _check(lib().slslam_detect_lines(C.byref(opt), C.byref(fr), C.byref(res)), "slslam_detect_lines")
    return _detect_dict(keep)


class LineDetector(_TimedHandle):
    """slslam_line_detector: the line segments of many frames per call; buffers kept between calls.  A frame is an image uint8 [H, W]."""
    _DESTROY, _STATS, _TIMING = "slslam_line_detector_destroy", "slslam_line_detector_stats", "slslam_line_detector_timing"

    def __init__(self, max_frames=2, max_pixels=752 * 480, device=-1, **options):
        self.opt = line_detect_options(**options)
        self._h = C.c_void_p()
        _check(lib().slslam_line_detector_create(int(device), C.byref(self.opt), int(max_frames), int(max_pixels), C.byref(self._h)),
               "slslam_line_detector_create")

    def run(self, images, labels=False):
        """Returns one dict per frame, as detect_lines returns it."""
        frs, outs, keep = _frame_arrays(LineDetectFrame, LineDetectResult, images,
                                        lambda image: _detect_frame(image, self.opt.max_segments, labels))
        _check(lib().slslam_line_detector_run(self._h, len(images), frs, outs), "slslam_line_detector_run")
        return [_detect_dict(k) for k in keep]


def detect_and_describe(detector, descriptor, images):
    """The segments of every image (detector: a LineDetector) and their MSLD descriptors (descriptor: a LineDescriptor): two calls, the
    images go to the device once for each.  Returns per frame the detector's dict with the descriptor's `descriptors`, `status` (as
    `descriptor_status`), `num_samples` and `polarity` added."""
    found = detector.run(images)
    described = descriptor.run([(image, f["segments"]) for image, f in zip(images, found)])
    for f, d in zip(found, described):
        f.update(descriptors=d["descriptors"], descriptor_status=d["status"], num_samples=d["num_samples"], polarity=d["polarity"])
    return found


# ----------------------------------------------------------------------------- stereo line matching (slslam_stereo_matcher_*)
def stereo_match_options(**options):
    """slslam_stereo_match_default_options with the given fields replaced: min_disparity, max_disparity, max_tan2, min_rows,
    min_overlap, ratio, max_distance, fx, fy, cx, cy."""
    return _float_options(StereoMatchOptions(), "slslam_stereo_match_default_options", "stereo match", options)


def _stereo_side(side):
    """(segments [n, 4], descriptors [n, D]) of one image: a pair of arrays, or a dict with those two keys (what detect_and_describe
    returns per image)."""
    seg, desc = (side["segments"], side["descriptors"]) if isinstance(side, dict) else side
    seg = np.ascontiguousarray(seg, dtype=np.float32).reshape(-1, 4)
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    desc = desc.reshape(len(seg), -1) if len(seg) else desc.reshape(0, desc.shape[-1] if desc.ndim == 2 else 0)
    return seg, desc


def _stereo_frame(left, right, D=None):
    """(StereoFrame, StereoResult, the arrays both point to, D)."""
    (ls, ld), (rs, rd) = _stereo_side(left), _stereo_side(right)
    dims = {d.shape[1] for s, d in ((ls, ld), (rs, rd)) if len(s)} | ({int(D)} if D is not None else set())
    if len(dims) > 1:
        raise ValueError("the descriptors of a stereo frame must all have the matcher's D floats")
    n, m = len(ls), len(rs)
    r, b = _mutual_buffers(StereoResult, ("match", "best", "best_distance", "second_distance", "num_admissible", "best_left"), n, m)
    b["segment_status"] = np.full(max(n, 1), -1, dtype=np.int32)
    b["observations"] = np.full((max(n, 1), 8), np.nan)
    b["disparity"] = np.full((max(n, 1), 2), np.nan)
    r.segment_status, r.observations, r.disparity = _ip(b["segment_status"]), _dp(b["observations"]), _dp(b["disparity"])
    fr = StereoFrame(n, _fp(ls), _fp(ld), m, _fp(rs), _fp(rd))
    return fr, r, (ls, ld, rs, rd, b), (dims.pop() if dims else 8)


def _stereo_dict(r, keep):
    ls, _, rs, _, b = keep
    out = _mutual_dict(STEREO_STATUS, r, b, len(ls), len(rs))
    out["segment_status"] = [STEREO_SEGMENT_STATUS.get(s, "?") for s in out["segment_status"].tolist()]
    return out


def match_stereo(left, right, **options):
    """slslam_match_stereo: the segments and descriptors of a rectified left image against those of the right one.  left, right:
    (segments [n, 4] float32, descriptors [n, D] float32) or a dict with those keys.  Returns dict(status, num_matched, match [n], best
    [n], best_distance [n] float32, second_distance [n] float32, num_admissible [n], best_left [m], segment_status [n] of
    STEREO_SEGMENT_STATUS's names, observations [n, 8] and disparity [n, 2] float64 - NaN in the rows that are not MATCHED, which
    the library leaves untouched)."""
    opt = stereo_match_options(**options)
    fr, r, keep, D = _stereo_frame(left, right)
    _check(lib().slslam_match_stereo(D, C.byref(opt), C.byref(fr), C.byref(r)), "slslam_match_stereo")
    return _stereo_dict(r, keep)


class StereoMatcher(_TimedHandle):
    """slslam_stereo_matcher: many stereo frames per call; buffers kept between calls.  A frame is (left, right) as match_stereo
    takes them.  The options given here are the defaults of run."""
    _DESTROY, _STATS, _TIMING = "slslam_stereo_matcher_destroy", "slslam_stereo_matcher_stats", "slslam_stereo_matcher_timing"

    def __init__(self, D, max_frames=2, max_segments=512, device=-1, **options):
        self.D = int(D)
        self.options = dict(options)
        stereo_match_options(**self.options)                        # (an unknown name fails here)
        self._h = C.c_void_p()
        _check(lib().slslam_stereo_matcher_create(int(device), self.D, int(max_frames), int(max_segments), C.byref(self._h)),
               "slslam_stereo_matcher_create")

    def run(self, frames, **options):
        """Returns one dict per frame, as match_stereo returns it."""
        opt = stereo_match_options(**dict(self.options, **options))
        frs, outs, keep = _frame_arrays(StereoFrame, StereoResult, frames, lambda f: _stereo_frame(f[0], f[1], self.D))
        _check(lib().slslam_stereo_matcher_run(self._h, C.byref(opt), len(frames), frs, outs), "slslam_stereo_matcher_run")
        return [_stereo_dict(outs[i], keep[i]) for i in range(len(frames))]


def stereo_observations(result):
    """From a stereo match result to what match_lines, PoseEstimator and the triangulator take: (observations [k, 8] float64 of the
    MATCHED left segments in ascending order, their left indices [k])."""
    idx = np.nonzero(np.asarray(result["match"]) >= 0)[0]
    return np.ascontiguousarray(np.asarray(result["observations"])[idx]), idx


def detect_describe_and_pair(detector, descriptor, matcher, stereo_images, **options):
    """The whole image front end for rectified stereo pairs: the segments of every image (detector: a LineDetector), their MSLD
    descriptors (descriptor: a LineDescriptor) and the pairing of every frame's left and right segments (matcher: a StereoMatcher;
    options: what its run takes) - three calls whatever the number of frames.  stereo_images: (left, right) uint8 images per frame.
    Only segments whose descriptor came out OK are paired.  Returns per frame dict(left, right: what detect_and_describe returns for
    the image; left_rows, right_rows: the rows of those that were paired; stereo: the matcher's result over those rows;
    observations [k, 8]: the stereo line observations of the matched pairs, as match_lines and PoseEstimator take them; left_index,
    right_index [k]: the detector's rows of each observation)."""
    flat = [img for pair in stereo_images for img in pair]
    found = detect_and_describe(detector, descriptor, flat)
    sides, rows = [], []
    for f in found:
        keep = np.nonzero(np.array([s == "OK" for s in f["descriptor_status"]], dtype=bool))[0]
        rows.append(keep)
        sides.append((f["segments"][keep], f["descriptors"][keep].reshape(len(keep), descriptor.D)))
    results = matcher.run([(sides[2 * i], sides[2 * i + 1]) for i in range(len(stereo_images))], **options)
    out = []
    for i, r in enumerate(results):
        obs, idx = stereo_observations(r)
        out.append(dict(left=found[2 * i], right=found[2 * i + 1], left_rows=rows[2 * i], right_rows=rows[2 * i + 1], stereo=r,
                        observations=obs, left_index=rows[2 * i][idx], right_index=rows[2 * i + 1][r["match"][idx]]))
    return out


# ----------------------------------------------------------------------------- line tracking (slslam_line_tracker_*)
def line_track_options(**options):
    """slslam_line_track_default_options with the given fields replaced: max_tan2, max_shift, max_offset, min_overlap, min_length,
    ratio, max_distance."""
    return _float_options(LineTrackOptions(), "slslam_line_track_default_options", "line track", options)


_TRACK_KEYS = ("match", "best", "best_distance", "second_distance", "num_admissible", "best_row")


def _track_frame(frame, m, D=None):
    """(LineTrackFrame, LineTrackResult, the arrays both point to, D); m: the segments of the frame before."""
    if isinstance(frame, dict):
        seg, desc, predict = frame["segments"], frame["descriptors"], frame.get("predict")
    else:
        seg, desc, predict = (tuple(frame) + (None,))[:3]
    seg, desc = _stereo_side((seg, desc))
    if len(seg) and D is not None and desc.shape[1] != int(D):
        raise ValueError("the descriptors of a frame must have the tracker's D floats")
    n = len(seg)
    r, b = _mutual_buffers(LineTrackResult, _TRACK_KEYS, n, m)
    for k in ("id", "age", "segment_status"):
        b[k] = np.full(max(n, 1), -2, dtype=np.int32)
        setattr(r, k, _ip(b[k]))
    r.num_continued = r.num_new = -1
    pre = None if predict is None else np.ascontiguousarray(predict, dtype=np.float64).reshape(6)
    fr = LineTrackFrame(n, _fp(seg), _fp(desc), _dp(pre) if pre is not None else None)
    return fr, r, (seg, desc, pre, b, m), (desc.shape[1] if len(seg) else (int(D) if D is not None else 8))


def _track_dict(r, keep):
    seg, _, _, b, m = keep
    n = len(seg)
    out = dict(status=TRACK_STATUS[r.status], num_continued=r.num_continued, num_new=r.num_new)
    out.update({k: b[k][:m if k == "best_row" else n] for k in _TRACK_KEYS + ("id", "age")})
    out["segment_status"] = [TRACK_SEGMENT_STATUS.get(s, "?") for s in b["segment_status"][:n].tolist()]
    return out


def _track_frames(frames, carried, D):
    state = [carried, D]                    # the segments of the frame before, and D once a frame has shown it

    def make(frame):
        made = _track_frame(frame, state[0], state[1])
        state[:] = made[0].num_segments, made[3]
        return made
    return _frame_arrays(LineTrackFrame, LineTrackResult, frames, make) + (state[1],)


def track_lines(frames, **options):
    """slslam_track_lines: a sequence of frames from an empty tracker (no carried frame, next_id 0).  A frame is (segments [n, 4]
    float32, descriptors [n, D] float32[, predict [6] float64 or None]) or a dict with those keys.  Returns per frame dict(status,
    num_continued, num_new, id, age, match, best, num_admissible [n], best_distance, second_distance [n] float32, best_row [the
    segments of the frame before], segment_status [n] of TRACK_SEGMENT_STATUS's names)."""
    opt = line_track_options(**options)
    frs, outs, keep, D = _track_frames(frames, 0, None)
    _check(lib().slslam_track_lines(int(D if D is not None else 8), C.byref(opt), len(frames), frs, outs), "slslam_track_lines")
    return [_track_dict(outs[i], keep[i]) for i in range(len(frames))]


class LineTracker(_TimedHandle):
    """slslam_line_tracker: persistent feature ids for the segments of many frames per call; the last frame and the next id are kept
    on the device and in the handle between calls.  A frame is what track_lines takes.  The options given here are the defaults
    of run."""
    _DESTROY, _STATS, _TIMING = "slslam_line_tracker_destroy", "slslam_line_tracker_stats", "slslam_line_tracker_timing"

    def __init__(self, D, max_frames=2, max_segments=512, device=-1, **options):
        self.D = int(D)
        self.options = dict(options)
        line_track_options(**self.options)                          # (an unknown name fails here)
        self._h = C.c_void_p()
        _check(lib().slslam_line_tracker_create(int(device), self.D, int(max_frames), int(max_segments), C.byref(self._h)),
               "slslam_line_tracker_create")

    def run(self, frames, **options):
        """Returns one dict per frame, as track_lines returns it."""
        opt = line_track_options(**dict(self.options, **options))
        frs, outs, keep, _ = _track_frames(frames, self.state()["carried_segments"], self.D)
        _check(lib().slslam_line_tracker_run(self._h, C.byref(opt), len(frames), frs, outs), "slslam_line_tracker_run")
        return [_track_dict(outs[i], keep[i]) for i in range(len(frames))]

    def reset(self, next_id=0):
        _check(lib().slslam_line_tracker_reset(self._h, int(next_id)), "slslam_line_tracker_reset")

    def state(self):
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().slslam_line_tracker_state(self._h, C.byref(a), C.byref(b)), "slslam_line_tracker_state")
        return {"next_id": a.value, "carried_segments": b.value}


def detect_describe_pair_and_track(detector, descriptor, matcher, tracker, stereo_images, predicts=None, **stereo_options):
    """detect_describe_and_pair, then the tracker over the left segments that were paired on (tracker: a LineTracker; predicts: per
    frame None or the six doubles of its predict) - four calls whatever the number of frames.  Returns per frame the dict of
    detect_describe_and_pair with `track` (the tracker's result over left_rows), and `ids` [k]: the feature id of every row of
    `observations` - with fx = fy = 1, cx = cy = 0 the [k] ids and [k, 8] pixels of one of the reference's frame files."""
    out = detect_describe_and_pair(detector, descriptor, matcher, stereo_images, **stereo_options)
    frames = []
    for i, o in enumerate(out):
        keep = o["left_rows"]
        frames.append((o["left"]["segments"][keep], o["left"]["descriptors"][keep].reshape(len(keep), descriptor.D),
                       None if predicts is None else predicts[i]))
    for o, t in zip(out, tracker.run(frames)):
        o["track"] = t
        o["ids"] = t["id"][stereo_observations(o["stereo"])[1]]
    return out


# ----------------------------------------------------------------------------- image rectification (slslam_image_rectifier_*)
def rectify_options(border="constant", border_value=0, smooth_sigma=0.0):
    """slslam_rectify_options: border "constant" or "replicate" (or the SLSLAM_RECTIFY_BORDER_* number), the value an invalid pixel gets,
    and the sigma of the pre-smoothing (0: none)."""
    mode = RECTIFY_BORDER[border] if isinstance(border, str) else int(border)
    return RectifyOptions(mode, int(border_value), float(smooth_sigma))


def smooth_taps(sigma):
    """slslam_rectify_smooth_taps: (radius, taps [8] int32: t_0 .. t_7, 0 beyond the radius)."""
    r, t = C.c_int(-1), np.zeros(8, dtype=np.int32)
    _check(lib().slslam_rectify_smooth_taps(float(sigma), C.byref(r), _ip(t)), "slslam_rectify_smooth_taps")
    return r.value, t


def stereo_rectify(left, right, R, t, dst_size=None, principal=None):
    """slslam_stereo_rectify.  left, right: dict(fx, fy, cx, cy, width, height[, k1, k2, p1, p2, k3]) of the raw cameras; R [3, 3], t [3]:
    x_right = R x_left + t; dst_size: (width, height) of both outputs, the left camera's size by default; principal: (cx2, cy2), the
    left principal point by default.  Returns dict(left, right: RectifyCamera; baseline; fx, fy, cx, cy: what stereo_match_options
    takes)."""
    g = StereoRig()
    for side, cam in (("left", left), ("right", right)):
        getattr(g, side + "_k")[:] = [float(cam[k]) for k in ("fx", "fy", "cx", "cy")]
        getattr(g, side + "_dist")[:] = [float(cam.get(k, 0.0)) for k in ("k1", "k2", "p1", "p2", "k3")]
        setattr(g, side + "_width", int(cam["width"]))
        setattr(g, side + "_height", int(cam["height"]))
    g.R[:] = np.asarray(R, dtype=np.float64).reshape(9).tolist()
    g.t[:] = np.asarray(t, dtype=np.float64).reshape(3).tolist()
    g.dst_width, g.dst_height = (int(left["width"]), int(left["height"])) if dst_size is None else (int(dst_size[0]), int(dst_size[1]))
    if principal is not None:
        g.has_principal, g.cx2, g.cy2 = 1, float(principal[0]), float(principal[1])
    a, b, base, k = RectifyCamera(), RectifyCamera(), C.c_double(0.0), np.zeros(4)
    _check(lib().slslam_stereo_rectify(C.byref(g), C.byref(a), C.byref(b), C.byref(base), _dp(k)), "slslam_stereo_rectify")
    return dict(left=a, right=b, baseline=base.value, fx=k[0], fy=k[1], cx=k[2], cy=k[3])


def _camera_array(cameras):
    arr = (RectifyCamera * max(len(cameras), 1))()
    for i, c in enumerate(cameras):
        arr[i] = c
    return arr


def _rectify_frame(cameras, camera, image, valid):
    """(RectifyFrame, RectifyResult, the arrays both point to); a camera index out of range is left for the library to refuse."""
    img = _image_rows(image)
    k = int(camera)
    c = cameras[k] if 0 <= k < len(cameras) else None
    shape = (c.dst_height, c.dst_width) if c is not None else (1, 1)
    b = {"image": np.zeros(shape, dtype=np.uint8), "valid": np.zeros(shape, dtype=np.uint8) if valid else None,
         "num_valid": np.full(1, -1, dtype=np.int32)}
    ub = C.POINTER(C.c_ubyte)
    fr = RectifyFrame(k, img.strides[0] if img.shape[0] > 0 else 0, img.ctypes.data_as(ub))
    res = RectifyResult(b["image"].ctypes.data_as(ub), shape[1], b["valid"].ctypes.data_as(ub) if valid else None, _ip(b["num_valid"]))
    return fr, res, (img, b)


def _rectify_dict(keep):
    _, b = keep
    out = {"image": b["image"], "num_valid": int(b["num_valid"][0])}
    if b["valid"] is not None:
        out["valid"] = b["valid"]
    return out


def _rectify_check_sizes(cameras, frames):
    for k, image in frames:
        if 0 <= int(k) < len(cameras) and np.asarray(image).shape != (cameras[int(k)].src_height, cameras[int(k)].src_width):
            raise ValueError("a frame has the source size of its camera")


def rectify_images(cameras, frames, valid=False, **options):
    """slslam_rectify_images: cameras: a list of RectifyCamera; frames: (camera index, raw uint8 image [src_height, src_width]) each.
    Returns per frame dict(image uint8 [dst_height, dst_width], num_valid; with valid=True also valid uint8 [dst_height, dst_width])."""
    opt = rectify_options(**options)
    _rectify_check_sizes(cameras, frames)
    frs, outs, keep = _frame_arrays(RectifyFrame, RectifyResult, frames, lambda f: _rectify_frame(cameras, f[0], f[1], valid))
    _check(lib().slslam_rectify_images(C.byref(opt), len(cameras), _camera_array(cameras), len(frames), frs, outs), "slslam_rectify_images")
    return [_rectify_dict(k) for k in keep]


class ImageRectifier(_TimedHandle):
    """slslam_image_rectifier: the rectified (and, with smooth_sigma > 0, smoothed) images of many raw frames per call; the cameras'
    maps stay on the device, buffers are kept between calls.  A frame is (camera index, raw uint8 image)."""
    _DESTROY, _STATS, _TIMING = "slslam_image_rectifier_destroy", "slslam_image_rectifier_stats", "slslam_image_rectifier_timing"

    def __init__(self, cameras, max_frames=2, max_pixels=752 * 480, device=-1, **options):
        self.opt = rectify_options(**options)
        self.cameras = list(cameras)
        self._h = C.c_void_p()
        _check(lib().slslam_image_rectifier_create(int(device), C.byref(self.opt), len(self.cameras), _camera_array(self.cameras),
                                                   int(max_frames), int(max_pixels), C.byref(self._h)), "slslam_image_rectifier_create")

    def run(self, frames, valid=False):
        """Returns one dict per frame, as rectify_images returns it."""
        _rectify_check_sizes(self.cameras, frames)
        frs, outs, keep = _frame_arrays(RectifyFrame, RectifyResult, frames, lambda f: _rectify_frame(self.cameras, f[0], f[1], valid))
        _check(lib().slslam_image_rectifier_run(self._h, len(frames), frs, outs), "slslam_image_rectifier_run")
        return [_rectify_dict(k) for k in keep]

    def get_map(self, camera, fp64=False):
        """The device's map of one camera: dict(qx, qy int32 [dst_height, dst_width], valid uint8; with fp64=True also sx, sy)."""
        c = self.cameras[int(camera)]
        shape = (c.dst_height, c.dst_width)
        out = {"qx": np.zeros(shape, dtype=np.int32), "qy": np.zeros(shape, dtype=np.int32), "valid": np.zeros(shape, dtype=np.uint8)}
        if fp64:
            out.update(sx=np.zeros(shape), sy=np.zeros(shape))
        _check(lib().slslam_image_rectifier_get_map(self._h, int(camera), _ip(out["qx"]), _ip(out["qy"]),
                                                    out["valid"].ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                    _dp(out["sx"]) if fp64 else None, _dp(out["sy"]) if fp64 else None),
               "slslam_image_rectifier_get_map")
        return out


def rectify_detect_describe_pair_and_track(rectifier, detector, descriptor, matcher, tracker, raw_stereo_images, predicts=None,
                                           cameras=(0, 1), intrinsics=None, **stereo_options):
    """The image front end from a rig's raw images: every (left, right) raw pair through the rectifier (an ImageRectifier whose cameras
    `cameras` = (left, right) are a rectified pair, as stereo_rectify makes them) in one call, then detect_describe_pair_and_track on
    the rectified images - five calls whatever the number of frames.  The stereo options fx, fy, cx, cy are the left camera's rectified
    intrinsics unless `intrinsics` (a dict of the four, e.g. what stereo_rectify returned) or stereo_options give them.  Returns
    what detect_describe_pair_and_track returns, each frame's dict with `rectified`: the (left, right) images."""
    flat = [(cameras[i], img) for pair in raw_stereo_images for i, img in enumerate(pair)]
    rect = rectifier.run(flat)
    pairs = [(rect[2 * i]["image"], rect[2 * i + 1]["image"]) for i in range(len(raw_stereo_images))]
    c = rectifier.cameras[cameras[0]]
    k = dict(fx=c.fx2, fy=c.fy2, cx=c.cx2, cy=c.cy2)
    if intrinsics is not None:
        k.update({n: float(intrinsics[n]) for n in ("fx", "fy", "cx", "cy")})
    k.update(stereo_options)
    out = detect_describe_pair_and_track(detector, descriptor, matcher, tracker, pairs, predicts, **k)
    for o, p in zip(out, pairs):
        o["rectified"] = p
    return out

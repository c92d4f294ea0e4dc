/* include/slslam_hip.h — C ABI of the MI355X-native SLSLAM optimisation back-end.
 *
 * Drop-in boundary for the reference's two optimisation hot paths.  The reference is C++ and has
 * no FFI of its own; what a maintainer binds is the triple
 *     XProblem::build(ceres::Problem*)  /  XProblem::set_options(ceres::Solver::Options*)  /
 *     ceres::Solve(options, &problem, &summary)
 * at the three call sites reference src/slam.cpp:643-663 (motion_only_ba), :924-952
 * (bundle_adjustment) and :1283-1293 (pose_optimization).  Every entry point below cites the
 * reference interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * The host-side C++ mirror of the reference classes (slslam_amd/host/lba_problem.h,
 * po_problem.h and the minimal ceres facade) marshals into these calls; see INTEGRATION.md.
 *
 * All solves run on the GPU in hand-written HIP kernels (slslam_amd/csrc).  There is no CPU
 * fallback: without a usable HIP device every compute entry point returns SLSLAM_ERR_NO_DEVICE.
 */
#ifndef SLSLAM_HIP_H_
#define SLSLAM_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status codes */
enum {
  SLSLAM_OK = 0,
  SLSLAM_ERR_INVALID_ARGUMENT = 1,
  SLSLAM_ERR_NO_DEVICE = 2,        /* no HIP device / HIP runtime error */
  SLSLAM_ERR_HIP = 3,
  SLSLAM_ERR_UNSUPPORTED = 4,      /* problem shape outside what the kernels support */
  SLSLAM_ERR_STATE = 5,            /* call sequence violated (e.g. solve before finalize) */
  SLSLAM_ERR_NO_MEMORY = 6         /* a host allocation failed while building a window (std::bad_alloc caught at the boundary) */
};

/* Termination of one solve: mirrors ceres::Solver::Summary::termination_type of Ceres 1.7.
 * The reference never inspects it (src/slam.cpp:663,944,1293); reported for diagnostics.
 * Known deviation: when max_num_iterations ends a solve right after an ACCEPTED step, Ceres 1.7 still evaluates the
 * gradient at the new point inside that iteration and can report GRADIENT_TOLERANCE; here the gradient of a point is
 * evaluated by the next linearisation, which never comes, so such a solve reports NO_CONVERGENCE and its last trace
 * record keeps the previous point's gradient_max_norm.  Parameters, costs and step counts are the same. */
enum {
  SLSLAM_NO_CONVERGENCE = 0,       /* max_num_iterations reached */
  SLSLAM_GRADIENT_TOLERANCE = 1,
  SLSLAM_FUNCTION_TOLERANCE = 2,
  SLSLAM_PARAMETER_TOLERANCE = 3,
  SLSLAM_NUMERICAL_FAILURE = 4,    /* parameters are left untouched, as Ceres does */
  SLSLAM_MIN_RADIUS = 5
};

/* ------------------------------------------------------------------ options
 * Replaces: ceres::Solver::Options as filled by LBAProblem::set_options
 * (reference src/lba_problem.cpp:95-132) and POProblem::set_options (src/po_problem.cpp:67-77),
 * plus the constants hard-coded in the hot path (baseline 0.12: src/lba_problem.h:101;
 * Huber scale 1/406.05: src/lba_problem.cpp:78) and the gflags read by it (FLAGS_robust,
 * src/lba_problem.cpp:35; FLAGS_max_num_iter, src/slam.cpp:647,928).
 * Trust-region constants are the Ceres 1.7 defaults the reference leaves untouched. */
typedef struct slslam_solver_options {
  int    max_num_iterations;            /* lba_param_t.num_iterations / POProblem n_iter        */
  double huber_delta;                   /* 1/406.05 when FLAGS_robust, <= 0 disables the loss   */
  double baseline;                      /* stereo baseline, 0.12                                */
  double initial_trust_region_radius;   /* 1e4   */
  double max_trust_region_radius;       /* 1e16  */
  double min_trust_region_radius;       /* 1e-32 */
  double min_relative_decrease;         /* 1e-3  */
  double min_lm_diagonal;               /* 1e-6  */
  double max_lm_diagonal;               /* 1e32  */
  int    max_num_consecutive_invalid_steps; /* 5 */
  double function_tolerance;            /* 1e-6  */
  double gradient_tolerance;            /* 1e-10 (relative to the initial max-norm, Ceres 1.7)  */
  double parameter_tolerance;           /* 1e-8  */
  int    jacobi_scaling;                /* 1     */
  int    use_graph;                     /* 1: replay the LM iteration as a captured hipGraph    */
  int    chunks_per_window;             /* 0 = auto; n > 0: n equal chunks (waves cooperating on one window); n < 0: -(1000 r + c), c chunks
                                           of GRADED sizes made for r rounds of the chip's wave slots - long chunks first, short ones last -
                                           as the automatic choice cuts the windows of a batch whose slots each run several chunks (what
                                           slslam_lba_batch_window_chunks reports for such a window: pass it back to get the same cut)     */
  int    reuse_elimination;             /* 0: the back-substitution re-linearises (HBM traffic ==
                                           algorithmic); 1: it streams Jacobian blocks the elimination
                                           spilled to HBM (+192 B per coupled observation)         */
  int    po_factor_fp32;                /* pose graph only: 1 = factor the normal matrix in fp32 (MFMA f32);
                                           residuals, gradient, costs and LM bookkeeping stay fp64
                                           (implies po_dense_factor)                                    */
  int    po_dense_factor;               /* pose graph only: 0 (default) = structured factorisation: chains of poses
                                           eliminated concurrently (block tridiagonal), dense MFMA Cholesky of the
                                           junction poses only; 1 = dense MFMA Cholesky of the whole normal matrix   */
  int    lba_fused_motion_only;         /* 1 (default): a batch whose windows all have one free camera and only constant lines
                                           (SLAM::motion_only_ba) is solved by one launch, one wave per window, the 6 x 6
                                           system in registers; 0: the general elimination / back-substitution path     */
  int    lba_elimination;               /* how the elimination sweep accumulates the reduced camera system: 0 (default) = 4 for a batch
                                           that fills the chip with long chunks (>= 16 tiles per resident wave) when its conditions
                                           hold, else 1; 1 = per-wave partial in LDS fed by fp64 atomics; 2 / 3 = Schur outer products on the matrix cores
                                           (v_mfma_f64_16x16x4_f64, accumulator tiles in registers) with one / two waves per chunk
                                           workgroup - for windows with <= 10 free cameras and one observation per (line, free
                                           camera), else the default sweep runs.  Same results to round-off; slower on MI355X
                                           (DESIGN.md section 7), kept as a measured alternative.  4 = matrix cores with GROUP-LOCAL
                                           accumulators: the lines of a window are packed by their first free camera and the wave
                                           keeps only the 48 x 48 sum of the current group in registers (same conditions)         */
  int    lba_keep_jacobian;             /* 0 (default): every elimination sweep linearises.  1: the sweep that follows a REJECTED step
                                           does not - the point has not moved, only the trust-region radius has: it replays the blocks
                                           J_c^T J_l of every observation and the line blocks the last linearising sweep left in HBM
                                           (+192 B per observation), as ceres::TrustRegionMinimizer evaluates the Jacobian only after
                                           a successful step.  Grouped sweep (lba_elimination 4) only; same results to round-off.
                                           Measured SLOWER on MI355X (the stores cost the linearising sweeps more than the replays
                                           save): kept as a tested alternative                              */
  int    refill_headroom_percent;       /* 0 (default): the batch holds exactly its windows.  > 0: a batch for a STREAM of windows - its device
                                           arrays get that much room beyond what the first windows need, a pinned host image of them is
                                           kept, results come back through pinned buffers - so that slslam_lba_batch_refill can replace
                                           all its windows without allocating, re-capturing the solve graph or synchronising          */
  int    host_threads;                  /* host threads for the per-window host work of a batch (packing = the LBAProblem::build stage,
                                           layout, result copies): 0 = automatic (up to 8 for batches of 64 windows or more), 1 = the
                                           calling thread only                                                                         */
  int    reproducible;                  /* 0 (default): the elimination sweep (lba_elimination = 0) and the cut of a window into chunks
                                           (chunks_per_window = 0) are chosen for the BATCH - fastest, but a window's result bytes then
                                           depend on its company (the sums run in another order).  1: both become functions of the window
                                           alone - lba_elimination = 0 means 1, a requested matrix-core sweep the batch cannot take is
                                           SLSLAM_ERR_UNSUPPORTED instead of a fallback, chunks of at most 34 tiles graded for three
                                           rounds of the wave slots (what the automatic choice gives a batch that fills the chip) - so
                                           that 1 / 2 / 4 / 8-rank runs and one-window batches return identical bytes with no caller
                                           bookkeeping                                                                                  */
  int    lba_precision;                 /* 0 (default): fp64 throughout, the reference's arithmetic.  1: MIXED - the steady elimination
                                           sweeps form the CAMERA Jacobian of an observation in packed fp32 (and park it as floats);
                                           geometry, residuals, the LINE Jacobian, every block product and accumulation (line blocks,
                                           reduced camera system, gradients), the cost, the candidate evaluation and all trust-region
                                           bookkeeping stay fp64, as does the first sweep of a solve.  Which parts may be float was
                                           measured (a float line Jacobian changes accept / reject decisions: its depth column carries
                                           d = cos t / sin t, reference src/lba_problem.h:63).  Grouped sweep only (lba_elimination 0 or
                                           4, at most 10 free cameras); opt-in; results within the tolerance stated in DESIGN.md 4 ("Mixed precision") and
                                           tests/test_gpu_lba.py::test_mixed_precision_solves of the fp64 path and of the oracle.
                                           MEASURED: buys nothing (0.997 x the fp64 step) - fp32 line Jacobians change LM accept / reject
                                           decisions, and what is left to fp32 is a few per cent of the sweep.  Kept as a tested option  */
  int    device_build;                  /* who runs the LBAProblem::build stage (reference src/lba_problem.cpp:54-93) of a REFILL
                                           (slslam_lba_batch_refill, slslam_lba_stream_submit): 0 (default) = the device when it can
                                           (csrc/lba_device_build.h: at most 64 cameras and 65534 lines per window; the windows' arrays are
                                           read by the GPU where they are when they lie in page-locked memory - slslam_pinned_alloc /
                                           slslam_pinned_register - else from a pinned staging copy the host threads make), with the host
                                           packer as the fallback; -1 = always the host packer (lba_pack.cpp, options.host_threads
                                           threads).  Same layout, same solved bytes either way                                          */
  double po_huber_delta;                /* pose graph only: 0 (default) = no loss function, the reference as it ships (robustify = false,
                                           src/po_problem.cpp:27); a > 0 = ceres::HuberLoss(a) on every edge, the other arm of the same
                                           switch (src/po_problem.cpp:55: robustify ? new HuberLoss(0.001) : NULL) - the reference's value
                                           is 0.001.  With s = |Te|^2 of an edge: s <= a^2 leaves the block alone, otherwise its residuals
                                           and both Jacobian blocks are scaled by sqrt(a / sqrt(s)) (Ceres 1.7's corrector for rho'' <= 0)
                                           and its cost is (2 a sqrt(s) - a^2) / 2.  For graphs whose loop closures may be false matches:
                                           one wrong edge wrecks the unweighted solve.  Negative or not finite:
                                           SLSLAM_ERR_INVALID_ARGUMENT.  Last field: the offsets of the others did not move              */
} slslam_solver_options;

/* Fills every field with the configuration the reference runs (robust loss on, 10 iterations). */
void slslam_default_options(slslam_solver_options* opt);

/* ------------------------------------------------------------------ summary
 * Replaces: the four ceres::Solver::Summary fields the reference reads back
 * (reference src/slam.cpp:949-952) + diagnostics. */
typedef struct slslam_summary {
  int    num_successful_steps;
  int    num_unsuccessful_steps;
  double initial_cost;
  double final_cost;
  double fixed_cost;
  int    termination_type;
  int    num_free_parameters;
  int    num_residual_blocks;
} slslam_summary;

/* One record per LM iteration (index 0 = initial evaluation), for parity tests. */
typedef struct slslam_iteration {
  int    iteration;
  int    step_is_valid;
  int    step_is_successful;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  double model_cost_change;
} slslam_iteration;

/* ------------------------------------------------------------------ LBA window
 * Replaces: ceres::lba_param_t (reference src/lba_problem.h:123-130) + the five arrays handed
 * to LBAProblem through set_line_index / set_camera_index / set_fixed_index / set_observations /
 * set_parameters (src/lba_problem.h:153-157); layouts as documented at src/lba_problem.h:188-196
 * and built at src/slam.cpp:899-920.  All pointers are HOST pointers owned by the caller. */
typedef struct slslam_lba_window {
  int num_cameras;                /* lba_param_t.num_cameras      */
  int num_lines;                  /* lba_param_t.num_lines        */
  int num_observations;           /* lba_param_t.num_observations */
  const int*    camera_index;     /* [M]                          */
  const int*    line_index;       /* [M]                          */
  const int*    fixed_index;      /* [2M]: [2i] camera constant, [2i+1] line constant */
  const double* observations;     /* [8M]: x0 y0 x1 y1 (camera 0), x2 y2 x3 y3 (camera 1) */
  double*       parameters;       /* [6C + 4L] in/out: cameras (w,t) then lines (a,b,g,t) */
} slslam_lba_window;

/* Replaces: LBAProblem::build + LBAProblem::set_options + ceres::Solve for ONE window
 * (reference src/slam.cpp:924-944 and :643-663).  Synchronous; parameters solved in place.
 * trace may be NULL; at most trace_cap records are written and *trace_len gets the count. */
int slslam_lba_solve(const slslam_lba_window* window, const slslam_solver_options* opt,
                     slslam_summary* summary, slslam_iteration* trace, int trace_cap, int* trace_len);

/* ---- batched form: many independent windows resident in HBM, solved in lock-step.
 * This is the throughput path (independent sliding windows / sequence shards);
 * each window goes through exactly the per-window algorithm of slslam_lba_solve. */
typedef struct slslam_lba_batch slslam_lba_batch;

/* device < 0 selects the current HIP device. */
int  slslam_lba_batch_create(int device, slslam_lba_batch** out);
void slslam_lba_batch_destroy(slslam_lba_batch* b);
/* Replaces LBAProblem::build for one more window: validates, copies and reorders the arrays on
 * the host (observations grouped by line).  Returns the window's index in *index. */
int  slslam_lba_batch_add(slslam_lba_batch* b, const slslam_lba_window* window, int* index);
/* Uploads every added window to HBM; no windows can be added afterwards (all of them can be REPLACED: slslam_lba_batch_refill). */
int  slslam_lba_batch_finalize(slslam_lba_batch* b, const slslam_solver_options* opt);
/* Replaces ceres::Solve for all windows: enqueues the complete LM solve on `stream`
 * (a hipStream_t passed as void*, NULL = default stream) and returns without synchronising. */
int  slslam_lba_batch_solve(slslam_lba_batch* b, void* stream);
/* Restores the initial parameters on the device (for repeated timing of the same inputs). */
int  slslam_lba_batch_reset(slslam_lba_batch* b, void* stream);
/* Trust-region steps (successful + unsuccessful, the count the reference accumulates at
 * src/slam.cpp:949-950) executed by all windows since the counter was last cleared; synchronises
 * the stream.  Lets a bench count iterations over several solves without per-window downloads. */
int  slslam_lba_batch_iterations(slslam_lba_batch* b, void* stream, long long* iterations, int clear);
/* Blocks until the stream's work is done and copies parameters + summaries back to the host. */
int  slslam_lba_batch_download(slslam_lba_batch* b, void* stream);
/* The two halves of download: _async enqueues the export and the device-to-host copies on `stream` and returns; _wait blocks until
 * they have arrived (results of a refillable batch land in pinned memory, so the copies overlap whatever else the host does). */
int  slslam_lba_batch_download_async(slslam_lba_batch* b, void* stream);
int  slslam_lba_batch_wait(slslam_lba_batch* b);
/* Replaces LBAProblem::build for ALL windows of a finalized batch at once - the next `n` windows of a stream take the place of the
 * present ones (reference: the five arrays a caller hands over per window, src/slam.cpp:899-921; n must equal the batch's window
 * count).  The batch must have been finalized with refill_headroom_percent > 0.  Packs the windows on options.host_threads host
 * threads straight into the batch's pinned host image, uploads the arrays with asynchronous copies on `stream`, rebuilds the tile
 * contexts and the initial parameter buffers on the device and resets the LM state - no allocation, no synchronisation, the captured
 * solve graph stays valid.  The windows are cut into chunks by the policy finalize resolved, so a refilled batch returns the bytes a
 * fresh batch of the same windows returns.  SLSLAM_ERR_UNSUPPORTED (batch unchanged, still solvable): the windows do not fit the
 * room the arrays have, or need another path / sweep - build a new batch then.
 * A batch finalized on the fused motion-only path (slslam_lba_batch_path = SLSLAM_PATH_FUSED_MOTION_ONLY: SLAM::motion_only_ba, reference
 * src/slam.cpp:578-675) is refilled in place too, by the same two builds, with windows of that shape only: every window must have exactly one
 * observed camera that no observation flags constant and no observed line that is left free - anything else is SLSLAM_ERR_UNSUPPORTED,
 * checked on the host before the batch is touched (a stream builds a new batch for such a set).
 * Host arrays are read before the call returns - EXCEPT arrays in page-locked memory (slslam_pinned_alloc / _register) when the device
 * builds (options.device_build = 0): those are read by the GPU after the call returns and must stay valid until the results have been
 * waited for.  For arrays in ordinary (pageable) memory the results depend only on what the arrays held when this call was made.  When the device builds, what only the build can find out arrives with the results: a window with bad input, of a shape
 * for the host path, or a refill that does not fit the room is flagged - slslam_lba_batch_get_parameters / _get_summary of such a window
 * return SLSLAM_ERR_INVALID_ARGUMENT / SLSLAM_ERR_UNSUPPORTED (the other windows are solved); sizes that cannot fit are still refused here.
 * `stream` must be the stream the batch is solved on. */
int  slslam_lba_batch_refill(slslam_lba_batch* b, const slslam_lba_window* windows, int n, void* stream);
/* After download: solved parameters of window `index` in the caller's original layout. */
int  slslam_lba_batch_get_parameters(const slslam_lba_batch* b, int index, double* parameters);
int  slslam_lba_batch_get_summary(const slslam_lba_batch* b, int index, slslam_summary* summary);
int  slslam_lba_batch_get_trace(const slslam_lba_batch* b, int index, slslam_iteration* trace,
                                int trace_cap, int* trace_len);
/* Copies all solved parameters, windows concatenated in add order, into a DEVICE buffer
 * (for a collective on the results without a host round trip). */
int  slslam_lba_batch_export_device(slslam_lba_batch* b, double* device_out, void* stream);
/* Problem-size accounting for throughput reporting: totals over the batch. */
int  slslam_lba_batch_counts(const slslam_lba_batch* b, long long* num_windows, long long* num_cameras,
                             long long* num_free_cameras, long long* num_lines, long long* num_observations);
/* After finalize: which device path the batch takes.  One window beyond the tiled sweeps (more than 20 free / 64 cameras, a line
 * with more than 64 observations: the reference's W = 40 study) takes the global-memory path (built for single large windows,
 * not for batch throughput).  A batch that mixes such windows with ordinary ones is solved as two batches side by side - the
 * ordinary windows on the tiled sweeps, the oversize ones on the global-memory path on a stream of the batch's own, joined to
 * the caller's before the call returns control of it: SLSLAM_PATH_MIXED. */
enum { SLSLAM_PATH_TILED = 0, SLSLAM_PATH_FUSED_MOTION_ONLY = 1, SLSLAM_PATH_GLOBAL_MEMORY = 2, SLSLAM_PATH_MIXED = 3 };
int  slslam_lba_batch_path(const slslam_lba_batch* b, int* path);
/* After finalize: the elimination sweep the batch runs, as a value of slslam_solver_options.lba_elimination that reproduces it
 * (1, 2, 3 or 4; never 0): what the automatic choice resolved to, or what the request fell back to.  A window's result depends on
 * this value (the sweeps sum in different orders) - a caller that wants one window of a large batch again, bit for bit, in a batch
 * of its own passes it back together with the window's chunk count.  0 for batches that do not take the tiled sweeps. */
int  slslam_lba_batch_elimination(const slslam_lba_batch* b, int* mode);
/* After finalize: the number of chunks (waves cooperating on the window's observation sweeps) window `index` was cut into.  A
 * window's result is a function of its inputs, the options and this number only (the chunk partials are summed in chunk order):
 * a window solved again with chunks_per_window set to it - in any batch that keeps the chunk count at 8 or below, or above 8 -
 * reproduces its result bit for bit, which is how results are compared across the ranks of a multi-GPU run (bench.py).
 * NEGATIVE: -(1000 r + c): c chunks of graded sizes made for r rounds of the wave slots (chunks_per_window set to it asks for the same cut). */
int  slslam_lba_batch_window_chunks(const slslam_lba_batch* b, int index, int* num_chunks);
/* Device time (ms) spent in each kernel family during the last solve, measured with HIP events
 * on the solve stream while profiling is enabled (solves are then launched eagerly instead of
 * replaying the captured graph); times accumulate over solves until set_profiling is called again.
 * names: 0 linearise+schur, 1 reduced solve, 2 back-substitution (includes the candidate cost and the candidate
 * lines' sin/cos table unless reuse_elimination is set), 3 line trig, 4 candidate cost (reuse_elimination only),
 * 5 LM update, 6 init.  launches[i] receives the number of launches. */
int  slslam_lba_batch_set_profiling(slslam_lba_batch* b, int enable);
int  slslam_lba_batch_kernel_times(const slslam_lba_batch* b, double ms[8], int launches[8]);

/* ---- posterior covariances of solved windows (csrc/lba_covariance.h).
 * Replaces nothing in the reference - its odometry edges are identity-weighted -; the Ceres counterpart is ceres::Covariance.
 * For a window at its CURRENT device parameters x (the solved ones after _solve, the initial ones after _finalize / _reset / _refill:
 * the point slslam_lba_batch_linearise evaluates), with J the Jacobian of all residual blocks w.r.t. the free blocks after the Huber
 * corrector (huber_delta <= 0: none), without Jacobi scaling or damping, and H = J^T J split into cameras (c) and lines (l):
 *   S = H_cc - sum_lines H_cl H_ll^-1 H_lc,  cov_cameras = S^-1 (the joint covariance of all free cameras, cross blocks included),
 *   cov_lines[l] = H_ll^-1 + K S^-1 K^T with K = H_ll^-1 H_lc (the line's own 4 x 4 marginal; no line-line or line-camera blocks).
 * A camera / line is free iff it is observed and no observation flags it constant (the rule of the solve); constant lines add to
 * H_cc only.  Units are Ceres': unit-variance residuals - multiply by the noise variance.
 * SLSLAM_COV_SINGULAR: a pivot <= 1e-10 in the Cholesky factorisation of S or of a line's H_ll, each scaled to unit diagonal (a
 * window without a constant camera has a 6-dimensional gauge null space): every output of that window is zero; the other windows
 * of the batch are not affected. */
enum { SLSLAM_COV_OK = 0, SLSLAM_COV_SINGULAR = 1 };
/* ceres::Covariance::Compute for every window of the batch: enqueues one launch on `stream` and returns.  with_lines = 0 skips the
 * lines' blocks and their buffer.  Changes nothing the solve reads or writes.  The result buffers are allocated by the first call
 * (the lines' by the first call that asks for them) and kept: a batch that never asks pays nothing.  Works on refilled batches and,
 * through slslam_lba_stream_batch, on a stream's.  SLSLAM_ERR_UNSUPPORTED (batch untouched): the batch takes
 * SLSLAM_PATH_GLOBAL_MEMORY or SLSLAM_PATH_MIXED - the reduced system of such a window (up to 240 x 240) does not fit LDS. */
int  slslam_lba_batch_covariance(slslam_lba_batch* b, void* stream, int with_lines);
/* ceres::Covariance::GetCovarianceBlock, after slslam_lba_batch_download / _wait (which bring the covariances enqueued since the last
 * download back with the other results): *status = SLSLAM_COV_*; *num_free_cameras = F; free_camera[C]: the free cameras' caller
 * indices, ascending, in [0, F), -1 behind; cov_cameras[(6F)^2] row-major, block order = free_camera[]; cov_lines[16 L]: row-major
 * 4 x 4 per caller line index, zeros for constant or unobserved lines.  Any output pointer may be NULL.
 * SLSLAM_ERR_INVALID_ARGUMENT: the last slslam_lba_batch_covariance call has not been downloaded - none was made, a newer one is
 * still on the device, or a refill has replaced the windows since;
 * SLSLAM_ERR_STATE: cov_lines asked for, but the downloaded call had with_lines = 0; a window a device-built refill flagged
 * returns that window's error, as slslam_lba_batch_get_parameters does. */
int  slslam_lba_batch_get_covariance(const slslam_lba_batch* b, int index, int* status, int* num_free_cameras, int* free_camera,
                                     double* cov_cameras, double* cov_lines);
/* Since create: slslam_lba_batch_covariance calls, and the device / host buffers they allocated.  Any pointer may be NULL. */
int  slslam_lba_batch_covariance_stats(const slslam_lba_batch* b, long long* calls, long long* allocations);
/* ceres::Covariance for ONE window, no solve: the covariance at window->parameters (validates as slslam_lba_solve does, then needs
 * a device).  opt: huber_delta and baseline are what matters (NULL = slslam_default_options).  cov_lines = NULL skips the lines. */
int  slslam_lba_covariance(const slslam_lba_window* window, const slslam_solver_options* opt, int* status, int* num_free_cameras,
                           int* free_camera, double* cov_cameras, double* cov_lines);

/* ---- which observations are outliers, which line is degenerate (csrc/lba_report.h).
 * The LBA counterpart of slslam_po_edge_report; the Ceres counterpart is ceres::Problem::Evaluate with per-block residuals.  For a
 * window at its CURRENT device parameters (the point slslam_lba_batch_linearise and slslam_lba_batch_covariance evaluate), with
 * a = huber_delta (a <= 0: no loss):
 *   per observation i, in the caller's order, for EVERY observation of the window - those Ceres' preprocessing drops because both
 *   their camera and their line are constant included:
 *     sq_norm[i] = s_i = |r_i|^2 of the four raw residuals, before the corrector;
 *     weight[i]  = rho'(s_i): 1 if s_i <= a^2 or the loss is off, else a / sqrt(s_i) (the semantics of slslam_po_edge_report);
 *   per line, at the caller's line index: status (SLSLAM_LBA_LINE_*: CONSTANT = some observation flags it), num_observations,
 *     num_downweighted (observations with weight < 1), sq_norm_sum = sum s_i, cost = sum rho(s_i) / 2, and - FREE lines only, 0 otherwise -
 *     min_pivot: H_ll = sum J_l^T J_l over the line's observations (J_l after the corrector: the covariance's H_ll) is scaled to unit
 *     diagonal and Cholesky-factored; min_pivot is the smallest value under the square roots, up to and including the first non-positive
 *     one (a non-positive diagonal entry gives that entry).  This is the number slslam_lba_batch_covariance tests against 1e-10:
 *     min_pivot <= 1e-10 names the line that makes its window SLSLAM_COV_SINGULAR;
 *   per camera, at the caller's camera index: status (SLSLAM_LBA_CAMERA_*), num_observations, num_downweighted, sq_norm_sum, cost.
 * The sum of the lines' (or the cameras') cost is the window's cost, the fixed part included. */
enum { SLSLAM_LBA_LINE_FREE = 0, SLSLAM_LBA_LINE_CONSTANT = 1, SLSLAM_LBA_LINE_NO_OBSERVATIONS = 2 };
enum { SLSLAM_LBA_CAMERA_FREE = 0, SLSLAM_LBA_CAMERA_CONSTANT = 1, SLSLAM_LBA_CAMERA_NO_OBSERVATIONS = 2 };
typedef struct slslam_lba_line_report {
  int    status;                  /* SLSLAM_LBA_LINE_* */
  int    num_observations;
  int    num_downweighted;
  int    reserved;
  double sq_norm_sum;
  double cost;
  double min_pivot;
} slslam_lba_line_report;
typedef struct slslam_lba_camera_report {
  int    status;                  /* SLSLAM_LBA_CAMERA_* */
  int    num_observations;
  int    num_downweighted;
  int    reserved;
  double sq_norm_sum;
  double cost;
} slslam_lba_camera_report;
/* The report on every window of the batch: enqueues at most two launches on `stream` and returns.  No host round trip; changes nothing
 * the solve or the covariance reads or writes.  The result buffers are allocated by the first call and kept: a batch that never asks
 * pays nothing.  Every path reports - SLSLAM_PATH_GLOBAL_MEMORY and SLSLAM_PATH_MIXED too, which the covariance refuses -, refilled
 * batches and, through slslam_lba_stream_batch, a stream's.  A report and a covariance may both be enqueued before one download. */
int  slslam_lba_batch_report(slslam_lba_batch* b, void* stream);
/* After slslam_lba_batch_download / _wait (which bring the report enqueued since the last download back with the other results):
 * sq_norm[M], weight[M], lines[L], cameras[C] of window `index`.  Any output pointer may be NULL.
 * SLSLAM_ERR_INVALID_ARGUMENT: the last slslam_lba_batch_report call has not been downloaded - none was made, a newer one is still
 * on the device, or a refill has replaced the windows since; a window a device-built refill flagged returns that window's error. */
int  slslam_lba_batch_get_report(const slslam_lba_batch* b, int index, double* sq_norm, double* weight,
                                 slslam_lba_line_report* lines, slslam_lba_camera_report* cameras);
/* Since create: slslam_lba_batch_report calls, and the device / host buffers they allocated.  Any pointer may be NULL. */
int  slslam_lba_batch_report_stats(const slslam_lba_batch* b, long long* calls, long long* allocations);
/* The report for ONE window, no solve: at window->parameters (validates as slslam_lba_solve does, then needs a device).
 * opt: huber_delta and baseline are what matters (NULL = slslam_default_options). */
int  slslam_lba_report(const slslam_lba_window* window, const slslam_solver_options* opt, double* sq_norm, double* weight,
                       slslam_lba_line_report* lines, slslam_lba_camera_report* cameras);

/* ---- the 3-D segment of every line landmark (csrc/lba_segments.h).
 * The solve returns infinite lines; a map, a viewer or a data association needs their extent.  This is the reference's
 * SLAM::extend_end_points (src/slam.cpp:979-1084) per observation, for a window at its CURRENT device parameters (the point
 * slslam_lba_batch_report and _covariance evaluate), for EVERY line of the window, constant ones included.  A line u = (a, b, g, t) is
 * cp + s dv, cp its point closest to the origin and dv its unit direction as in the residual; a segment is an interval of s.
 *   per observation i of line l from camera c (R, t_c world to camera), LEFT image only (observations[8 i + 0..3] = x0 y0 x1 y1), in the
 *   caller's order:
 *     1. pc = R cp + t_c, dc = R dv; p1 = (x0, y0, 1), p2 = (x1, y1, 1); ln = (p1 x p2)[0:2] / its norm sqrt(lx^2 + ly^2).  A zero norm or a
 *        non-finite input: DEGENERATE.
 *     2. per endpoint p: the plane through the camera centre, p and p + (ln, 0) - normal m = p x (ln, 0) - cuts the line at
 *        s = -(m . pc) / (m . dc) (the reference's Lc * pi).  |m . dc| <= 1e-6 |m| for either endpoint: DEGENERATE.
 *     3. (pc + s dc).z < 0 for either endpoint: BEHIND.
 *     4. only with max_range > 0 (the reference: extension_length = 5.0): q = pc . dc, p0 = pc - q dc the line's point closest to the
 *        camera centre.  |p0| > max_range: OUT_OF_RANGE.  Else e = sqrt(max_range^2 - |p0|^2) and an endpoint with |s + q| > e moves to
 *        s = sign(s + q) e - q; the observation is then USED_CLAMPED.
 *     5. lo = min(s_1, s_2), hi = max(s_1, s_2); lo == hi: COLLAPSED, else USED / USED_CLAMPED.
 *     obs_status[i] = SLSLAM_SEGMENT_OBS_*; obs_range[2 i] = lo, hi - zeros unless USED / USED_CLAMPED;
 *   per line, at the caller's line index: status (OK; NO_OBSERVATIONS; NONE = observed, but no observation was used), num_observations,
 *     num_used, num_clamped, t_min = min lo and t_max = max hi over the used observations, p_min = cp + t_min dv and p_max = cp + t_max dv in
 *     the window's world frame.  All doubles are 0 unless the status is OK.
 * The union over a line's observations is what the reference's keyframe-by-keyframe update (slam.cpp:1065-1074) arrives at for a line
 * that does not move.  The reference's reset of tt when the direction pvn turns is map bookkeeping and stays with the caller. */
enum { SLSLAM_SEGMENT_OK = 0, SLSLAM_SEGMENT_NO_OBSERVATIONS = 1, SLSLAM_SEGMENT_NONE = 2 };
enum { SLSLAM_SEGMENT_OBS_USED = 0, SLSLAM_SEGMENT_OBS_USED_CLAMPED = 1, SLSLAM_SEGMENT_OBS_DEGENERATE = 2, SLSLAM_SEGMENT_OBS_BEHIND = 3,
       SLSLAM_SEGMENT_OBS_OUT_OF_RANGE = 4, SLSLAM_SEGMENT_OBS_COLLAPSED = 5 };
typedef struct slslam_lba_line_segment {
  int    status;                  /* SLSLAM_SEGMENT_* */
  int    num_observations;
  int    num_used;                /* USED + USED_CLAMPED */
  int    num_clamped;             /* USED_CLAMPED */
  double t_min, t_max;
  double p_min[3], p_max[3];
} slslam_lba_line_segment;
/* The segments of every window of the batch: enqueues one launch on `stream` and returns.  No host round trip; changes nothing the
 * solve, the covariance or the report reads or writes.  The result buffers are allocated by the first call and kept.  Every path
 * answers (SLSLAM_PATH_GLOBAL_MEMORY and SLSLAM_PATH_MIXED too), refilled batches and, through slslam_lba_stream_batch, a stream's.
 * Segments, a report and a covariance may all be enqueued before one download.  max_range <= 0: no clamp, nothing out of range; a
 * non-finite max_range: SLSLAM_ERR_INVALID_ARGUMENT. */
int  slslam_lba_batch_segments(slslam_lba_batch* b, void* stream, double max_range);
/* After slslam_lba_batch_download / _wait: obs_status[M], obs_range[2 M], lines[L] of window `index`.  Any output pointer may be NULL.
 * SLSLAM_ERR_INVALID_ARGUMENT: the last slslam_lba_batch_segments call has not been downloaded - none was made, a newer one is still
 * on the device, or a refill has replaced the windows since; a window a device-built refill flagged returns that window's error. */
int  slslam_lba_batch_get_segments(const slslam_lba_batch* b, int index, int* obs_status, double* obs_range, slslam_lba_line_segment* lines);
/* Since create: slslam_lba_batch_segments calls, and the device / host buffers they allocated.  Any pointer may be NULL. */
int  slslam_lba_batch_segments_stats(const slslam_lba_batch* b, long long* calls, long long* allocations);
/* The segments of ONE window, no solve: at window->parameters (validates as slslam_lba_report does, then needs a device).
 * opt: NULL = slslam_default_options. */
int  slslam_lba_segments(const slslam_lba_window* window, const slslam_solver_options* opt, double max_range, int* obs_status,
                         double* obs_range, slslam_lba_line_segment* lines);

/* Test hook: evaluate residuals / Jacobians (after the Huber corrector, before Jacobi scaling)
 * of window `index` at its CURRENT device parameters, returned in the caller's observation order:
 * residuals[4M], j_cam[24M] (row-major 4x6), j_line[16M] (row-major 4x4), cost[1]. */
int  slslam_lba_batch_linearise(slslam_lba_batch* b, int index, double* residuals, double* j_cam,
                                double* j_line, double* cost);

/* ---- page-locked host memory the GPU reads and writes IN PLACE.
 * Replaces: the `new int[...]` / `new double[...]` of the caller's five arrays per window (reference src/slam.cpp:899-903) for a caller
 * that streams windows: arrays allocated here (or in a range registered once with slslam_pinned_register - an arena the caller owns) are
 * read by the device straight over the host link during slslam_lba_batch_refill / slslam_lba_stream_submit (no host thread touches the
 * data; 57 GB/s measured, tools/micro/zero_copy_bench.hip) and the solved `parameters` are written back the same way.  Such arrays
 * must stay valid and unmodified until the results have been waited for / collected.  Arrays anywhere else keep working: the host threads
 * copy them into a pinned staging buffer first.  slslam_pinned_contains: 1 when [p, p + bytes) lies in one such range. */
int  slslam_pinned_alloc(size_t bytes, void** out);
int  slslam_pinned_free(void* p);
int  slslam_pinned_register(void* p, size_t bytes);
int  slslam_pinned_unregister(void* p);
int  slslam_pinned_contains(const void* p, size_t bytes);
/* The three index arrays of a window narrowed to ONE 32-bit word per observation - line | camera << 16 | camera constant << 24 |
 * line constant << 25 - the form the device build works on (16 -> 4 bytes per observation over the host link: what the staging copy
 * produces on the way).  SLSLAM_ERR_UNSUPPORTED when a camera index exceeds 255 or a line index 65534. */
int  slslam_pack_indices(int n, const int* camera_index, const int* line_index, const int* fixed_index, unsigned int* packed);

/* ---- a STREAM of windows (BASELINE config 4: many independent windows arriving in host memory): `depth` refillable batches in
 * flight on HIP streams of their own, so that packing (host threads), upload (copy engine), solve and download of consecutive
 * batches overlap.  submit() = LBAProblem::build + ceres::Solve for `n` windows, asynchronous: it returns when the windows' arrays
 * have been read or handed to the GPU (`parameters` of each window must stay valid - it is written by collect -, and so must arrays in
 * page-locked memory, which the GPU reads in place: slslam_pinned_alloc).  For arrays in ordinary (pageable) memory the results depend
 * only on what the arrays held when submit() was called: the caller may reuse or free them once it returns - all but `parameters`,
 * which must stay allocated but whose content is not read again.  collect() waits for that submit's
 * results and writes every window's solved parameters in place (the in/out contract of reference src/slam.cpp:957-972) and, when
 * `summaries` is not NULL, summaries[0 .. n).  Tickets must be collected before their slot comes round again (every `depth` submits:
 * SLSLAM_ERR_STATE otherwise).  options: as for a batch; host_threads (0 = up to 16) pack and copy; refill_headroom_percent 0 = 10. */
typedef struct slslam_lba_stream slslam_lba_stream;
int  slslam_lba_stream_create(int device, const slslam_solver_options* opt, int depth, slslam_lba_stream** out);
void slslam_lba_stream_destroy(slslam_lba_stream* s);
int  slslam_lba_stream_submit(slslam_lba_stream* s, const slslam_lba_window* windows, int n, int* ticket);
int  slslam_lba_stream_collect(slslam_lba_stream* s, int ticket, slslam_summary* summaries);
/* submit() for a caller whose packer writes the indices NARROWED: packed_index[i] (when not NULL) replaces window i's camera_index /
 * line_index / fixed_index by one 32-bit word per observation (slslam_pack_indices: what the loop at reference src/slam.cpp:904-912 would
 * store instead of four ints) - 68 instead of 80 bytes per observation over the host link, which is what a stream of windows is bound
 * by.  The words are validated on the device (or by the staging copy); everything else as submit(). */
int  slslam_lba_stream_submit_packed(slslam_lba_stream* s, const slslam_lba_window* windows, const unsigned int* const* packed_index, int n, int* ticket);
/* Host-side accounting since create: wall-clock ms the caller spent in submit (pack + layout + enqueue), waiting in collect, copying
 * results out; submits served by a refill / by building a batch; windows submitted; trust-region steps (successful + unsuccessful, the
 * count of reference src/slam.cpp:949-950) of the windows collected; host threads in use.  Any pointer may be NULL. */
int  slslam_lba_stream_stats(const slslam_lba_stream* s, double* ms_submit, double* ms_collect_wait, double* ms_collect_copy,
                             long long* refills, long long* builds, long long* windows, long long* lm_iterations, int* host_threads);
/* Of the refills: how many were built on the device, how many of those read the callers' page-locked observations and parameters in place (no
 * staging copy; the index arrays are narrowed by the host threads on the way); windows the
 * device build handed back to the host path at collect time (a camera that sees a line twice, a line with more than 64 observations, more
 * than 20 free cameras, no room in the slot's arrays).  A set that does not fit the slot AS A WHOLE (only the device knows the tiles it needs) is
 * packed by the host threads at collect time, solved as one batch that then takes the slot - its windows count here and as one `builds`.
 * Any pointer may be NULL. */
int  slslam_lba_stream_build_stats(const slslam_lba_stream* s, long long* device_builds, long long* zero_copy, long long* fallback_windows);
/* The batch that served `ticket` (valid until its slot is submitted to again; after collect: its traces, chunk cuts and sweep can be read
 * with the slslam_lba_batch_* getters).  Read only. */
int  slslam_lba_stream_batch(slslam_lba_stream* s, int ticket, slslam_lba_batch** batch);

/* ------------------------------------------------------------------ pose graph
 * Replaces: POProblem(size, n_iter) + set_pose_index_1/2 + set_constraints + set_parameters
 * (reference src/po_problem.h:112-130) and the arrays built at src/slam.cpp:1262-1280. */
typedef struct slslam_po_graph {
  int num_poses;                  /* kfs.size()                                        */
  int num_edges;                  /* POProblem::num_size()                             */
  const int*    pose_index_1;     /* [E]                                               */
  const int*    pose_index_2;     /* [E]                                               */
  const double* constraints;      /* [6E]: (w,t) of C = T_{n2<-n1}                     */
  double*       parameters;       /* [6N] in/out: (w,t) per pose; pose_index_1[0] is held constant */
  const double* sqrt_information; /* [36E] row-major W_e, or NULL: identity */
} slslam_po_graph;
/* sqrt_information (an extension: the reference's edges are unweighted, src/po_problem.h:68-108): W_e is ANY 6 x 6 matrix with
 * W_e^T W_e = Omega_e, the edge's information matrix - it need not be symmetric or triangular, any finite values are accepted, and a
 * non-finite entry is SLSLAM_ERR_INVALID_ARGUMENT, found before a device is needed.  The residual block of edge e becomes W_e Te and
 * its two Jacobian blocks W_e J1, W_e J2; the loss of po_huber_delta acts on s = |W_e Te|^2 (the weight inside the functor, as Ceres
 * has it), so every cost, the Jacobi scale, the gradient and the model see whitened blocks.  With the edges' true information matrices
 * s is chi-square with 6 degrees of freedom.  An all-zero W_e removes its edge (the LM damping keeps the solve defined).  NULL runs
 * the kernels there were before the field existed.  Fill the struct value-initialised (slslam_po_graph g = {0}) so that the field is
 * NULL unless set.  slslam_po_sqrt_information (below) makes W_e from a covariance block.  Honoured by slslam_po_solve,
 * slslam_po_edge_report, slslam_po_covariance and slslam_po_batch_add (a batch may mix graphs with and without); slslam_po_structure
 * ignores it. */

/* Replaces: POProblem::build + POProblem::set_options + ceres::Solve
 * (reference src/slam.cpp:1283-1293).  Synchronous; parameters solved in place.
 * opt->huber_delta (the LBA loss) and opt->baseline are ignored; the edges' loss is opt->po_huber_delta, 0 by default
 * (robustify ? new HuberLoss(0.001) : NULL with robustify = false: src/po_problem.cpp:27,55). */
int slslam_po_solve(const slslam_po_graph* graph, const slslam_solver_options* opt,
                    slslam_summary* summary, slslam_iteration* trace, int trace_cap, int* trace_len);

/* Per-edge report at graph->parameters - which slslam_po_solve has just updated in place -: sq_norm[e] = |Te|^2 of edge e (its six
 * residuals, src/po_problem.h:74-105; |W_e Te|^2 with graph->sqrt_information) and weight[e] = rho'(sq_norm[e]) under ceres::HuberLoss(po_huber_delta), the loss of
 * src/po_problem.cpp:27,55: 1 for an inlier (sq_norm <= delta^2) and whenever po_huber_delta is 0, else delta / sqrt(sq_norm).  The edge
 * with the smallest weight is the loop closure to drop.  sq_norm, weight: [num_edges] host arrays, either may be NULL.  Synchronous;
 * validates as slslam_po_solve does (SLSLAM_ERR_INVALID_ARGUMENT also for a negative or non-finite po_huber_delta), then needs a
 * device (SLSLAM_ERR_NO_DEVICE). */
int slslam_po_edge_report(const slslam_po_graph* graph, double po_huber_delta, double* sq_norm, double* weight);

/* The symbolic analysis behind the structured pose-graph factorisation (host only, no device needed), for
 * inspection and tests: slot[N] = offset of each pose in the reduced vector (-1: the constant pose of edge 0 or a
 * pose no edge references), chains first, junction poses last; chain_start / chain_len / chain_left / chain_right
 * [*num_chains, capacity max_chains] describe the chains (left / right = slot of what the chain ends at - a junction or, for a piece of a
 * long path, a cut pose -, -1 when free).  Returns SLSLAM_ERR_INVALID_ARGUMENT on malformed graphs, SLSLAM_ERR_UNSUPPORTED if max_chains is too small. */
int slslam_po_structure(const slslam_po_graph* graph, int* slot, int max_chains, int* num_chains, int* chain_start,
                        int* chain_len, int* chain_left, int* chain_right, int* num_chain_unknowns, int* num_unknowns);
/* The chains come on several levels (a long path is cut into pieces of ~L^(1/levels) poses by single cut poses; a path's cut poses form a
 * chain of the next level, eliminated after the pieces, and so on - up to three levels): how many of the chains the calling thread's last
 * slslam_po_structure listed - the first ones - are level-1 chains (consecutive poses are graph neighbours); the others are higher-level
 * chains (consecutive poses are cut poses of one path; left / right = a cut pose of a still higher level or the path's junction). */
int slslam_po_structure_level1(void);

/* ---- batched form: many independent pose graphs (sequence shards, cameras, replayed sessions) solved by one launch sequence.
 * Each graph goes through exactly the per-graph algorithm of slslam_po_solve's default path (structured fp64 factorisation): the
 * same slots, chain order and operation order; only the order of fp64 atomic sums can differ, so a graph's result does not depend
 * on the other graphs of the batch beyond that round-off.  Every launch of an LM iteration (~14) covers every graph.
 * create and add touch no device (a machine without one can validate); finalize is the first call that needs one
 * (SLSLAM_ERR_NO_DEVICE without).  device < 0 selects the device current at finalize. */
typedef struct slslam_po_batch slslam_po_batch;
int  slslam_po_batch_create(int device, slslam_po_batch** out);
void slslam_po_batch_destroy(slslam_po_batch* b);
/* Copies the graph's arrays (sqrt_information too, or notes its absence: per graph) and runs slslam_po_solve's validation (SLSLAM_ERR_INVALID_ARGUMENT, nothing added) and symbolic
 * analysis (slslam_po_structure).  Returns the graph's index in *index.  SLSLAM_ERR_STATE after finalize. */
int  slslam_po_batch_add(slslam_po_batch* b, const slslam_po_graph* graph, int* index);
/* One options struct for every graph, as for slslam_po_solve (huber_delta, baseline ignored; po_huber_delta honoured and checked); po_dense_factor = 1 or
 * po_factor_fp32 = 1: SLSLAM_ERR_UNSUPPORTED.  Allocates and uploads.  Device memory per graph of n = 6 x (free poses) unknowns
 * with nj of them on junction poses: the n x ld normal matrix plus the nj x ld junction factor in doubles, ld = n rounded up to 8,
 * plus 8 (about 20 MB for a 260-pose graph with 8 loop closures), and a few vectors.  A failed allocation returns SLSLAM_ERR_HIP
 * and leaves the batch unfinalized. */
int  slslam_po_batch_finalize(slslam_po_batch* b, const slslam_solver_options* opt);
/* Enqueues the complete LM solve of every graph on `stream` (a hipStream_t passed as void*, NULL = default stream).  Like
 * slslam_po_solve it asks the device, now and then, whether every graph has finished and then stops enqueueing: that question
 * synchronises the stream. */
int  slslam_po_batch_solve(slslam_po_batch* b, void* stream);
/* Initial poses back, LM state fresh (asynchronous on `stream`): the next solve starts over. */
int  slslam_po_batch_reset(slslam_po_batch* b, void* stream);
/* Blocks until the stream's work is done and copies every graph's poses, summary and trace back to the host. */
int  slslam_po_batch_download(slslam_po_batch* b, void* stream);
/* After download (SLSLAM_ERR_STATE before it, and after a reset or solve that followed it): what slslam_po_solve returns for the
 * graph - parameters[6N] (untouched for NUMERICAL_FAILURE, a graph without edges, unreferenced poses), summary, trace. */
int  slslam_po_batch_get_parameters(const slslam_po_batch* b, int index, double* parameters);
int  slslam_po_batch_get_summary(const slslam_po_batch* b, int index, slslam_summary* summary);
int  slslam_po_batch_get_trace(const slslam_po_batch* b, int index, slslam_iteration* trace, int trace_cap, int* trace_len);
/* slslam_po_edge_report for the graph, in the same states as slslam_po_batch_get_parameters and at the parameters it returns (a graph
 * whose solve ended in NUMERICAL_FAILURE: its untouched ones), under the po_huber_delta the batch was finalized with (the loss of
 * src/po_problem.cpp:27,55).  download computes every graph's report in one launch ahead of its copy.  Either output may be NULL. */
int  slslam_po_batch_get_edge_report(const slslam_po_batch* b, int index, double* sq_norm, double* weight);

/* ---- posterior covariances of pose graphs (csrc/po_covariance.h).
 * Replace nothing in the reference - consistency_broken() (src/slam.cpp:1215-1232) judges a loop closure by two fixed thresholds -;
 * the Ceres counterpart is ceres::Covariance on the problem POProblem::build wires up.
 * For a graph at its CURRENT parameters x (graph->parameters for the one-graph call; what slslam_po_batch_get_parameters would return
 * for a batch - the poses as added for a graph whose solve ended in NUMERICAL_FAILURE):
 *   free pose: referenced by at least one edge and not pose_index_1[0] (the rule of the solve: slslam_po_structure's slot >= 0);
 *   J: the Jacobian of all edges' six residuals (src/po_problem.h:68-108) w.r.t. the free poses, in the global (angle-axis, translation)
 *      coordinates, every block whitened by its W_e when the graph has sqrt_information, then the Huber corrector of po_huber_delta (a
 *      block with s = |W_e Te|^2 > delta^2 is scaled by sqrt(delta / sqrt(s)); 0: no loss), without Jacobi scaling or damping;
 *   H = J^T J, n = 6 x (free poses);  Sigma = H^-1.  Sigma is the covariance when W_e^T W_e are the edges' true information matrices;
 *   with sqrt_information NULL it is the covariance for unit-variance residuals - multiply by the noise variance.
 *   cov_poses[36 N]: the row-major 6 x 6 marginal Sigma_aa per caller pose index, zeros for the constant pose and unreferenced poses;
 *   cov_pairs[36 P]: for the caller's pairs (pair_a[k], pair_b[k]) the row-major block Sigma_ab, rows of a, columns of b; a == b gives
 *      the marginal; a pair that touches a constant or unreferenced pose gives zeros.
 * SLSLAM_COV_SINGULAR: a pivot <= 1e-10 in the Cholesky factorisation of H scaled to unit diagonal (the scaling is internal: outputs
 * are unscaled) - a component not connected to the constant pose has a 6-dimensional null space.  Every output of that graph is zero;
 * the other graphs of a batch are not affected.  The covariance of an edge error Te follows from Sigma_aa, Sigma_bb, Sigma_ab and the
 * Jacobians of the caller's functor. */
/* One graph, no solve, synchronous.  Validates as slslam_po_edge_report does - and SLSLAM_ERR_INVALID_ARGUMENT for a pair index outside
 * [0, num_poses), num_pairs < 0, or cov_pairs with num_pairs > 0 and a NULL pair array - before it needs a device
 * (SLSLAM_ERR_NO_DEVICE).  status, cov_poses, cov_pairs: any may be NULL. */
int  slslam_po_covariance(const slslam_po_graph* graph, double po_huber_delta, int num_pairs, const int* pair_a, const int* pair_b,
                          int* status, double* cov_poses, double* cov_pairs);
/* The pairs slslam_po_batch_covariance reports for graph `index` (none until set).  Host only: copies the pairs, replaces the graph's
 * previous list; allowed before and after finalize.  SLSLAM_ERR_INVALID_ARGUMENT as above.  Results of a covariance call made with
 * the previous list can no longer be read (slslam_po_batch_get_covariance). */
int  slslam_po_batch_set_covariance_pairs(slslam_po_batch* b, int index, int num_pairs, const int* pair_a, const int* pair_b);
/* Enqueues the covariance of every graph on `stream` and returns (after the first call, or a call that follows a replaced pair list:
 * those build the work lists and wait for their upload).  SLSLAM_ERR_STATE before finalize.  Under the po_huber_delta of finalize.
 * Changes nothing a solve, reset or download reads or returns.  Its buffers are allocated by the first call and kept; they grow only
 * when a pair list grew.  Device memory per graph: two n x ld matrices of doubles (the normal matrix, which the inverse factor
 * overwrites, and the Cholesky factor; ld = n rounded up to 8, plus 8: 39 MB for a 260-pose graph), 32 KB per 64 unknowns for the
 * diagonal blocks' inverses, 288 bytes per pose and per pair of results, and a few vectors. */
int  slslam_po_batch_covariance(slslam_po_batch* b, void* stream);
/* After slslam_po_batch_download, which brings the covariances enqueued since the last download back with the other results:
 * *status = SLSLAM_COV_*, cov_poses[36 N], cov_pairs[36 P] as above (a graph without edges: SLSLAM_COV_OK and zeros).  Any output
 * pointer may be NULL.  SLSLAM_ERR_INVALID_ARGUMENT: no covariance call has been downloaded, or a solve, a reset, a newer covariance
 * call or slslam_po_batch_set_covariance_pairs came after it. */
int  slslam_po_batch_get_covariance(const slslam_po_batch* b, int index, int* status, double* cov_poses, double* cov_pairs);
/* Since create: slslam_po_batch_covariance calls, and the device / host buffers they allocated.  Any pointer may be NULL. */
int  slslam_po_batch_covariance_stats(const slslam_po_batch* b, long long* calls, long long* allocations);
/* Host only, no device: the square-root information of an edge from a covariance.  cov[36]: a symmetric positive-definite 6 x 6 matrix
 * (row-major; the lower triangle is read), Sigma = L L^T; writes W = L^-1, lower triangular, row-major, so that W^T W = Sigma^-1 - what
 * slslam_po_graph.sqrt_information takes.  Factored after scaling to unit diagonal, by the rule of slslam_po_covariance: a scaled pivot
 * <= 1e-10 (or a diagonal entry <= 0) gives *status = SLSLAM_COV_SINGULAR and zeros, else SLSLAM_COV_OK.  Non-finite input, or a NULL cov
 * or sqrt_information: SLSLAM_ERR_INVALID_ARGUMENT.  status may be NULL.  This is the bridge from the 6 x 6 blocks slslam_lba_covariance,
 * slslam_lba_batch_get_covariance and slslam_po_covariance return (the covariance of a relative pose, in the edge error's coordinates:
 * INTEGRATION.md) to edge weights. */
int  slslam_po_sqrt_information(const double cov[36], double sqrt_information[36], int* status);

/* ---- statistics of an edge under the posterior covariance of its two poses (csrc/po_gate.h).
 * Serves the two places where the reference has an edge and no uncertainty for it: consistency_broken() (src/slam.cpp:1215-1232), which
 * judges a loop closure by two fixed thresholds on |w| and |t| of the edge error, and the odometry constraints built at
 * src/slam.cpp:1403-1416 (C = T_b o T_a^-1 at :1410-1412), which enter the graph unweighted.
 * One item: two poses x_a, x_b (angle-axis, translation), a constraint C, the joint covariance blocks Sigma_aa, Sigma_bb, Sigma_ab (row-major,
 * Sigma_ab = rows of a, columns of b) and a measurement covariance R (its lower triangle is read).  With
 *   Te = the edge error of the solve (src/po_problem.h:74-105; T1 = x_a, T2 = x_b), unwhitened;  Ja = dTe/dx_a, Jb = dTe/dx_b;
 *   S  = sigma2 (Ja Saa Ja^T + Jb Sbb Jb^T + Ja Sab Jb^T + Jb Sab^T Ja^T) + R;
 *   W  = slslam_po_sqrt_information(S): lower triangular, W^T W = S^-1;   m2 = Te^T S^-1 Te = |W Te|^2,
 * the outputs per item are status[1] (SLSLAM_COV_*), error[6] = Te, cov[36] = S, sqrt_information[36] = W, mahalanobis2[1] = m2.
 * SLSLAM_COV_SINGULAR by the rule of slslam_po_sqrt_information (a pivot <= 1e-10 of S scaled to unit diagonal, or a diagonal entry
 * <= 0): that item gets zeros for cov, sqrt_information and mahalanobis2, its error is still written, the other items are unaffected.
 * |w| and |t| of error are what consistency_broken() thresholds; m2 is chi-square with 6 degrees of freedom for a consistent edge.
 * sigma2: finite and positive, for the whole call - the noise variance that multiplies unit-variance covariances (slslam_po_covariance of
 * an unweighted graph), 1 for covariances of weighted graphs and for slslam_lba_batch_get_covariance blocks already scaled. */
typedef struct slslam_po_edge_items {
  int n;
  const double* pose_a;        /* [6 n]  */
  const double* pose_b;        /* [6 n]  */
  const double* constraints;   /* [6 n]  */
  const double* cov_aa;        /* [36 n] or NULL = zeros (a constant pose) */
  const double* cov_bb;        /* [36 n] or NULL */
  const double* cov_ab;        /* [36 n] or NULL */
  const double* cov_meas;      /* [36 n] R, or NULL = zeros (slslam_po_constraint_covariance makes it) */
  double sigma2;
} slslam_po_edge_items;
/* n independent items, host pointers, synchronous: one upload, one launch, one download.  Any output may be NULL.
 * SLSLAM_ERR_INVALID_ARGUMENT - found before an output is written or a device is needed -: items NULL, n < 0, sigma2 not finite or <= 0,
 * a NULL pose or constraint array with n > 0, a non-finite input.  n == 0 succeeds and does nothing.  With x_a, x_b two cameras of a
 * solved LBA window, C = T_b o T_a^-1 and the camera blocks of slslam_lba_batch_get_covariance, sqrt_information is the odometry
 * edge's W_e for slslam_po_graph.sqrt_information. */
int  slslam_po_edge_statistics(const slslam_po_edge_items* items, int* status, double* error, double* cov, double* sqrt_information,
                               double* mahalanobis2);
/* Candidate edges between poses of a graph: item k is (x[pose_a[k]], x[pose_b[k]], constraints[k], the graph's own Sigma blocks, cov_meas[k]). */
typedef struct slslam_po_candidates {
  int num;
  const int* pose_a;           /* [num] pose indices of the graph, a != b */
  const int* pose_b;           /* [num] */
  const double* constraints;   /* [6 num] */
  const double* cov_meas;      /* [36 num] or NULL (slslam_po_constraint_covariance makes it) */
  double sigma2;
} slslam_po_candidates;
/* One graph at graph->parameters, no solve, synchronous: the launch sequence of slslam_po_covariance (weights and po_huber_delta
 * honoured) with the candidates as its pairs, then one launch that reads Sigma_aa, Sigma_bb, Sigma_ab and the poses where they are on the
 * device; only the statistics come back.  *cov_status: the graph's SLSLAM_COV_*; when it is SLSLAM_COV_SINGULAR every candidate is
 * singular (zeros, error written).  A candidate that touches the constant pose has zero blocks for it.  Outputs as above, [num] items;
 * any may be NULL.  Validates as slslam_po_covariance does, and the candidates (NULL, num < 0, an index outside [0, num_poses), a == b,
 * sigma2, non-finite values): SLSLAM_ERR_INVALID_ARGUMENT before an output is written or a device is needed. */
int  slslam_po_gate(const slslam_po_graph* graph, double po_huber_delta, const slslam_po_candidates* candidates, int* cov_status, int* status,
                    double* error, double* cov, double* sqrt_information, double* mahalanobis2);
/* The candidates slslam_po_batch_gate judges for graph `index` (none until set).  Host only: copies them, replaces the previous list
 * (num == 0 clears it); before or after finalize.  Results of an earlier gate or covariance call can no longer be read. */
int  slslam_po_batch_set_candidates(slslam_po_batch* b, int index, const slslam_po_candidates* candidates);
/* slslam_po_batch_covariance with, per graph, the caller's pairs followed by the candidates, plus one launch over every (graph,
 * candidate).  Same states, same invalidation rules, counted by slslam_po_batch_covariance_stats; slslam_po_batch_get_covariance
 * returns afterwards what it would after slslam_po_batch_covariance.  A second call with unchanged lists allocates nothing.  A graph
 * without edges is not on the device (no free pose: S = R): its candidates, if it has any, are judged inside this call through
 * slslam_po_edge_statistics - a synchronous upload, launch and download on the default stream, not on `stream`. */
int  slslam_po_batch_gate(slslam_po_batch* b, void* stream);
/* After slslam_po_batch_download: graph `index`'s statistics, [num] items (any output may be NULL).  SLSLAM_ERR_INVALID_ARGUMENT under
 * the rules of slslam_po_batch_get_covariance - no gate call has been downloaded, or a solve, a reset, a newer covariance or gate call,
 * or a replaced pair or candidate list came after it. */
int  slslam_po_batch_get_gate(const slslam_po_batch* b, int index, int* status, double* error, double* cov, double* sqrt_information,
                              double* mahalanobis2);

/* ---- the covariance of a constraint in the coordinates of its edge's error (csrc/po_constraint_cov.h): the R above.
 * A loop-closure edge of the reference is the output of pose_estimation on the matched lines (src/slam.cpp:1146-1155: edge_t e(best_motion)
 * between lc_kf_id and the current keyframe); here that is slslam_pose_estimator_run, whose covariance
 * (slslam_pose_estimator_get_covariance) is over the constraint's own six parameters (w_C, t_C).  Per item, with Te the edge error above
 * and J_C = dTe/dC (6 x 6; not the identity: a rotation by R_a, the lever arm t_a, and T_b^-1 in front of both):
 *   error[6] = Te,  jacobian[36] = J_C row-major,  cov_meas[36] = sigma2 J_C Sigma_C J_C^T, exactly symmetric.
 * cov_meas is what slslam_po_edge_items.cov_meas and slslam_po_candidates.cov_meas take. */
typedef struct slslam_po_constraint_items {
  int n;
  const double* pose_a;          /* [6 n]  */
  const double* pose_b;          /* [6 n]  */
  const double* constraints;     /* [6 n]  */
  const double* cov_constraint;  /* [36 n] covariance of (w_C, t_C); the lower triangle is read; NULL = zeros */
  double sigma2;                 /* finite, > 0: multiplies cov_constraint */
} slslam_po_constraint_items;
/* n independent items, host pointers, synchronous: one upload, one launch, one download.  Any output may be NULL.
 * SLSLAM_ERR_INVALID_ARGUMENT - found before an output is written or a device is needed -: items NULL, n < 0, sigma2 not finite or <= 0,
 * a NULL pose or constraint array with n > 0, a non-finite input.  n == 0 succeeds and does nothing. */
int  slslam_po_constraint_covariance(const slslam_po_constraint_items* items, double* error, double* jacobian, double* cov_meas);

/* ------------------------------------------------------------------ RANSAC hypothesis scoring
 * (the per-frame cost centre next to the hot path.)
 * Replaces: the scoring loop of SLAM::ransac_motion (reference src/slam.cpp:396-413) with
 * SLAM::reprojection_error (src/slam.cpp:691-726) as its body: for every motion hypothesis and every
 * common line, the mean absolute endpoint-to-line distance in both stereo images, an inlier when it is
 * below error_thr = 5 / focal_length (src/parameter.h:56); hypotheses with |t| > 1 are skipped
 * (src/slam.cpp:398-399) and score -1 here.  The reference's float/double mix (float `sql`, float
 * error accumulator) is reproduced exactly, so scores and inlier sets are bit-identical. */
typedef struct slslam_ransac_frame {
  int num_hypotheses;             /* motions to score                                           */
  int num_lines;                  /* comm_size: lines visible in both frames                    */
  const double* poses;            /* [12 H]: R row-major (9) then t (3) of each motion pose_t    */
  const double* observations;     /* [8 K]: obs1 of each common line (current frame)            */
  const double* lines;            /* [6 K]: (closest point, direction) of each line, world frame */
} slslam_ransac_frame;

/* scores[H]: inlier count per hypothesis (-1 when skipped);
 * inlier_bits[H * ((K + 63) / 64)]: bit k of word k / 64 set when line k is an inlier (may be NULL).
 * Synchronous; host pointers. */
int slslam_ransac_score(const slslam_ransac_frame* frame, double baseline, double error_thr,
                        int* scores, unsigned long long* inlier_bits);

/* ------------------------------------------------------------------ RANSAC hypothesis generation + trial loop
 * Replaces: SLAM::vo_angle_axis_approx (reference src/slam.cpp:433-574) — the linearised stereo-line motion from
 * s = max_feat_num = 5 sampled correspondences — for EVERY pre-drawn trial at once (lane <-> trial), and
 * SLAM::ransac_motion (src/slam.cpp:322-427): generate, score, then replay the reference's adaptive trial loop
 * (`trial_cnt < ransac_trial && trial_cnt <= max_trials`, ransac_trial re-estimated whenever the best score
 * improves, :363, :415-423) in trial order over the scores, so that best pose, best score, inlier set and
 * trial_cnt are what the sequential loop returns for the same sample sequence.  The caller draws the samples
 * (the reference: rand.rand_sample(sample, comm_size, s) once per trial, :366). */
typedef struct slslam_ransac_trials {
  int num_trials;                 /* pre-drawn trials (<= max_trials + 1 are ever looked at)            */
  int sample_size;                /* s = max_feat_num (src/parameter.h:25), 1..16                       */
  int num_lines;                  /* comm_size                                                          */
  const int*    samples;          /* [num_trials * s] indices into the common-line arrays               */
  const double* observations0;    /* [8 K] obs0: previous frame                                         */
  const double* observations1;    /* [8 K] obs1: current frame                                          */
} slslam_ransac_trials;

/* poses[12 H] (R row-major | t), valid[H] = num_sol (0 when a degenerate sample made the reference return 0).
 * `baseline` is passed through as given (the reference calls it with -baseline, src/slam.cpp:392). */
int slslam_ransac_generate(const slslam_ransac_trials* trials, double baseline, double* poses, int* valid);

/* Whole ransac_motion.  lines [6 K] as in slslam_ransac_frame.  *best_score_io: in = the caller's running best
 * (SLAM::pose_estimation starts it at -1, reference src/slam.cpp:283: a trial that scores 0 then becomes the best, and the
 * re-estimated trial count lets the loop run to max_trials), out = best score; *trial_cnt = trials executed; best_pose[12] and best_inlier_bits[(K+63)/64]
 * (may be NULL) are written only when some trial beat the incoming best score. */
int slslam_ransac_motion(const slslam_ransac_trials* trials, const double* lines, double baseline, double error_thr,
                         double prob_free_outliers, int max_trials, int* best_score_io, int* trial_cnt,
                         double* best_pose, unsigned long long* best_inlier_bits);

/* slslam_ransac_motion for many frames at once (sequence replay, several cameras): one upload, two launches per
 * frame enqueued back to back, one download.  frames[F], lines[F] (pointer per frame), best_score_io[F] in/out,
 * trial_cnt[F], best_pose[12 F], best_inlier_bits[F] (pointer per frame; the array or an entry may be NULL). */
int slslam_ransac_motion_batch(int num_frames, const slslam_ransac_trials* frames, const double* const* lines,
                               double baseline, double error_thr, double prob_free_outliers, int max_trials,
                               int* best_score_io, int* trial_cnt, double* best_pose,
                               unsigned long long* const* best_inlier_bits);

/* ------------------------------------------------------------------ per-frame pose estimation
 * Replaces: SLAM::pose_estimation (reference src/slam.cpp:244-319) after its merge by feature id (:250-272; the host layer's
 * slslam_pose_estimation_inputs, slslam_amd/host/window_packer.h, restates it), for many independent frames per call.  Per frame:
 *   1. fewer than 5 common lines (:275): SLSLAM_POSE_TOO_FEW_FEATURES, nothing else runs;
 *   2. RANSAC exactly as slslam_ransac_motion_batch with best_score starting at -1 (:283) and the start pose at identity;
 *   3. best score < 5 = max_feat_num (:295): SLSLAM_POSE_RANSAC_FAILED, no motion-only solve;
 *   4. motion-only bundle adjustment on the RANSAC inliers (:303, :578-675), packed as slslam_pack_motion_only documents, solved with
 *      the estimator's options on the fused motion-only path; pose = gc_wt_to_Rt of the solved camera;
 *   5. final inliers (:305-312): the common lines whose reprojection error under the refined pose is below error_thr (every line:
 *      no |t| > 1 test), with the float/double arithmetic of slslam_ransac_score.
 * Frames are independent: a frame's results do not depend on the others in the call.
 * The whole chain stays on the device: one upload, two launches for the RANSAC of every frame, one download of the scores (the adaptive
 * trial loop runs on the host), one launch that packs every motion-only window, a refill of the estimator's batch from those device
 * windows and its solve, one launch that finishes every frame, one download - two host round trips per call whatever the frame count. */
typedef struct slslam_pose_estimator slslam_pose_estimator;
enum { SLSLAM_POSE_OK = 0, SLSLAM_POSE_TOO_FEW_FEATURES = 1, SLSLAM_POSE_RANSAC_FAILED = 2 };
typedef struct slslam_pose_estimate {
  int    status;                  /* SLSLAM_POSE_*                                                                         */
  int    trial_cnt;               /* RANSAC trials executed (0 for TOO_FEW_FEATURES)                                       */
  int    ransac_score;            /* best RANSAC score (-1 when no trial beat the start)                                   */
  double ransac_pose[12];         /* the RANSAC winner, R row-major | t (identity when no trial won)                       */
  unsigned long long* ransac_inlier_bits;  /* in: caller-owned [(K + 63) / 64] or NULL; out: the winner's inlier bits (0 when none)  */
  slslam_summary summary;         /* of the motion-only solve (zeroed unless status is OK)                                  */
  double pose[12];                /* the refined pose (status OK), else ransac_pose                                         */
  int    num_inliers;             /* final inliers (0 unless status is OK)                                                  */
  unsigned long long* inlier_bits;         /* in: caller-owned [(K + 63) / 64] or NULL; out: bit k of word k / 64 = line k is a final inlier */
} slslam_pose_estimate;

/* device < 0 selects the current HIP device.  opt: the motion-only solve's options (NULL = slslam_default_options); the estimator's
 * batch always takes the fused motion-only path, refillable (refill_headroom_percent 0 becomes 10), built on the device.
 * max_frames / max_lines: the capacity its device buffers and batch are made for (at the first run); a run that needs more frames with
 * a motion-only solve, or more common lines, makes them anew.  Touches no device: a machine without one fails at run. */
int  slslam_pose_estimator_create(int device, const slslam_solver_options* opt, int max_frames, int max_lines, slslam_pose_estimator** out);
void slslam_pose_estimator_destroy(slslam_pose_estimator* est);
/* frames[F], lines[F] and the thresholds as slslam_ransac_motion_batch (samples of frame f index its K common lines; observations0 =
 * obs0, the previous frame, observations1 = obs1, the current one; lines [6 K] in the previous frame's coordinates); out[F].
 * Every argument is validated before an output is written or the device is asked: SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched.
 * Synchronous; host pointers. */
int  slslam_pose_estimator_run(slslam_pose_estimator* est, int num_frames, const slslam_ransac_trials* frames, const double* const* lines,
                               double baseline, double error_thr, double prob_free_outliers, int max_trials, slslam_pose_estimate* out);
/* Since create: runs, device / page-locked buffer allocations of the estimator (with covariance enabled: those of
 * slslam_lba_batch_covariance in its batch included), batches finalized, batch refills.  Any pointer may be NULL. */
int  slslam_pose_estimator_stats(const slslam_pose_estimator* est, long long* calls, long long* allocations, long long* finalizes,
                                 long long* refills);
/* Test hook: the motion-only window the last run packed on the device for `frame` (status OK only, else SLSLAM_ERR_STATE) -
 * *num_lines = n inliers, index_words[2n] (slslam_pack_indices form), observations[16n], parameters[12 + 4n] - and solved_camera[6],
 * the solved (angle-axis, t) of camera 0.  Any array may be NULL. */
int  slslam_pose_estimator_window(const slslam_pose_estimator* est, int frame, unsigned int* index_words, double* observations,
                                  double* parameters, double* solved_camera, int* num_lines);

/* The covariance of every solved frame's motion, opt-in (default 0).  Host only; takes effect at the next slslam_pose_estimator_run.
 * With enable == 0 a run is the run it was: the same launches, the same allocations, the same bytes out.  With it, the run enqueues
 * slslam_lba_batch_covariance (cameras only) on its motion-only batch behind the solve and one launch that gathers the blocks into the
 * result block of the run's one download; slslam_pose_estimate does not change. */
int  slslam_pose_estimator_set_covariance(slslam_pose_estimator* est, int enable);
/* After a run that had covariance enabled, for a frame whose status is SLSLAM_POSE_OK:
 *   constraint[6]  the solved camera 0 (angle-axis, t) - the six doubles slslam_pose_estimator_window returns as solved_camera: the C of an
 *                  edge previous frame -> current frame (T_{b<-a}), in the parameters cov is over;
 *   cov[36]        row-major, exactly symmetric: the camera block slslam_lba_covariance defines for the frame's motion-only window at its
 *                  solved parameters under the estimator's options (H = sum J_cam^T J_cam over the kept residual blocks after the Huber
 *                  corrector, no Jacobi scaling, no damping; cov = H^-1), in unit-variance units;
 *   *status        SLSLAM_COV_* by the pivot rule of slslam_lba_batch_covariance; SLSLAM_COV_SINGULAR: zeros in cov, the rest still written;
 *   *dof           4 num_residual_blocks - 6 (>= 14: a solved frame has >= 5 inliers);
 *   *sigma2        2 (summary.final_cost - summary.fixed_cost) / dof: the summary's final_cost includes fixed_cost (the cost of the
 *                  blocks between the constant camera and the constant lines), so this is the cost of the kept blocks alone at the
 *                  solved pose.  sigma2 cov is the covariance of constraint.
 * Any output pointer may be NULL.  SLSLAM_ERR_INVALID_ARGUMENT: a NULL estimator or a negative frame; then SLSLAM_ERR_STATE: no run has
 * been made, or the last one had covariance disabled or failed; then SLSLAM_ERR_INVALID_ARGUMENT: frame beyond the last run's frames;
 * then SLSLAM_ERR_STATE: the frame is not SLSLAM_POSE_OK.  Nothing is written in any of these cases. */
int  slslam_pose_estimator_get_covariance(const slslam_pose_estimator* est, int frame, int* status, double constraint[6], double cov[36],
                                          double* sigma2, int* dof);

/* ------------------------------------------------------------------ line matching: which observation of a frame sees which map line
 * The link in front of the pose estimator (csrc/line_match.h).  The reference pairs observations by landmark id
 * (SLAM::pose_estimation, src/slam.cpp:250-272) or takes the pairs of its place recogniser, which is commented out; a caller who has a
 * predicted pose, a frame of stereo line observations and a map of solved lines - loop closure, relocalisation, landmarks whose track
 * was lost - has no correspondences.  Every observation k of a frame is tried against every map line l:
 *   e(k, l)     the float SLAM::reprojection_error(obs_k, pose, line_l) returns (src/slam.cpp:691-726), with the arithmetic of
 *               slslam_ransac_score: the bits are the same;
 *   admissible  e is finite and (double)e < error_thr and, when the frame gives extents, the 3-D interval [lo, hi] that the
 *               observation's LEFT segment cuts out of line l (the per-observation steps of slslam_lba_batch_segments with max_range 0;
 *               pc, dc under the frame's pose) is SLSLAM_SEGMENT_OBS_USED and meets [t_min - margin, t_max + margin]:
 *               hi >= t_min - margin and lo <= t_max + margin.  Any other segment status (a line behind the camera, a segment of zero
 *               length, ...) makes the pair inadmissible; so does a NaN extent.  A line without a segment: pass t_min > t_max.
 *   per k       best_line = the admissible l of the smallest e, the lowest l on ties (-1: none); best_error = that e, second_error = the
 *               smallest admissible e over l != best_line (+inf each when absent); num_admissible = admissible l;
 *   per l       best_observation = the admissible k of the smallest e, the lowest k on ties (-1: none);
 *   match[k]    best_line[k] when best_line[k] >= 0, best_observation[best_line[k]] == k (mutual) and
 *               (double)best_error[k] * ratio <= (double)second_error[k] (unambiguous; ratio <= 1 switches this test off), else -1.
 * Minima and counts only: a frame's results do not depend on the other frames of the call or on the order of evaluation. */
typedef struct slslam_match_frame {
  int num_observations;          /* K >= 0 */
  int num_lines;                 /* L >= 0 */
  const double* pose;            /* [12] predicted pose_t of the frame, R row-major | t, as in slslam_ransac_frame */
  const double* observations;    /* [8 K] */
  const double* lines;           /* [6 L] (closest point, direction), world frame, as in slslam_ransac_frame */
  const double* extents;         /* [2 L] t_min, t_max of each line along its direction (slslam_lba_line_segment), or NULL */
} slslam_match_frame;
enum { SLSLAM_MATCH_OK = 0, SLSLAM_MATCH_EMPTY = 1, SLSLAM_MATCH_INVALID_POSE = 2 };
typedef struct slslam_match_result {
  int    status;                 /* SLSLAM_MATCH_*: EMPTY when K = 0 or L = 0 (the pose is not read), else INVALID_POSE when one of the    */
                                 /* pose's 12 doubles is not finite; either way nothing is admissible and the arrays say so               */
  int    num_matched;            /* match[k] >= 0                                                                                         */
  int*   match;                  /* in: caller-owned arrays, any of them may be NULL; out: as above.  [K]                                 */
  int*   best_line;              /* [K] */
  float* best_error;             /* [K] */
  float* second_error;           /* [K] */
  int*   num_admissible;         /* [K] */
  int*   best_observation;       /* [L] */
} slslam_match_result;
typedef struct slslam_line_matcher slslam_line_matcher;

/* device < 0 selects the current HIP device.  max_observations / max_lines (>= 1): the most a frame of a run may hold; max_frames (>= 1)
 * with them: what the matcher's one device block and one page-locked block are made for at the first run.  A run of more frames makes
 * larger ones; a run that fits allocates nothing.  Touches no device: a machine without one fails at run. */
int  slslam_line_matcher_create(int device, int max_frames, int max_observations, int max_lines, slslam_line_matcher** out);
void slslam_line_matcher_destroy(slslam_line_matcher* matcher);
/* frames[F], out[F].  baseline, error_thr as slslam_ransac_score; ratio, margin as above (none of the four may be NaN, margin >= 0).
 * Every argument is validated before an output is written or the device is asked - a negative count, a missing array of a non-zero
 * count, K or L beyond the matcher's maximum: SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched.  Synchronous; host pointers; one upload,
 * three launches (per line, per pair, finish) and one download per call whatever the number of frames. */
int  slslam_line_matcher_run(slslam_line_matcher* matcher, int num_frames, const slslam_match_frame* frames, double baseline,
                             double error_thr, double ratio, double margin, slslam_match_result* out);
/* Since create: runs, and how often the matcher's blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_line_matcher_stats(const slslam_line_matcher* matcher, long long* calls, long long* allocations);
/* One frame, one call (its own buffers, made and freed). */
int  slslam_match_lines(const slslam_match_frame* frame, double baseline, double error_thr, double ratio, double margin,
                        slslam_match_result* out);

/* ------------------------------------------------------------------ structure-only refinement: every camera constant, every line free
 * The mirror image of the motion-only window (multi-view line triangulation): with the cameras fixed every line is its own 4-unknown
 * Levenberg-Marquardt problem with its own trust region.  Where it is used: a landmark made from one stereo pair (initialize_lm,
 * reference src/slam.cpp:161-219) has a poor depth until two free keyframes see it; the lines seen from a frame whose pose
 * slslam_pose_estimator_run has just fixed; the lines of keyframes a pose-graph solve has moved.  One launch solves every line of every
 * window of a call, lane <-> line (csrc/lba_refine_lines.h); a line's result does not depend on the other lines or windows of the call. */
typedef struct slslam_line_refiner slslam_line_refiner;
enum { SLSLAM_LINE_REFINED = 0, SLSLAM_LINE_CONSTANT = 1, SLSLAM_LINE_NO_OBSERVATIONS = 2, SLSLAM_LINE_INVALID = 3 };
typedef struct slslam_line_result {       /* one per line of a window */
  int    status;                  /* SLSLAM_LINE_*; anything but REFINED: the line's four doubles are untouched, the fields below 0  */
  int    termination_type;        /* as slslam_summary.termination_type                                                             */
  int    num_successful_steps, num_unsuccessful_steps;
  int    num_observations;        /* observations that name the line (every status)                                                 */
  double initial_cost, final_cost;
} slslam_line_result;

/* device < 0 selects the current HIP device.  opt (NULL = slslam_default_options): max_num_iterations (0: the costs only), huber_delta,
 * baseline, the trust-region constants and jacobi_scaling are used, everything else is ignored.  max_lines / max_observations: what the
 * device and page-locked buffers are made for at the first run - lines in whole waves of 64 per window, observations with each wave's
 * lines padded to its longest (at most 126 x a window's longest line); a run that needs more makes larger ones, a run that does not
 * allocates nothing.  Touches no device: a machine without one fails at run. */
int  slslam_line_refiner_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations,
                                slslam_line_refiner** out);
void slslam_line_refiner_destroy(slslam_line_refiner* refiner);
/* windows[n]: fixed_index[2i] (camera) is ignored - every camera is constant; fixed_index[2i+1] keeps the solve's meaning - one flagged
 * observation makes the line constant (SLSLAM_LINE_CONSTANT).  A line nobody observes: SLSLAM_LINE_NO_OBSERVATIONS.  A line with a
 * non-finite parameter or observation, or seen from a camera with a non-finite parameter: SLSLAM_LINE_INVALID; the other lines are
 * unaffected.  windows[i].parameters: the refined lines in place (a line that ends in SLSLAM_NUMERICAL_FAILURE keeps its values), the
 * camera part is read and never written.  results (may be NULL; results[i] may be NULL): windows[i].num_lines records; totals (may be
 * NULL): per window the sums over its refined lines (steps, costs, 4 parameters and the observations of each; termination_type:
 * NUMERICAL_FAILURE if a line failed, else NO_CONVERGENCE if a line stopped at the iteration cap, else the largest of the lines').
 * An index out of range, a negative count or a missing array: SLSLAM_ERR_INVALID_ARGUMENT for the call, nothing written.  More than
 * 630 cameras in a window: SLSLAM_ERR_UNSUPPORTED.  Synchronous; host pointers; one upload, one launch, one download per call. */
int  slslam_line_refiner_run(slslam_line_refiner* refiner, int n, const slslam_lba_window* windows,
                             slslam_line_result* const* results, slslam_summary* totals);
/* Since create: runs, device / page-locked buffer allocations.  Either pointer may be NULL. */
int  slslam_line_refiner_stats(const slslam_line_refiner* refiner, long long* calls, long long* allocations);
/* One window, one call (its own buffers, made and freed). */
int  slslam_lba_refine_lines(const slslam_lba_window* window, const slslam_solver_options* opt,
                             slslam_line_result* results, slslam_summary* total);

/* ------------------------------------------------------------------ line triangulation: making a landmark from all its observations
 * Replaces: SLAM::add_lms -> SLAM::initialize_lm (reference src/slam.cpp:161-219), which makes a line from the first stereo pair that
 * sees it and never revisits that start, and the gc_line_from_pose + gc_av_to_orth that put it into a window (src/slam.cpp:884-888).
 * Fills the line part of slslam_lba_window.parameters from the window's cameras and observations (csrc/lba_triangulate.h):
 *   stereo-first  initialize_lm of the line's first observation in the caller's order, in its operation order - gc_ppp_pi of the left and
 *                 right segments, gc_pipi_plk, gc_plucker_origin, the |cp| < 0.1 || > 10 clamp to cp / |cp| / inverse_depth, the cp.z < 0
 *                 flip - then gc_line_from_pose under that observation's camera;
 *   multi-view    (method 1) the two back-projected planes of EVERY observation of the line, in the world, scaled to a unit normal (a
 *                 plane whose normal has no length - a segment of zero length - is skipped); their symmetric 4 x 4 Gram matrix, summed in
 *                 the caller's order; the line of the two eigenvectors of its two largest eigenvalues (gc_pipi_plk, gc_plucker_origin),
 *                 its direction signed like the stereo-first one.  Neither the clamp nor the flip applies to it;
 *   choice        with the eigenvalues l1 >= l2 >= l3 >= l4: the multi-view line when the line has >= 2 observations, every number of it
 *                 is finite and l2 >= min_parallax l1, else the stereo-first line.  l2 / l1 is a parallax measure.
 * Where it is used: the unmatched observations slslam_line_matcher_run leaves, once slslam_pose_estimator_run has fixed their frame;
 * the lines of a window rebuilt after a pose-graph solve; in front of slslam_line_refiner_run or the window solve.  One launch handles
 * every line of every window of a call, lane <-> line; a line's bytes do not depend on the other lines or windows of the call. */
typedef struct slslam_line_triangulator slslam_line_triangulator;
enum { SLSLAM_TRI_MULTIVIEW = 0, SLSLAM_TRI_STEREO = 1, SLSLAM_TRI_CONSTANT = 2, SLSLAM_TRI_NO_OBSERVATIONS = 3, SLSLAM_TRI_INVALID = 4 };
typedef struct slslam_triangulated_line {  /* one per line of a window */
  int    status;                  /* SLSLAM_TRI_*; anything but MULTIVIEW / STEREO: the line's four doubles are untouched               */
  int    num_observations;        /* observations that name the line (every status)                                                   */
  int    num_planes;              /* planes that entered the Gram matrix: 2 per observation less the skipped ones; 0 for method 0     */
                                  /* and for a line that is not MULTIVIEW / STEREO                                                    */
  int    first_camera;            /* camera of the line's first observation (every status; -1: nobody observes the line)              */
  double eigenvalues[4];          /* descending; zeros for method 0 and for every line that is not MULTIVIEW: read as "no parallax"   */
  int    clamped;                 /* the stereo-first line was taken and its depth clamp fired                                        */
  int    reserved;
} slslam_triangulated_line;

/* device < 0 selects the current HIP device.  opt (NULL = slslam_default_options): baseline is used, everything else is ignored.
 * max_lines / max_observations: as for slslam_line_refiner_create.  Touches no device: a machine without one fails at run. */
int  slslam_line_triangulator_create(int device, const slslam_solver_options* opt, long long max_lines, long long max_observations,
                                     slslam_line_triangulator** out);
void slslam_line_triangulator_destroy(slslam_line_triangulator* triangulator);
/* windows[n].  method 0: the reference's start (stereo-first) for every line; method 1: as above.  inverse_depth: what the clamp puts a
 * line at (the reference's value is 0.1, src/parameter.h:55).  min_parallax: 0 never falls back on parallax.
 * fixed_index[2i] (camera) is ignored; one flagged fixed_index[2i+1] makes the line SLSLAM_TRI_CONSTANT, as in the refiner.  A line
 * nobody observes: SLSLAM_TRI_NO_OBSERVATIONS.  SLSLAM_TRI_INVALID: a non-finite observation of the line or a non-finite parameter of
 * a camera that sees it, or a stereo-first line with v = 0 (the two planes of the first observation are parallel or coincide, or one
 * of its segments has no length) or with a non-finite number.  The four doubles of such lines are untouched and the other lines
 * unaffected; the current values of the line parameters are never read.  windows[i].parameters: the lines in place (slslam_gc
 * av_to_orth of the chosen line); the camera part is read and never written.  results (may be NULL; results[i] may be NULL):
 * windows[i].num_lines records.  lines_av (may be NULL; lines_av[i] may be NULL): [6 num_lines] (closest point, direction) of the chosen
 * line in the world; the six doubles of a line that is not MULTIVIEW / STEREO are untouched.
 * Every argument is validated before an output is written or the device is asked - an index out of range, a negative count, a missing
 * array of a non-zero count, a method outside {0, 1}, a NaN or negative min_parallax, an inverse_depth that is not finite or <= 0:
 * SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched.  More than 630 cameras in a window: SLSLAM_ERR_UNSUPPORTED.  Synchronous; host
 * pointers; one upload, one launch, one download per call. */
int  slslam_line_triangulator_run(slslam_line_triangulator* triangulator, int n, const slslam_lba_window* windows, int method,
                                  double inverse_depth, double min_parallax, slslam_triangulated_line* const* results,
                                  double* const* lines_av);
/* Since create: runs, device / page-locked buffer allocations.  Either pointer may be NULL. */
int  slslam_line_triangulator_stats(const slslam_line_triangulator* triangulator, long long* calls, long long* allocations);
/* Host wall-clock milliseconds of the last successful run, ms[5]: validation + layout + upload image, upload, kernel, download, scatter
 * of the results (tools/lba_triangulate_bench.py). */
int  slslam_line_triangulator_timing(const slslam_line_triangulator* triangulator, double* ms);
/* One window, one call (its own buffers, made and freed). */
int  slslam_lba_triangulate_lines(const slslam_lba_window* window, const slslam_solver_options* opt, int method, double inverse_depth,
                                  double min_parallax, slslam_triangulated_line* results, double* lines_av);
/* Test hook: ONE line through the same header functions on the host, in the kernel's order.  observations[8 n] in the caller's order,
 * cameras[6 n]: the (w, t) of each observation's camera.  line_av[6] (written unless *status is SLSLAM_TRI_INVALID), eigenvalues[4],
 * *status, *num_planes, *clamped as the device reports them; *offdiagonal: the off-diagonal norm the Jacobi sweeps left (method 1).
 * Any output may be NULL.  Needs no device. */
int  slslam_debug_triangulate_host(int num_observations, const double* observations, const double* cameras, double baseline, int method,
                                   double inverse_depth, double min_parallax, double* line_av, double* eigenvalues, int* status,
                                   int* num_planes, int* clamped, double* offdiagonal);

/* ------------------------------------------------------------------ place recognition: which old keyframe does this frame look like
 * The first link of the loop-closure chain (csrc/place_recognition.h, host/place_filter.h), after the reference's
 * src/voctree_bf.h: a K-ary vocabulary tree of L levels over descriptors of D floats, tf-idf scores against the documents of the visible
 * keyframes, and a Bayes filter over "which keyframe am I at, or none".  A reported document feeds slslam_descriptor_matcher_run.
 *   tree      (K^L - 1) / (K - 1) interior nodes of K x D floats, breadth-first, child j of node i at i K + j + 1, raw floats without a
 *             header: what voctree_t::load reads.  K^L leaves; leaf index = node index - interior nodes.
 *   word      of a descriptor f (find_leaf): from the root, L times, go to the child c of the smallest distance
 *             r = 1.0f; for i in 0 .. D-1: r -= c[i] * f[i]  - float, in this order, product and difference rounded separately -, the
 *             first minimum under a strict < : ties go to the lowest child.  The word of every finite descriptor is the reference's.
 *   document  of a frame of n descriptors: its distinct words, ascending, each with tf = (float)count / (float)n.
 *   database  documents in insertion order.  A document becomes visible once more than `recent` documents have been inserted after it
 *             (the reference's doc_buffer: the front is released while more than `recent` documents are pending behind it): after
 *             recent + 1 inserts none is visible, after recent + 2 the first.  Visible documents are numbered 0, 1, ... in insertion
 *             order.  df[word] = visible documents that contain the word.
 *   virtual   document (the reference's document -1, "no place"): exists exactly when more than num_avg_words words have df > 0; it is
 *             the num_avg_words words of the largest df, the lower word on ties, each with tf = 1.0f / num_avg_words; while it exists
 *             it counts as one document in doc_size and in the df of its words.  doc_size = visible documents + (virtual ? 1 : 0).
 *   states    of a query: -1 (index 0 of every per-state array; scored only while the virtual document exists), then the visible
 *             documents d at index d + 1.
 *   score     of a scored state = the float sum, over the words common to the query and the state's document in ascending word
 *             order, of l = -((|n - m| - n) - m) with n = tf_query * idf, m = tf_document * idf, idf = (float)log10((double)doc_size /
 *             (double)df[word]) (libm on the host, uploaded): all float, every operation rounded separately.  touched = the state has
 *             a common word.  An untouched scored state gets score = (float)(sum / (1 + touched states)), sum = the double sum of
 *             every l: per state in ascending word order, then over the states in ascending order.
 *   likelihood over the scored states after the fill: mean and sigma = sqrt(E[s^2] - mean^2) in double; (float)((s - 2 sigma) / mean)
 *             where s > mean + 2 sigma, else 1; all 1 when mean == 0.  An unscored state -1: score 0, touched 0, likelihood 1.
 * Departures from voctree_bf.h, which the reference never compiled in: its `n *= log10(...)` inside the per-document loop compounds
 * the idf once per document of a word - here the idf is applied once; a document's weight is count / n, not count float additions of
 * 1 / n; the L1 term is evaluated in float as written above; its fill loop `for (i = -1; i < doc_size - 1; ...)` assumes the virtual
 * document always exists - here the scored states are exactly the ones listed; a frame without descriptors is not inserted. */
enum { SLSLAM_PLACE_MAX_K = 64, SLSLAM_PLACE_MAX_L = 4, SLSLAM_PLACE_MAX_D = 128, SLSLAM_PLACE_MAX_WORDS = 512, SLSLAM_PLACE_MAX_TOP_K = 32 };
typedef struct slslam_voctree slslam_voctree;
typedef struct slslam_place_db slslam_place_db;
typedef struct slslam_place_filter slslam_place_filter;
/* device < 0 selects the current HIP device.  2 <= K <= 64, 1 <= L <= 4, 1 <= D <= 128, K^L <= 2^24; nodes: the interior nodes as
 * above (copied).  Touches no device: the nodes are uploaded at the first insert or run of a database. */
int  slslam_voctree_create(int device, int K, int L, int D, const float* nodes, slslam_voctree** out);
/* The same from a file of exactly that many floats; a file that cannot be read, is shorter or is longer (it was made for another K, L
 * or D): SLSLAM_ERR_INVALID_ARGUMENT, *out untouched. */
int  slslam_voctree_load(const char* path, int device, int K, int L, int D, slslam_voctree** out);
void slslam_voctree_destroy(slslam_voctree* tree);   /* after the databases that use it */

typedef struct slslam_place_frame {
  int num_descriptors;           /* n >= 0, at most the database's max_words */
  const float* descriptors;      /* [n D] row-major */
} slslam_place_frame;
enum { SLSLAM_PLACE_OK = 0, SLSLAM_PLACE_EMPTY = 1, SLSLAM_PLACE_INVALID_DESCRIPTOR = 2 };
typedef struct slslam_place_result {
  int    status;                 /* SLSLAM_PLACE_*: INVALID_DESCRIPTOR when one of the n D floats is not finite (words all -1), else EMPTY */
                                 /* when n = 0 or no document is visible; unless OK: score 0, touched 0, likelihood 1, top_id -1    */
  int    num_states;             /* visible documents + 1: the length of the per-state arrays                                      */
  int    has_virtual;            /* state -1 was scored                                                                            */
  int*   words;                  /* in: caller-owned arrays, any of them may be NULL; out: as above.  [n]                          */
  float* score;                  /* [num_states] */
  unsigned char* touched;        /* [num_states] */
  float* likelihood;             /* [num_states] */
  int*   top_id;                 /* [top_k] the documents (never state -1) of the largest scores, the lower id on ties; -1 beyond   */
  float* top_score;              /* [top_k] their scores; 0 beyond                                                                  */
} slslam_place_result;

/* 1 <= max_docs (inserted documents, pending ones included), 1 <= max_words <= 512 (descriptors of a frame), 1 <= max_frames (frames of
 * a run: what the blocks are made for), recent >= 0, num_avg_words >= 1.  The tree's device.  Touches no device. */
int  slslam_place_db_create(slslam_voctree* tree, int max_docs, int max_words, int max_frames, int recent, int num_avg_words,
                            slslam_place_db** out);
void slslam_place_db_destroy(slslam_place_db* db);
/* Quantises the frame on the device and appends its document.  *status (may be NULL): SLSLAM_PLACE_OK; EMPTY (n = 0) or
 * INVALID_DESCRIPTOR: the database is unchanged.  words (may be NULL): [n].  SLSLAM_ERR_STATE: max_docs documents are in. */
int  slslam_place_db_insert(slslam_place_db* db, const slslam_place_frame* frame, int* status, int* words);
/* frames[F] (F <= max_frames), out[F], all against the same visible set; 0 <= top_k <= 32.  Every argument is validated before an
 * output is written or the device is asked: SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched, nothing launched.  Synchronous; host
 * pointers; one upload, three launches (documents, scores, likelihoods) and one download per call whatever the number of frames; a
 * frame's bytes do not depend on the other frames of the call. */
int  slslam_place_db_run(slslam_place_db* db, int num_frames, const slslam_place_frame* frames, int top_k, slslam_place_result* out);
/* Documents inserted, visible, and doc_size (visible + the virtual one).  Any pointer may be NULL. */
int  slslam_place_db_size(const slslam_place_db* db, int* inserted, int* visible, int* doc_size);
/* The virtual document's words, ascending: words[num_avg_words] (may be NULL); *num = num_avg_words, or 0 while it does not exist. */
int  slslam_place_db_virtual(const slslam_place_db* db, int* words, int* num);
/* Since create: inserts + runs, and how often the database's blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_place_db_stats(const slslam_place_db* db, long long* calls, long long* allocations);

/* The Bayes filter and the loop decision (host/place_filter.h has the rule): sigma > 0 of the transition's Gaussian, threshold on the
 * posterior mass of seq_len + 1 consecutive documents, no decision while fewer than min_docs documents are visible.  The reference's
 * presets (recent, sigma, threshold, seq_len; min_docs = recent): indoor 40, 1.0, 0.7, 10; outdoor 100, 0.8, 0.8, 15; outdoor
 * long-loop 300, 0.8, 0.5, 5.  Needs no device. */
int  slslam_place_filter_create(double sigma, double threshold, int seq_len, int min_docs, slslam_place_filter** out);
void slslam_place_filter_destroy(slslam_place_filter* filter);
/* One step: likelihood[num_docs + 1] as slslam_place_db_run returns it (state -1 first); the visible set may have grown since the last
 * step.  posterior[num_docs + 1], *loop (0 / 1), *keyframe (the reported document, -1 without a loop): any of them may be NULL. */
int  slslam_place_filter_update(slslam_place_filter* filter, int num_docs, const float* likelihood, float* posterior, int* loop,
                                int* keyframe);

/* ------------------------------------------------------------------ descriptor matching: which feature of a frame is which of a keyframe
 * The link between the place recogniser and the pose estimator in a loop closure (csrc/descriptor_match.h).
 * SLAM::loop_closure (src/slam.cpp:1108-1143) starts from match_result, a map from the current frame's features to the loop keyframe's
 * landmarks, which the commented-out pr.pr_DB_query was to deliver from appearance.  slslam_line_matcher_run scores pairs under a
 * predicted pose; a loop closes because that pose has drifted, so the pairs have to come from the descriptors that made the recogniser
 * fire: the nearest neighbours between the query frame and the reported keyframe, by the recogniser's own distance.
 *   distance    of a query descriptor q and a keyframe descriptor k of D floats each:
 *               r = 1.0f; for i in 0 .. D-1: r -= q[i] * k[i]  - float, in this order, product and difference rounded separately, no
 *               contraction: the chain of `word` above (slslam_place::nearest_child).  The fixed order is why this is not a matrix
 *               product: every decision below is a function of the two frames alone, bit for bit.  r of two equal unit descriptors may
 *               lie a few ulp below zero.
 *   admissible  a pair (a, j) of a query frame of n descriptors and a keyframe of m: r is finite and (double)r < max_distance.
 *   per a       best = the admissible j of the smallest r, the lowest j on ties (-1: none); best_distance = that r, second_distance =
 *               the smallest admissible r over j != best (+inf each when absent); num_admissible = admissible j;
 *   per j       best_query = the admissible a of the smallest r, the lowest a on ties (-1: none);
 *   match[a]    best[a] when best[a] >= 0, best_query[best[a]] == a (mutual) and
 *               (double)best_distance[a] * ratio <= (double)second_distance[a] (unambiguous; ratio <= 1 switches this test off), else -1.
 * Minima and counts only: a pair's results do not depend on the other pairs of the call or on the order of evaluation.
 * The store numbers its keyframes 0, 1, ... in the order of accepted inserts and refuses what slslam_place_db_insert refuses: fed the
 * same frames, a store id is the database's document id. */
enum { SLSLAM_DESC_MAX_D = 128, SLSLAM_DESC_MAX_DESCRIPTORS = 512, SLSLAM_DESC_MAX_CANDIDATES = 8 };
enum { SLSLAM_DESC_OK = 0, SLSLAM_DESC_EMPTY = 1, SLSLAM_DESC_INVALID_DESCRIPTOR = 2 };
typedef struct slslam_descriptor_query {
  int num_descriptors;           /* n >= 0, at most the matcher's max_descriptors */
  const float* descriptors;      /* [n D] row-major */
  int num_candidates;            /* 0 .. the matcher's max_candidates: the frame's pairs, in this order */
  const int* candidates;         /* [num_candidates] store ids, each in [-1, inserted); -1 (what top_id holds beyond the last document) */
                                 /* gives an EMPTY pair                                                                               */
} slslam_descriptor_query;
typedef struct slslam_descriptor_result {
  int    status;                 /* SLSLAM_DESC_*: INVALID_DESCRIPTOR when one of the query's n D floats is not finite, else EMPTY when  */
                                 /* n = 0 or the candidate is -1; unless OK no pair is evaluated and the arrays say "none"              */
  int    num_matched;            /* match[a] >= 0                                                                                        */
  int    num_keyframe_descriptors;   /* m of the candidate (0 for candidate -1): the length of best_query                              */
  int*   match;                  /* in: caller-owned arrays, any of them may be NULL; out: as above.  [n]                                */
  int*   best;                   /* [n] */
  float* best_distance;          /* [n] */
  float* second_distance;        /* [n] */
  int*   num_admissible;         /* [n] */
  int*   best_query;             /* [m]; a caller that does not track m passes max_descriptors entries */
} slslam_descriptor_result;
typedef struct slslam_descriptor_matcher slslam_descriptor_matcher;

/* device < 0 selects the current HIP device.  1 <= D <= 128 and 1 <= max_descriptors <= 512 (descriptors of a frame): the place
 * recogniser's limits; 1 <= max_keyframes: the store's one device block [max_keyframes][max_descriptors][D], made at the first insert;
 * 1 <= max_frames and 1 <= max_candidates <= 8 (candidates of one frame): what the run's one device block and one page-locked block are
 * made for at the first run.  A run of more frames makes larger ones; a run that fits allocates nothing.  Touches no device. */
int  slslam_descriptor_matcher_create(int device, int D, int max_keyframes, int max_descriptors, int max_frames, int max_candidates,
                                      slslam_descriptor_matcher** out);
void slslam_descriptor_matcher_destroy(slslam_descriptor_matcher* matcher);
/* Uploads one keyframe's descriptors [n D].  *status (may be NULL): SLSLAM_DESC_OK; EMPTY (n = 0) or INVALID_DESCRIPTOR (a non-finite
 * float): the store is unchanged.  *id (may be NULL): the keyframe's id, -1 when refused.  n < 0, n > max_descriptors or a missing
 * array: SLSLAM_ERR_INVALID_ARGUMENT; SLSLAM_ERR_STATE: max_keyframes keyframes are in. */
int  slslam_descriptor_matcher_insert(slslam_descriptor_matcher* matcher, int n, const float* descriptors, int* status, int* id);
/* queries[F]; out[num_pairs], frame-major: the pairs of frame 0 in the order of its candidates, then those of frame 1, ...; num_pairs
 * must be the sum of num_candidates.  ratio, max_distance as above (neither may be NaN).  Every argument is validated before an output
 * is written or the device is asked - a negative count, a missing array of a non-zero count, n beyond max_descriptors, more candidates
 * than max_candidates, a candidate outside [-1, inserted), a wrong num_pairs, a NaN: SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched.
 * Synchronous; host pointers; one upload, two launches (per pair, finish) and one download per call whatever F; a frame's descriptors
 * are uploaded once for all its candidates. */
int  slslam_descriptor_matcher_run(slslam_descriptor_matcher* matcher, int num_frames, const slslam_descriptor_query* queries, double ratio,
                                   double max_distance, int num_pairs, slslam_descriptor_result* out);
/* Keyframes inserted.  The pointer may be NULL. */
int  slslam_descriptor_matcher_size(const slslam_descriptor_matcher* matcher, int* inserted);
/* Since create: inserts + runs, and how often the store or the run's blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_descriptor_matcher_stats(const slslam_descriptor_matcher* matcher, long long* calls, long long* allocations);
/* One query frame [n D] against one keyframe [m D], one call (its own buffers, made and freed); n, m <= 512.  The keyframe goes through
 * the store's insert: m = 0 gives EMPTY, a non-finite keyframe float INVALID_DESCRIPTOR, num_keyframe_descriptors 0 either way. */
int  slslam_match_descriptors(int D, int n, const float* query, int m, const float* keyframe, double ratio, double max_distance,
                              slslam_descriptor_result* out);

/* ------------------------------------------------------------------ training a vocabulary tree: hierarchical spherical k-means
 * Makes the nodes slslam_voctree_create takes from the caller's own descriptors (csrc/voctree_train.h, host/voctree_host.h, DESIGN.md
 * 6.5); the reference has no trainer and ships no tree.  The distance is the recogniser's (`word` above, slslam_place::nearest_child),
 * so the training descriptors' words equal find_leaf on the finished tree.  Every sum that decides a centre is an int64 sum of
 * fixed-point values and so independent of its order: nodes, words and counts are a function of the arguments alone, bit for bit.
 *   inputs    n descriptors [n D] float, 1 <= n <= 2^24, every value finite and |f| <= 16; K, L, D within slslam_voctree_create's
 *             limits and K^L D <= 2^27 (the last level's accumulators); 0 <= max_iterations <= 1000; a 64-bit seed.
 *   q(f)      = llrint((double)f * 2^30): round to nearest even, the product is exact.  Sums of q are int64: |sum| <= 2^58.
 *   centre(acc, prev), on the host: s_i = (double)acc_i; n2 = the sum over i ascending of s_i * s_i, each operation rounded on its own;
 *             n2 == 0: the centre stays prev; otherwise c_i = (float)(s_i / sqrt(n2)).
 *   key(m)    = splitmix64(seed ^ splitmix64(m)), splitmix64(x): x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31 - all mod 2^64.
 *   levels    l = 0 .. L-1, one after the other; every descriptor is in exactly one node of its level, all start at the root; all nodes
 *             of a level iterate together.
 *   initial   centres of a node with n members: every centre starts at 0; child j < min(n, K) is centre(q(member), 0) of the member of
 *             the j-th smallest (key, m); children n .. K-1 are copies of child 0 (they never win under the strict <).  A node without
 *             members gets K copies of the centre its parent holds for it.
 *   loop      assign every descriptor to the nearest child of its node; changed = labels that differ from the previous assignment
 *             (the first assignment changes all n).  Stop when max_iterations updates are done, or when at least one is done and
 *             changed == 0.  Otherwise acc[node][child] += q(f), every centre of the level becomes centre(acc, its previous value) - an
 *             empty child keeps its centre - and the loop goes round again.  It always ends on an assignment under the final centres:
 *             those labels are the descriptors' nodes of the next level and, after the last level, their words.
 *   report    per level: iterations = updates done; changed = of the last assignment; empty_children = children (of all K^l nodes)
 *             without a member after the last assignment; distortion = the double mean of the winning r - the one field whose
 *             summation order is free (here: fixed per call shape, so two calls give the same bits).  The *_ms fields are wall-clock
 *             times of the call's phases, for tools/voctree_train_bench.py. */
typedef struct slslam_voctree_train_options {
  int K, L, D;
  int max_iterations;
  unsigned long long seed;
} slslam_voctree_train_options;
typedef struct slslam_voctree_train_report {
  int       levels;                                    /* L */
  int       iterations[SLSLAM_PLACE_MAX_L];
  long long changed[SLSLAM_PLACE_MAX_L];
  long long empty_children[SLSLAM_PLACE_MAX_L];
  double    distortion[SLSLAM_PLACE_MAX_L];
  double    setup_ms[SLSLAM_PLACE_MAX_L];              /* host: partition by node, initial centres; their upload                       */
  double    kernel_ms[SLSLAM_PLACE_MAX_L];             /* every assign-and-accumulate launch of the level, to the arrival of `changed` */
  double    download_ms[SLSLAM_PLACE_MAX_L];           /* the accumulators of every update; labels and counts at the level's end       */
  double    centre_ms[SLSLAM_PLACE_MAX_L];             /* host: centre() over the level's rows, every update                           */
  double    upload_ms[SLSLAM_PLACE_MAX_L];             /* the level's centres, every update                                            */
  double    total_ms;                                  /* the call, validation and the descriptors' upload included                    */
} slslam_voctree_train_report;
/* nodes: [(K^L - 1) / (K - 1)][K][D], breadth-first as slslam_voctree_create takes them; words (may be NULL): [n]; report (may be
 * NULL).  Shape errors (NULL options / descriptors / nodes, n, K, L, D, max_iterations outside the limits above) return
 * SLSLAM_ERR_INVALID_ARGUMENT before any device call, value errors (a non-finite value, |f| > 16) the same status; a failed
 * allocation, on the host or on the device, returns SLSLAM_ERR_NO_MEMORY.  On every error no output is written.  Synchronous; host
 * pointers; the descriptors are uploaded once and stay on the device for the call.  device < 0 selects the current HIP device. */
int  slslam_voctree_train(int device, const slslam_voctree_train_options* options, long long n, const float* descriptors, float* nodes,
                          int* words, slslam_voctree_train_report* report);
/* Writes the file slslam_voctree_load reads (raw floats, no header).  Needs no device.  A shape outside slslam_voctree_create's limits
 * or a file that cannot be written: SLSLAM_ERR_INVALID_ARGUMENT. */
int  slslam_voctree_save(const char* path, int K, int L, int D, const float* nodes);
/* The host half of the trainer, exported so that it can be pinned without a device: centre(acc, prev) of `rows` rows of D values
 * (out may be prev), and key(m). */
int  slslam_voctree_centres(long long rows, int D, const long long* acc, const float* prev, float* out);
unsigned long long slslam_voctree_key(unsigned long long seed, unsigned long long m);
/* Test hook: ONE assignment plus accumulation through the kernel slslam_voctree_train uses, after the same partition by node, for an
 * arbitrary unsorted node[n] (0 <= node < num_nodes): centres [num_nodes][K][D]; label [n], acc [num_nodes K][D] and count
 * [num_nodes K] come back.  Inputs as for slslam_voctree_train, and num_nodes K D <= 2^27. */
int  slslam_debug_voctree_step(int device, int K, int D, long long num_nodes, const float* centres, long long n, const float* descriptors,
                               const int* node, int* label, long long* acc, long long* count);

/* ------------------------------------------------------------------ line descriptors from images: MSLD
 * What makes the [n, D] float descriptors that slslam_place_db_*, slslam_voctree_train and slslam_descriptor_matcher_* take, from grey
 * images and line segments (csrc/line_descriptor.h).  The reference assumes an external tracker for them
 * (src/voctree_bf.h: DESC_DIM 72) and ships none; 72 floats are the shape of MSLD, the mean - standard-deviation line descriptor of Wang,
 * Wu and Hu (Pattern Recognition 42, 2009): 9 bands x 4 gradient components x (mean, standard deviation).
 *   inputs     per frame an 8-bit grey image[height][stride], row-major, stride >= width, 1 <= width, height <= 8192, and segments[n][4]
 *              floats (x0, y0, x1, y1) in pixels; pixel centres lie at integers.
 *   options    bands M in 1 .. 16 (default 9), band_width w in 1 .. 9 (default 5), M w <= 144, orient 0 / 1 (default 1); D = 8 M.
 * Per segment, in real numbers (the device's precisions: DESIGN.md 6.7; tests/line_descriptor_reference.py restates this in fp64):
 *   geometry   L = |p1 - p0|, evaluated as sqrt(dx dx + dy dy) in double; d_L = (p1 - p0) / L, d_perp = (-d_L.y, d_L.x).  N = floor(L)
 *              samples along the line, centred on the segment: s_j = L / 2 + j - (N - 1) / 2, j = 0 .. N-1 - centring makes the
 *              descriptor independent of the order of the end points.
 *   rows       M w support rows at signed offsets rho_r = r - (M w - 1) / 2; the sample point of row r is q = p0 + s_j d_L + rho_r d_perp.
 *   gradient   at integer pixels by central differences with coordinates clamped to the image (replicated border):
 *              gx(x, y) = (I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y)) / 2, gy likewise; at q by bilinear interpolation of gx and gy
 *              from the four surrounding integer pixels, each clamped the same way.
 *   components g_L = g . d_L, g_perp = g . d_perp; (max(g_perp, 0), max(-g_perp, 0), max(g_L, 0), max(-g_L, 0)).
 *   weights    a fixed table of M w x 2 numbers, computed in double and rounded to float: with f_r = exp(-rho_r^2 / (2 sigma^2)),
 *              sigma = (M w - 1) / 2 (1 when M w = 1), t_r = (r + 0.5) / w - 0.5, i0 = floor(t_r), a = t_r - i0, row r adds f_r (1 - a)
 *              times its components to band i0 and f_r a times them to band i0 + 1; a band outside 0 .. M-1 is dropped.
 *   statistics v[j][i][c] = the weighted sum over the rows for sample j, band i, component c; mu[i][c] its mean over j, s[i][c] its
 *              population standard deviation over j (never negative).
 *   polarity   = the sum over j and r of f_r g_perp.  With orient = 1 and polarity < 0 the descriptor is that of the segment with its end
 *              points swapped - g_L and g_perp negated, the rows in reverse order - and -polarity is reported; polarity == 0 does not
 *              flip.  The rows are symmetric about 0, so with orient = 1 swapping the end points of a segment changes nothing.
 *   layout     the 4 M means are scaled to unit L2 norm, the 4 M standard deviations likewise, a half of norm 0 stays 0, both are
 *              multiplied by 1 / sqrt 2: out[4 i + c] = mean part, out[4 M + 4 i + c] = std part.  A descriptor of two non-zero halves
 *              has unit norm, which is what the recogniser's distance 1 - c . f assumes.
 *   status     SLSLAM_MSLD_INVALID: a coordinate is not finite; else OUTSIDE: an end point lies outside [0, W-1] x [0, H-1] (support
 *              rows that stick out of the image are fine: that is what the clamp is for); else TOO_SHORT: L < 2; else FLAT: both
 *              halves have norm 0; else OK (one zero half is OK).  Unless OK the descriptor is all zeros; num_samples is N for OK and
 *              FLAT and 0 otherwise, polarity 0 for a refused segment.
 * Frames are independent: a frame's results do not depend on the rest of the call. */
enum { SLSLAM_MSLD_MAX_BANDS = 16, SLSLAM_MSLD_MAX_BAND_WIDTH = 9, SLSLAM_MSLD_MAX_ROWS = 144, SLSLAM_MSLD_MAX_SIDE = 8192 };
enum { SLSLAM_MSLD_OK = 0, SLSLAM_MSLD_FLAT = 1, SLSLAM_MSLD_TOO_SHORT = 2, SLSLAM_MSLD_OUTSIDE = 3, SLSLAM_MSLD_INVALID = 4 };
typedef struct slslam_msld_options {
  int bands;                     /* M */
  int band_width;                /* w */
  int orient;                    /* 1: flip on a negative polarity */
} slslam_msld_options;
typedef struct slslam_msld_frame {
  int width, height;
  long long stride;              /* bytes from one row to the next, >= width */
  const unsigned char* image;
  int num_segments;              /* n >= 0 */
  const float* segments;         /* [n 4] */
} slslam_msld_frame;
typedef struct slslam_msld_result {
  float* descriptors;            /* caller-owned arrays, any of them may be NULL.  [n D] */
  int*   status;                 /* [n] SLSLAM_MSLD_* */
  int*   num_samples;            /* [n] */
  float* polarity;               /* [n], after a flip */
} slslam_msld_result;
typedef struct slslam_line_descriptor slslam_line_descriptor;

/* bands 9, band_width 5, orient 1 */
void slslam_msld_default_options(slslam_msld_options* opt);
/* device < 0 selects the current HIP device.  options as above, fixed for the handle.  max_frames >= 1 frames of max_pixels >= 1 pixels
 * and max_segments >= 1 segments each: what the one device block and the one page-locked block are made for at the first run.  A larger
 * call makes larger ones and counts one allocation; a call that fits allocates nothing.  max_pixels <= 8192^2, max_frames x max_segments <= 2^24 and max_frames x max_pixels
 * <= 2^32 (what the first run allocates), else SLSLAM_ERR_INVALID_ARGUMENT.  Touches no device. */
int  slslam_line_descriptor_create(int device, const slslam_msld_options* options, int max_frames, long long max_pixels, int max_segments,
                                   slslam_line_descriptor** out);
void slslam_line_descriptor_destroy(slslam_line_descriptor* handle);
/* frames[F], results[F].  Every argument is validated before an output is written or the device is asked - a negative count, a missing
 * array, a size out of range, stride < width: SLSLAM_ERR_INVALID_ARGUMENT; more than 2^24 segments in one call: SLSLAM_ERR_UNSUPPORTED.
 * Synchronous; host pointers; one upload (the images with `width` bytes per row: the stride stays on the host), one launch and one
 * download per call whatever F. */
int  slslam_line_descriptor_run(slslam_line_descriptor* handle, int num_frames, const slslam_msld_frame* frames,
                                const slslam_msld_result* results);
/* Since create: runs, and how often the blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_line_descriptor_stats(const slslam_line_descriptor* handle, long long* calls, long long* allocations);
/* One frame, one call (its own buffers, made and freed). */
int  slslam_describe_lines(const slslam_msld_options* options, const slslam_msld_frame* frame, const slslam_msld_result* result);

/* ------------------------------------------------------------------ line segments from images: the detector
 * What makes the segments[n][4] that slslam_line_descriptor_run takes, from grey images alone (csrc/line_detect.h).  The
 * reference assumes an external tracker for them and ships none, so there is no code to restate: this block is the contract, a function
 * of the image and the options alone whatever order a device visits the pixels in.  It is the region idea of LSD (Grompone von Gioi et
 * al., PAMI 32, 2010) without the sequential region growing: connected components of aligned gradients, each fitted by its moments.
 * tests/line_detect_reference.py restates it in numpy.
 *   inputs     per frame an 8-bit grey image[height][stride], row-major, stride >= width, 1 <= width, height <= 8192; pixel centres lie at
 *              integers; the pixel index of (x, y) is y width + x.
 *   options    grad_threshold T in 1 .. 1024 (default 24); tol_num / tol_den = tan^2 of the angle two linked gradients may differ by, 0 <=
 *              tol_num, 1 <= tol_den, both <= 2^20 (default 11 / 64, about 22.5 degrees); min_pixels >= 1 (12); min_length >= 0 (10.0)
 *              and max_thickness >= 0 (3.0) in pixels, finite; max_segments in 1 .. 2^20 (512), the segments written per frame.
 *   1 gradient in integers, not halved: gx(x, y) = I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y), gy likewise; m2 = gx gx + gy gy.  A pixel
 *              is strong when m2 >= T T; its weight w is the largest integer with w w <= m2, exactly.
 *   2 links    two 8-neighbours a and b are linked when both are strong, dot = ga . gb > 0 and tol_den cross^2 <= tol_num dot^2 with
 *              cross = ga.x gb.y - ga.y gb.x; all in 64-bit integers.
 *   3 components  the connected components of the link graph.  A component's label is the smallest pixel index in it; components are
 *              numbered in ascending label order, which is the order of every output.
 *   4 sums     in 64-bit integers per component, with u = x - xr, v = y - yr the offsets from the label's pixel (xr, yr): n, Sw, Swu, Swv,
 *              Swuu, Swuv, Swvv, Sgx, Sgy.  None can overflow at 8192 x 8192.
 *   5 fit      in double, every operation rounded on its own, in this order: cx = Swu / Sw, cy = Swv / Sw; sxx = Swuu / Sw - cx cx,
 *              syy = Swvv / Sw - cy cy, sxy = Swuv / Sw - cx cy; h = (sxx - syy) / 2, rt = sqrt(h h + sxy sxy), lmin = (sxx + syy) / 2 - rt;
 *              the axis e = (h + rt, sxy) when h >= 0, else (sxy, rt - h), divided by its norm sqrt(ex ex + ey ey) - a norm of 0 is the
 *              status ISOTROPIC; thickness = sqrt(max(lmin, 0)), the RMS distance of the weight from the line.
 *   6 extent   over the component's pixels t = (u - cx) ex + (v - cy) ey; tmin and tmax are exact whatever the order; length = tmax - tmin;
 *              the end point at t is (xr + cx) + t ex, (yr + cy) + t ey.
 *   7 orientation  p0 is the end point at tmin and p1 the one at tmax when ex Sgy - ey Sgx >= 0, else the two are swapped: cross(p1 - p0,
 *              (Sgx, Sgy)) >= 0, the sign of the MSLD polarity above, so orient = 1 there leaves a detected segment as it is.
 *   8 status   SMALL: n < min_pixels (no fit is made); else ISOTROPIC; else SHORT: length < min_length; else THICK: thickness >
 *              max_thickness (how curved chains and blobs leave); else OK.  Only OK components become segments.
 *   9 outputs  per frame, any pointer may be NULL: of the first num_written = min(num_ok, max_segments) OK components in label order
 *              (truncation never reorders) segments (x0, y0, x1, y1) rounded to float, length, thickness and strength = Sw / n in double,
 *              pixels = n and label; num_components, num_ok, num_written, status_counts[5] indexed by SLSLAM_LSD_*; and the label plane
 *              labels[height][width], -1 where a pixel is not strong (for viewers and tests; it is a download of 4 bytes a pixel).
 * Links are pairwise: two lines joined by a smoothly rounded corner are one component and leave as THICK.  No NFA validation, no image
 * pyramid, no smoothing.  Frames are independent: a frame's results do not depend on the rest of the call. */
enum { SLSLAM_LSD_MAX_SIDE = 8192, SLSLAM_LSD_TILE = 32 };     /* TILE: the side of the labelling's tiles, for tests at its borders */
enum { SLSLAM_LSD_OK = 0, SLSLAM_LSD_SMALL = 1, SLSLAM_LSD_ISOTROPIC = 2, SLSLAM_LSD_SHORT = 3, SLSLAM_LSD_THICK = 4 };
typedef struct slslam_line_detect_options {
  int grad_threshold;            /* T, on the scale of the gradient that is not halved */
  int tol_num, tol_den;
  int min_pixels;
  double min_length, max_thickness;
  int max_segments;
} slslam_line_detect_options;
typedef struct slslam_line_detect_frame {
  int width, height;
  long long stride;              /* bytes from one row to the next, >= width */
  const unsigned char* image;
} slslam_line_detect_frame;
typedef struct slslam_line_detect_result {
  float*  segments;              /* caller-owned arrays, any of them may be NULL.  [max_segments 4]: what slslam_msld_frame.segments takes */
  double* length;                /* [max_segments] */
  double* thickness;
  double* strength;
  int*    pixels;
  int*    label;
  int*    num_components;        /* one int each */
  int*    num_ok;
  int*    num_written;
  int*    status_counts;         /* [5] */
  int*    labels;                /* [height width] */
} slslam_line_detect_result;
typedef struct slslam_line_detector slslam_line_detector;

/* grad_threshold 24, tol 11 / 64, min_pixels 12, min_length 10, max_thickness 3, max_segments 512 */
void slslam_line_detect_default_options(slslam_line_detect_options* opt);
/* device < 0 selects the current HIP device.  options as above, fixed for the handle.  max_frames >= 1 frames of max_pixels >= 1 pixels
 * each: what the one device block and the one page-locked block are made for at the first run (about 21 bytes a pixel on the device at
 * the default min_pixels: 128 / min_pixels + 10.  The page-locked block holds no label plane until a call asks for one).  A larger call
 * makes larger ones and counts one allocation; a call that fits allocates nothing.  max_pixels <= 8192^2, max_frames x max_pixels <= 2^30
 * and max_frames x max_segments <= 2^24, else SLSLAM_ERR_INVALID_ARGUMENT.  Touches no device. */
int  slslam_line_detector_create(int device, const slslam_line_detect_options* options, int max_frames, long long max_pixels,
                                 slslam_line_detector** out);
void slslam_line_detector_destroy(slslam_line_detector* handle);
/* frames[F], results[F].  Every argument is validated before an output is written or the device is asked - a negative count, a missing
 * array or image, a size out of range, stride < width: SLSLAM_ERR_INVALID_ARGUMENT; more than 65535 frames, 2^24 segments or 2^32 pixels
 * in one call: SLSLAM_ERR_UNSUPPORTED.  Synchronous; host pointers; one upload (the images with `width` bytes per row: the stride stays on
 * the host), eleven launches and one download per call whatever F. */
int  slslam_line_detector_run(slslam_line_detector* handle, int num_frames, const slslam_line_detect_frame* frames,
                              const slslam_line_detect_result* results);
/* Since create: runs, and how often the blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_line_detector_stats(const slslam_line_detector* handle, long long* calls, long long* allocations);
/* One frame, one call (its own buffers, made and freed). */
int  slslam_detect_lines(const slslam_line_detect_options* options, const slslam_line_detect_frame* frame,
                         const slslam_line_detect_result* result);

/* ------------------------------------------------------------------ stereo line matching: a left and a right segment become one observation
 * What makes the stereo line observation - eight doubles x0 y0 x1 y1 (left) x2 y2 x3 y3 (right), normalised with the left camera's
 * intrinsics: slslam_frame.observations (host/sequence_io.h), the input of slslam_line_matcher_run, slslam_ransac_motion,
 * slslam_pose_estimator_run, the triangulator and the LBA - from the segments and descriptors of a rectified left and right image
 * (csrc/stereo_match.h).
 * Replaces: nothing the reference ships.  It reads its observations from the files of an external tracker (SLAM::grab_new_frame,
 * src/slam.cpp:62-135) and has no code that pairs the two images' segments; this block produces the eight numbers of one line of such
 * a file, after SLAM::insert_curr_obs (src/slam.cpp:121-135).  So there is no code to restate: this block is the contract, a function
 * of the arguments alone; tests/stereo_match_reference.py restates it in numpy.
 *   inputs     per stereo frame n left segments [n 4] float (x0, y0, x1, y1) in pixels of the rectified left image with their descriptors
 *              [n D] float, and m right segments [m 4] with [m D]; n, m <= 512; D a multiple of 8, 8 <= D <= 128.
 *   segment    in double from the float end points, every operation rounded on its own (no contraction), here and below:
 *              lo = min(y0, y1), hi = max(y0, y1), ext = hi - lo (= |y1 - y0|), dx = x1 - x0, dy = y1 - y0, slope = dx / dy;
 *              x(y) = x0 + (y - y0) * slope.  A segment is valid when its four floats and its D descriptor floats are finite.
 *   admissible a pair (left a, right b) when both are valid and all of these hold, in this order:
 *              rows       ext_a >= min_rows and ext_b >= min_rows;
 *              overlap    top = max(lo_a, lo_b), bot = min(hi_a, hi_b), o = bot - top: o >= min_overlap * min(ext_a, ext_b) and o > 0;
 *              direction  dot = dx_a dx_b + dy_a dy_b, cross = dx_a dy_b - dy_a dx_b: cross cross <= max_tan2 * (dot dot) and dot != 0;
 *              disparity  yc = 0.5 * (top + bot), d = x_a(yc) - x_b(yc): min_disparity <= d and d <= max_disparity;
 *              distance   r = 1.0f; for i in 0 .. D-1: r -= left[a][i] * right[b][i] - the float chain of slslam_match_descriptors, in
 *                         that order: r is finite and (double)r < max_distance.
 *   per a      best = the admissible b of the smallest r, the lowest b on ties (-1: none); best_distance, second_distance (+inf each
 *              when absent), num_admissible: as slslam_descriptor_result has them;
 *   per b      best_left = the admissible a of the smallest r, the lowest a on ties (-1: none);
 *   match[a]   best[a] when best[a] >= 0, best_left[best[a]] == a and (double)best_distance[a] * ratio <= (double)second_distance[a]
 *              (ratio <= 1 switches this test off), else -1.
 *   segment_status[a]  INVALID: a is not valid; else FLAT: ext_a < min_rows (the segment lies along the epipolar line and carries no depth:
 *              no pair of it is admissible); else MATCHED: match[a] >= 0; else UNMATCHED.
 *   observations[a]  for MATCHED a only, b = match[a]: (x0, y0, x1, y1) of a, then of b - b's two end points swapped when dot < 0, so
 *              that right end point 0 answers left end point 0 - each value v as v / fx - cx / fx (x) or v / fy - cy / fy (y): the
 *              operation order of SLAM::insert_curr_obs, the left camera's intrinsics for both images.
 *   disparity[a]  for MATCHED a only: x0_a - x_b(y0_a), x1_a - x_b(y1_a), in pixels: the right LINE (from b's end point 0 as given, not
 *              swapped) evaluated at the rows of the left end points; what a caller turns into depth.
 * Frame status: EMPTY when n = 0 or m = 0 (then nothing is admissible), else OK.  Minima, counts and per-row arithmetic only: a
 * frame's results do not depend on the other frames of the call or on the order of evaluation. */
enum { SLSLAM_STEREO_MAX_D = 128, SLSLAM_STEREO_MAX_SEGMENTS = 512 };
enum { SLSLAM_STEREO_OK = 0, SLSLAM_STEREO_EMPTY = 1 };
enum { SLSLAM_STEREO_MATCHED = 0, SLSLAM_STEREO_UNMATCHED = 1, SLSLAM_STEREO_FLAT = 2, SLSLAM_STEREO_INVALID = 3 };
typedef struct slslam_stereo_match_options {
  double min_disparity, max_disparity;   /* px, finite, min <= max                                                          */
  double max_tan2;                       /* squared tangent of the largest direction difference, finite, >= 0               */
  double min_rows;                       /* px, finite, >= 0                                                                */
  double min_overlap;                    /* in [0, 1]: the share of the shorter row extent the common rows must cover       */
  double ratio, max_distance;            /* as slslam_descriptor_matcher_run takes them; neither may be NaN                 */
  double fx, fy, cx, cy;                 /* the left camera; finite, fx and fy not 0                                        */
} slslam_stereo_match_options;
typedef struct slslam_stereo_frame {
  int num_left;                          /* n >= 0, at most the matcher's max_segments */
  const float* left_segments;            /* [n 4] */
  const float* left_descriptors;         /* [n D] row-major */
  int num_right;                         /* m */
  const float* right_segments;           /* [m 4] */
  const float* right_descriptors;        /* [m D] */
} slslam_stereo_frame;
typedef struct slslam_stereo_result {
  int     status;                        /* SLSLAM_STEREO_OK / _EMPTY                                                        */
  int     num_matched;                   /* match[a] >= 0                                                                    */
  int*    match;                         /* caller-owned arrays, any of them may be NULL.  [n]                               */
  int*    best;                          /* [n] */
  float*  best_distance;                 /* [n] */
  float*  second_distance;               /* [n] */
  int*    num_admissible;                /* [n] */
  int*    best_left;                     /* [m] */
  int*    segment_status;                /* [n] SLSLAM_STEREO_MATCHED ... _INVALID */
  double* observations;                  /* [n 8]; only the rows of MATCHED segments are written */
  double* disparity;                     /* [n 2]; likewise */
} slslam_stereo_result;
typedef struct slslam_stereo_matcher slslam_stereo_matcher;

/* disparity 0 .. 128 px, max_tan2 0.03 (about 10 degrees), min_rows 3, min_overlap 0.5, ratio 1.5, max_distance 0.25, fx = fy = 1,
 * cx = cy = 0 (pixels stay pixels) */
void slslam_stereo_match_default_options(slslam_stereo_match_options* opt);
/* device < 0 selects the current HIP device.  D as above, fixed for the handle.  max_frames >= 1 stereo frames of max_segments in
 * 1 .. 512 segments per image: what the one device block and the one page-locked block are made for at the first run.  A run of more
 * frames makes larger ones and counts one allocation; a run that fits allocates nothing.  Touches no device. */
int  slslam_stereo_matcher_create(int device, int D, int max_frames, int max_segments, slslam_stereo_matcher** out);
void slslam_stereo_matcher_destroy(slslam_stereo_matcher* matcher);
/* frames[F], out[F].  Every argument is validated before an output is written or the device is asked - missing or invalid options, a
 * negative count, a count beyond max_segments, a missing array of a non-zero count: SLSLAM_ERR_INVALID_ARGUMENT, outputs untouched.
 * Synchronous; host pointers; one upload, three launches (pairs, finish, emit) and one download per call whatever F. */
int  slslam_stereo_matcher_run(slslam_stereo_matcher* matcher, const slslam_stereo_match_options* options, int num_frames,
                               const slslam_stereo_frame* frames, slslam_stereo_result* out);
/* Since create: runs, and how often the blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_stereo_matcher_stats(const slslam_stereo_matcher* matcher, long long* calls, long long* allocations);
/* For tools/stereo_match_bench.py: enable > 0 brackets the three launches of the handle's following runs with two events on its
 * stream, enable == 0 stops that, enable < 0 leaves the switch as it is; *kernel_ms (may be NULL): the last bracketed run, 0 before one. */
int  slslam_stereo_matcher_timing(slslam_stereo_matcher* matcher, int enable, double* kernel_ms);
/* One stereo frame, one call (its own buffers, made and freed); n, m <= 512. */
int  slslam_match_stereo(int D, const slslam_stereo_match_options* options, const slslam_stereo_frame* frame, slslam_stereo_result* out);

/* ------------------------------------------------------------------ line tracking: which segment of this frame is which feature of the last
 * Gives every segment of every frame a persistent feature id - the `id` in front of the eight numbers of a line of the reference's
 * frame files (SLAM::grab_new_frame, src/slam.cpp:62-108), by which curr_obs, lms.find, the id merge of pose_estimation
 * (slslam_pose_estimation_inputs), the window packer and match_lookup are keyed (csrc/line_track.h).
 * Replaces: nothing the reference ships; its ids come from the files of an external tracker.  So there is no code to restate: this
 * block is the contract; tests/line_track_reference.py restates it in numpy.
 *   inputs     a run is T >= 1 frames in time order, each n_t <= 512 segments [n 4] float (x0, y0, x1, y1) in pixels of the left image
 *              with their descriptors [n D] float, D a multiple of 8, 8 <= D <= 128, and optionally predict[6] = a11 a12 tx a21 a22 ty
 *              (finite): an affine map from the previous frame's pixel coordinates to this frame's; NULL: the identity.
 *   state      the handle keeps the carried frame - segments, descriptors, validity, ids and ages of the last frame of the run before -
 *              and next_id.  After create: no carried segments, next_id = 0; _reset empties the former and sets the latter.
 *   problem t  rows: the segments of frame t; columns: those of frame t - 1, for frame 0 the carried frame.
 *   segment    in double from the float end points, every operation rounded on its own (no contraction), here and below; no division:
 *              dx = x1 - x0, dy = y1 - y0, len2 = dx dx + dy dy, m = (0.5 (x0 + x1), 0.5 (y0 + y1)).  A segment is valid when its four
 *              floats and its D descriptor floats are finite; a carried segment that got no id counts as not valid.  It is short when
 *              len2 < min_length^2, of the segment as it lies in its own frame.
 *   warp       the end points of a column b go through predict first: x' = (a11 x + a12 y) + tx, y' = (a21 x + a22 y) + ty; all of
 *              b's quantities below are of the warped segment.
 *   admissible a pair (row a, column b) when both are valid, neither is short and all of these hold, in this order:
 *              direction  dot = dx_a dx_b + dy_a dy_b, cross = dx_a dy_b - dy_a dx_b: cross cross <= max_tan2 * (dot dot) and dot != 0;
 *              shift      e = m_a - m_b: e.x e.x + e.y e.y <= max_shift^2;
 *              offset     e_ab = (m_a.x - x0_b) dy_b - (m_a.y - y0_b) dx_b: e_ab e_ab <= max_offset^2 * len2_b; and the same with a and
 *                         b exchanged (each midpoint lies near the other's line);
 *              overlap    s0 = (x0_b - x0_a) dx_a + (y0_b - y0_a) dy_a, s1 likewise of b's other end; lo = min(s0, s1),
 *                         hi = max(s0, s1), o = min(hi, len2_a) - max(lo, 0): o >= min_overlap * min(len2_a, hi - lo) and o > 0;
 *              distance   r = 1.0f; for i in 0 .. D-1: r -= row[i] * col[i] - the float chain of slslam_match_descriptors, in that
 *                         order: r is finite and (double)r < max_distance.
 *   per a / b  best, best_distance, second_distance, num_admissible [n_t], best_row [the columns] and match [n_t] - mutual, then the
 *              ratio test - exactly as the stereo block above defines best .. match (best_row as its best_left): the lowest index on
 *              ties, ratio <= 1 switches the test off.  match[a] is an index into the frame before.
 *   segment_status[a]  INVALID: a is not valid; else SHORT; else CONTINUED: match[a] >= 0; else NEW.
 *   id, age    INVALID, SHORT: -1, 0.  CONTINUED: the id of prev[match[a]], its age + 1.  NEW: age 1 and
 *              id = next_id + the NEW segments of frames 0 .. t-1 of this run + the NEW segments a' < a of frame t:
 *              fresh ids ascend in (frame, row) order.
 *   after      next_id grows by the run's NEW segments; the run's last frame becomes the carried frame (a frame with n = 0 ends every
 *              track: a track does not survive a frame its segment is missing from).
 * Frame status: EMPTY when n = 0 or there are no columns, else OK.  The outputs are a function of the frames and the handle's state
 * alone: T frames in one run give the same bytes as one frame per run, and as any other cut.  Minima, counts and per-row arithmetic
 * only. */
enum { SLSLAM_TRACK_MAX_D = 128, SLSLAM_TRACK_MAX_SEGMENTS = 512 };
enum { SLSLAM_TRACK_OK = 0, SLSLAM_TRACK_EMPTY = 1 };
enum { SLSLAM_TRACK_CONTINUED = 0, SLSLAM_TRACK_NEW = 1, SLSLAM_TRACK_SHORT = 2, SLSLAM_TRACK_INVALID = 3 };
typedef struct slslam_line_track_options {
  double max_tan2;                       /* squared tangent of the largest direction difference, finite, >= 0                 */
  double max_shift;                      /* px between the midpoints, finite, >= 0                                            */
  double max_offset;                     /* px of a midpoint from the other segment's line, finite, >= 0                      */
  double min_overlap;                    /* in [0, 1]: the share of the shorter extent along a the common part must cover     */
  double min_length;                     /* px, finite, >= 0                                                                  */
  double ratio, max_distance;            /* as slslam_descriptor_matcher_run takes them; neither may be NaN                   */
} slslam_line_track_options;
typedef struct slslam_line_track_frame {
  int num_segments;                      /* n >= 0, at most the tracker's max_segments */
  const float* segments;                 /* [n 4] */
  const float* descriptors;              /* [n D] row-major */
  const double* predict;                 /* [6] or NULL */
} slslam_line_track_frame;
typedef struct slslam_line_track_result {
  int     status;                        /* SLSLAM_TRACK_OK / _EMPTY                                                          */
  int     num_continued, num_new;
  int*    id;                            /* caller-owned arrays, any of them may be NULL.  [n]                                */
  int*    age;                           /* [n] */
  int*    segment_status;                /* [n] SLSLAM_TRACK_CONTINUED ... _INVALID */
  int*    match;                         /* [n] */
  int*    best;                          /* [n] */
  float*  best_distance;                 /* [n] */
  float*  second_distance;               /* [n] */
  int*    num_admissible;                /* [n] */
  int*    best_row;                      /* [the segments of the frame before; for frame 0 the carried segments] */
} slslam_line_track_result;
typedef struct slslam_line_tracker slslam_line_tracker;

/* max_tan2 0.03, max_shift 40 px, max_offset 12 px, min_overlap 0.5, min_length 8 px, ratio 1.5, max_distance 0.25 */
void slslam_line_track_default_options(slslam_line_track_options* opt);
/* device < 0 selects the current HIP device.  D as above, fixed for the handle.  max_frames >= 1 frames of max_segments in 1 .. 512
 * segments: what the one device block and the one page-locked block are made for at the first run, with the carried frame's block.
 * A run of more frames makes larger ones and counts one allocation; a run that fits allocates nothing.  Touches no device. */
int  slslam_line_tracker_create(int device, int D, int max_frames, int max_segments, slslam_line_tracker** out);
void slslam_line_tracker_destroy(slslam_line_tracker* tracker);
/* frames[T], out[T].  Every argument is validated before an output is written, the device is asked or the state changes - missing or
 * invalid options, a negative count, a count beyond max_segments, a missing array of a non-zero count, a predict that is not finite,
 * next_id + the run's segments beyond INT_MAX: SLSLAM_ERR_INVALID_ARGUMENT, outputs and state untouched.  T = 0 changes nothing
 * and is not counted as a run.
 * Synchronous; host pointers; one upload, seven launches and one download per run whatever T; the carried frame stays on the device. */
int  slslam_line_tracker_run(slslam_line_tracker* tracker, const slslam_line_track_options* options, int num_frames,
                             const slslam_line_track_frame* frames, slslam_line_track_result* out);
/* Empties the carried frame and sets next_id (>= 0). */
int  slslam_line_tracker_reset(slslam_line_tracker* tracker, int next_id);
/* Either pointer may be NULL. */
int  slslam_line_tracker_state(const slslam_line_tracker* tracker, int* next_id, int* carried_segments);
/* Since create: runs, and how often the blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_line_tracker_stats(const slslam_line_tracker* tracker, long long* calls, long long* allocations);
/* For benches: as slslam_stereo_matcher_timing; the events bracket the launches of a run. */
int  slslam_line_tracker_timing(slslam_line_tracker* tracker, int enable, double* kernel_ms);
/* A sequence without a handle: no carried frame, next_id = 0 (its own buffers, made and freed). */
int  slslam_track_lines(int D, const slslam_line_track_options* options, int num_frames, const slslam_line_track_frame* frames,
                        slslam_line_track_result* out);

/* ------------------------------------------------------------------ image rectification: from a rig's raw images to what the detector takes
 * What turns the raw, lens-distorted, not row-aligned grey images of a stereo rig into the rectified - and optionally pre-smoothed -
 * images that slslam_line_detector_run, slslam_line_descriptor_run and the "common rows" gate of slslam_stereo_matcher_run assume
 * (csrc/image_rectify.h).  The reference reads a tracker's files and has no code for any of it - no camera model, no
 * map, no remap, no smoothing, no rig rectification: there is no counterpart to restate for any entry below, so this block is the
 * contract, and tests/image_rectify_reference.py restates it in numpy.  The device is held to it bit for bit.
 *   camera     slslam_rectify_camera (no counterpart in the reference): raw intrinsics fx, fy, cx, cy; Brown-Conrady distortion k1, k2,
 *              p1, p2, k3; R[9] row-major with x_rect = R x_raw; rectified intrinsics fx2, fy2, cx2, cy2; src_width, src_height (the
 *              raw image) and dst_width, dst_height (the output), each in 1 .. SLSLAM_LSD_MAX_SIDE.  Every double finite, the four
 *              focal lengths > 0.  Pixel centres lie at integers.
 *   map        (no counterpart) for the output pixel (u, v), in double, every operation rounded on its own (no fused multiply-add), in
 *              this order:  xr = (u - cx2) / fx2, yr = (v - cy2) / fy2;  (X, Y, Z) = R^T (xr, yr, 1), each component as (a xr + b yr)
 *              + c: X = (R[0] xr + R[3] yr) + R[6], Y = (R[1] xr + R[4] yr) + R[7], Z = (R[2] xr + R[5] yr) + R[8].  Z <= 0 (or NaN), or
 *              a non-finite sx or sy below: the pixel is invalid and has no coordinates.  Else x = X / Z, y = Y / Z, r2 = x x + y y,
 *              rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),  xd = x rad + ((2 p1) x y + p2 (r2 + 2 (x x))),  yd = y rad + (p1 (r2 + 2 (y y)) +
 *              (2 p2) x y), with (2 p1) x y = ((2 p1) x) y;  sx = fx xd + cx, sy = fy yd + cy.
 *   quantise   (no counterpart) qx = floor(sx 256 + 0.5), qy likewise, as 64-bit integers; the pixel is also invalid when (sx, sy) lies
 *              outside [-0.5, src_width - 0.5) x [-0.5, src_height - 0.5).  Stored in 32 bits as min(max(qx, -256), 256 src_width) - no
 *              valid pixel is changed by that, and for an invalid one the remap below reads the same bytes - and as
 *              SLSLAM_RECTIFY_NO_COORD (with sx = sy = NaN) where the pixel has no coordinates.  The map depends on the camera alone:
 *              it is computed on the device once per camera and kept in the handle.
 *   remap      (no counterpart) integers only: ix = qx >> 8, ax = qx & 255 (arithmetic shift, two's complement), the same for y; the
 *              four neighbours p00 = I(ix, iy), p01 = I(ix + 1, iy), p10 = I(ix, iy + 1), p11 = I(ix + 1, iy + 1) with every index
 *              clamped into the source; p = ((256 - ax) (256 - ay) p00 + ax (256 - ay) p01 + (256 - ax) ay p10 + ax ay p11 + 32768) >> 16
 *              (below 2^25).  An invalid pixel gets border_value under SLSLAM_RECTIFY_BORDER_CONSTANT; under _REPLICATE it gets p of
 *              its stored coordinates - the value at the clamped position - or border_value when it has none.
 *   smoothing  (no counterpart) off at smooth_sigma = 0, else 0 < smooth_sigma <= 16, applied to the remapped 8-bit image, so a fused
 *              and an unfused implementation give the same bytes: a separable Gaussian with the integer taps of
 *              slslam_rectify_smooth_taps: radius = min(7, max(1, ceil(3 sigma))), t_i = floor(w_i / sum_w 16384 + 0.5) for i >= 1 with
 *              w_i = exp(-i i / (2 sigma sigma)) and sum_w = 1 + 2 sum w_i, t_0 = 16384 - 2 sum t_i.  The taps are an input of the
 *              contract.  Horizontal: h = (sum t p + 32) >> 6, at most 65280, the value x 256; vertical: (sum t h + 2^21) >> 22; both
 *              within 31 bits, both replicate at the border of the output image.
 *   outputs    per frame the image[dst_height][stride], stride >= dst_width; num_valid and valid[dst_height dst_width] (1 / 0), which
 *              are the camera's (either may be NULL).
 *   rig        slslam_stereo_rectify (no counterpart; host only, double): from both cameras' raw intrinsics and distortion and the
 *              pose of the right camera relative to the left, x_right = R x_left + t, by the construction of Fusiello, Trucco and Verri
 *              (MVA 12, 2000): c = -R^T t, the right centre in the left camera; baseline b = |c| > 0; e1 = c / b; e2 = (-e1.y, e1.x, 0)
 *              / its norm, which is (0, 0, 1) x e1 - a baseline along the optical axis is SLSLAM_ERR_INVALID_ARGUMENT -; e3 = e1 x e2;
 *              the left camera's R = rows e1, e2, e3, the right camera's = that R R^T.  Both views share fx2 = fy2 = ((fx + fy of the
 *              left) + (fx + fy of the right)) / 4 and the left principal point unless has_principal gives (cx2, cy2).  Returns the two
 *              cameras, b, and intrinsics[4] = fx2, fy2, cx2, cy2: the fx, fy, cx, cy of slslam_stereo_match_options.  The right view
 *              lies at +b along the rectified x axis: x_right_pixel = x_left_pixel - fx2 b / depth.
 * No image pyramid, no 16-bit or colour input, no fisheye model; the rectified images return to the host before the detector takes
 * them.  Frames are independent. */
enum { SLSLAM_RECTIFY_BORDER_CONSTANT = 0, SLSLAM_RECTIFY_BORDER_REPLICATE = 1 };
enum { SLSLAM_RECTIFY_SUBPIXEL_BITS = 8, SLSLAM_RECTIFY_MAX_RADIUS = 7,
       SLSLAM_RECTIFY_TILE_WIDTH = 64, SLSLAM_RECTIFY_TILE_HEIGHT = 16,         /* the smoothing kernel's tile, for tests at its borders */
       SLSLAM_RECTIFY_NO_COORD = (-2147483647 - 1) };
typedef struct slslam_rectify_options {
  int border_mode;               /* SLSLAM_RECTIFY_BORDER_* */
  int border_value;              /* 0 .. 255 */
  double smooth_sigma;           /* 0: no smoothing */
} slslam_rectify_options;
typedef struct slslam_rectify_camera {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
  double R[9];
  double fx2, fy2, cx2, cy2;
  int src_width, src_height, dst_width, dst_height;
} slslam_rectify_camera;
typedef struct slslam_rectify_frame {
  int camera;                    /* which of the handle's cameras took it */
  long long stride;              /* bytes from one row to the next, src_width <= stride < 2^31 */
  const unsigned char* image;    /* [src_height][stride] */
} slslam_rectify_frame;
typedef struct slslam_rectify_result {
  unsigned char* image;          /* caller-owned [dst_height][stride]; only the dst_width bytes of a row are written */
  long long stride;              /* >= dst_width */
  unsigned char* valid;          /* [dst_height dst_width] or NULL */
  int* num_valid;                /* one int or NULL */
} slslam_rectify_result;
typedef struct slslam_stereo_rig {
  double left_k[4], left_dist[5];       /* fx fy cx cy; k1 k2 p1 p2 k3 */
  double right_k[4], right_dist[5];
  double R[9], t[3];                    /* x_right = R x_left + t */
  int left_width, left_height, right_width, right_height, dst_width, dst_height;
  int has_principal, reserved;
  double cx2, cy2;                      /* the rectified principal point when has_principal != 0 */
} slslam_stereo_rig;
typedef struct slslam_image_rectifier slslam_image_rectifier;

/* border constant 0, no smoothing */
void slslam_rectify_default_options(slslam_rectify_options* opt);
/* Host only.  sigma in [0, 16]: *radius and taps[8] = t_0 .. t_7 (0 beyond the radius); sigma = 0 gives radius 0 and t_0 = 16384. */
int  slslam_rectify_smooth_taps(double sigma, int* radius, int* taps);
/* Host only: "rig" above.  Outputs are written only on SLSLAM_OK. */
int  slslam_stereo_rectify(const slslam_stereo_rig* rig, slslam_rectify_camera* left, slslam_rectify_camera* right, double* baseline,
                           double* intrinsics);
/* device < 0 selects the current HIP device.  options and the 1 .. 64 cameras are fixed for the handle; the output pixels of all
 * cameras together <= 2^28 (their maps take 25 bytes a pixel on the device, made with the first call that reaches it and not counted
 * in `allocations`).  max_frames >= 1 frames of max_pixels >= 1 pixels each - the larger of source and output -: what the one device
 * block and the one page-locked block are made for at the first run.  A larger call makes larger ones and counts one allocation; a call
 * that fits allocates nothing.  max_pixels <= 8192^2, max_frames x max_pixels <= 2^30.  Touches no device. */
int  slslam_image_rectifier_create(int device, const slslam_rectify_options* options, int num_cameras, const slslam_rectify_camera* cameras,
                                   int max_frames, long long max_pixels, slslam_image_rectifier** out);
void slslam_image_rectifier_destroy(slslam_image_rectifier* handle);
/* frames[F], results[F].  Every argument is validated before an output is written or the device is asked - a negative count, a missing
 * array or image, a camera index out of range, a stride below the width: SLSLAM_ERR_INVALID_ARGUMENT; more than 65535 frames or 2^32
 * bytes in one call: SLSLAM_ERR_UNSUPPORTED.  Synchronous; host pointers; one upload, one launch and one download per call whatever F.
 * num_frames = 0 is a counted call that does nothing. */
int  slslam_image_rectifier_run(slslam_image_rectifier* handle, int num_frames, const slslam_rectify_frame* frames,
                                const slslam_rectify_result* results);
/* The map of one camera as the device computed it, any pointer may be NULL: qx, qy [dst_height dst_width] int32, valid bytes, and
 * the doubles sx, sy (NaN where a pixel has no coordinates). */
int  slslam_image_rectifier_get_map(slslam_image_rectifier* handle, int camera, int* qx, int* qy, unsigned char* valid, double* sx,
                                    double* sy);
/* Since create: runs, and how often the blocks were made or made larger.  Either pointer may be NULL. */
int  slslam_image_rectifier_stats(const slslam_image_rectifier* handle, long long* calls, long long* allocations);
/* Any number of frames, one call (its own handle, maps and buffers, made and freed). */
int  slslam_rectify_images(const slslam_rectify_options* options, int num_cameras, const slslam_rectify_camera* cameras, int num_frames,
                           const slslam_rectify_frame* frames, const slslam_rectify_result* results);

/* ------------------------------------------------------------------ diagnostics (benches, timing experiments)
 * Not part of the reference's surface: the reference times its back-end with StopWatch accumulators around whole calls
 * (src/stopwatch.h:42-157, proc_2 / proc_3 at src/slam.cpp:1384-1386, :1237,1312); these give the device-side split. */
/* Per-thread switch: slslam_po_solve brackets its device work and every factorisation (+ triangular solve) with HIP events. */
int slslam_po_set_profiling(int enable);
/* Timing of the calling thread's last profiled slslam_po_solve: device time of the whole solve, of its slowest factorisation
 * (iterations enqueued after the solve has converged are no-ops), how many factorisations were enqueued, unknowns of the reduced program and of the junction block (0 with the dense factorisations). */
int slslam_po_last_timing(double* total_ms, double* factor_ms, int* factor_calls, int* unknowns, int* junction_unknowns);
/* For tools/line_descriptor_bench.py (the kernel alone, beside the call's wall time): enable > 0 brackets the launch of the handle's
 * following runs with two events on its stream, enable == 0 stops that, enable < 0 leaves the switch as it is; *kernel_ms (may be NULL):
 * the last bracketed launch, 0 before one. */
int slslam_line_descriptor_timing(slslam_line_descriptor* handle, int enable, double* kernel_ms);
/* The same for the line detector (tools/line_detect_bench.py): the events bracket the eleven launches of a run. */
int slslam_line_detector_timing(slslam_line_detector* handle, int enable, double* kernel_ms);
/* The same for the image rectifier (tools/image_rectify_bench.py): the events bracket the one launch of a run. */
int slslam_image_rectifier_timing(slslam_image_rectifier* handle, int enable, double* kernel_ms);
/* Timing builds only (a variant library compiled with -DSLSLAM_K1_TIMING=1, -DSLSLAM_K1_WALL=1 or -DSLSLAM_SOLVE_TIMING=1: the elimination
 * sweeps / the reduced solve and k_big_solve): wave-clock cycles per phase summed over the batch since finalize; out[16].  The product
 * library has no stamps and no stamp buffer: SLSLAM_ERR_STATE there, from this call and the next. */
int slslam_debug_phase_cycles(slslam_lba_batch* batch, double* out);
/* The same buffer raw (-DSLSLAM_K1_TIMING=1 / -DSLSLAM_K1_WALL=1: 32 words per chunk - the elimination sweep's phase cycles and, in words
 * 30 / 31, the constant-clock (s_memrealtime, 100 MHz) times at which the chunk's wave started and ended its last sweep: what
 * tools/chunk_timeline.py reads).  Copies min(n, size) words; *size = words the buffer holds. */
int slslam_debug_read_cycles(slslam_lba_batch* batch, unsigned long long* out, long long n, long long* size);

/* Test hook of the device build (csrc/lba_device_build.h): ONE window through k_ingest / k_build_window / k_build_layout / k_build_tiles
 * alone; everything the host packer emits for the window comes back (counts: Cf, tiles, items, free parameters, kept residual blocks;
 * tiles: line_begin, nlines, flags, nitems per tile) so that tests compare the two byte for byte.  *status: 0 built, else the reason
 * bits (1 bad input, 2 a shape for the host path). */
int slslam_debug_device_pack(const slslam_lba_window* window, int grouping, int* counts, int* line_order, int* line_ptr, int* ob_orig,
                             int* ob_cam, int* tiles, unsigned char* items, int* cam_cf, int max_tiles, int max_items,
                             unsigned short* lane_map, unsigned* line_desc, int* status);
/* ... with the shader-clock stamps of k_build_window's phases (tools/build_phases.py): phase_clocks[0 .. 9], or NULL. */
int slslam_debug_device_pack_timed(const slslam_lba_window* window, int grouping, int* counts, int* line_order, int* line_ptr, int* ob_orig,
                                   int* ob_cam, int* tiles, unsigned char* items, int* cam_cf, int max_tiles, int max_items,
                                   unsigned short* lane_map, unsigned* line_desc, int* status, unsigned long long* phase_clocks);

/* ------------------------------------------------------------------ misc */
int         slslam_device_count(void);          /* 0 when no HIP device is usable */
/* The one-shot entry points (slslam_lba_solve, slslam_po_solve) keep the device block of their last call per host thread
 * and reuse it when it is large enough (allocation costs as much as a small solve).  Frees the calling thread's block. */
void        slslam_release_cached_memory(void);
const char* slslam_version(void);
const char* slslam_status_string(int status);

#ifdef __cplusplus
}
#endif
#endif /* SLSLAM_HIP_H_ */

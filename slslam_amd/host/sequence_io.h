// slslam_amd/host/sequence_io.h — the data formats on either side of the hot path,
// restated on plain arrays for callers that replay sequences:
//   tracked-line frame reader   SLAM::grab_new_frame + SLAM::insert_curr_obs   reference src/slam.cpp:62-135
//   tracked-line frame writer   the file that reader takes, from the line tracker's ids and the stereo matcher's pixels
//   metric embedding            SLAM::metric_embedding                          reference src/slam.cpp:1317-1366
//   trajectory writer           SLAM::save_trajectory                           reference src/slam.cpp:1470-1496
//   landmark writer             SLAM::save_landmark                             reference src/slam.cpp:1431-1468
// Host-only; no GPU content.  Exported from libslslam_host.so.
#ifndef SLSLAM_SEQUENCE_IO_H_
#define SLSLAM_SEQUENCE_IO_H_

#include <stddef.h>

#include "gc_lite.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slslam_intrinsics { double fx, fy, cx, cy; } slslam_intrinsics;   /* fx1 fy1 cx1 cy1, src/parameter.h:48-52 */

/* One frame of tracked stereo lines, as curr_obs holds it after grab_new_frame: ascending feature id,
 * first occurrence of an id wins (std::map::insert), endpoints normalised x/f - c/f with the LEFT
 * camera's intrinsics for all eight values (src/slam.cpp:121-128). */
typedef struct slslam_frame {
  int     num_lines;
  int*    ids;            /* [n] feature ids (after the optional alias remap, src/slam.cpp:130-132) */
  double* observations;   /* [8 n] x0 y0 x1 y1 (left) x2 y2 x3 y3 (right), normalised */
} slslam_frame;

/* Text format: one line per feature, "id x0 y0 x1 y1 x2 y2 x3 y3 [ignored]" separated by blanks, lines
 * shorter than 256 characters (the reference reads with getline(line, 256): a longer line ends the read).
 * alias_from / alias_to (n_alias entries, may be NULL): match_lookup, feature id -> canonical id.
 * Returns 0, or 1 when the file cannot be opened (the reference returns false). */
int  slslam_read_frame_file(const char* path, const slslam_intrinsics* K, const int* alias_from, const int* alias_to,
                            int n_alias, slslam_frame* out);
int  slslam_parse_frame_text(const char* text, size_t len, const slslam_intrinsics* K, const int* alias_from,
                             const int* alias_to, int n_alias, slslam_frame* out);
/* obs_dir/%04d.txt (src/slam.cpp:73) */
int  slslam_frame_path(const char* obs_dir, int frame_id, char* buf, size_t cap);
void slslam_free_frame(slslam_frame* f);

/* The writer of such a file: line i = "ids[i] x0 y0 x1 y1 x2 y2 x3 y3\n", blanks between.  observations_px [8 n]: PIXELS - the
 * stereo matcher's observations made with fx = fy = 1, cx = cy = 0 (slslam_stereo_matcher_run), which are float values; ids: the line
 * tracker's (slslam_line_tracker_run) of the same rows.  A value is written as %.9g where the reader's atof gives it back exactly,
 * else as %.17g: nine digits name a float among floats, but the reader takes the text as a double, and only the exact double makes
 * its normalisation under K the matcher's under K, bit for bit.  A line is at most 11 + 8 * 25 = 211 characters, below the reader's
 * 255.  slslam_format_frame_text writes up to cap - 1 characters and a 0 into buf (may be NULL with cap 0) and returns the length the
 * whole text has, as snprintf does, or -1 for a missing array; slslam_write_frame_file returns 0, 1 when the file cannot be written,
 * 2 for a missing argument. */
long slslam_format_frame_text(int n, const int* ids, const double* observations_px, char* buf, size_t cap);
int  slslam_write_frame_file(const char* path, int n, const int* ids, const double* observations_px);

/* Pose-graph edge as edges[(from, to)].T: the pose of keyframe `to` relative to keyframe `from`. */
typedef struct slslam_me_edge { int from, to; slslam_pose T; } slslam_me_edge;

/* metric_embedding(id, mes): re-roots every keyframe pose at keyframe `root` by walking the keyframe graph in
 * order of accumulated edge length (multimap<double,int>, ties in insertion order), kfs[end]->T =
 * gc_T_20(edge(start,end).T, kfs[start]->T); a missing edge is the identity (std::map::operator[]).
 * kf_ids[n] ascending; neighbours of keyframe i are nbr[nbr_ptr[i] .. nbr_ptr[i+1]) (ids, ascending as set<int>).
 * Outputs: T[n] (poses of the keyframes that were reached; others untouched), order_ids / order_dist
 * [*n_embedded] = the mes multimap in order.  Returns 0, or 1 if root is not a keyframe. */
int slslam_metric_embedding(int root, int n, const int* kf_ids, const int* nbr_ptr, const int* nbr,
                            const slslam_me_edge* edges, int num_edges, slslam_pose* T, int* order_ids,
                            double* order_dist, int* n_embedded);

/* save_trajectory: line i = "i \t z \t -x \t -y \t w0 \t w1 \t w2" of gc_T_inv(kfs[i]->T) (camera position in the
 * root frame, axes permuted, rotation as angle-axis), operator<< formatting (6 significant digits).
 * T[n] = keyframe poses in ascending keyframe id (after metric_embedding(0)). */
int slslam_format_trajectory_line(int index, const slslam_pose* T_kf, char* buf, size_t cap);
int slslam_write_trajectory(const char* path, const slslam_pose* T, int n);

/* save_landmark: the two 3-D endpoints of every landmark in the root frame: the point of the line closest to the
 * origin of its initial keyframe, moved tt[0] / tt[1] along the unit direction, taken to the world with the
 * initial keyframe's pose; line i = "z1 \t -y1 \t x1 \t z2 \t -y2 \t x2".
 * lines[6 n] = (point, direction) in the initial keyframe's frame, tt[2 n], T_init[n].
 * Where tt comes from: SLAM::extend_end_points in the reference; here slslam_lba_batch_segments / slslam_lba_segments
 * (include/slslam_hip.h) give t_min, t_max of every line of a solved window - along the line's unit direction from its point closest
 * to the WINDOW's origin, and the end points p_min, p_max in the window's frame: a caller whose landmark lives in its initial
 * keyframe's frame moves the two end points there (or re-bases t by the shift of the closest point) before this call. */
int slslam_landmark_endpoints(const double line[6], const double tt[2], const slslam_pose* T_init, double endpoints[6]);
int slslam_write_landmarks(const char* path, const double* lines, const double* tt, const slslam_pose* T_init, int n);

#ifdef __cplusplus
}
#endif
#endif

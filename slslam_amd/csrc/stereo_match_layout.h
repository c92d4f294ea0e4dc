// slslam_amd/csrc/stereo_match_layout.h — the host half of the stereo line matcher (include/slslam_hip.h: slslam_stereo_matcher_*): the
// limits, the validation of options and frames, what the contract derives per segment and per pair (the geometric gate and the emitted
// row: the same functions run in the kernels of stereo_match.h and, on the host, in tests/host_cxx/stereo_match_layout_check.cpp), and
// where everything of a call lies in its one block.  Plain C++ with no HIP in it, so that the check program runs it on the host under
// the sanitizers.  Internal: not part of the C ABI.
#ifndef SLSLAM_STEREO_MATCH_LAYOUT_H_
#define SLSLAM_STEREO_MATCH_LAYOUT_H_

#include <cmath>
#include <cstddef>

#include "../../include/slslam_hip.h"
#include "call_layout.h"

#if defined(__HIPCC__)
#define SLSLAM_STEREO_HD __host__ __device__
#else
#define SLSLAM_STEREO_HD
#endif

// every operation of the contract is rounded on its own
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace slslam_stereo {

// the limits and the validation of a gated problem (call_layout.h)
using slslam::gated::kMaxD;
using slslam::gated::kMaxSegments;
using slslam::gated::segment_ok;
using slslam::gated::shape_valid;

// per-segment status: the values of SLSLAM_STEREO_* (the api file asserts it)
enum Status { kMatched = 0, kUnmatched = 1, kFlat = 2, kInvalid = 3 };

// The options as the kernels take them
struct Gate {
  double min_disparity, max_disparity, max_tan2, min_rows, min_overlap, max_distance;
};
struct Camera {
  double fx, fy, cx, cy;
};

// One stereo frame among those of a call: rows = left segments, columns = right segments.  Its segments lie at 4 a0 / 4 j0 floats of
// the left / right segment region, its flags at a0 / j0, its descriptors at D a0 / D j0 floats.
struct FrameDesc {
  slslam::Span span;
};

inline bool options_valid(const slslam_stereo_match_options* o) {
  if (!o) return false;
  const bool f = std::isfinite(o->min_disparity) && std::isfinite(o->max_disparity) && std::isfinite(o->max_tan2) &&
                 std::isfinite(o->min_rows) && std::isfinite(o->min_overlap) && std::isfinite(o->fx) && std::isfinite(o->fy) &&
                 std::isfinite(o->cx) && std::isfinite(o->cy);
  return f && o->min_disparity <= o->max_disparity && o->max_tan2 >= 0.0 && o->min_rows >= 0.0 && o->min_overlap >= 0.0 &&
         o->min_overlap <= 1.0 && !std::isnan(o->ratio) && !std::isnan(o->max_distance) && o->fx != 0.0 && o->fy != 0.0;
}

inline bool frame_valid(const slslam_stereo_frame& f, int max_segments) {
  if (f.num_left < 0 || f.num_left > max_segments || f.num_right < 0 || f.num_right > max_segments) return false;
  if (f.num_left > 0 && (!f.left_segments || !f.left_descriptors)) return false;
  if (f.num_right > 0 && (!f.right_segments || !f.right_descriptors)) return false;
  return true;
}

inline Gate gate_of(const slslam_stereo_match_options& o) {
  return Gate{o.min_disparity, o.max_disparity, o.max_tan2, o.min_rows, o.min_overlap, o.max_distance};
}
inline Camera camera_of(const slslam_stereo_match_options& o) { return Camera{o.fx, o.fy, o.cx, o.cy}; }

// ---- the contract's arithmetic, in its order
struct Segment {
  double x0, y0, x1, y1, lo, hi, ext, dx, dy, slope;
};

// slope given: what a kernel that has staged the quotient reads instead of dividing again
SLSLAM_STEREO_HD inline Segment segment_with(float x0, float y0, float x1, float y1, double slope) {
  Segment s;
  s.x0 = x0; s.y0 = y0; s.x1 = x1; s.y1 = y1;
  s.lo = s.y1 < s.y0 ? s.y1 : s.y0;
  s.hi = s.y1 < s.y0 ? s.y0 : s.y1;
  s.ext = s.hi - s.lo;
  s.dx = s.x1 - s.x0;
  s.dy = s.y1 - s.y0;
  s.slope = slope;
  return s;
}

// slope = dx / dy where ext > 0, else 0: it is only read where ext > 0
SLSLAM_STEREO_HD inline double slope_of(float x0, float y0, float x1, float y1) {
  const double dx = (double)x1 - (double)x0, dy = (double)y1 - (double)y0;
  return dy != 0.0 ? dx / dy : 0.0;
}

SLSLAM_STEREO_HD inline Segment segment_of(float x0, float y0, float x1, float y1) {
  return segment_with(x0, y0, x1, y1, slope_of(x0, y0, x1, y1));
}

SLSLAM_STEREO_HD inline double dot_of(const Segment& a, const Segment& b) {
  const double p1 = a.dx * b.dx, p2 = a.dy * b.dy;
  return p1 + p2;
}

// rows, overlap, direction, disparity: everything of admissibility but validity and the descriptor distance
SLSLAM_STEREO_HD inline bool gate_admits(const Segment& a, const Segment& b, const Gate& g) {
  const bool rows = (a.ext >= g.min_rows) & (b.ext >= g.min_rows);
  const double top = a.lo > b.lo ? a.lo : b.lo, bot = a.hi < b.hi ? a.hi : b.hi;
  const double o = bot - top, mn = a.ext < b.ext ? a.ext : b.ext;
  const double need = g.min_overlap * mn;
  const bool overlap = (o >= need) & (o > 0.0);
  const double dot = dot_of(a, b);
  const double q1 = a.dx * b.dy, q2 = a.dy * b.dx;
  const double cross = q1 - q2;
  const double c2 = cross * cross, d2 = dot * dot;
  const double lim = g.max_tan2 * d2;
  const bool direction = (c2 <= lim) & (dot != 0.0);
  const double yc = 0.5 * (top + bot);
  const double ta = (yc - a.y0) * a.slope, tb = (yc - b.y0) * b.slope;
  const double xa = a.x0 + ta, xb = b.x0 + tb;
  const double d = xa - xb;
  const bool disparity = (g.min_disparity <= d) & (d <= g.max_disparity);
  return rows & overlap & direction & disparity;
}

// the row of a MATCHED left segment a and its right segment b: observations[8], disparity[2]
SLSLAM_STEREO_HD inline void emit_row(const Segment& a, const Segment& b, const Camera& k, double* obs, double* disp) {
  const bool swap = dot_of(a, b) < 0.0;
  const double v[8] = {a.x0, a.y0, a.x1, a.y1, swap ? b.x1 : b.x0, swap ? b.y1 : b.y0, swap ? b.x0 : b.x1, swap ? b.y0 : b.y1};
  const double ox = k.cx / k.fx, oy = k.cy / k.fy;
  for (int q = 0; q < 8; q += 2) {
    const double sx = v[q] / k.fx, sy = v[q + 1] / k.fy;
    obs[q] = sx - ox;
    obs[q + 1] = sy - oy;
  }
  const double t0 = (a.y0 - b.y0) * b.slope, t1 = (a.y1 - b.y0) * b.slope;
  const double xb0 = b.x0 + t0, xb1 = b.x0 + t1;
  disp[0] = a.x0 - xb0;
  disp[1] = a.x1 - xb1;
}

SLSLAM_STEREO_HD inline int status_of(int ok, const Segment& a, const Gate& g, int match) {
  return !ok ? kInvalid : !(a.ext >= g.min_rows) ? kFlat : match >= 0 ? kMatched : kUnmatched;
}

// Where everything of a call lies.  Upload, the same offsets on the host and on the device: FrameDesc[F] at 0, the left and the right
// segments (4 floats each), their flags (an int each), their descriptors.  On the device the keys follow, then the result block: the
// matchers' MatchBlock, then segment_status [A], observations [A 8], disparity [A 2]; on the host the result block follows the upload.
struct CallLayout {
  size_t off_lseg = 0, off_rseg = 0, off_lok = 0, off_rok = 0, off_ldesc = 0, off_rdesc = 0, in_bytes = 0;
  size_t off_keys = 0, off_out = 0;
  slslam::MatchBlock out;
  size_t o_status = 0, o_obs = 0, o_disp = 0, out_bytes = 0;      // within the result block, behind `out`
  slslam::BlockBytes bytes;
};

inline CallLayout call_layout(size_t F, size_t A, size_t J, size_t D) {
  CallLayout y;
  slslam::Carve c;
  c.take(sizeof(FrameDesc) * F);
  y.off_lseg = c.take(16 * A);
  y.off_rseg = c.take(16 * J);
  y.off_lok = c.take(4 * A);
  y.off_rok = c.take(4 * J);
  y.off_ldesc = c.take(4 * A * D);
  y.off_rdesc = c.take(4 * J * D);
  y.in_bytes = c.at;
  y.out = slslam::match_block(F, A, J);
  slslam::Carve o;
  o.take(y.out.bytes);
  y.o_status = o.take(4 * A);
  y.o_obs = o.take(64 * A);
  y.o_disp = o.take(16 * A);
  y.out_bytes = o.at;
  y.bytes.host = y.in_bytes + y.out_bytes;
  y.off_keys = c.take(8 * J);
  y.off_out = c.at;
  y.bytes.dev = y.off_out + y.out_bytes;
  return y;
}

}  // namespace slslam_stereo

#endif  // SLSLAM_STEREO_MATCH_LAYOUT_H_

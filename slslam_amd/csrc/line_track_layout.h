// slslam_amd/csrc/line_track_layout.h — the host half of the line tracker (include/slslam_hip.h: slslam_line_tracker_*): the limits, the
// validation of options and frames, what the contract derives per segment and per pair (the warp, the temporal gate, the status and
// the id rule: the same functions run in the kernels of line_track.h and, on the host, in tests/host_cxx/line_track_layout_check.cpp),
// and where everything of a run lies in its one block.  Plain C++ with no HIP in it, so that the check program runs it on the host
// under the sanitizers.  Internal: not part of the C ABI.
#ifndef SLSLAM_LINE_TRACK_LAYOUT_H_
#define SLSLAM_LINE_TRACK_LAYOUT_H_

#include <climits>
#include <cmath>
#include <cstddef>

#include "../../include/slslam_hip.h"
#include "call_layout.h"

#if defined(__HIPCC__)
#define SLSLAM_TRACK_HD __host__ __device__
#else
#define SLSLAM_TRACK_HD
#endif

// every operation of the contract is rounded on its own
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace slslam_track {

// the limits and the validation of a gated problem (call_layout.h)
using slslam::gated::kMaxD;
using slslam::gated::kMaxSegments;
using slslam::gated::segment_ok;
using slslam::gated::shape_valid;
constexpr int kScanWidth = 64;                           // frames k_track_prefix sums per pass: one wave

// per-segment status: the values of SLSLAM_TRACK_* (the api file asserts it)
enum Status { kContinued = 0, kNew = 1, kShort = 2, kInvalid = 3 };

// The options as the kernels take them: the squares are taken once, on the host
struct Gate {
  double max_tan2, max_shift2, max_offset2, min_overlap, min_length2, max_distance;
};

// The affine map from the previous frame's pixels to this frame's: x' = (a11 x + a12 y) + tx, y' = (a21 x + a22 y) + ty
struct Warp {
  double a11, a12, tx, a21, a22, ty;
};

// One frame among those of a run.  Everything per segment lies in regions over [carried | frame 0 | ... | frame T-1]: the frame's own
// segments (the rows) start at a0, those of the frame before it (the columns; for frame 0 the carried frame) at j0.
struct FrameDesc {
  slslam::Span span;
  Warp warp;
};

inline bool options_valid(const slslam_line_track_options* o) {
  if (!o) return false;
  const bool f = std::isfinite(o->max_tan2) && std::isfinite(o->max_shift) && std::isfinite(o->max_offset) && std::isfinite(o->min_overlap) &&
                 std::isfinite(o->min_length);
  return f && o->max_tan2 >= 0.0 && o->max_shift >= 0.0 && o->max_offset >= 0.0 && o->min_overlap >= 0.0 && o->min_overlap <= 1.0 &&
         o->min_length >= 0.0 && !std::isnan(o->ratio) && !std::isnan(o->max_distance);
}

inline bool frame_valid(const slslam_line_track_frame& f, int max_segments) {
  if (f.num_segments < 0 || f.num_segments > max_segments) return false;
  if (f.num_segments > 0 && (!f.segments || !f.descriptors)) return false;
  if (f.predict)
    for (int q = 0; q < 6; ++q)
      if (!std::isfinite(f.predict[q])) return false;
  return true;
}

// next_id + the run's segments must stay an int: every one of them may be NEW
inline bool ids_fit(int next_id, long long segments) { return next_id >= 0 && (long long)next_id + segments <= (long long)INT_MAX; }

inline Gate gate_of(const slslam_line_track_options& o) {
  return Gate{o.max_tan2, o.max_shift * o.max_shift, o.max_offset * o.max_offset, o.min_overlap, o.min_length * o.min_length, o.max_distance};
}
inline Warp warp_of(const double* predict) {
  return predict ? Warp{predict[0], predict[1], predict[2], predict[3], predict[4], predict[5]} : Warp{1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
}

// ---- the contract's arithmetic, in its order
struct Ends {
  double x0, y0, x1, y1;
};
struct Segment {
  double x0, y0, x1, y1, dx, dy, len2, mx, my;
};

SLSLAM_TRACK_HD inline Ends ends_of(float x0, float y0, float x1, float y1) { return Ends{x0, y0, x1, y1}; }

SLSLAM_TRACK_HD inline Ends warped(const Ends& e, const Warp& w) {
  Ends r;
  { const double t1 = w.a11 * e.x0, t2 = w.a12 * e.y0; const double s = t1 + t2; r.x0 = s + w.tx; }
  { const double t1 = w.a21 * e.x0, t2 = w.a22 * e.y0; const double s = t1 + t2; r.y0 = s + w.ty; }
  { const double t1 = w.a11 * e.x1, t2 = w.a12 * e.y1; const double s = t1 + t2; r.x1 = s + w.tx; }
  { const double t1 = w.a21 * e.x1, t2 = w.a22 * e.y1; const double s = t1 + t2; r.y1 = s + w.ty; }
  return r;
}

SLSLAM_TRACK_HD inline Segment segment_of(const Ends& e) {
  Segment s;
  s.x0 = e.x0; s.y0 = e.y0; s.x1 = e.x1; s.y1 = e.y1;
  s.dx = s.x1 - s.x0;
  s.dy = s.y1 - s.y0;
  const double p1 = s.dx * s.dx, p2 = s.dy * s.dy;
  s.len2 = p1 + p2;
  const double sx = s.x0 + s.x1, sy = s.y0 + s.y1;
  s.mx = 0.5 * sx;
  s.my = 0.5 * sy;
  return s;
}

// short: of the segment as it lies in its own frame (not warped)
SLSLAM_TRACK_HD inline bool is_short(const Segment& s, const Gate& g) { return s.len2 < g.min_length2; }

// e = (p - q0) x d of the point p against the line through q0 along d
SLSLAM_TRACK_HD inline double offset_of(double px, double py, const Segment& q) {
  const double u = px - q.x0, v = py - q.y0;
  const double q1 = u * q.dy, q2 = v * q.dx;
  return q1 - q2;
}

// (p - a0) . d_a
SLSLAM_TRACK_HD inline double along_of(double px, double py, const Segment& a) {
  const double u = px - a.x0, v = py - a.y0;
  const double p1 = u * a.dx, p2 = v * a.dy;
  return p1 + p2;
}

// direction, shift, offset, overlap: everything of admissibility but validity, shortness and the descriptor distance.  a: a row, b: a
// column after the warp.
SLSLAM_TRACK_HD inline bool gate_admits(const Segment& a, const Segment& b, const Gate& g) {
  const double p1 = a.dx * b.dx, p2 = a.dy * b.dy;
  const double dot = p1 + p2;
  const double q1 = a.dx * b.dy, q2 = a.dy * b.dx;
  const double cross = q1 - q2;
  const double c2 = cross * cross, d2 = dot * dot;
  const double lim = g.max_tan2 * d2;
  const bool direction = (c2 <= lim) & (dot != 0.0);
  const double ex = a.mx - b.mx, ey = a.my - b.my;
  const double e1 = ex * ex, e2 = ey * ey;
  const double s2 = e1 + e2;
  const bool shift = s2 <= g.max_shift2;
  const double eab = offset_of(a.mx, a.my, b), eba = offset_of(b.mx, b.my, a);
  const double eab2 = eab * eab, eba2 = eba * eba;
  const double lab = g.max_offset2 * b.len2, lba = g.max_offset2 * a.len2;
  const bool offset = (eab2 <= lab) & (eba2 <= lba);
  const double s0 = along_of(b.x0, b.y0, a), s1 = along_of(b.x1, b.y1, a);
  const double lo = s1 < s0 ? s1 : s0, hi = s1 < s0 ? s0 : s1;
  const double top = hi < a.len2 ? hi : a.len2, bot = lo > 0.0 ? lo : 0.0;
  const double o = top - bot, span = hi - lo;
  const double mn = span < a.len2 ? span : a.len2;
  const double need = g.min_overlap * mn;
  const bool overlap = (o >= need) & (o > 0.0);
  return direction & shift & offset & overlap;
}

SLSLAM_TRACK_HD inline int status_of(int ok, bool shrt, int match) { return !ok ? kInvalid : shrt ? kShort : match >= 0 ? kContinued : kNew; }

// ---- the id rule.  Over the regions' positions: status, match (an index into the frame before) and rank (the NEW segments of the
// same frame before this one) of every segment of the run, id and age of the carried frame (positions below frames[0].span.a0);
// new_before[t]: the NEW segments of frames 0 .. t-1.  Follows match back from segment a of frame t until it reaches a NEW segment or
// the carried frame: at most t + 1 steps, reading what the kernels before it wrote.
struct IdAge {
  int id, age;
};

SLSLAM_TRACK_HD inline IdAge id_of(const FrameDesc* frames, int t, int a, const int* status, const int* match, const int* rank,
                                   const int* new_before, const int* id, const int* age, int next_id) {
  long long pos = frames[t].span.a0 + a;
  if (status[pos] == kInvalid || status[pos] == kShort) return IdAge{-1, 0};
  int steps = 0;
  while (status[pos] == kContinued) {
    pos = frames[t].span.j0 + match[pos];
    ++steps;
    if (--t < 0) return IdAge{id[pos], age[pos] + steps};
  }
  return IdAge{next_id + new_before[t] + rank[pos], 1 + steps};
}

// Where everything of a run lies; S = the carried segments + those of all frames.  Upload, the same offsets on the host and on the
// device: FrameDesc[F] at 0, then the segments (4 floats each), their flags (an int each), their descriptors - each region with the
// carried frame's places in front, which are filled on the device after the upload from the handle's carried block (line_track.h:
// k_track_copy): the regions move with the size of a run, the carried block does not.  On the device the keys follow, then the result block: the matchers' MatchBlock
// over S rows and S columns, then segment_status, id, age, rank [S] and num_new, new_before [F]; on the host the result block
// follows the upload.
struct CallLayout {
  size_t off_seg = 0, off_ok = 0, off_desc = 0, in_bytes = 0;
  size_t off_keys = 0, off_out = 0;
  slslam::MatchBlock out;
  size_t o_status = 0, o_id = 0, o_age = 0, o_rank = 0, o_new = 0, o_before = 0, out_bytes = 0;      // within the result block
  slslam::BlockBytes bytes;
};

inline CallLayout call_layout(size_t F, size_t S, size_t D) {
  CallLayout y;
  slslam::Carve c;
  c.take(sizeof(FrameDesc) * F);
  y.off_seg = c.take(16 * S);
  y.off_ok = c.take(4 * S);
  y.off_desc = c.take(4 * S * D);
  y.in_bytes = c.at;
  y.out = slslam::match_block(F, S, S);
  slslam::Carve o;
  o.take(y.out.bytes);
  y.o_status = o.take(4 * S);
  y.o_id = o.take(4 * S);
  y.o_age = o.take(4 * S);
  y.o_rank = o.take(4 * S);
  y.o_new = o.take(4 * F);
  y.o_before = o.take(4 * (F + 1));
  y.out_bytes = o.at;
  y.bytes.host = y.in_bytes + y.out_bytes;
  y.off_keys = c.take(8 * S);
  y.off_out = c.at;
  y.bytes.dev = y.off_out + y.out_bytes;
  return y;
}

// The carried frame's block on the device, made once for the handle's max_segments: segments, flags, descriptors, ids, ages
struct CarryLayout {
  size_t off_seg = 0, off_ok = 0, off_desc = 0, off_id = 0, off_age = 0, bytes = 0;
};

inline CarryLayout carry_layout(size_t max_segments, size_t D) {
  CarryLayout y;
  slslam::Carve c;
  y.off_seg = c.take(16 * max_segments);
  y.off_ok = c.take(4 * max_segments);
  y.off_desc = c.take(4 * max_segments * D);
  y.off_id = c.take(4 * max_segments);
  y.off_age = c.take(4 * max_segments);
  y.bytes = c.at;
  return y;
}

}  // namespace slslam_track

#endif  // SLSLAM_LINE_TRACK_LAYOUT_H_

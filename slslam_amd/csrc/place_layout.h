// slslam_amd/csrc/place_layout.h — where everything of the place database (place_api.hip) lies: its persistent device block and the
// block of a call.  Plain C++ (call_layout.h), checked on the host by tests/host_cxx/call_block_check.cpp.  Internal: not part of the
// C ABI.
#ifndef SLSLAM_PLACE_LAYOUT_H_
#define SLSLAM_PLACE_LAYOUT_H_

#include "call_layout.h"

namespace slslam_place {

// the persistent device block of a database
struct DbLayout {
  size_t o_word = 0, o_tf = 0, o_n = 0, o_df = 0, o_idf = 0, o_vword = 0, o_sw = 0, o_sv = 0, bytes = 0;
  size_t max_changes = 0;
};

inline DbLayout db_layout(size_t cap, size_t mw, size_t num_leaf, size_t navg) {
  DbLayout y;
  slslam::Carve c;
  y.max_changes = mw + 2 * navg;
  y.o_word = c.take(4 * mw * cap);
  y.o_tf = c.take(4 * mw * cap);
  y.o_n = c.take(4 * cap);                                    // (df follows n: one memset clears both)
  y.o_df = c.take(4 * num_leaf);
  y.o_idf = c.take(4 * (cap + 2));
  y.o_vword = c.take(4 * navg);
  y.o_sw = c.take(4 * y.max_changes);
  y.o_sv = c.take(4 * y.max_changes);
  y.bytes = c.at;
  return y;
}

// a call: the upload (the same offsets on the host and on the device; frame_bytes = sizeof(Frame)), the device's work arrays, the
// result block (the same offsets on the device and on the host, there behind the upload)
struct CallLayout {
  size_t off_desc = 0, in_bytes = 0;
  size_t off_dtf = 0, off_dsum = 0, off_out = 0;
  size_t o_words = 0, o_dword = 0, o_topid = 0, o_topscore = 0, o_score = 0, o_lik = 0, o_touched = 0, doc_bytes = 0, out_bytes = 0;
  slslam::BlockBytes bytes;
};

inline CallLayout call_layout(size_t frame_bytes, size_t F, size_t nfloats, size_t mw, size_t S, size_t top_k) {
  CallLayout y;
  slslam::Carve out, c;
  out.take(4 * F);                                            // doc_n at 0
  y.o_words = out.take(4 * F * mw);
  y.o_dword = out.take(4 * F * mw);
  y.doc_bytes = out.at;                                       // what an insert downloads
  y.o_topid = out.take(4 * F * top_k);
  y.o_topscore = out.take(4 * F * top_k);
  y.o_score = out.take(4 * F * S);
  y.o_lik = out.take(4 * F * S);
  y.o_touched = out.take(F * S);
  y.out_bytes = out.at;
  c.take(frame_bytes * F);
  y.off_desc = c.take(4 * nfloats);
  y.in_bytes = y.off_desc + 4 * nfloats;
  y.bytes.host = c.at + y.out_bytes;
  y.off_dtf = c.take(4 * F * mw);
  y.off_dsum = c.take(8 * F * S);
  y.off_out = c.at;
  y.bytes.dev = y.off_out + y.out_bytes;
  return y;
}

}  // namespace slslam_place

#endif  // SLSLAM_PLACE_LAYOUT_H_

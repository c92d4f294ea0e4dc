// tests/host_cxx/call_block_check.cpp — the host half of the call-block scaffold (slslam_amd/csrc/call_layout.h, place_layout.h), no
// device: the layout builder gives the matchers' result block and the place database's two layouts the offsets their hand-written
// sums gave (the sums are written out below), every region at a multiple of 256 bytes and none over another; the result scatter
// writes exactly the ranges asked for, under NULL arrays and empty problems; the image copy drops the stride and nothing else; a gated
// problem's upload copies its segments and descriptors to their places and flags the non-finite ones.  Built with -fsanitize=address,undefined and run by
// tests/test_call_block_cpu.py.  Prints "call block ok" and exits 0, or says what is wrong and exits 1.
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>
#include <vector>

#include "../../slslam_amd/csrc/call_layout.h"
#include "../../slslam_amd/csrc/place_layout.h"

using slslam::MatchArrays;
using slslam::MatchBlock;
using slslam::Span;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("%s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)
static char ctx[128];                   // the sizes of the layout under test
#define SAME(got, want, what) EXPECT((got) == (want), what ": %zu, expected %zu (%s)", (size_t)(got), (size_t)(want), ctx)

static size_t a256(size_t x) { return (x + 255) / 256 * 256; }

// regions (offset, bytes) of a block of `total` bytes: each at a multiple of 256, inside the block, none over another
static void check_regions(const char* name, std::vector<std::pair<size_t, size_t>> r, size_t total) {
  EXPECT(total % 256 == 0, "%s: %zu bytes in all", name, total);
  for (size_t i = 0; i < r.size(); ++i) {
    EXPECT(r[i].first % 256 == 0, "%s: region %zu at %zu", name, i, r[i].first);
    EXPECT(r[i].first + r[i].second <= total, "%s: region %zu ends at %zu of %zu", name, i, r[i].first + r[i].second, total);
    for (size_t j = 0; j < i; ++j) {
      const bool apart = r[i].first + r[i].second <= r[j].first || r[j].first + r[j].second <= r[i].first;
      EXPECT(apart || r[i].second == 0 || r[j].second == 0, "%s: regions %zu and %zu overlap", name, j, i);
    }
  }
}

static void check_match_block(size_t P, size_t A, size_t J) {
  std::snprintf(ctx, sizeof ctx, "P %zu, rows %zu, columns %zu", P, A, J);
  const MatchBlock b = slslam::match_block(P, A, J);
  const size_t o_match = a256(4 * P);
  const size_t o_best = o_match + a256(4 * A);
  const size_t o_count = o_best + a256(4 * A);
  const size_t o_bv = o_count + a256(4 * A);
  const size_t o_sv = o_bv + a256(4 * A);
  const size_t o_row = o_sv + a256(4 * A);
  const size_t bytes = o_row + a256(4 * J);
  SAME(b.o_match, o_match, "o_match");
  SAME(b.o_best, o_best, "o_best");
  SAME(b.o_count, o_count, "o_count");
  SAME(b.o_best_value, o_bv, "o_best_value");
  SAME(b.o_second_value, o_sv, "o_second_value");
  SAME(b.o_best_row, o_row, "o_best_row");
  SAME(b.bytes, bytes, "bytes");
  check_regions("match block", { { 0, 4 * P }, { b.o_match, 4 * A }, { b.o_best, 4 * A }, { b.o_count, 4 * A }, { b.o_best_value, 4 * A },
                                 { b.o_second_value, 4 * A }, { b.o_best_row, 4 * J } }, b.bytes);
}

static void check_db_layout(size_t cap, size_t mw, size_t num_leaf, size_t navg) {
  std::snprintf(ctx, sizeof ctx, "cap %zu, max_words %zu, leaves %zu, navg %zu", cap, mw, num_leaf, navg);
  const slslam_place::DbLayout y = slslam_place::db_layout(cap, mw, num_leaf, navg);
  const size_t max_changes = mw + 2 * navg;
  const size_t o_word = 0;
  const size_t o_tf = o_word + a256(4 * mw * cap);
  const size_t o_n = o_tf + a256(4 * mw * cap);
  const size_t o_df = o_n + a256(4 * cap);
  const size_t o_idf = o_df + a256(4 * num_leaf);
  const size_t o_vword = o_idf + a256(4 * (cap + 2));
  const size_t o_sw = o_vword + a256(4 * navg);
  const size_t o_sv = o_sw + a256(4 * max_changes);
  const size_t bytes = o_sv + a256(4 * max_changes);
  SAME(y.max_changes, max_changes, "max_changes");
  SAME(y.o_word, o_word, "o_word");
  SAME(y.o_tf, o_tf, "o_tf");
  SAME(y.o_n, o_n, "o_n");
  SAME(y.o_df, o_df, "o_df");
  SAME(y.o_idf, o_idf, "o_idf");
  SAME(y.o_vword, o_vword, "o_vword");
  SAME(y.o_sw, o_sw, "o_sw");
  SAME(y.o_sv, o_sv, "o_sv");
  SAME(y.bytes, bytes, "bytes");
  check_regions("place database", { { y.o_word, 4 * mw * cap }, { y.o_tf, 4 * mw * cap }, { y.o_n, 4 * cap }, { y.o_df, 4 * num_leaf },
                                    { y.o_idf, 4 * (cap + 2) }, { y.o_vword, 4 * navg }, { y.o_sw, 4 * max_changes },
                                    { y.o_sv, 4 * max_changes } }, y.bytes);
}

static void check_call_layout(size_t F, size_t nfloats, size_t mw, size_t S, size_t top_k) {
  const size_t frame_bytes = 16;                              // sizeof(slslam_place::Frame): two ints and a long long
  std::snprintf(ctx, sizeof ctx, "F %zu, floats %zu, max_words %zu, S %zu, top_k %zu", F, nfloats, mw, S, top_k);
  const slslam_place::CallLayout y = slslam_place::call_layout(frame_bytes, F, nfloats, mw, S, top_k);
  const size_t off_desc = a256(frame_bytes * F);
  const size_t in_bytes = off_desc + 4 * nfloats;
  const size_t o_words = a256(4 * F);
  const size_t o_dword = o_words + a256(4 * F * mw);
  const size_t doc_bytes = o_dword + a256(4 * F * mw);
  const size_t o_topid = doc_bytes;
  const size_t o_topscore = o_topid + a256(4 * F * top_k);
  const size_t o_score = o_topscore + a256(4 * F * top_k);
  const size_t o_lik = o_score + a256(4 * F * S);
  const size_t o_touched = o_lik + a256(4 * F * S);
  const size_t out_bytes = o_touched + a256(F * S);
  const size_t off_dtf = a256(in_bytes);
  const size_t off_dsum = off_dtf + a256(4 * F * mw);
  const size_t off_out = off_dsum + a256(8 * F * S);
  const size_t dev_bytes = off_out + out_bytes;
  const size_t host_bytes = a256(in_bytes) + out_bytes;
  SAME(y.off_desc, off_desc, "off_desc");
  SAME(y.in_bytes, in_bytes, "in_bytes");
  SAME(y.o_words, o_words, "o_words");
  SAME(y.o_dword, o_dword, "o_dword");
  SAME(y.doc_bytes, doc_bytes, "doc_bytes");
  SAME(y.o_topid, o_topid, "o_topid");
  SAME(y.o_topscore, o_topscore, "o_topscore");
  SAME(y.o_score, o_score, "o_score");
  SAME(y.o_lik, o_lik, "o_lik");
  SAME(y.o_touched, o_touched, "o_touched");
  SAME(y.out_bytes, out_bytes, "out_bytes");
  SAME(y.off_dtf, off_dtf, "off_dtf");
  SAME(y.off_dsum, off_dsum, "off_dsum");
  SAME(y.off_out, off_out, "off_out");
  SAME(y.bytes.dev, dev_bytes, "dev_bytes");
  SAME(y.bytes.host, host_bytes, "host_bytes");
  check_regions("place call, result block", { { 0, 4 * F }, { y.o_words, 4 * F * mw }, { y.o_dword, 4 * F * mw }, { y.o_topid, 4 * F * top_k },
                                              { y.o_topscore, 4 * F * top_k }, { y.o_score, 4 * F * S }, { y.o_lik, 4 * F * S },
                                              { y.o_touched, F * S } }, y.out_bytes);
  check_regions("place call, device block", { { 0, frame_bytes * F }, { y.off_desc, 4 * nfloats }, { y.off_dtf, 4 * F * mw },
                                              { y.off_dsum, 8 * F * S }, { y.off_out, y.out_bytes } }, y.bytes.dev);
  check_regions("place call, host block", { { 0, frame_bytes * F }, { y.off_desc, 4 * nfloats }, { a256(y.in_bytes), y.out_bytes } },
                y.bytes.host);
}

// A caller's array of `len` 4-byte values on the heap with a guard value on either side
struct Guarded {
  static constexpr int kGuard = 0x5a5a5a5a, kUntouched = 0x31313131;
  std::vector<int> v;
  explicit Guarded(size_t len) : v(len + 2, kUntouched) { v.front() = v.back() = kGuard; }
  int* p() { return v.data() + 1; }
  size_t len() const { return v.size() - 2; }
  bool guards_hold() const { return v.front() == kGuard && v.back() == kGuard; }
};

// what the block holds at value `i` of array `which` (0 num_matched, 1 .. 5 the row arrays, 6 the column array)
static int value(int which, size_t i) { return (which << 24) | (int)i; }

static void check_scatter() {
  // four problems; the first has no rows, the second no columns, the third neither, the fourth crosses 64
  const Span spans[4] = { { 0, 0, 0, 5 }, { 0, 5, 3, 0 }, { 3, 5, 0, 0 }, { 3, 5, 65, 64 } };
  const size_t P = 4, A = 68, J = 69;
  const MatchBlock b = slslam::match_block(P, A, J);
  const size_t off[7] = { 0, b.o_match, b.o_best, b.o_best_value, b.o_second_value, b.o_count, b.o_best_row };   // in MatchArrays' order
  std::vector<char> block(b.bytes, 0x77);                     // exactly the block: a read past it is the sanitizer's
  for (int w = 0; w < 7; ++w)
    for (size_t i = 0; i < (w == 0 ? P : w == 6 ? J : A); ++i) {
      const int x = value(w, i);
      std::memcpy(block.data() + off[w] + 4 * i, &x, 4);
    }
  for (int mask = 0; mask < 64; mask += 7) {                   // which arrays the caller leaves out: 0, 7, 14, ... 63 (all)
    for (size_t p = 0; p < P; ++p) {
      const Span& s = spans[p];
      std::vector<Guarded> g;
      for (int w = 1; w <= 6; ++w) g.emplace_back((size_t)(w == 6 ? s.m : s.n));
      void* ptr[7] = { nullptr };
      for (int w = 1; w <= 6; ++w) ptr[w] = (mask >> (w - 1)) & 1 ? nullptr : (void*)g[(size_t)w - 1].p();
      const MatchArrays r = { (int*)ptr[1], (int*)ptr[2], (float*)ptr[3], (float*)ptr[4], (int*)ptr[5], (int*)ptr[6] };
      const int nm = slslam::match_scatter(block.data(), b, p, s, r);
      EXPECT(nm == value(0, p), "num_matched of problem %zu: %d", p, nm);
      for (int w = 1; w <= 6; ++w) {
        Guarded& a = g[(size_t)w - 1];
        EXPECT(a.guards_hold(), "problem %zu, array %d: written outside its range", p, w);
        const size_t first = (size_t)(w == 6 ? s.j0 : s.a0);
        for (size_t i = 0; i < a.len(); ++i) {
          const int want = ptr[w] ? value(w, first + i) : Guarded::kUntouched;
          EXPECT(a.p()[i] == want, "problem %zu, array %d, entry %zu: %#x, expected %#x", p, w, i, a.p()[i], want);
        }
      }
    }
  }
}

// pack_rows: destinations of exactly width * height bytes on the heap; the bytes of a source row past `width` carry a poison value
static void check_pack_rows() {
  const unsigned char kPoison = 0xEE;
  const int shapes[][3] = { { 5, 4, 5 }, { 5, 4, 9 }, { 7, 0, 7 }, { 1, 6, 1 }, { 1, 6, 3 }, { 64, 3, 100 } };      // width, height, stride
  for (const auto& s : shapes) {
    const int w = s[0], h = s[1], stride = s[2];
    std::snprintf(ctx, sizeof ctx, "width %d, height %d, stride %d", w, h, stride);
    std::vector<unsigned char> src((size_t)h * (size_t)stride, kPoison);
    for (int r = 0; r < h; ++r)
      for (int c = 0; c < w; ++c) src[(size_t)r * stride + c] = (unsigned char)((r * 31 + c * 7) % 200);        // (never the poison)
    unsigned char* dst = new unsigned char[(size_t)w * (size_t)h];                // exactly: a write past it is the sanitizer's
    std::memset(dst, 0x11, (size_t)w * (size_t)h);
    slslam::pack_rows(dst, h > 0 ? src.data() : nullptr, w, h, stride);
    for (int r = 0; r < h; ++r)
      for (int c = 0; c < w; ++c)
        EXPECT(dst[(size_t)r * w + c] == (unsigned char)((r * 31 + c * 7) % 200), "pack_rows (%s): row %d, column %d: %d", ctx, r, c,
               dst[(size_t)r * w + c]);
    delete[] dst;
  }
}

// fill_side: regions of exactly a0 + n entries; the places below a0 stay as they were
static void check_fill_side() {
  const float kInf = std::numeric_limits<float>::infinity(), kNan = std::numeric_limits<float>::quiet_NaN();
  {                                                            // nothing to copy: null sources are not read, nothing is written
    std::vector<float> seg(4 * 3, 7.0f), desc(8 * 3, 7.0f);
    std::vector<int> ok(3, 7);
    slslam::gated::fill_side(seg.data(), desc.data(), ok.data(), 3, nullptr, nullptr, 0, 8);
    for (float v : seg) EXPECT(v == 7.0f, "fill_side, n 0: a segment float was written");
    for (float v : desc) EXPECT(v == 7.0f, "fill_side, n 0: a descriptor float was written");
    for (int v : ok) EXPECT(v == 7, "fill_side, n 0: a flag was written");
  }
  const size_t cases[][3] = { { 1, 8, 0 }, { 1, 128, 2 }, { 5, 8, 3 }, { 5, 128, 0 }, { 65, 8, 1 } };            // n, D, a0
  for (const auto& c : cases) {
    const size_t n = c[0], D = c[1], a0 = c[2];
    for (int bad = 0; bad < 3; ++bad) {                        // 0: all finite; 1: a segment float is not; 2: a descriptor float is not
      const size_t victim = n / 2;
      std::snprintf(ctx, sizeof ctx, "n %zu, D %zu, a0 %zu, bad %d", n, D, a0, bad);
      std::vector<float> src_seg(4 * n), src_desc(D * n);
      for (size_t i = 0; i < src_seg.size(); ++i) src_seg[i] = (float)i + 0.5f;
      for (size_t i = 0; i < src_desc.size(); ++i) src_desc[i] = 0.001f * (float)i - 1.0f;
      if (bad == 1) src_seg[4 * victim + 3] = kNan;
      if (bad == 2) src_desc[D * victim + D - 1] = kInf;
      std::vector<float> seg(4 * (a0 + n), -3.0f), desc(D * (a0 + n), -3.0f);      // exactly sized
      std::vector<int> ok(a0 + n, -3);
      slslam::gated::fill_side(seg.data(), desc.data(), ok.data(), a0, src_seg.data(), src_desc.data(), n, (int)D);
      for (size_t i = 0; i < 4 * a0; ++i) EXPECT(seg[i] == -3.0f, "fill_side (%s): segment float %zu below a0 written", ctx, i);
      for (size_t i = 0; i < D * a0; ++i) EXPECT(desc[i] == -3.0f, "fill_side (%s): descriptor float %zu below a0 written", ctx, i);
      for (size_t i = 0; i < a0; ++i) EXPECT(ok[i] == -3, "fill_side (%s): flag %zu below a0 written", ctx, i);
      EXPECT(std::memcmp(seg.data() + 4 * a0, src_seg.data(), 16 * n) == 0, "fill_side (%s): segments", ctx);
      EXPECT(std::memcmp(desc.data() + D * a0, src_desc.data(), 4 * D * n) == 0, "fill_side (%s): descriptors", ctx);
      for (size_t i = 0; i < n; ++i) {
        const int want = bad != 0 && i == victim ? 0 : 1;
        EXPECT(ok[a0 + i] == want, "fill_side (%s): flag %zu is %d, expected %d", ctx, i, ok[a0 + i], want);
      }
    }
  }
}

// shape_valid: the table the stereo matcher's and the tracker's layout checks assert
static void check_shape_valid() {
  using slslam::gated::shape_valid;
  EXPECT(shape_valid(8, 1, 1) && shape_valid(72, 64, 512) && shape_valid(128, 1, 512), "shape_valid refuses a valid shape");
  EXPECT(!shape_valid(0, 1, 1) && !shape_valid(12, 1, 1) && !shape_valid(136, 1, 1) && !shape_valid(72, 0, 1) && !shape_valid(72, 1, 0) &&
         !shape_valid(72, 1, 513), "shape_valid takes an invalid shape");
}

int main() {
  // every total 0, P = 1, totals that are and are not multiples of 64 (a region of 64 values is exactly 256 bytes)
  const size_t sizes[][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 1, 1, 0 }, { 1, 0, 1 }, { 1, 1, 1 }, { 1, 64, 64 }, { 1, 63, 65 }, { 3, 128, 1 },
                              { 64, 4096, 640 }, { 65, 4097, 641 }, { 70000, 70000 * 3, 70000 * 5 } };
  for (const auto& s : sizes) check_match_block(s[0], s[1], s[2]);
  const size_t dbs[][4] = { { 1, 1, 2, 1 }, { 64, 64, 4096, 100 }, { 63, 65, 1000, 7 }, { 4096, 512, 1 << 20, 100 }, { 5, 3, 9, 64 } };
  for (const auto& d : dbs) check_db_layout(d[0], d[1], d[2], d[3]);
  const size_t calls[][5] = { { 0, 0, 1, 1, 0 }, { 1, 0, 1, 1, 0 }, { 1, 64 * 16, 64, 1, 0 }, { 1, 63, 65, 2, 1 }, { 64, 64 * 512 * 32, 512, 4097, 16 },
                              { 7, 1000, 100, 64, 3 }, { 16, 16 * 65, 65, 257, 0 } };
  for (const auto& c : calls) check_call_layout(c[0], c[1], c[2], c[3], c[4]);
  check_scatter();
  check_pack_rows();
  check_fill_side();
  check_shape_valid();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("call block ok\n");
  return 0;
}

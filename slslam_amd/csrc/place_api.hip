// slslam_amd/csrc/place_api.hip — the place recogniser's tree and database (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*); the
// Bayes filter behind them is host/place_filter.cpp.  Per run, whatever the number of frames:
//   upload   one block [Frame F | floats: the descriptors of every frame]
//   launches k_place_document (words, documents), k_place_score (every scored state of every frame), k_place_finish (fill, likelihoods,
//            top_k)
//   download one block [doc_n F | words | document words | top_id | top_score | score | likelihood | touched]
// An insert is the first launch alone with the document also written into the database's column; the host keeps the words of every
// document, df and the virtual document (all of it bookkeeping over a few hundred integers per insert) and, when a document becomes
// visible, uploads the df entries that changed, the idf table of the new doc_size and the virtual document.
// The kernels are in place_recognition.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "place_layout.h"
#include "place_recognition.h"

using namespace slslam_place;
using slslam::align256;
using slslam::GrowBuf;
using slslam::Mem;

static_assert(kMaxK == SLSLAM_PLACE_MAX_K && kMaxL == SLSLAM_PLACE_MAX_L && kMaxD == SLSLAM_PLACE_MAX_D &&
              kMaxWords == SLSLAM_PLACE_MAX_WORDS && kMaxTopK == SLSLAM_PLACE_MAX_TOP_K, "the header's limits are the kernels'");

struct slslam_voctree {
  int device = -1, K = 0, L = 0, D = 0;
  size_t num_int = 0, num_leaf = 0;
  std::vector<float> nodes;
  float* d_nodes = nullptr;
  ~slslam_voctree() {
    if (d_nodes) (void)hipFree(d_nodes);
  }
};

namespace {

// interior nodes and leaves of a (K, L) tree; false outside the limits
bool tree_shape(int K, int L, int D, size_t* num_int, size_t* num_leaf) {
  if (K < 2 || K > kMaxK || L < 1 || L > kMaxL || D < 1 || D > kMaxD) return false;
  size_t ni = 0, level = 1;
  for (int l = 0; l < L; ++l) { ni += level; level *= (size_t)K; }
  if (level > ((size_t)1 << 24)) return false;
  *num_int = ni; *num_leaf = level;
  return true;
}

}  // namespace

struct slslam_place_db : slslam::Handle {                // (the device is the tree's)
  slslam_voctree* tree = nullptr;
  int max_docs = 0, max_words = 0, max_frames = 0, recent = 0, navg = 0;
  int inserted = 0, visible = 0;
  bool has_virtual = false;
  std::vector<std::vector<int>> doc_words;     // of every inserted document
  std::vector<int> df;                         // [leaves] over the visible documents, the virtual one not counted
  std::vector<int> nonempty;                   // words with df > 0, in the order they became so
  std::vector<int> vwords;                     // the virtual document, ascending (empty: none)
  GrowBuf d_db{Mem::kDevice}, d_block{Mem::kDevice}, h_block{Mem::kPinned}, h_rel{Mem::kPinned};
  DbLayout dl;
};

namespace {

bool frame_valid(const slslam_place_frame& f, int max_words) {
  return f.num_descriptors >= 0 && f.num_descriptors <= max_words && (f.num_descriptors == 0 || f.descriptors);
}

// The device, the stream, the tree's nodes and every block of the database, made once for its capacity
int ensure_device(slslam_place_db* db) {
  slslam_voctree* t = db->tree;
  const int rc = db->ensure(t->device);
  if (rc != SLSLAM_OK) return rc;
  if (!t->d_nodes) {
    float* p = nullptr;
    HIP_TRY(hipMalloc((void**)&p, 4 * t->nodes.size()));
    hipError_t e = hipMemcpy(p, t->nodes.data(), 4 * t->nodes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p); HIP_TRY(e); }
    t->d_nodes = p;
  }
  if (!db->d_db.p) {
    long long unused = 0;
    const size_t mw = (size_t)db->max_words, F = (size_t)db->max_frames;
    db->dl = db_layout((size_t)db->max_docs, mw, t->num_leaf, (size_t)db->navg);
    const CallLayout cap = call_layout(sizeof(Frame), F, F * mw * (size_t)t->D, mw, (size_t)db->max_docs + 1, kMaxTopK);
    HIP_TRY(db->d_db.need(db->dl.bytes, &unused));
    HIP_TRY(hipMemsetAsync(db->d_db.p + db->dl.o_n, 0, db->dl.o_idf - db->dl.o_n, db->stream));    // n and df
    HIP_TRY(db->d_block.need(cap.bytes.dev, &unused));
    HIP_TRY(db->h_block.need(cap.bytes.host, &unused));
    HIP_TRY(db->h_rel.need(8 * db->dl.max_changes + 4 * ((size_t)db->max_docs + 2) + 4 * (size_t)db->navg, &unused));
    ++db->allocations;
  }
  return SLSLAM_OK;
}

// Copies the frames into the upload block; status per frame.  Returns the floats written.
size_t stage_frames(const slslam_place_db* db, int F, const slslam_place_frame* frames, const CallLayout& y, int* status) {
  const int D = db->tree->D;
  char* h = db->h_block.p;
  Frame* fd = reinterpret_cast<Frame*>(h);
  float* hd = reinterpret_cast<float*>(h + y.off_desc);
  size_t nf = 0;
  for (int f = 0; f < F; ++f) {
    const int n = frames[f].num_descriptors;
    const size_t cnt = (size_t)n * (size_t)D;
    int st = n == 0 ? SLSLAM_PLACE_EMPTY : SLSLAM_PLACE_OK;
    const float* src = frames[f].descriptors;
    for (size_t i = 0; i < cnt; ++i)
      if (!std::isfinite(src[i])) { st = SLSLAM_PLACE_INVALID_DESCRIPTOR; break; }
    fd[f].n = n;
    fd[f].run = st == SLSLAM_PLACE_OK ? 1 : 0;
    fd[f].desc = (long long)nf;
    if (fd[f].run) { std::memcpy(hd + nf, src, 4 * cnt); nf += cnt; }
    status[f] = st;
  }
  return nf;
}

QueryOut query_out(char* dv, const CallLayout& y) {
  QueryOut o;
  char* d_out = dv + y.off_out;
  o.doc_n = reinterpret_cast<int*>(d_out);
  o.words = reinterpret_cast<int*>(d_out + y.o_words);
  o.doc_word = reinterpret_cast<int*>(d_out + y.o_dword);
  o.doc_tf = reinterpret_cast<float*>(dv + y.off_dtf);
  o.dsum = reinterpret_cast<double*>(dv + y.off_dsum);
  o.top_id = reinterpret_cast<int*>(d_out + y.o_topid);
  o.top_score = reinterpret_cast<float*>(d_out + y.o_topscore);
  o.score = reinterpret_cast<float*>(d_out + y.o_score);
  o.likelihood = reinterpret_cast<float*>(d_out + y.o_lik);
  o.touched = reinterpret_cast<unsigned char*>(d_out + y.o_touched);
  return o;
}

Tree device_tree(const slslam_voctree* t) { return Tree{t->K, t->L, t->D, t->d_nodes}; }

// The front pending document becomes visible: df, the virtual document, then the device's copy of what changed
int release_front(slslam_place_db* db) {
  const DbLayout& dl = db->dl;
  std::vector<int> changed;
  for (int w : db->doc_words[(size_t)db->visible]) {
    if (db->df[(size_t)w]++ == 0) db->nonempty.push_back(w);
    changed.push_back(w);
  }
  ++db->visible;
  changed.insert(changed.end(), db->vwords.begin(), db->vwords.end());   // (they lose the virtual document's count, or keep it below)
  db->vwords.clear();
  const size_t navg = (size_t)db->navg;
  if (db->nonempty.size() > navg) {
    std::vector<int> c(db->nonempty);
    const std::vector<int>& df = db->df;
    auto before = [&df](int a, int b) { return df[(size_t)a] != df[(size_t)b] ? df[(size_t)a] > df[(size_t)b] : a < b; };
    std::nth_element(c.begin(), c.begin() + (long)navg - 1, c.end(), before);
    db->vwords.assign(c.begin(), c.begin() + (long)navg);
    std::sort(db->vwords.begin(), db->vwords.end());
    changed.insert(changed.end(), db->vwords.begin(), db->vwords.end());
  }
  db->has_virtual = !db->vwords.empty();
  std::sort(changed.begin(), changed.end());
  changed.erase(std::unique(changed.begin(), changed.end()), changed.end());

  const int doc_size = db->visible + (db->has_virtual ? 1 : 0);
  const size_t nc = changed.size();                           // <= max_words + 2 num_avg_words
  int* h_w = reinterpret_cast<int*>(db->h_rel.p);
  int* h_v = h_w + dl.max_changes;
  float* h_idf = reinterpret_cast<float*>(h_v + dl.max_changes);
  int* h_vw = reinterpret_cast<int*>(h_idf + (size_t)db->max_docs + 2);
  for (size_t i = 0; i < nc; ++i) {
    h_w[i] = changed[i];
    h_v[i] = db->df[(size_t)changed[i]] + (std::binary_search(db->vwords.begin(), db->vwords.end(), changed[i]) ? 1 : 0);
  }
  h_idf[0] = 0.0f;
  for (int d = 1; d <= doc_size; ++d) h_idf[d] = (float)std::log10((double)doc_size / (double)d);
  std::copy(db->vwords.begin(), db->vwords.end(), h_vw);
  char* dd = db->d_db.p;
  hipStream_t s = db->stream;
  HIP_TRY(hipMemcpyAsync(dd + dl.o_sw, h_w, 4 * nc, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(dd + dl.o_sv, h_v, 4 * nc, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(dd + dl.o_idf, h_idf, 4 * ((size_t)doc_size + 1), hipMemcpyHostToDevice, s));
  if (db->has_virtual) HIP_TRY(hipMemcpyAsync(dd + dl.o_vword, h_vw, 4 * navg, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_place_scatter, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, (int)nc,
                     reinterpret_cast<const int*>(dd + dl.o_sw), reinterpret_cast<const int*>(dd + dl.o_sv),
                     reinterpret_cast<int*>(dd + dl.o_df));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return SLSLAM_OK;
}

}  // namespace

extern "C" int slslam_voctree_create(int device, int K, int L, int D, const float* nodes, slslam_voctree** out) {
  size_t ni = 0, nl = 0;
  if (!out || !nodes || !tree_shape(K, L, D, &ni, &nl)) return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_voctree* t = new (std::nothrow) slslam_voctree();
  if (!t) return SLSLAM_ERR_NO_MEMORY;
  t->device = device; t->K = K; t->L = L; t->D = D; t->num_int = ni; t->num_leaf = nl;
  try {
    t->nodes.assign(nodes, nodes + ni * (size_t)K * (size_t)D);
  } catch (const std::bad_alloc&) {
    delete t;
    return SLSLAM_ERR_NO_MEMORY;
  }
  *out = t;
  return SLSLAM_OK;
}

extern "C" int slslam_voctree_load(const char* path, int device, int K, int L, int D, slslam_voctree** out) {
  size_t ni = 0, nl = 0;
  if (!out || !path || !tree_shape(K, L, D, &ni, &nl)) return SLSLAM_ERR_INVALID_ARGUMENT;
  std::FILE* fp = std::fopen(path, "rb");
  if (!fp) return SLSLAM_ERR_INVALID_ARGUMENT;
  const size_t want = ni * (size_t)K * (size_t)D;
  std::vector<float> nodes;
  int rc = SLSLAM_OK;
  try {
    nodes.resize(want);
    char extra;
    if (std::fread(nodes.data(), sizeof(float), want, fp) != want || std::fread(&extra, 1, 1, fp) != 0) rc = SLSLAM_ERR_INVALID_ARGUMENT;
  } catch (const std::bad_alloc&) {
    rc = SLSLAM_ERR_NO_MEMORY;
  }
  std::fclose(fp);
  return rc == SLSLAM_OK ? slslam_voctree_create(device, K, L, D, nodes.data(), out) : rc;
}

extern "C" void slslam_voctree_destroy(slslam_voctree* tree) { delete tree; }

extern "C" int slslam_place_db_create(slslam_voctree* tree, int max_docs, int max_words, int max_frames, int recent, int num_avg_words,
                                      slslam_place_db** out) {
  if (!out || !tree || max_docs < 1 || max_words < 1 || max_words > kMaxWords || max_frames < 1 || recent < 0 || num_avg_words < 1 ||
      num_avg_words > (1 << 24))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_place_db* db = new (std::nothrow) slslam_place_db();
  if (!db) return SLSLAM_ERR_NO_MEMORY;
  db->tree = tree;
  db->max_docs = max_docs; db->max_words = max_words; db->max_frames = max_frames; db->recent = recent; db->navg = num_avg_words;
  try {
    db->df.assign(tree->num_leaf, 0);
  } catch (const std::bad_alloc&) {
    delete db;
    return SLSLAM_ERR_NO_MEMORY;
  }
  *out = db;
  return SLSLAM_OK;
}

extern "C" void slslam_place_db_destroy(slslam_place_db* db) { delete db; }

extern "C" int slslam_place_db_size(const slslam_place_db* db, int* inserted, int* visible, int* doc_size) {
  if (!db) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (inserted) *inserted = db->inserted;
  if (visible) *visible = db->visible;
  if (doc_size) *doc_size = db->visible + (db->has_virtual ? 1 : 0);
  return SLSLAM_OK;
}

extern "C" int slslam_place_db_virtual(const slslam_place_db* db, int* words, int* num) {
  if (!db) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (words) std::copy(db->vwords.begin(), db->vwords.end(), words);
  if (num) *num = (int)db->vwords.size();
  return SLSLAM_OK;
}

extern "C" int slslam_place_db_stats(const slslam_place_db* db, long long* calls, long long* allocations) {
  return slslam::handle_stats(db, calls, allocations);
}

extern "C" int slslam_place_db_insert(slslam_place_db* db, const slslam_place_frame* frame, int* status, int* words) {
  if (!db || !frame || !frame_valid(*frame, db->max_words)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (db->inserted >= db->max_docs) return SLSLAM_ERR_STATE;
  int rc = ensure_device(db);
  if (rc != SLSLAM_OK) return rc;
  ++db->calls;
  const size_t mw = (size_t)db->max_words;
  const int n = frame->num_descriptors;
  const CallLayout y = call_layout(sizeof(Frame), 1, (size_t)n * (size_t)db->tree->D, mw, 1, 0);
  int st = SLSLAM_PLACE_OK;
  stage_frames(db, 1, frame, y, &st);
  if (status) *status = st;
  if (st != SLSLAM_PLACE_OK) {
    if (words) std::fill(words, words + n, -1);
    return SLSLAM_OK;
  }
  try {
    db->doc_words.reserve((size_t)db->inserted + 1);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  hipStream_t s = db->stream;
  char* h = db->h_block.p;
  char* dv = db->d_block.p;
  char* dd = db->d_db.p;
  HIP_TRY(hipMemcpyAsync(dv, h, y.in_bytes, hipMemcpyHostToDevice, s));
  const QueryOut o = query_out(dv, y);
  const Tree tree = device_tree(db->tree);
  hipLaunchKernelGGL(k_place_document, dim3(1), dim3(kDocThreads), 4 * (size_t)tree.K * (size_t)tree.D, s, tree,
                     reinterpret_cast<const Frame*>(dv), reinterpret_cast<const float*>(dv + y.off_desc), db->max_words, o, db->inserted,
                     (long long)db->max_docs, reinterpret_cast<int*>(dd + db->dl.o_word), reinterpret_cast<float*>(dd + db->dl.o_tf),
                     reinterpret_cast<int*>(dd + db->dl.o_n));
  HIP_TRY(hipGetLastError());
  char* h_out = h + align256(y.in_bytes);
  HIP_TRY(hipMemcpyAsync(h_out, dv + y.off_out, y.doc_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int nw = *reinterpret_cast<const int*>(h_out);
  const int* dw = reinterpret_cast<const int*>(h_out + y.o_dword);
  if (words) std::memcpy(words, h_out + y.o_words, 4 * (size_t)n);
  try {
    db->doc_words.emplace_back(dw, dw + nw);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  ++db->inserted;
  // the reference's doc_buffer: the front is released while more than `recent` documents are pending behind it
  while (db->inserted - db->visible - 1 > db->recent) {
    try {
      rc = release_front(db);
    } catch (const std::bad_alloc&) {
      rc = SLSLAM_ERR_NO_MEMORY;
    }
    if (rc != SLSLAM_OK) return rc;
  }
  return SLSLAM_OK;
}

extern "C" int slslam_place_db_run(slslam_place_db* db, int num_frames, const slslam_place_frame* frames, int top_k,
                                   slslam_place_result* out) {
  // ---- every argument before anything is written or the device is asked
  if (!db || num_frames < 0 || num_frames > db->max_frames || (num_frames > 0 && (!frames || !out)) || top_k < 0 || top_k > kMaxTopK)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  for (int f = 0; f < F; ++f)
    if (!frame_valid(frames[f], db->max_words)) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = ensure_device(db);
  if (rc != SLSLAM_OK) return rc;
  ++db->calls;
  if (F == 0) return SLSLAM_OK;

  const size_t mw = (size_t)db->max_words, S = (size_t)db->visible + 1, tk = (size_t)top_k;
  size_t nfloats = 0;
  for (int f = 0; f < F; ++f) nfloats += (size_t)frames[f].num_descriptors * (size_t)db->tree->D;
  const CallLayout y = call_layout(sizeof(Frame), (size_t)F, nfloats, mw, S, tk);
  std::vector<int> status((size_t)F);
  const size_t staged = stage_frames(db, F, frames, y, status.data());

  hipStream_t s = db->stream;
  char* h = db->h_block.p;
  char* dv = db->d_block.p;
  char* dd = db->d_db.p;
  const DbLayout& dl = db->dl;
  HIP_TRY(hipMemcpyAsync(dv, h, y.off_desc + 4 * staged, hipMemcpyHostToDevice, s));
  const Frame* d_fr = reinterpret_cast<const Frame*>(dv);
  const QueryOut o = query_out(dv, y);
  const Tree tree = device_tree(db->tree);
  Db g;
  g.cap = db->max_docs;
  g.word = reinterpret_cast<const int*>(dd + dl.o_word);
  g.tf = reinterpret_cast<const float*>(dd + dl.o_tf);
  g.n = reinterpret_cast<const int*>(dd + dl.o_n);
  g.df = reinterpret_cast<const int*>(dd + dl.o_df);
  g.idf = reinterpret_cast<const float*>(dd + dl.o_idf);
  g.vword = reinterpret_cast<const int*>(dd + dl.o_vword);
  g.navg = db->navg;
  g.vtf = 1.0f / (float)db->navg;
  g.visible = db->visible;
  g.has_virtual = db->has_virtual ? 1 : 0;
  const int scored = g.visible + g.has_virtual;

  hipLaunchKernelGGL(k_place_document, dim3((unsigned)F), dim3(kDocThreads), 4 * (size_t)tree.K * (size_t)tree.D, s, tree, d_fr,
                     reinterpret_cast<const float*>(dv + y.off_desc), db->max_words, o, -1, 0LL, (int*)nullptr, (float*)nullptr,
                     (int*)nullptr);
  if (g.visible > 0)
    hipLaunchKernelGGL(k_place_score, dim3((unsigned)((scored + 63) / 64), (unsigned)F), dim3(64), 0, s, d_fr, g, db->max_words, o);
  hipLaunchKernelGGL(k_place_finish, dim3((unsigned)F), dim3(kFinishThreads), 0, s, d_fr, g.visible, g.has_virtual, top_k, o);
  HIP_TRY(hipGetLastError());

  // ---- one download
  char* h_out = h + align256(y.in_bytes);
  HIP_TRY(hipMemcpyAsync(h_out, dv + y.off_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int f = 0; f < F; ++f) {
    slslam_place_result& r = out[f];
    const size_t n = (size_t)frames[f].num_descriptors;
    r.status = status[(size_t)f] == SLSLAM_PLACE_OK && db->visible == 0 ? SLSLAM_PLACE_EMPTY : status[(size_t)f];
    r.num_states = (int)S;
    r.has_virtual = g.has_virtual;
    if (r.words && n > 0) std::memcpy(r.words, h_out + y.o_words + 4 * (size_t)f * mw, 4 * n);
    if (r.score) std::memcpy(r.score, h_out + y.o_score + 4 * (size_t)f * S, 4 * S);
    if (r.likelihood) std::memcpy(r.likelihood, h_out + y.o_lik + 4 * (size_t)f * S, 4 * S);
    if (r.touched) std::memcpy(r.touched, h_out + y.o_touched + (size_t)f * S, S);
    if (r.top_id && tk > 0) std::memcpy(r.top_id, h_out + y.o_topid + 4 * (size_t)f * tk, 4 * tk);
    if (r.top_score && tk > 0) std::memcpy(r.top_score, h_out + y.o_topscore + 4 * (size_t)f * tk, 4 * tk);
  }
  return SLSLAM_OK;
}

// slslam_amd/csrc/place_recognition.h — the device half of the place recogniser (include/slslam_hip.h: slslam_voctree_*, slslam_place_db_*;
// DESIGN.md 6.4): vocabulary-tree words of line descriptors, a frame's document, tf-idf scores against every visible document and the
// likelihoods the Bayes filter (host/place_filter.h) takes.  After the reference's src/voctree_bf.h (find_leaf, insert_doc, query_doc),
// which the reference never compiled in; the contract and the departures from that file are in the header.
//   k_place_document   block <-> frame, thread <-> descriptor: the word of every descriptor (root node in LDS, deeper nodes gathered), a
//                      bitonic sort of the block's words in LDS, run lengths -> the document (distinct words ascending, tf); for an
//                      insert also written into the database's column
//   k_place_scatter    df changes of a visibility change (word, value) into the per-word df array
//   k_place_score      lane <-> scored state, the frame in grid y: the state's sorted words looked up in the query's sorted words (LDS)
//                      in ascending word order -> score, touched, the double sum of the terms; no atomics, so the order is the contract's
//   k_place_finish     block <-> frame: the ordered fill sum, the fill, mean and sigma, likelihoods, the top_k documents
// Every float operation of the contract is rounded on its own: contraction is off for the whole file.
#ifndef SLSLAM_PLACE_RECOGNITION_H_
#define SLSLAM_PLACE_RECOGNITION_H_

#include <hip/hip_runtime.h>

#pragma STDC FP_CONTRACT OFF

namespace slslam_place {

constexpr int kMaxK = 64, kMaxL = 4, kMaxD = 128, kMaxWords = 512, kMaxTopK = 32;
constexpr int kDocThreads = 512;        // = kMaxWords: thread <-> descriptor
constexpr int kFinishThreads = 256;
constexpr int kFillChunk = 1024;        // states the ordered fill sum takes through LDS at a time
constexpr int kChildBlock = 8;          // children whose distances a lane carries at a time: the descriptor is read K / 8 times per level

struct Tree {
  int K, L, D;
  const float* nodes;                   // [(K^L - 1) / (K - 1)][K][D]
};

struct Frame {
  int n;                                // descriptors
  int run;                              // 1: quantise and score (n > 0, every float finite)
  long long desc;                       // float offset of its [n D] descriptors in the upload
};

// the database on the device; documents are columns (word j of document d at j * cap + d): the lanes of k_place_score, one document
// each, read neighbouring addresses while they advance together
struct Db {
  long long cap;                        // max_docs
  const int* word;                      // [max_words][cap]
  const float* tf;                      // [max_words][cap]
  const int* n;                         // [cap] distinct words
  const int* df;                        // [K^L] with the virtual document counted
  const float* idf;                     // [doc_size + 1] by df; idf[0] = 0
  const int* vword;                     // [navg] the virtual document, ascending
  int navg;
  float vtf;                            // 1.0f / navg
  int visible, has_virtual;
};

struct QueryOut {
  int* words;                           // [F][max_words]
  int* doc_n;                           // [F]
  int* doc_word;                        // [F][max_words]
  float* doc_tf;                        // [F][max_words]
  float* score;                         // [F][S], S = visible + 1, index 0 = state -1
  float* likelihood;                    // [F][S]
  unsigned char* touched;               // [F][S]
  double* dsum;                         // [F][S] work: the double sum of a state's terms
  int* top_id;                          // [F][top_k]
  float* top_score;                     // [F][top_k]
};

// the child of `node` nearest to f by r = 1 - <c, f>, evaluated as the contract says; ties to the lowest child
__device__ inline int nearest_child(const float* node, const float* f, int K, int D) {
  float best = 0.0f;
  int arg = 0;
  for (int c0 = 0; c0 < K; c0 += kChildBlock) {
    const float* cp[kChildBlock];
    float r[kChildBlock];
#pragma unroll
    for (int j = 0; j < kChildBlock; ++j) {
      const int c = c0 + j < K ? c0 + j : K - 1;               // (past the last child: a copy of it, never compared)
      cp[j] = node + (size_t)c * D;
      r[j] = 1.0f;
    }
    for (int i = 0; i < D; ++i) {
      const float fi = f[i];
#pragma unroll
      for (int j = 0; j < kChildBlock; ++j) {
        const float p = cp[j][i] * fi;
        r[j] = r[j] - p;
      }
    }
#pragma unroll
    for (int j = 0; j < kChildBlock; ++j) {
      const int c = c0 + j;
      if (c == 0) best = r[0];
      else if (c < K && r[j] < best) { best = r[j]; arg = c; }
    }
  }
  return arg;
}

// The kernels are static: voctree_train.h includes this header for nearest_child, in a second translation unit.
// grid F, block kDocThreads, dynamic LDS K D floats.  db_slot >= 0 (F = 1, an insert): the document also goes into that column.
static __global__ __launch_bounds__(kDocThreads) void k_place_document(Tree tree, const Frame* __restrict__ frames,
                                                                       const float* __restrict__ desc, int max_words, QueryOut o, int db_slot,
                                                                       long long db_cap, int* __restrict__ db_word, float* __restrict__ db_tf,
                                                                       int* __restrict__ db_n) {
  extern __shared__ float s_root[];
  __shared__ int s_w[kDocThreads];
  __shared__ int s_start[kDocThreads + 1];
  __shared__ int s_cnt[kDocThreads / 64];
  const int f = blockIdx.x, t = threadIdx.x;
  const Frame fr = frames[f];
  if (!fr.run) {                                               // uniform over the block
    if (t == 0) o.doc_n[f] = 0;
    if (t < fr.n) o.words[(size_t)f * max_words + t] = -1;
    return;
  }
  const int K = tree.K, D = tree.D, n = fr.n;
  for (int i = t; i < K * D; i += kDocThreads) s_root[i] = tree.nodes[i];
  __syncthreads();

  int word = 0x7fffffff;                                       // threads without a descriptor sort behind every word
  if (t < n) {
    const float* fp = desc + fr.desc + (size_t)t * D;
    size_t idx = (size_t)nearest_child(s_root, fp, K, D) + 1;
    size_t num_int = 1, level = 1;
    for (int lvl = 1; lvl < tree.L; ++lvl) {
      idx = idx * K + (size_t)nearest_child(tree.nodes + idx * K * D, fp, K, D) + 1;
      level *= K;
      num_int += level;
    }
    word = (int)(idx - num_int);
    o.words[(size_t)f * max_words + t] = word;
  }
  s_w[t] = word;
  __syncthreads();
  for (int k = 2; k <= kDocThreads; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int p = t ^ j;
      if (p > t) {
        const int a = s_w[t], b = s_w[p];
        if ((a > b) == ((t & k) == 0)) { s_w[t] = b; s_w[p] = a; }
      }
      __syncthreads();
    }

  // run lengths: thread t starts a run when its word differs from the one before
  const bool start = t < n && (t == 0 || s_w[t] != s_w[t - 1]);
  const unsigned long long bal = __ballot(start);
  const int lane = t & 63, wv = t >> 6;
  if (lane == 0) s_cnt[wv] = __popcll(bal);
  __syncthreads();
  int base = 0, runs = 0;
  for (int w = 0; w < kDocThreads / 64; ++w) {
    if (w < wv) base += s_cnt[w];
    runs += s_cnt[w];
  }
  if (start) s_start[base + __popcll(bal & ((1ull << lane) - 1ull))] = t;
  if (t == 0) { s_start[runs] = n; o.doc_n[f] = runs; }
  __syncthreads();
  if (t < runs) {
    const int b = s_start[t], w = s_w[b];
    const float tf = __fdiv_rn((float)(s_start[t + 1] - b), (float)n);
    o.doc_word[(size_t)f * max_words + t] = w;
    o.doc_tf[(size_t)f * max_words + t] = tf;
    if (db_slot >= 0) {
      db_word[(size_t)t * db_cap + db_slot] = w;
      db_tf[(size_t)t * db_cap + db_slot] = tf;
    }
  }
  if (db_slot >= 0 && t == 0) db_n[db_slot] = runs;
}

static __global__ __launch_bounds__(256) void k_place_scatter(int num, const int* __restrict__ word, const int* __restrict__ value,
                                                              int* __restrict__ df) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < num) df[word[i]] = value[i];
}

// grid (ceil(scored states / 64), F), block 64
static __global__ __launch_bounds__(64) void k_place_score(const Frame* __restrict__ frames, Db db, int max_words, QueryOut o) {
  __shared__ int s_qw[kMaxWords];
  __shared__ float s_qtf[kMaxWords];
  const int f = blockIdx.y, lane = threadIdx.x;
  if (!frames[f].run) return;
  const int nq = o.doc_n[f];
  for (int i = lane; i < nq; i += 64) {
    s_qw[i] = o.doc_word[(size_t)f * max_words + i];
    s_qtf[i] = o.doc_tf[(size_t)f * max_words + i];
  }
  __syncthreads();
  const int scored = db.visible + db.has_virtual;
  const int st = blockIdx.x * 64 + lane;
  if (st >= scored) return;
  const int d = st - db.has_virtual;                           // -1: the virtual document
  const int nd = d < 0 ? db.navg : db.n[d];
  const int* wp = d < 0 ? db.vword : db.word + d;
  const float* tp = db.tf + (d < 0 ? 0 : d);
  const size_t stride = d < 0 ? 1 : (size_t)db.cap;
  float s = 0.0f;
  double ds = 0.0;
  int touched = 0;
  for (int j = 0; j < nd; ++j) {
    const int w = wp[j * stride];
    int lo = 0, hi = nq;
    while (lo < hi) {                                          // first query word >= w
      const int mid = (lo + hi) >> 1;
      if (s_qw[mid] < w) lo = mid + 1;
      else hi = mid;
    }
    if (lo < nq && s_qw[lo] == w) {
      const float idf = db.idf[db.df[w]];
      const float tfd = d < 0 ? db.vtf : tp[j * stride];
      const float n = s_qtf[lo] * idf;
      const float m = tfd * idf;
      const float l = -((fabsf(n - m) - n) - m);
      s = s + l;
      ds = ds + (double)l;
      touched = 1;
    }
  }
  const size_t oi = (size_t)f * (db.visible + 1) + (size_t)(d + 1);
  o.score[oi] = s;
  o.touched[oi] = (unsigned char)touched;
  o.dsum[oi] = ds;
}

// grid F, block kFinishThreads
static __global__ __launch_bounds__(kFinishThreads) void k_place_finish(const Frame* __restrict__ frames, int visible, int has_virtual,
                                                                        int top_k, QueryOut o) {
  __shared__ double s_d[kFillChunk];
  __shared__ double s_r0[kFinishThreads], s_r1[kFinishThreads];
  __shared__ unsigned long long s_key[kFinishThreads];
  __shared__ int s_touched;
  __shared__ double s_fill_sum;
  const int f = blockIdx.x, t = threadIdx.x;
  const int S = visible + 1;
  float* score = o.score + (size_t)f * S;
  float* lik = o.likelihood + (size_t)f * S;
  unsigned char* touched = o.touched + (size_t)f * S;
  if (!frames[f].run || visible == 0) {                         // EMPTY / INVALID_DESCRIPTOR: nothing is scored
    for (int i = t; i < S; i += kFinishThreads) { score[i] = 0.0f; lik[i] = 1.0f; touched[i] = 0; }
    for (int i = t; i < top_k; i += kFinishThreads) { o.top_id[(size_t)f * top_k + i] = -1; o.top_score[(size_t)f * top_k + i] = 0.0f; }
    return;
  }
  const int first = 1 - has_virtual;                            // the scored states are the indices first .. S - 1
  const double* dsum = o.dsum + (size_t)f * S;
  if (t == 0) { s_touched = 0; s_fill_sum = 0.0; }
  __syncthreads();

  // the fill: touched states counted by everyone, their double sums added by one thread in ascending state order
  int cnt = 0;
  for (int i = first + t; i < S; i += kFinishThreads) cnt += touched[i];
  if (cnt) atomicAdd(&s_touched, cnt);
  for (int c0 = first; c0 < S; c0 += kFillChunk) {
    const int m = S - c0 < kFillChunk ? S - c0 : kFillChunk;
    for (int i = t; i < m; i += kFinishThreads) s_d[i] = touched[c0 + i] ? dsum[c0 + i] : 0.0;
    __syncthreads();
    if (t == 0) {
      double a = s_fill_sum;
      for (int i = 0; i < m; ++i) a = a + s_d[i];             // (an untouched state adds +0.0: the sum does not change)
      s_fill_sum = a;
    }
    __syncthreads();
  }
  const float fill = (float)(s_fill_sum / (double)(1 + s_touched));

  // mean and sigma over the scored states after the fill
  double a0 = 0.0, a1 = 0.0;
  for (int i = first + t; i < S; i += kFinishThreads) {
    float s = score[i];
    if (!touched[i]) { s = fill; score[i] = s; }
    a0 += (double)s;
    a1 += (double)s * (double)s;
  }
  s_r0[t] = a0; s_r1[t] = a1;
  __syncthreads();
  for (int w = kFinishThreads / 2; w > 0; w >>= 1) {
    if (t < w) { s_r0[t] += s_r0[t + w]; s_r1[t] += s_r1[t + w]; }
    __syncthreads();
  }
  const double num = (double)(S - first);
  const double mean = s_r0[0] / num;
  const double sigma = sqrt(s_r1[0] / num - mean * mean);
  const double bar = mean + 2.0 * sigma;
  if (t == 0 && !has_virtual) { score[0] = 0.0f; lik[0] = 1.0f; touched[0] = 0; }
  for (int i = first + t; i < S; i += kFinishThreads) {
    const double s = (double)score[i];
    lik[i] = (mean != 0.0 && s > bar) ? (float)((s - 2.0 * sigma) / mean) : 1.0f;
  }
  __syncthreads();                                              // (s_r0 is read above and the filled scores below)

  // the top_k documents: round r takes the largest key below the last winner's; key = (score bits, ~document) - scores are >= +0
  unsigned long long below = ~0ull;
  for (int r = 0; r < top_k; ++r) {
    unsigned long long best = 0ull;
    for (int i = 1 + t; i < S; i += kFinishThreads) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(score[i]) << 32) | (unsigned)(0xffffffffu - (unsigned)(i - 1));
      if (key < below && key > best) best = key;
    }
    s_key[t] = best;
    __syncthreads();
    for (int w = kFinishThreads / 2; w > 0; w >>= 1) {
      if (t < w && s_key[t + w] > s_key[t]) s_key[t] = s_key[t + w];
      __syncthreads();
    }
    below = s_key[0];
    __syncthreads();
    if (t == 0) {
      const bool any = below != 0ull;                           // (a real key is never 0: its low word is ~document > 0)
      o.top_id[(size_t)f * top_k + r] = any ? (int)(0xffffffffu - (unsigned)(below & 0xffffffffu)) : -1;
      o.top_score[(size_t)f * top_k + r] = any ? __uint_as_float((unsigned)(below >> 32)) : 0.0f;
    }                                                           // (below == 0: no key is < 0, the rounds that follow find nothing)
  }
}

}  // namespace slslam_place

#endif  // SLSLAM_PLACE_RECOGNITION_H_

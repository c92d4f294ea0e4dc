// slslam_amd/csrc/descriptor_api.hip — the descriptor matcher (include/slslam_hip.h: slslam_descriptor_matcher_*, slslam_match_descriptors):
// the link between the place recogniser and the pose estimator in a loop closure.  The store keeps the descriptors of every inserted
// keyframe on the device, in the layout the pair kernel reads (groups of eight descriptors, [D][8] each, zeros past the last).  Per run,
// whatever the number of frames and candidates:
//   upload   one block [PairDesc P | floats: the descriptors of every query frame that runs, once per frame]
//   pairs    k_desc_pairs: every query descriptor against every descriptor of the candidate -> per query descriptor (best, second,
//            count), per keyframe descriptor the key of its best query descriptor
//   finish   k_mutual_finish (mutual_match.h): mutual and ratio tests, matches, num_matched
//   download one block [num_matched P | match, best, num_admissible, best_distance, second_distance: sum n each | best_query: sum m]
// The pair index lies in the grid.  The kernels are in descriptor_match.h, the scaffold in call_block.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "call_block.h"
#include "descriptor_match.h"

using namespace slslam_desc;
using slslam::device_present;
using slslam::kMaxGridY;

static_assert(kMaxD == SLSLAM_DESC_MAX_D && kMaxDescriptors == SLSLAM_DESC_MAX_DESCRIPTORS && kMaxCandidates == SLSLAM_DESC_MAX_CANDIDATES,
              "the header's limits are the kernels'");

namespace {

// Where everything of a run lies: the upload (the same offsets on the host and on the device), the device's keys behind it, and the
// result block (on the host behind the upload)
struct CallLayout {
  size_t off_f = 0, in_bytes = 0;                        // upload: PairDesc[P] at 0, floats at off_f
  size_t off_keys = 0, off_out = 0;
  slslam::MatchBlock out;
  slslam::BlockBytes bytes;
};

CallLayout call_layout(size_t P, size_t nfloats, size_t Atot, size_t Jtot) {
  CallLayout y;
  slslam::Carve c;
  c.take(sizeof(PairDesc) * P);
  y.off_f = c.take(4 * nfloats);
  y.in_bytes = y.off_f + 4 * nfloats;
  y.out = slslam::match_block(P, Atot, Jtot);
  y.bytes.host = c.at + y.out.bytes;
  y.off_keys = c.take(8 * Jtot);
  y.off_out = c.at;
  y.bytes.dev = y.off_out + y.out.bytes;
  return y;
}

bool all_finite(const float* p, size_t cnt) {
  for (size_t i = 0; i < cnt; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

struct slslam_descriptor_matcher : slslam::Handle {
  int D = 0, max_keyframes = 0, max_descriptors = 0, max_frames = 0, max_candidates = 0;
  int inserted = 0;
  size_t slot_floats = 0;                                // ceil(max_descriptors / 8) groups of [D][8]
  std::vector<int> counts;                               // descriptors of every inserted keyframe
  slslam::BlockPair store;                               // the keyframes on the device; one keyframe on its way there
  slslam::BlockPair block;                               // a run
};

namespace {

bool query_valid(const slslam_descriptor_matcher* m, const slslam_descriptor_query& q) {
  if (q.num_descriptors < 0 || q.num_descriptors > m->max_descriptors || (q.num_descriptors > 0 && !q.descriptors)) return false;
  if (q.num_candidates < 0 || q.num_candidates > m->max_candidates || (q.num_candidates > 0 && !q.candidates)) return false;
  for (int c = 0; c < q.num_candidates; ++c)
    if (q.candidates[c] < -1 || q.candidates[c] >= m->inserted) return false;
  return true;
}

}  // namespace

extern "C" int slslam_descriptor_matcher_create(int device, int D, int max_keyframes, int max_descriptors, int max_frames, int max_candidates,
                                                slslam_descriptor_matcher** out) {
  if (!out || D < 1 || D > kMaxD || max_keyframes < 1 || max_descriptors < 1 || max_descriptors > kMaxDescriptors || max_frames < 1 ||
      max_candidates < 1 || max_candidates > kMaxCandidates)
    return SLSLAM_ERR_INVALID_ARGUMENT;
  slslam_descriptor_matcher* m = new (std::nothrow) slslam_descriptor_matcher();
  if (!m) return SLSLAM_ERR_NO_MEMORY;
  m->device = device;
  m->D = D; m->max_keyframes = max_keyframes; m->max_descriptors = max_descriptors; m->max_frames = max_frames;
  m->max_candidates = max_candidates;
  m->slot_floats = (size_t)((max_descriptors + kGroup - 1) / kGroup) * group_floats(D);
  try {
    m->counts.reserve((size_t)max_keyframes);
  } catch (const std::bad_alloc&) {
    delete m;
    return SLSLAM_ERR_NO_MEMORY;
  }
  *out = m;
  return SLSLAM_OK;
}

extern "C" void slslam_descriptor_matcher_destroy(slslam_descriptor_matcher* m) { delete m; }

extern "C" int slslam_descriptor_matcher_size(const slslam_descriptor_matcher* m, int* inserted) {
  if (!m) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (inserted) *inserted = m->inserted;
  return SLSLAM_OK;
}

extern "C" int slslam_descriptor_matcher_stats(const slslam_descriptor_matcher* m, long long* calls, long long* allocations) {
  return slslam::handle_stats(m, calls, allocations);
}

extern "C" int slslam_descriptor_matcher_insert(slslam_descriptor_matcher* m, int n, const float* descriptors, int* status, int* id) {
  if (!m || n < 0 || n > m->max_descriptors || (n > 0 && !descriptors)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (m->inserted >= m->max_keyframes) return SLSLAM_ERR_STATE;
  int rc = m->ensure();
  if (rc != SLSLAM_OK) return rc;
  ++m->calls;
  const int D = m->D;
  const int st = n == 0 ? SLSLAM_DESC_EMPTY : all_finite(descriptors, (size_t)n * (size_t)D) ? SLSLAM_DESC_OK : SLSLAM_DESC_INVALID_DESCRIPTOR;
  if (status) *status = st;
  if (id) *id = st == SLSLAM_DESC_OK ? m->inserted : -1;
  if (st != SLSLAM_DESC_OK) return SLSLAM_OK;
  const slslam::BlockBytes store = { 4 * m->slot_floats * (size_t)m->max_keyframes, 4 * m->slot_floats };
  if ((rc = m->store.fit(store, store, &m->allocations)) != SLSLAM_OK) return rc;
  // the keyframe as the pair kernel reads it: descriptor j, value i at group j / 8, [i][j % 8]; zeros past n
  float* h = reinterpret_cast<float*>(m->store.host.p);
  const size_t used = (size_t)((n + kGroup - 1) / kGroup) * group_floats(D);
  std::memset(h, 0, 4 * used);
  for (int j = 0; j < n; ++j) {
    float* g = h + (size_t)(j / kGroup) * group_floats(D) + (size_t)(j % kGroup);
    const float* src = descriptors + (size_t)j * D;
    for (int i = 0; i < D; ++i) g[(size_t)i * kGroup] = src[i];
  }
  float* slot = reinterpret_cast<float*>(m->store.dev.p) + m->slot_floats * (size_t)m->inserted;
  HIP_TRY(hipMemcpyAsync(slot, h, 4 * used, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->counts.push_back(n);                                  // (reserved at create)
  ++m->inserted;
  return SLSLAM_OK;
}

extern "C" int slslam_descriptor_matcher_run(slslam_descriptor_matcher* m, int num_frames, const slslam_descriptor_query* queries,
                                             double ratio, double max_distance, int num_pairs, slslam_descriptor_result* out) {
  // ---- every argument before anything is written or the device is asked
  if (!m || num_frames < 0 || num_pairs < 0 || (num_frames > 0 && !queries) || (num_pairs > 0 && !out)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (std::isnan(ratio) || std::isnan(max_distance)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const int F = num_frames;
  long long pairs = 0;
  for (int f = 0; f < F; ++f) {
    if (!query_valid(m, queries[f])) return SLSLAM_ERR_INVALID_ARGUMENT;
    pairs += queries[f].num_candidates;
  }
  if (pairs != num_pairs) return SLSLAM_ERR_INVALID_ARGUMENT;
  int rc = m->ensure();
  if (rc != SLSLAM_OK) return rc;
  hipStream_t s = m->stream;
  ++m->calls;
  const int P = num_pairs;
  if (P == 0) return SLSLAM_OK;

  // ---- layout
  const int D = m->D;
  std::vector<PairDesc> pd((size_t)P);
  std::vector<int> status((size_t)P);
  std::vector<char> frame_ok((size_t)F);
  size_t nfloats = 0, Atot = 0, Jtot = 0;
  int maxN = 0, maxM = 0, p = 0;
  for (int f = 0; f < F; ++f) {
    const slslam_descriptor_query& q = queries[f];
    const int n = q.num_descriptors;
    const size_t cnt = (size_t)n * (size_t)D;
    const int fst = n == 0 ? SLSLAM_DESC_EMPTY : all_finite(q.descriptors, cnt) ? SLSLAM_DESC_OK : SLSLAM_DESC_INVALID_DESCRIPTOR;
    frame_ok[(size_t)f] = fst == SLSLAM_DESC_OK && q.num_candidates > 0;
    for (int c = 0; c < q.num_candidates; ++c, ++p) {
      const int kf = q.candidates[c];
      PairDesc& d = pd[(size_t)p];
      d.q = (long long)nfloats;
      d.k = kf >= 0 ? (long long)(m->slot_floats * (size_t)kf) : 0;
      d.span.n = n; d.span.m = kf >= 0 ? m->counts[(size_t)kf] : 0;
      d.span.a0 = (long long)Atot; d.span.j0 = (long long)Jtot;
      status[(size_t)p] = fst != SLSLAM_DESC_OK ? fst : kf < 0 ? SLSLAM_DESC_EMPTY : SLSLAM_DESC_OK;
      d.run = status[(size_t)p] == SLSLAM_DESC_OK ? 1 : 0;
      d.pad = 0;
      Atot += (size_t)n; Jtot += (size_t)d.span.m;
      maxN = std::max(maxN, n); maxM = std::max(maxM, d.span.m);
    }
    if (frame_ok[(size_t)f]) nfloats += cnt;
  }
  // the blocks: made for the matcher's capacity at the first run, larger only when a call exceeds them
  const size_t capF = (size_t)std::max(F, m->max_frames), capP = capF * (size_t)m->max_candidates, md = (size_t)m->max_descriptors;
  const CallLayout y = call_layout((size_t)P, nfloats, Atot, Jtot);
  if ((rc = m->block.fit(call_layout(capP, capF * md * (size_t)D, capP * md, capP * md).bytes, y.bytes, &m->allocations)) != SLSLAM_OK) return rc;

  // ---- one upload
  char* h = m->block.host.p;
  char* dv = m->block.dev.p;
  std::memcpy(h, pd.data(), sizeof(PairDesc) * (size_t)P);
  float* hf = reinterpret_cast<float*>(h + y.off_f);
  size_t at = 0;
  for (int f = 0; f < F; ++f) {
    if (!frame_ok[(size_t)f]) continue;
    const size_t cnt = (size_t)queries[f].num_descriptors * (size_t)D;
    std::memcpy(hf + at, queries[f].descriptors, 4 * cnt);
    at += cnt;
  }
  HIP_TRY(hipMemcpyAsync(dv, h, y.in_bytes, hipMemcpyHostToDevice, s));
  const PairDesc* d_pd = reinterpret_cast<const PairDesc*>(dv);
  const float* d_qd = reinterpret_cast<const float*>(dv + y.off_f);
  const float* d_store = reinterpret_cast<const float*>(m->store.dev.p);    // (NULL before the first insert: then no pair runs)
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(dv + y.off_keys);
  char* d_out = dv + y.off_out;
  const Out o = slslam::match_bind(d_out, y.out);
  if ((rc = slslam::match_clear(o, (size_t)P, d_keys, Jtot, s)) != SLSLAM_OK) return rc;

  // ---- two launches for all pairs
  const unsigned tn = (unsigned)((maxN + 63) / 64), tm = (unsigned)((maxM + 63) / 64);
  for (int p0 = 0; p0 < P; p0 += kMaxGridY) {
    const unsigned np = (unsigned)std::min(P - p0, kMaxGridY);
    Out op = o;
    op.num_matched += p0;
    if (tn > 0)
      hipLaunchKernelGGL(k_desc_pairs, dim3(tn, np), dim3(64), pairs_lds_bytes(D), s, d_pd + p0, d_qd, d_store, D, max_distance, d_keys, op);
    if (std::max(tn, tm) > 0)
      hipLaunchKernelGGL(slslam::k_mutual_finish<PairDesc>, dim3(std::max(tn, tm), np), dim3(64), 0, s, d_pd + p0,
                         (const unsigned long long*)d_keys, ratio, op);
  }
  HIP_TRY(hipGetLastError());

  // ---- one download
  char* h_out = h + slslam::align256(y.in_bytes);
  if ((rc = slslam::match_download(h_out, d_out, y.out, s)) != SLSLAM_OK) return rc;
  for (p = 0; p < P; ++p) {
    const slslam::Span& sp = pd[(size_t)p].span;
    slslam_descriptor_result& r = out[p];
    r.status = status[(size_t)p];
    r.num_keyframe_descriptors = sp.m;
    r.num_matched = slslam::match_scatter(h_out, y.out, (size_t)p, sp,
                                          {r.match, r.best, r.best_distance, r.second_distance, r.num_admissible, r.best_query});
  }
  return SLSLAM_OK;
}

extern "C" int slslam_match_descriptors(int D, int n, const float* query, int m, const float* keyframe, double ratio, double max_distance,
                                        slslam_descriptor_result* out) {
  if (!out || D < 1 || D > kMaxD || n < 0 || n > kMaxDescriptors || m < 0 || m > kMaxDescriptors || (n > 0 && !query) ||
      (m > 0 && !keyframe) || std::isnan(ratio) || std::isnan(max_distance))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  slslam_descriptor_matcher* h = nullptr;
  int rc = slslam_descriptor_matcher_create(-1, D, 1, std::max(std::max(n, m), 1), 1, 1, &h);
  int st = SLSLAM_DESC_EMPTY, id = -1;
  if (rc == SLSLAM_OK) rc = slslam_descriptor_matcher_insert(h, m, keyframe, &st, &id);
  if (rc == SLSLAM_OK) {
    const slslam_descriptor_query q = { n, query, 1, &id };
    rc = slslam_descriptor_matcher_run(h, 1, &q, ratio, max_distance, 1, out);
    // a keyframe the store refuses for a non-finite float: the pair ran against candidate -1, and says why
    if (rc == SLSLAM_OK && st == SLSLAM_DESC_INVALID_DESCRIPTOR) out->status = SLSLAM_DESC_INVALID_DESCRIPTOR;
  }
  slslam_descriptor_matcher_destroy(h);
  return rc;
}

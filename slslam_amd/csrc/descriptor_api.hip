// slslam_amd/csrc/descriptor_api.hip — the descriptor matcher (include/slslam_hip.h: slslam_descriptor_matcher_*, slslam_match_descriptors):
// the link between the place recogniser and the pose estimator in a loop closure.  The store keeps the descriptors of every inserted
// keyframe on the device, in the layout the pair kernel reads (groups of eight descriptors, [D][8] each, zeros past the last).  Per run,
// whatever the number of frames and candidates:
//   upload   one block [PairDesc P | floats: the descriptors of every query frame that runs, once per frame]
//   pairs    k_desc_pairs: every query descriptor against every descriptor of the candidate -> per query descriptor (best, second,
//            count), per keyframe descriptor the key of its best query descriptor
//   finish   k_desc_finish: mutual and ratio tests, matches, num_matched
//   download one block [num_matched P | match, best, num_admissible, best_distance, second_distance: sum n each | best_query: sum m]
// The pair index lies in the grid.  The kernels are in descriptor_match.h.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/slslam_hip.h"
#include "descriptor_match.h"
#include "grow_buf.h"
#include "hip_status.h"

using namespace slslam_desc;
using slslam::align256;
using slslam::GrowBuf;
using slslam::Mem;

static_assert(kMaxD == SLSLAM_DESC_MAX_D && kMaxDescriptors == SLSLAM_DESC_MAX_DESCRIPTORS && kMaxCandidates == SLSLAM_DESC_MAX_CANDIDATES,
              "the header's limits are the kernels'");

namespace {

constexpr int kMaxGrid = 65535;         // what the y dimension of a grid takes: pairs go in slices of it

// Where everything of a run lies: the upload (the same offsets on the host and on the device), the device's keys behind it, and the
// result block (the same offsets on the device and on the host)
struct Layout {
  size_t off_f = 0, in_bytes = 0;                        // upload: PairDesc[P] at 0, floats at off_f
  size_t off_keys = 0, off_out = 0, dev_bytes = 0;
  size_t o_match = 0, o_best = 0, o_count = 0, o_bd = 0, o_sd = 0, o_bq = 0, out_bytes = 0;     // in the result block; num_matched[P] at 0
  size_t host_bytes = 0;                                 // upload, then the result block at align256(in_bytes)
};

Layout make_layout(size_t P, size_t nfloats, size_t Atot, size_t Jtot) {
  Layout y;
  y.off_f = align256(sizeof(PairDesc) * P);
  y.in_bytes = y.off_f + 4 * nfloats;
  y.o_match = align256(4 * P);
  y.o_best = y.o_match + align256(4 * Atot);
  y.o_count = y.o_best + align256(4 * Atot);
  y.o_bd = y.o_count + align256(4 * Atot);
  y.o_sd = y.o_bd + align256(4 * Atot);
  y.o_bq = y.o_sd + align256(4 * Atot);
  y.out_bytes = y.o_bq + align256(4 * Jtot);
  y.off_keys = align256(y.in_bytes);
  y.off_out = y.off_keys + align256(8 * Jtot);
  y.dev_bytes = y.off_out + y.out_bytes;
  y.host_bytes = align256(y.in_bytes) + y.out_bytes;
  return y;
}

bool device_present() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

bool all_finite(const float* p, size_t cnt) {
  for (size_t i = 0; i < cnt; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

struct slslam_descriptor_matcher {
  int device = -1;
  int D = 0, max_keyframes = 0, max_descriptors = 0, max_frames = 0, max_candidates = 0;
  int inserted = 0;
  size_t slot_floats = 0;                                // ceil(max_descriptors / 8) groups of [D][8]
  std::vector<int> counts;                               // descriptors of every inserted keyframe
  GrowBuf d_store{Mem::kDevice}, h_slot{Mem::kPinned};   // the keyframes; one keyframe on its way there
  GrowBuf d_block{Mem::kDevice}, h_block{Mem::kPinned};  // a run
  hipStream_t stream = nullptr;
  long long calls = 0, allocations = 0;
  ~slslam_descriptor_matcher() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

int ensure_device(slslam_descriptor_matcher* m) {
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  if (m->device >= 0) HIP_TRY(hipSetDevice(m->device));
  else HIP_TRY(hipGetDevice(&m->device));
  if (!m->stream) HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  return SLSLAM_OK;
}

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
  if (!m) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (calls) *calls = m->calls;
  if (allocations) *allocations = m->allocations;
  return SLSLAM_OK;
}

extern "C" int slslam_descriptor_matcher_insert(slslam_descriptor_matcher* m, int n, const float* descriptors, int* status, int* id) {
  if (!m || n < 0 || n > m->max_descriptors || (n > 0 && !descriptors)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (m->inserted >= m->max_keyframes) return SLSLAM_ERR_STATE;
  int rc = ensure_device(m);
  if (rc != SLSLAM_OK) return rc;
  ++m->calls;
  const int D = m->D;
  const int st = n == 0 ? SLSLAM_DESC_EMPTY : all_finite(descriptors, (size_t)n * (size_t)D) ? SLSLAM_DESC_OK : SLSLAM_DESC_INVALID_DESCRIPTOR;
  if (status) *status = st;
  if (id) *id = st == SLSLAM_DESC_OK ? m->inserted : -1;
  if (st != SLSLAM_DESC_OK) return SLSLAM_OK;
  if (!m->d_store.p) {
    long long unused = 0;
    HIP_TRY(m->d_store.need(4 * m->slot_floats * (size_t)m->max_keyframes, &unused));
    HIP_TRY(m->h_slot.need(4 * m->slot_floats, &unused));
    ++m->allocations;
  }
  // the keyframe as the pair kernel reads it: descriptor j, value i at group j / 8, [i][j % 8]; zeros past n
  float* h = reinterpret_cast<float*>(m->h_slot.p);
  const size_t used = (size_t)((n + kGroup - 1) / kGroup) * group_floats(D);
  std::memset(h, 0, 4 * used);
  for (int j = 0; j < n; ++j) {
    float* g = h + (size_t)(j / kGroup) * group_floats(D) + (size_t)(j % kGroup);
    const float* src = descriptors + (size_t)j * D;
    for (int i = 0; i < D; ++i) g[(size_t)i * kGroup] = src[i];
  }
  float* slot = reinterpret_cast<float*>(m->d_store.p) + m->slot_floats * (size_t)m->inserted;
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
  int rc = ensure_device(m);
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
      d.n = n; d.m = kf >= 0 ? m->counts[(size_t)kf] : 0;
      d.a0 = (long long)Atot; d.j0 = (long long)Jtot;
      status[(size_t)p] = fst != SLSLAM_DESC_OK ? fst : kf < 0 ? SLSLAM_DESC_EMPTY : SLSLAM_DESC_OK;
      d.run = status[(size_t)p] == SLSLAM_DESC_OK ? 1 : 0;
      d.pad = 0;
      Atot += (size_t)n; Jtot += (size_t)d.m;
      maxN = std::max(maxN, n); maxM = std::max(maxM, d.m);
    }
    if (frame_ok[(size_t)f]) nfloats += cnt;
  }
  // the blocks: made for the matcher's capacity at the first run, larger only when a call exceeds them
  const size_t capF = (size_t)std::max(F, m->max_frames), capP = capF * (size_t)m->max_candidates, md = (size_t)m->max_descriptors;
  const Layout cap = make_layout(capP, capF * md * (size_t)D, capP * md, capP * md);
  const Layout y = make_layout((size_t)P, nfloats, Atot, Jtot);
  if (m->d_block.n < y.dev_bytes || m->h_block.n < y.host_bytes || !m->d_block.p || !m->h_block.p) {
    long long unused = 0;
    HIP_TRY(m->d_block.need(std::max(cap.dev_bytes, y.dev_bytes), &unused));
    HIP_TRY(m->h_block.need(std::max(cap.host_bytes, y.host_bytes), &unused));
    ++m->allocations;
  }

  // ---- one upload
  char* h = m->h_block.p;
  char* dv = m->d_block.p;
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
  const float* d_store = reinterpret_cast<const float*>(m->d_store.p);      // (NULL before the first insert: then no pair runs)
  unsigned long long* d_keys = reinterpret_cast<unsigned long long*>(dv + y.off_keys);
  char* d_out = dv + y.off_out;
  Out o;
  o.num_matched = reinterpret_cast<int*>(d_out);
  o.match = reinterpret_cast<int*>(d_out + y.o_match);
  o.best = reinterpret_cast<int*>(d_out + y.o_best);
  o.num_admissible = reinterpret_cast<int*>(d_out + y.o_count);
  o.best_distance = reinterpret_cast<float*>(d_out + y.o_bd);
  o.second_distance = reinterpret_cast<float*>(d_out + y.o_sd);
  o.best_query = reinterpret_cast<int*>(d_out + y.o_bq);
  HIP_TRY(hipMemsetAsync(o.num_matched, 0, 4 * (size_t)P, s));
  if (Jtot > 0) HIP_TRY(hipMemsetAsync(d_keys, 0xff, 8 * Jtot, s));

  // ---- two launches for all pairs
  const unsigned tn = (unsigned)((maxN + 63) / 64), tm = (unsigned)((maxM + 63) / 64);
  for (int p0 = 0; p0 < P; p0 += kMaxGrid) {
    const unsigned np = (unsigned)std::min(P - p0, kMaxGrid);
    Out op = o;
    op.num_matched += p0;
    if (tn > 0)
      hipLaunchKernelGGL(k_desc_pairs, dim3(tn, np), dim3(64), pairs_lds_bytes(D), s, d_pd + p0, d_qd, d_store, D, max_distance, d_keys, op);
    if (std::max(tn, tm) > 0)
      hipLaunchKernelGGL(k_desc_finish, dim3(std::max(tn, tm), np), dim3(64), 0, s, d_pd + p0, (const unsigned long long*)d_keys, ratio, op);
  }
  HIP_TRY(hipGetLastError());

  // ---- one download
  char* h_out = h + align256(y.in_bytes);
  HIP_TRY(hipMemcpyAsync(h_out, d_out, y.out_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int* r_nm = reinterpret_cast<const int*>(h_out);
  for (p = 0; p < P; ++p) {
    const PairDesc& d = pd[(size_t)p];
    slslam_descriptor_result& r = out[p];
    r.status = status[(size_t)p];
    r.num_matched = r_nm[p];
    r.num_keyframe_descriptors = d.m;
    const size_t nb = 4 * (size_t)d.n, no = 4 * (size_t)d.a0;
    if (r.match && d.n > 0) std::memcpy(r.match, h_out + y.o_match + no, nb);
    if (r.best && d.n > 0) std::memcpy(r.best, h_out + y.o_best + no, nb);
    if (r.num_admissible && d.n > 0) std::memcpy(r.num_admissible, h_out + y.o_count + no, nb);
    if (r.best_distance && d.n > 0) std::memcpy(r.best_distance, h_out + y.o_bd + no, nb);
    if (r.second_distance && d.n > 0) std::memcpy(r.second_distance, h_out + y.o_sd + no, nb);
    if (r.best_query && d.m > 0) std::memcpy(r.best_query, h_out + y.o_bq + 4 * (size_t)d.j0, 4 * (size_t)d.m);
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

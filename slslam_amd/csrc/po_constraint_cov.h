// slslam_amd/csrc/po_constraint_cov.h — the covariance of a constraint in the coordinates of its edge's error: slslam_po_constraint_covariance.
// What it serves: the R of po_gate.h.  A loop-closure edge of the reference is the output of pose_estimation on the matched lines
// (src/slam.cpp:1146-1155), here slslam_pose_estimator_run, whose covariance (slslam_pose_estimator_get_covariance) is over the
// constraint's own six parameters (w_C, t_C); the gate's S lives in the coordinates of Te = T_b^-1 o (C o T_a).  Part of po_api.hip's
// translation unit, behind po_gate.h.
//
// One item: poses x_a, x_b, a constraint C and its covariance Sigma_C (absent: zeros; the lower triangle is read).  With
// Te = pose_constraint_error(x_a, x_b, C) - the solve's functor, unwhitened - and J_C = dTe/dC by the dual numbers of po_kernels.h,
// seeded on C instead of on the poses:
//   cov_meas = sigma2 J_C Sigma_C J_C^T
// J_C is not the identity: C o T_a puts C's rotation in front of T_a's translation (the lever arm t_a) and T_b^-1 rotates the result,
// and the angle-axis coordinates of the composed rotation are not additive in those of C.
//
// k_po_constraint_cov: lane <-> (item, column d of J_C), six lanes per item, ten items per wave (lanes 60 .. 63 idle).  fp64, no
// atomics, every sum in a fixed order: the same bits run to run.
//   1  every lane evaluates the functor on duals seeded in its column: all six Te[q].v and its column Te[q].d      -> Js[item][d][.]  (LDS)
//   2  lane d: row d of Sigma_C (symmetrised from its lower triangle) times J_C^T                                   -> Vs[item][d][.]
//   3  the 21 entries of the lower triangle of J_C V, spread over the item's six lanes, summed over d = 0 .. 5,
//      times sigma2                                                                                                  -> Ss[item]  (mirrored)
//   4  all six lanes copy the item's results out
// LDS: 10 items x (36 + 36 + 36) doubles = 8640 bytes.
#ifndef SLSLAM_PO_CONSTRAINT_COV_H_
#define SLSLAM_PO_CONSTRAINT_COV_H_

namespace {

struct PoConsCovArrays {
  const double *pa, *pb, *c, *sc;                    // [6n] x 3, [36n] (sc may be null: zeros)
  int n;
  double sigma2;
  double *err, *jac, *cov;                           // [6n], [36n], [36n]
};

__global__ __launch_bounds__(64) void k_po_constraint_cov(PoConsCovArrays A) {
  const int lane = threadIdx.x;
  const int el = lane / 6, d = lane - 6 * el;
  const int e10 = el < 10 ? el : 9;                  // (lanes 60 .. 63 have no item: they read item 9's tiles and write nothing)
  const long long i = (long long)blockIdx.x * 10 + el;
  const bool ok = el < 10 && i < A.n;
  const size_t s = ok ? (size_t)i : 0;               // (the launch has n >= 1: item 0 exists)
  __shared__ double Js[10][6][6];
  __shared__ double Vs[10][6][6];
  __shared__ double Ss[10][36];
  const double *xa = A.pa + 6 * s, *xb = A.pb + 6 * s, *cc = A.c + 6 * s;
  const double* sc = A.sc ? A.sc + 36 * s : nullptr;
  Dual T1[6], T2[6], C[6], Te[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    T1[q] = mk(xa[q]);
    T2[q] = mk(xb[q]);
    C[q] = mk(cc[q], d == q ? 1.0 : 0.0);
  }
  pose_constraint_error<Dual>(T1, T2, C, Te);
  if (el < 10) {
#pragma unroll
    for (int q = 0; q < 6; ++q) Js[el][d][q] = Te[q].d;
  }
  __syncthreads();
  {
    double v[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int dp = 0; dp < 6; ++dp) {
      const double sg = sc ? sc[d >= dp ? 6 * d + dp : 6 * dp + d] : 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] = fma(sg, Js[e10][dp][q], v[q]);
    }
    if (el < 10) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Vs[el][d][q] = v[q];
    }
  }
  __syncthreads();
  for (int k = d; k < 21 && el < 10; k += 6) {       // entry k of the packed lower triangle: (p, q), q <= p
    int p = 0;
    while ((p + 1) * (p + 2) / 2 <= k) ++p;
    const int q = k - p * (p + 1) / 2;
    double t = 0.0;
    for (int dd = 0; dd < 6; ++dd) t = fma(Js[el][dd][p], Vs[el][dd][q], t);
    t = A.sigma2 * t;
    Ss[el][6 * p + q] = t;
    Ss[el][6 * q + p] = t;
  }
  __syncthreads();
  if (!ok) return;
  double* err = A.err + 6 * s;
  double* jac = A.jac + 36 * s;
  double* cov = A.cov + 36 * s;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    if (d == q) err[q] = Te[q].v;
    jac[6 * q + d] = Te[q].d;                        // J_C row-major: row q = component of Te, column d = parameter of C
  }
  for (int k = d; k < 36; k += 6) cov[k] = Ss[el][k];
}

}  // namespace

// n independent items: one upload, one launch, one download.
extern "C" int slslam_po_constraint_covariance(const slslam_po_constraint_items* it, double* error, double* jacobian, double* cov_meas) {
  if (!it || it->n < 0 || !po_sigma2_ok(it->sigma2)) return SLSLAM_ERR_INVALID_ARGUMENT;
  const size_t n = (size_t)it->n;
  if (n > 0 && (!it->pose_a || !it->pose_b || !it->constraints)) return SLSLAM_ERR_INVALID_ARGUMENT;
  if (!po_all_finite(it->pose_a, 6 * n) || !po_all_finite(it->pose_b, 6 * n) || !po_all_finite(it->constraints, 6 * n) ||
      !po_all_finite(it->cov_constraint, 36 * n))
    return SLSLAM_ERR_INVALID_ARGUMENT;
  if (n == 0) return SLSLAM_OK;
  if (!device_present()) return SLSLAM_ERR_NO_DEVICE;
  try {
    PoCarve a;
    const size_t o_pa = a.take(sizeof(double) * 6 * n), o_pb = a.take(sizeof(double) * 6 * n), o_c = a.take(sizeof(double) * 6 * n),
                 o_sc = a.take(it->cov_constraint ? sizeof(double) * 36 * n : 0), up_bytes = a.off;
    const size_t o_err = a.take(sizeof(double) * 6 * n), o_jac = a.take(sizeof(double) * 36 * n), o_cov = a.take(sizeof(double) * 36 * n),
                 down_bytes = a.off - up_bytes;
    struct Block {                          // the calling thread's cached device block, handed back on every path
      char* p = nullptr; size_t bytes = 0; int device = 0;
      ~Block() { DeviceBlockCache::give_back(p, bytes, device); }
    } blk;
    blk.bytes = a.off;
    HIP_TRY(hipGetDevice(&blk.device));
    HIP_TRY(DeviceBlockCache::acquire(blk.bytes, blk.device, &blk.p));
    std::vector<char> img(std::max(up_bytes, down_bytes));
    std::memcpy(img.data() + o_pa, it->pose_a, sizeof(double) * 6 * n); std::memcpy(img.data() + o_pb, it->pose_b, sizeof(double) * 6 * n);
    std::memcpy(img.data() + o_c, it->constraints, sizeof(double) * 6 * n);
    if (it->cov_constraint) std::memcpy(img.data() + o_sc, it->cov_constraint, sizeof(double) * 36 * n);
    HIP_TRY(hipMemcpy(blk.p, img.data(), up_bytes, hipMemcpyHostToDevice));
    PoConsCovArrays A;
    A.pa = (const double*)(blk.p + o_pa); A.pb = (const double*)(blk.p + o_pb); A.c = (const double*)(blk.p + o_c);
    A.sc = it->cov_constraint ? (const double*)(blk.p + o_sc) : nullptr;
    A.n = it->n; A.sigma2 = it->sigma2;
    A.err = (double*)(blk.p + o_err); A.jac = (double*)(blk.p + o_jac); A.cov = (double*)(blk.p + o_cov);
    hipLaunchKernelGGL(k_po_constraint_cov, dim3((unsigned)((n + 9) / 10)), dim3(64), 0, 0, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(img.data(), blk.p + up_bytes, down_bytes, hipMemcpyDeviceToHost));
    const char* down = img.data() - up_bytes;
    if (error) std::memcpy(error, down + o_err, sizeof(double) * 6 * n);
    if (jacobian) std::memcpy(jacobian, down + o_jac, sizeof(double) * 36 * n);
    if (cov_meas) std::memcpy(cov_meas, down + o_cov, sizeof(double) * 36 * n);
  } catch (const std::bad_alloc&) {
    return SLSLAM_ERR_NO_MEMORY;
  }
  return SLSLAM_OK;
}

#endif  // SLSLAM_PO_CONSTRAINT_COV_H_

// Device-side record of one pair of FCGF_APR's tester (scripts/test_apr.py:120-186, scripts/test_fcgf.py:121-195).
//
// apr_fcgf_test_pair: what the two scripts compute on the host per pair around their RANSAC call -- evaluate_nn_dist on
// find_corr's correspondences (test_apr.py:64-67, :142-143: the pair's row of dists_nn, which the hit-ratio and FMR tables
// at :200-213 are made from), the translation error, the arccos of the rotation trace, the 2 m / 5 deg flag (:162-177),
// |t_gt| (:123) -- plus the two inlier shares of the correspondences RANSAC ran on, taken from the RAW RANSAC result where
// apr_ransac_pose_async left it (ransac_raw.h: one layout, one decoder), into a 48-double record.  The per-pair fetch of
// the pose and of the nearest-neighbour indices goes away; the epoch (apr_amd/fcgf/lib/tester.py: FCGFTestEpoch.epoch,
// through ops.fcgf_test_pair) reads its records with one copy per `pairs_per_fetch` pairs.
//
// This removes host round trips and per-pair host arithmetic, not FLOPs (a few thousand rows).  k_fcgf_test_pair is one
// 1024-thread workgroup in the style of k_predator_test_pair (predator_valid.hip) and k_valid_pair (valid.hip): per-thread
// partial counts in row order (stride 1024), a wave64 butterfly, then the 16 wave partials added in wave order by thread 0
// -- integer sums only, a fixed tree, no floating-point atomics, the same bits on every run.
#include "common.h"
#include "inlier_dist.h"
#include "ransac_raw.h"

// The record states its operation order (include/apr_hip.h) and the tests repeat it bit for bit: no fused multiply-adds in
// the arithmetic written in this file.  hipcc contracts a * b + c by default, and through __fmul_rn / __dmul_rn too (they
// are inline functions of the HIP headers, compiled under the default), so the stated sums are plain operators below this
// pragma; the float32 point arithmetic of inlier_dist.h (the two inlier shares) stays as every other kernel compiles it.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;
constexpr int kHitLevels = 10;                 // thresholds k * 0.1, k = 1 .. 10 (test_apr.py:202-204)
constexpr long long kRansacChunk = 1 << 20;    // the hypothesis list of a single RANSAC round (ransac.hip: kChunk)

struct HitLevels {
  double t[kHitLevels];
};

// block-wide integer sum (every thread calls it); the result is valid in thread 0
__device__ inline long long block_sum(long long v, long long* s_part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();            // s_part may still be read from the previous sum
  if (lane == 0) s_part[wave] = v;
  __syncthreads();
  long long t = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kThreads / 64; ++k) t += s_part[k];
  return t;
}

__device__ inline int64_t clamp_row(int64_t i, int64_t n, long long& bad) {      // reads row 0 and is counted
  if (i < 0 || i >= n) {
    ++bad;
    return 0;
  }
  return i;
}

__global__ __launch_bounds__(kThreads) void k_fcgf_test_pair(
    const float* __restrict__ xyz0, int64_t n0, const float* __restrict__ xyz1, int64_t n1, const int64_t* __restrict__ sel0,
    const int64_t* __restrict__ sel1, int64_t m0, int64_t m1, const int64_t* __restrict__ nn, const float* __restrict__ r0,
    int64_t k0, const float* __restrict__ r1, int64_t k1, const int64_t* __restrict__ corr, const float* __restrict__ T_gt,
    const char* __restrict__ raw, float distance_threshold, double rte_thresh, double rre_thresh_rad, long long max_iter,
    HitLevels levels, float* __restrict__ dists, double* __restrict__ rec) {
  __shared__ long long s_part[kThreads / 64];
  const Hyp* hb = (const Hyp*)raw;
  // T_ransac: the estimate rounded to float32 (test_apr.py:156); the ground truth is float32 already
  float Re[9], te[3], Rg[9], tg[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Re[3 * a + b] = (float)hb->T[4 * a + b];
      Rg[3 * a + b] = T_gt[4 * a + b];
    }
    te[a] = (float)hb->T[4 * a + 3];
    tg[a] = T_gt[4 * a + 3];
  }
  long long bad = 0;
  // 1. evaluate_nn_dist over find_corr's correspondences xyz0[sel0] <-> xyz1[sel1[nn]]
  long long hit[kHitLevels];
#pragma unroll
  for (int k = 0; k < kHitLevels; ++k) hit[k] = 0;
  for (int64_t i = threadIdx.x; i < m0; i += kThreads) {
    const int64_t a = sel0 ? clamp_row(sel0[i], n0, bad) : i;
    int64_t b = clamp_row(nn[i], m1, bad);
    if (sel1) b = clamp_row(sel1[b], n1, bad);
    // every operation rounded to float32, products added left to right (the order of inlier_dist.h, unfused)
    const float* p = xyz0 + 3 * a;
    const float* t = xyz1 + 3 * b;
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((Rg[3 * c] * p[0] + Rg[3 * c + 1] * p[1]) + Rg[3 * c + 2] * p[2]) + tg[c];
    const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
    const float s = (dx * dx + dy * dy) + dz * dz;
    const float d = sqrtf(s + 1e-6f);      // correctly rounded (__fsqrt_rn is the 1-ulp native instruction here)
    if (dists) dists[i] = d;
#pragma unroll
    for (int k = 0; k < kHitLevels; ++k) hit[k] += (double)d < levels.t[k] ? 1 : 0;
  }
  // 2. the correspondences RANSAC ran on, under the estimate and under the ground truth
  long long c_est = 0, c_gt = 0;
  for (int64_t i = threadIdx.x; i < k0; i += kThreads) {
    const int64_t j = clamp_row(corr[i], k1, bad);
    float q[3];
    transform_f32(Re, te, r0 + 3 * i, q);
    c_est += dist_f32(q, r1 + 3 * j) < distance_threshold ? 1 : 0;
    transform_f32(Rg, tg, r0 + 3 * i, q);
    c_gt += dist_f32(q, r1 + 3 * j) < distance_threshold ? 1 : 0;
  }
  long long n_hit[kHitLevels];
  for (int k = 0; k < kHitLevels; ++k) n_hit[k] = block_sum(hit[k], s_part);
  const long long n_est = block_sum(c_est, s_part);
  const long long n_gt = block_sum(c_gt, s_part);
  const long long n_bad = block_sum(bad, s_part);
  if (threadIdx.x != 0) return;
  long long tv;
  memcpy(&tv, raw + sizeof(Hyp), 8);
  double r20[20];
  raw_decode20(*hb, tv, r20);
  // test_apr.py:163 in double on the float32 matrices: trace(R_est^T R_gt) = sum of the elementwise products, row by row
  double tr = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) s = s + (double)Re[3 * a + b] * (double)Rg[3 * a + b];
    tr = tr + s;
  }
  const double rre = acos((tr - 1.0) / 2.0);      // unclipped: NaN when the argument leaves [-1, 1], as apr_valid_pair
  double e2 = 0.0, g2 = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = (double)te[a] - (double)tg[a];
    e2 = e2 + d * d;
    g2 = g2 + (double)tg[a] * (double)tg[a];
  }
  const double rte = sqrt(e2);
  rec[0] = rte;
  rec[1] = rre;
  rec[2] = (rte < rte_thresh && rre == rre && rre < rre_thresh_rad) ? 1.0 : 0.0;      // both strict (test_apr.py:177)
  rec[3] = sqrt(g2);
  rec[4] = (double)m0;
  rec[5] = (double)k0;
  rec[6] = (double)k1;
  rec[7] = (double)n_bad;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) rec[8 + 4 * a + b] = (double)Re[3 * a + b];
    rec[8 + 4 * a + 3] = (double)te[a];
  }
  rec[20] = 0.0; rec[21] = 0.0; rec[22] = 0.0; rec[23] = 1.0;
  rec[24] = r20[16];      // inliers
  rec[25] = r20[17];      // rmse
  rec[26] = r20[19];      // total_valid
  rec[27] = r20[18];      // best iteration
  rec[28] = (tv > kRansacChunk && max_iter > kRansacChunk) ? 1.0 : 0.0;      // the single round overflowed: not final
  // (dist < thr).float().mean(): a float32 quotient of two integers, as apr_inlier_ratio forms it
  rec[29] = (double)__fdiv_rn((float)n_est, (float)k0);
  rec[30] = (double)__fdiv_rn((float)n_gt, (float)k0);
  rec[31] = 0.0;
  for (int k = 0; k < kHitLevels; ++k) rec[32 + k] = (double)n_hit[k];
  for (int k = 32 + kHitLevels; k < APR_FCGF_TEST_RECORD_FLOATS; ++k) rec[k] = 0.0;
}

}  // namespace

APR_API int apr_fcgf_test_pair(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int64_t* sel0,
                               const int64_t* sel1, int64_t m0, int64_t m1, const int64_t* nn, const float* r0, int64_t k0,
                               const float* r1, int64_t k1, const int64_t* corr, const float* T_gt, const void* raw_dev,
                               double distance_threshold, double rte_thresh, double rre_thresh_deg, int64_t max_iter,
                               float* dists, double* records, int64_t n_slots, int64_t slot, void* stream) {
  APR_CHECK_ARG(xyz0 && xyz1 && nn && r0 && r1 && corr && T_gt && raw_dev && records, "apr_fcgf_test_pair: NULL argument");
  APR_CHECK_ARG(n0 > 0 && n1 > 0 && m1 > 0 && k1 > 0, "apr_fcgf_test_pair: empty cloud");
  // the counts become float32 quotients: exact below 2^24
  APR_CHECK_ARG(m0 > 0 && k0 > 0 && m0 < (1ll << 24) && k0 < (1ll << 24), "apr_fcgf_test_pair: need 0 < m0, k0 < 2^24");
  APR_CHECK_ARG(sel0 || m0 == n0, "apr_fcgf_test_pair: sel0 == NULL needs m0 == n0");
  APR_CHECK_ARG(sel1 || m1 == n1, "apr_fcgf_test_pair: sel1 == NULL needs m1 == n1");
  APR_CHECK_ARG(max_iter > 0 && distance_threshold > 0, "apr_fcgf_test_pair: bad max_iter / distance_threshold");
  APR_CHECK_ARG(((uintptr_t)raw_dev & 7) == 0, "apr_fcgf_test_pair: raw_dev must be 8-byte aligned");
  APR_CHECK_ARG(slot >= 0 && slot < n_slots, "apr_fcgf_test_pair: slot outside the record buffer");
  HitLevels levels;
  for (int k = 0; k < kHitLevels; ++k) levels.t[k] = (double)(k + 1) * 0.1;      // the Python double k * 0.1
  const double rre_thresh_rad = 3.141592653589793 / 180.0 * rre_thresh_deg;      // np.pi / 180 * rre_thresh
  hipLaunchKernelGGL(k_fcgf_test_pair, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, xyz0, n0, xyz1, n1, sel0, sel1, m0,
                     m1, nn, r0, k0, r1, k1, corr, T_gt, (const char*)raw_dev, (float)distance_threshold, rte_thresh,
                     rre_thresh_rad, (long long)max_iter, levels, dists, records + slot * APR_FCGF_TEST_RECORD_FLOATS);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Device-side records of Predator_APR's validation pass and tester epoch.
//
// apr_predator_valid_record: Trainer.inference_one_batch(inputs, 'val') (Predator_APR/lib/trainer.py:223-280) ends with five
// float() conversions (:274-278), each a host synchronisation, behind about ten elementwise launches that pick the stats
// out of the loss kernels' result vectors and add the two frames' NPR terms.  Here ONE small launch packs all of it into a
// 16-float record of a caller-owned [pairs, 16] buffer; an epoch reads the buffer back with one copy.
//
// apr_predator_test_pair: the arithmetic KITTITester.test runs on the host AFTER its per-pair loop (lib/tester.py:104-124:
// get_angle_deviation, the translation error, the 5 deg / 2 m flags, |t_gt|), plus the two inlier shares, taken per pair
// from the RAW RANSAC result where apr_ransac_pose_geometric_async left it (ransac_raw.h: one layout, one decoder), into a
// 32-double record.  The per-batch fetch of raw results goes away; the epoch reads its records once.
//
// Both remove host round trips and per-pair host arithmetic, not FLOPs (a few thousand rows).  k_predator_test_pair is one
// 1024-thread workgroup in the style of k_valid_pair (valid.hip): per-thread partial sums in row order (stride 1024), a
// wave64 butterfly, then the 16 wave partials added in wave order by thread 0 -- a fixed tree, no floating-point atomics,
// the same bits on every run.
#include "common.h"
#include "inlier_dist.h"
#include "ransac_raw.h"

namespace {

constexpr int kThreads = 1024;

__global__ void k_predator_valid_record(const float* __restrict__ overlap8, const float* __restrict__ saliency8,
                                        const float* __restrict__ circle4, const int* __restrict__ count,
                                        const float* __restrict__ c0, const float* __restrict__ c1,
                                        const float* __restrict__ r0, const float* __restrict__ r1, float n_src, float n_tgt,
                                        float* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  // the eight MetricLoss keys; a weighted_bce vector is loss, w_negative, precision, recall, ...
  rec[0] = circle4[0];       // circle_loss
  rec[1] = circle4[1];       // recall
  rec[2] = overlap8[0];      // overlap_loss
  rec[3] = overlap8[3];      // overlap_recall
  rec[4] = overlap8[2];      // overlap_precision
  rec[5] = saliency8[0];     // saliency_loss
  rec[6] = saliency8[3];     // saliency_recall
  rec[7] = saliency8[2];     // saliency_precision
  const float a = *c0, b = *c1;
  rec[8] = __fadd_rn(a, b);                // chamfer_loss: 0 + c0 + c1 (trainer.py:255, :264)
  rec[9] = __fadd_rn(*r0, *r1);            // regularization_loss (:253, :262)
  rec[10] = (float)*count;
  rec[11] = circle4[2];
  rec[12] = n_src;
  rec[13] = n_tgt;
  rec[14] = (a != a ? 1.f : 0.f) + (b != b ? 1.f : 0.f);
  rec[15] = 0.f;
}

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

__global__ __launch_bounds__(kThreads) void k_predator_test_pair(const float* __restrict__ s_p, int64_t ns,
                                                                 const float* __restrict__ t_p, int64_t nt,
                                                                 const int64_t* __restrict__ corr,
                                                                 const float* __restrict__ rot_gt, const float* __restrict__ trans_gt,
                                                                 const char* __restrict__ raw, float distance_threshold,
                                                                 float inlier_distance_threshold, double rot_threshold,
                                                                 double trans_threshold, double* __restrict__ rec) {
  __shared__ long long s_part[kThreads / 64];
  const Hyp* hb = (const Hyp*)raw;
  // the estimate in the float32 of the clouds, for the inlier share under it
  float Re[9], te[3], Rg[9], tg[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Re[3 * a + b] = (float)hb->T[4 * a + b];
      Rg[3 * a + b] = rot_gt[3 * a + b];
    }
    te[a] = (float)hb->T[4 * a + 3];
    tg[a] = trans_gt[a];
  }
  long long c_gt = 0, c_est = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < ns; i += kThreads) {
    int64_t j = corr[i];
    if (j < 0 || j >= nt) {        // reads row 0 and is counted
      ++bad;
      j = 0;
    }
    float q[3];
    transform_f32(Rg, tg, s_p + 3 * i, q);
    c_gt += dist_f32(q, t_p + 3 * j) < inlier_distance_threshold ? 1 : 0;
    transform_f32(Re, te, s_p + 3 * i, q);
    c_est += dist_f32(q, t_p + 3 * j) < distance_threshold ? 1 : 0;
  }
  const long long n_gt = block_sum(c_gt, s_part);
  const long long n_est = block_sum(c_est, s_part);
  const long long n_bad = block_sum(bad, s_part);
  if (threadIdx.x != 0) return;
  long long tv;
  memcpy(&tv, raw + sizeof(Hyp), 8);
  double r20[20];
  raw_decode20(*hb, tv, r20);
  // get_angle_deviation (lib/benchmark_utils.py:170-185): R = R_est R_gt^T, its trace, arccos(clip((tr - 1) / 2, -1, 1)) / pi * 180
  double tr = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) s = __dadd_rn(s, __dmul_rn(hb->T[4 * a + b], (double)Rg[3 * a + b]));
    tr = __dadd_rn(tr, s);
  }
  double cosv = (tr - 1.0) / 2.0;
  cosv = cosv < -1.0 ? -1.0 : (cosv > 1.0 ? 1.0 : cosv);
  const double rre = acos(cosv) / 3.141592653589793 * 180.0;
  double e2 = 0.0, g2 = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = hb->T[4 * a + 3] - (double)tg[a];
    e2 = __dadd_rn(e2, __dmul_rn(d, d));
    g2 = __dadd_rn(g2, __dmul_rn((double)tg[a], (double)tg[a]));
  }
  const double rte = sqrt(e2);
  rec[0] = rre;
  rec[1] = rte;
  rec[2] = (rre < rot_threshold && rte < trans_threshold) ? 1.0 : 0.0;      // both strict (lib/tester.py:115-117)
  rec[3] = sqrt(g2);
  // (dist < thr).float().mean(): a float32 quotient of two integers, as apr_inlier_ratio forms it
  rec[4] = (double)__fdiv_rn((float)n_gt, (float)ns);
  rec[5] = (double)__fdiv_rn((float)n_est, (float)ns);
  rec[6] = (double)ns;
  rec[7] = (double)nt;
  for (int k = 0; k < 16; ++k) rec[8 + k] = r20[k];
  rec[24] = r20[16];      // inliers
  rec[25] = r20[17];      // rmse
  rec[26] = r20[19];      // n_valid
  rec[27] = r20[18];      // best_iteration
  rec[28] = (double)n_bad;
  rec[29] = 0.0;
  rec[30] = 0.0;
  rec[31] = 0.0;
}

}  // namespace

APR_API int apr_predator_valid_record(const float* overlap8, const float* saliency8, const float* circle4,
                                      const int32_t* count, const float* chamfer0, const float* chamfer1, const float* reg0,
                                      const float* reg1, int64_t n_src, int64_t n_tgt, float* records, int64_t n_slots,
                                      int64_t slot, void* stream) {
  APR_CHECK_ARG(overlap8 && saliency8 && circle4 && count && chamfer0 && chamfer1 && reg0 && reg1 && records,
                "apr_predator_valid_record: NULL argument");
  // the row counts travel as float32: exact below 2^24
  APR_CHECK_ARG(n_src > 0 && n_tgt > 0 && n_src < (1ll << 24) && n_tgt < (1ll << 24),
                "apr_predator_valid_record: need 0 < n_src, n_tgt < 2^24");
  APR_CHECK_ARG(slot >= 0 && slot < n_slots, "apr_predator_valid_record: slot outside the record buffer");
  hipLaunchKernelGGL(k_predator_valid_record, dim3(1), dim3(64), 0, (hipStream_t)stream, overlap8, saliency8, circle4,
                     (const int*)count, chamfer0, chamfer1, reg0, reg1, (float)n_src, (float)n_tgt,
                     records + slot * APR_PREDATOR_VALID_RECORD_FLOATS);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_predator_test_pair(const float* s_p, int64_t ns, const float* t_p, int64_t nt, const int64_t* corr,
                                   const float* rot_gt, const float* trans_gt, const void* raw_dev, double distance_threshold,
                                   double inlier_distance_threshold, double rot_threshold, double trans_threshold,
                                   double* records, int64_t n_slots, int64_t slot, void* stream) {
  APR_CHECK_ARG(s_p && t_p && corr && rot_gt && trans_gt && raw_dev && records, "apr_predator_test_pair: NULL argument");
  // the inlier counts become float32 quotients: exact below 2^24
  APR_CHECK_ARG(ns > 0 && nt > 0 && ns < (1ll << 24), "apr_predator_test_pair: need 0 < ns < 2^24 and nt > 0");
  APR_CHECK_ARG(((uintptr_t)raw_dev & 7) == 0, "apr_predator_test_pair: raw_dev must be 8-byte aligned");
  APR_CHECK_ARG(slot >= 0 && slot < n_slots, "apr_predator_test_pair: slot outside the record buffer");
  hipLaunchKernelGGL(k_predator_test_pair, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, s_p, ns, t_p, nt, corr, rot_gt,
                     trans_gt, (const char*)raw_dev, (float)distance_threshold, (float)inlier_distance_threshold,
                     rot_threshold, trans_threshold, records + slot * APR_PREDATOR_TEST_RECORD_FLOATS);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Matching metrics of one validation pair in ONE launch (GenerativePairTrainer._valid_epoch,
// FCGF_APR/lib/complement_trainer.py:555-572).
//
// The reference chains, per pair: find_corr's two gathers, est_quad_linear_robust, corr_dist, |t_est - t_gt|, the
// arccos of the rotation trace, evaluate_hit_ratio -- every one of them hands a value to the host before the next
// starts.  Here a single persistent 1024-thread workgroup gathers the correspondences from the feature-NN result, runs
// the 20 IRLS iterations (irls.h: the device code k_irls runs, hence the same bits), and reduces the metrics into one
// 24-float record of a caller-owned [pairs, 24] buffer: a whole epoch is read back with one copy.  The data is a few
// thousand rows; what this removes is host round trips, not arithmetic.
//
// Every sum is a per-thread partial in row order (stride 1024), a wave64 butterfly, then the 16 wave partials added in
// wave order by thread 0: a fixed tree, no floating-point atomics, the same bits on every run.
#include "irls.h"

namespace {

struct Rigid {
  float r[12];   // rows of [R | t]
};

__device__ inline void apply(const Rigid& T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = T.r[0] * x + T.r[1] * y + T.r[2] * z + T.r[3];
  oy = T.r[4] * x + T.r[5] * y + T.r[6] * z + T.r[7];
  oz = T.r[8] * x + T.r[9] * y + T.r[10] * z + T.r[11];
}

__device__ inline int64_t clamp_row(int64_t i, int64_t n, int& bad) {
  if (i < 0 || i >= n) {
    ++bad;
    return 0;
  }
  return i;
}

// s_part: [16] doubles of the caller; the result is valid in thread 0 only
__device__ inline double block_sum(double v, double* s_part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();            // s_part may still be read from the previous sum
  if (lane == 0) s_part[wave] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < 16; ++k) t += s_part[k];
  return t;
}

__global__ __launch_bounds__(1024) void k_valid_pair(const float* __restrict__ xyz0, int64_t n0,
                                                     const float* __restrict__ xyz1, int64_t n1,
                                                     const int64_t* __restrict__ sel0, const int64_t* __restrict__ sel1,
                                                     int64_t m0, int64_t m1, const int64_t* __restrict__ nn,
                                                     const float* __restrict__ T_gt, float hit_thresh,
                                                     float* p0, float* p1, float* cur, float* w, float* rec) {
  __shared__ float s_T[16];
  __shared__ double s_part[16];
  const int tid = threadIdx.x;
  // 1. correspondences: xyz0[sel0], xyz1[sel1[nn]] (an index out of range reads row 0 and is counted)
  int bad = 0;
  for (int64_t i = tid; i < m0; i += 1024) {
    const int64_t a = sel0 ? clamp_row(sel0[i], n0, bad) : i;
    int64_t b = clamp_row(nn[i], m1, bad);
    if (sel1) b = clamp_row(sel1[b], n1, bad);
    p0[3 * i] = xyz0[3 * a]; p0[3 * i + 1] = xyz0[3 * a + 1]; p0[3 * i + 2] = xyz0[3 * a + 2];
    p1[3 * i] = xyz1[3 * b]; p1[3 * i + 1] = xyz1[3 * b + 1]; p1[3 * i + 2] = xyz1[3 * b + 2];
  }
  __syncthreads();
  // 2. est_quad_linear_robust
  irls_run(p0, p1, nullptr, m0, cur, w, s_T);
  Rigid E, G;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    E.r[k] = s_T[k];
    G.r[k] = T_gt[k];
  }
  // 3. corr_dist over all rows of xyz0: min(|T_est x - T_gt x|, 1)
  double acc = 0.0;
  for (int64_t i = tid; i < n0; i += 1024) {
    const float x = xyz0[3 * i], y = xyz0[3 * i + 1], z = xyz0[3 * i + 2];
    float ex, ey, ez, gx, gy, gz;
    apply(E, x, y, z, ex, ey, ez);
    apply(G, x, y, z, gx, gy, gz);
    const float dx = ex - gx, dy = ey - gy, dz = ez - gz;
    acc += (double)fminf(sqrtf(dx * dx + dy * dy + dz * dz), 1.0f);
  }
  const double gap_sum = block_sum(acc, s_part);
  // 4. hits among the correspondences: sqrt(|T_gt x0 - x1|^2 + 1e-6) < hit_thresh
  double hits = 0.0;
  for (int64_t i = tid; i < m0; i += 1024) {
    float gx, gy, gz;
    apply(G, p0[3 * i], p0[3 * i + 1], p0[3 * i + 2], gx, gy, gz);
    const float dx = gx - p1[3 * i], dy = gy - p1[3 * i + 1], dz = gz - p1[3 * i + 2];
    hits += sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f) < hit_thresh ? 1.0 : 0.0;
  }
  const double hit_sum = block_sum(hits, s_part);
  const double bad_sum = block_sum((double)bad, s_part);
  if (tid == 0) {
    // 5. rte, rre; the cosine is exact in double for the float32 matrices, outside [-1, 1] the angle is NaN
    const float tx = E.r[3] - G.r[3], ty = E.r[7] - G.r[7], tz = E.r[11] - G.r[11];
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) tr += (double)E.r[4 * a + b] * (double)G.r[4 * a + b];
    rec[0] = (float)(gap_sum / (double)n0);
    rec[1] = sqrtf(tx * tx + ty * ty + tz * tz);
    rec[2] = (float)acos((tr - 1.0) * 0.5);
    rec[3] = (float)hit_sum / (float)m0;
    rec[4] = bad_sum > 0.0 ? -(float)bad_sum : (float)m0;
    rec[23] = (float)hit_sum;
  }
  if (tid < 16) rec[5 + tid] = s_T[tid];
}

}  // namespace

APR_API size_t apr_valid_pair_scratch_bytes(int64_t m0) { return m0 > 0 ? (size_t)m0 * 40 + 256 : 0; }

APR_API int apr_valid_pair(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int64_t* sel0,
                           const int64_t* sel1, int64_t m0, int64_t m1, const int64_t* nn, const float* T_gt,
                           float hit_thresh, float* records, int64_t n_slots, int64_t slot, void* scratch, size_t scratch_bytes,
                           void* stream) {
  APR_CHECK_ARG(n0 > 0 && n1 > 0 && m0 > 0 && m1 > 0, "apr_valid_pair: empty cloud or no correspondences");
  APR_CHECK_ARG(xyz0 && xyz1 && nn && T_gt && records && scratch, "apr_valid_pair: NULL argument");
  APR_CHECK_ARG(sel0 || m0 == n0, "apr_valid_pair: sel0 == NULL needs m0 == n0");
  APR_CHECK_ARG(sel1 || m1 == n1, "apr_valid_pair: sel1 == NULL needs m1 == n1");
  APR_CHECK_ARG(slot >= 0 && slot < n_slots, "apr_valid_pair: slot outside the record buffer");
  APR_CHECK_ARG(scratch_bytes >= apr_valid_pair_scratch_bytes(m0), "apr_valid_pair: scratch too small");
  float* p0 = (float*)scratch;
  float* p1 = p0 + 3 * m0;
  float* cur = p1 + 3 * m0;
  float* w = cur + 3 * m0;
  hipLaunchKernelGGL(k_valid_pair, dim3(1), dim3(1024), 0, (hipStream_t)stream, xyz0, n0, xyz1, n1, sel0, sel1, m0, m1,
                     nn, T_gt, hit_thresh, p0, p1, cur, w, records + slot * APR_VALID_RECORD_FLOATS);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

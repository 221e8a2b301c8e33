// Mutual nearest-neighbour selection and the two inlier ratios of the Predator tester
// (Predator_APR/lib/benchmark_utils.py:227-268 get_inlier_ratio, :271-295 mutual_selection).
//
// The reference forms the n_src x n_tgt score matrix on the GPU, copies it to the host and builds three more host arrays
// of that size to find the entries that are the maximum of both their row and their column.  Here the matrix never
// exists: apr_gathered_argmax (metric_loss.hip) leaves row_arg / col_arg, and
//   apr_mutual_select  keeps the pairs (i, row_arg[i]) with col_arg[row_arg[i]] == i in ascending i -- the order of
//                      np.where(selection) -- at positions fixed by ballot + popcount + a block scan (no atomics: the
//                      list is the same bits run to run),
//   apr_inlier_ratio   writes the distances and the inlier ratios of both legs in one launch (integer counts, each ratio
//                      formed once from its count),
//   apr_dense_argmax   serves the compatibility form mutual_selection(score_mat) for a caller that already holds a matrix.
// All three are latency / HBM-stream bound at the tester's sizes (5000 .. 14 k points: a few hundred KB); the list kernels
// run as ONE workgroup that walks the input in chunks of 1024, which keeps positions and sums in a fixed order without a
// second launch or a device-scope fence.  The pair-list RANSAC that consumes the list lives in ransac.hip, next to the
// device functions it shares with the other RANSAC entries.
#include "common.h"
#include "inlier_dist.h"

namespace {

constexpr int kListThreads = 1024;

// pairs[k] = (i, row_arg[i]) for the k-th mutual i; *count = their number (<= cap = min(n_src_max, n_tgt_max): a mutual
// pair is the only one of its row AND of its column).  A row_arg outside [0, n_tgt) is no pair.
__global__ __launch_bounds__(kListThreads) void k_mutual_select(const int* __restrict__ row_arg, const int* __restrict__ n_src_dev,
                                                                int n_src_max, const int* __restrict__ col_arg,
                                                                const int* __restrict__ n_tgt_dev, int n_tgt_max, int cap,
                                                                int* __restrict__ pairs, int* __restrict__ count) {
  __shared__ int s_wave[kListThreads / 64];
  __shared__ int s_carry;
  int n_src = n_src_max, n_tgt = n_tgt_max;
  if (n_src_dev) n_src = max(0, min(n_src, *n_src_dev));
  if (n_tgt_dev) n_tgt = max(0, min(n_tgt, *n_tgt_dev));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n_src; base += kListThreads) {      // workgroup-uniform trip count
    const int i = base + (int)threadIdx.x;
    int j = -1;
    bool f = false;
    if (i < n_src) {
      j = row_arg[i];
      f = j >= 0 && j < n_tgt && col_arg[j] == i;
    }
    const unsigned long long b = __ballot(f);
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    const int carry = s_carry;
    int pos = carry + __popcll(b & ((1ull << lane) - 1ull));
    int total = 0;
    for (int w = 0; w < kListThreads / 64; ++w) {
      const int c = s_wave[w];
      if (w < wave) pos += c;
      total += c;
    }
    if (f && pos < cap) {
      pairs[2 * pos] = i;
      pairs[2 * pos + 1] = j;
    }
    __syncthreads();
    if (threadIdx.x == 0) s_carry = carry + total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = min(s_carry, cap);
}

// transform_f32 / dist_f32 (benchmark_utils.py:246, :252 in float32): inlier_dist.h

// block-wide integer sum (every thread calls it); the result is valid in thread 0
__device__ inline int block_sum(int v, int* s_wave) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kListThreads / 64; ++w) s += s_wave[w];
  return s;
}

// out8 = ratio_wo, ratio_w, #inliers wo, #inliers w, n_src, #mutual pairs, 0, 0.  A row_arg / pair entry outside its cloud
// gives distance +inf (never an inlier) instead of a read outside the buffers.
__global__ __launch_bounds__(kListThreads) void k_inlier_ratio(const float* __restrict__ src, int n_src,
                                                               const float* __restrict__ tgt, int n_tgt,
                                                               const float* __restrict__ rot9, const float* __restrict__ trans3,
                                                               const int* __restrict__ row_arg, const int* __restrict__ pairs,
                                                               const int* __restrict__ count, int cap, float thr,
                                                               float* __restrict__ dist_wo, float* __restrict__ dist_w,
                                                               float* __restrict__ out8) {
  __shared__ int s_wave[kListThreads / 64];
  const float inf = __uint_as_float(0x7f800000u);
  int c_wo = 0, c_w = 0;
  for (int i = threadIdx.x; i < n_src; i += kListThreads) {
    const int j = row_arg[i];
    float d = inf;
    if (j >= 0 && j < n_tgt) {
      float q[3];
      transform_f32(rot9, trans3, src + 3 * (int64_t)i, q);
      d = dist_f32(q, tgt + 3 * (int64_t)j);
    }
    dist_wo[i] = d;
    c_wo += d < thr ? 1 : 0;
  }
  const int np = max(0, min(*count, cap));
  for (int k = threadIdx.x; k < np; k += kListThreads) {
    const int i = pairs[2 * k], j = pairs[2 * k + 1];
    float d = inf;
    if (i >= 0 && i < n_src && j >= 0 && j < n_tgt) {
      float q[3];
      transform_f32(rot9, trans3, src + 3 * (int64_t)i, q);
      d = dist_f32(q, tgt + 3 * (int64_t)j);
    }
    dist_w[k] = d;
    c_w += d < thr ? 1 : 0;
  }
  const int t_wo = block_sum(c_wo, s_wave);
  const int t_w = block_sum(c_w, s_wave);
  if (threadIdx.x == 0) {
    // (dist < thr).float().mean(): a float32 quotient of two integers; the mean of nothing is NaN
    out8[0] = __fdiv_rn((float)t_wo, (float)n_src);
    out8[1] = __fdiv_rn((float)t_w, (float)np);
    out8[2] = (float)t_wo;
    out8[3] = (float)t_w;
    out8[4] = (float)n_src;
    out8[5] = (float)np;
    out8[6] = 0.f;
    out8[7] = 0.f;
  }
}

// arg-max along each row: one wave per row, lanes stride the columns; ties (and equal maxima across lanes) to the lowest
// column.  A NaN never wins (np.argmax would return the first NaN: score matrices of finite descriptors have none).
__global__ __launch_bounds__(256) void k_argmax_rows(const float* __restrict__ m, int n, int mm, int* __restrict__ row_arg) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;                       // wave-uniform
  const float* row = m + (int64_t)r * mm;
  float best = -__uint_as_float(0x7f800000u);
  int arg = 0x7fffffff;
  for (int c = lane; c < mm; c += 64) {
    const float v = row[c];
    if (v > best || arg == 0x7fffffff) {
      best = v;
      arg = c;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const float ob = __shfl_xor(best, d);
    const int oa = __shfl_xor(arg, d);
    if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) {
      best = ob;
      arg = oa;
    }
  }
  if (lane == 0) row_arg[r] = arg;
}

// arg-max along each column: one thread per column walks the rows (a wave reads 256 contiguous bytes per row); the first
// maximum wins
__global__ __launch_bounds__(256) void k_argmax_cols(const float* __restrict__ m, int n, int mm, int* __restrict__ col_arg) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= mm) return;
  float best = m[c];
  int arg = 0;
  for (int r = 1; r < n; ++r) {
    const float v = m[(int64_t)r * mm + c];
    if (v > best) {
      best = v;
      arg = r;
    }
  }
  col_arg[c] = arg;
}

}  // namespace

APR_API int apr_mutual_select(const int32_t* row_arg, const int32_t* n_src_dev, int64_t n_src_max, const int32_t* col_arg,
                              const int32_t* n_tgt_dev, int64_t n_tgt_max, int32_t* pairs, int32_t* count, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_src_max > 0 && n_tgt_max > 0 && n_src_max < (1ll << 30) && n_tgt_max < (1ll << 30),
                "apr_mutual_select: need 0 < n_src_max, n_tgt_max < 2^30");
  APR_CHECK_ARG(row_arg && col_arg && pairs && count, "apr_mutual_select: NULL argument");
  const int cap = (int)(n_src_max < n_tgt_max ? n_src_max : n_tgt_max);
  hipLaunchKernelGGL(k_mutual_select, dim3(1), dim3(kListThreads), 0, st, (const int*)row_arg, (const int*)n_src_dev,
                     (int)n_src_max, (const int*)col_arg, (const int*)n_tgt_dev, (int)n_tgt_max, cap, (int*)pairs, (int*)count);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_inlier_ratio(const float* src_pcd, int64_t n_src, const float* tgt_pcd, int64_t n_tgt, const float* rot9,
                             const float* trans3, const int32_t* row_arg, const int32_t* pairs, const int32_t* count,
                             int64_t pairs_cap, float threshold, float* dist_wo, float* dist_w, float* out8, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  // the counts travel as float32: exact below 2^24
  APR_CHECK_ARG(n_src > 0 && n_tgt > 0 && n_src < (1ll << 24) && n_tgt < (1ll << 30), "apr_inlier_ratio: need 0 < n_src < 2^24, 0 < n_tgt < 2^30");
  APR_CHECK_ARG(pairs_cap > 0 && pairs_cap <= n_src, "apr_inlier_ratio: need 0 < pairs_cap <= n_src");
  APR_CHECK_ARG(src_pcd && tgt_pcd && rot9 && trans3 && row_arg && pairs && count && dist_wo && dist_w && out8,
                "apr_inlier_ratio: NULL argument");
  hipLaunchKernelGGL(k_inlier_ratio, dim3(1), dim3(kListThreads), 0, st, src_pcd, (int)n_src, tgt_pcd, (int)n_tgt, rot9, trans3,
                     (const int*)row_arg, (const int*)pairs, (const int*)count, (int)pairs_cap, threshold, dist_wo, dist_w, out8);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_dense_argmax(const float* scores, int64_t n, int64_t m, int32_t* row_arg, int32_t* col_arg, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n > 0 && m > 0 && n < (1ll << 30) && m < (1ll << 30), "apr_dense_argmax: need 0 < n, m < 2^30");
  APR_CHECK_ARG(scores && row_arg && col_arg, "apr_dense_argmax: NULL argument");
  hipLaunchKernelGGL(k_argmax_rows, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, st, scores, (int)n, (int)m, (int*)row_arg);
  hipLaunchKernelGGL(k_argmax_cols, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, st, scores, (int)n, (int)m, (int*)col_arg);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

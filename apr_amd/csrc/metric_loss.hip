// Predator_APR's descriptor loss, `MetricLoss` (Predator_APR/lib/loss.py:16-178), as device-side kernels.
//
// The reference goes to the host three times per call (two Python `set`s :114-115, two sklearn calls :94-95, the
// permutation :157), materialises `scores = src_feats_sel @ tgt_feats_sel.T` (:134) only to take an arg-max along each
// axis, and runs the circle loss as ~40 elementwise / reduction launches over a max_points^2 matrix.  Here:
//
//   overlap labels   gt vectors + ascending unique index lists with device-side counts           (:114-123)
//   weighted BCE     one pass of per-block fp64 partial sums, one closing block: loss, w_negative, tp / fp / fn,
//                    precision, recall; backward = nn.BCELoss's own formula                           (:79-97)
//   mutual arg-max   rows gathered by index list inside the kernel, 16 x 16 score tiles in MFMA accumulators, the
//                    column block in LDS, nothing sized ns * nt; launched twice with the roles swapped (:132-138)
//   saliency labels  partner distance < matchability_radius, gathered saliency scores                 (:136-144)
//   circle loss      filter + compaction, gather by `choice`, one wave per anchor row with the other side's features
//                    in LDS, launched twice with the roles swapped; closing block; backward + ordered scatter
//                                                                                             (:34-77, :153-167)
//
// Determinism: no float atomics anywhere.  Every sum is a per-lane serial sum over a fixed stride followed by a
// shuffle butterfly, or a serial loop of one thread over per-block partials; a scatter of duplicates adds in ascending
// anchor order.  Same bits run to run.
//
// MFMA form: v_mfma_f32_16x16x4_f32.  The arg-max must agree with an fp32 matmul to fp32 rounding, so bf16 operands would
// need the three-way split (3 MFMAs + 2 splits per operand); at D = 32 the whole 12 k x 11 k sweep is 8.4 GFLOP per
// direction, ~0.1 ms at the f32 MFMA rate, and is bound by staging the gathered rows, not by the matrix unit.  The exact
// f32 form is simpler and leaves nothing to a refinement pass.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ML_D = 32;          // final_feats_dim of every shipped config
constexpr int ML_MAXP = 512;      // max_points: 512 KITTI, 256 indoor

// exclusive prefix sum over the block (blockDim.x a multiple of 64, <= 1024); *total = block sum
__device__ inline int block_excl_scan(int v, int* total, int* s_w /*[16]*/) {
  const int inc = apr_wave_incl_scan(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 63) s_w[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
    const int t = s_w[k];
    if (k < w) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

__device__ inline void rigid(const float* __restrict__ R, const float* __restrict__ t, const float* __restrict__ p,
                             float* o) {
  // rot @ p + trans (:111), fp32
  for (int r = 0; r < 3; ++r) o[r] = fmaf(R[3 * r + 2], p[2], fmaf(R[3 * r + 1], p[1], R[3 * r] * p[0])) + t[r];
}

// ---------------------------------------------------------------------------------------------------------------------
// overlap labels (:114-123)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void k_labels_clear(int64_t ns, int64_t nt, float* __restrict__ gt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ns + nt) gt[i] = 0.f;
}

__global__ void k_labels_set(const long long* __restrict__ corr, int64_t n_corr, int64_t ns, int64_t nt,
                             float* __restrict__ gt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_corr) return;
  const long long s = corr[2 * i], t = corr[2 * i + 1];
  // every writer stores the same 1.0f: the race between duplicates cannot change the result
  if (s >= 0 && s < ns) gt[s] = 1.f;
  if (t >= 0 && t < nt) gt[ns + t] = 1.f;
}

// The index lists come out in ASCENDING order.  Python's `set` order (:114-115) is unspecified; no result of the
// reference depends on it beyond the order in which the saliency BCE terms are summed.
__global__ __launch_bounds__(1024) void k_labels_compact(const float* __restrict__ gt, int64_t ns, int64_t nt,
                                                         int* __restrict__ src_idx, int* __restrict__ tgt_idx,
                                                         int* __restrict__ counts /*[3]*/) {
  __shared__ int s_w[16];
  int both = 0;
  for (int side = 0; side < 2; ++side) {
    const float* g = side ? gt + ns : gt;
    const int64_t n = side ? nt : ns;
    int* out = side ? tgt_idx : src_idx;
    const int64_t per = (n + blockDim.x - 1) / blockDim.x;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < n ? lo + per : n;
    int cnt = 0;
    for (int64_t i = lo; i < hi; ++i) cnt += g[i] != 0.f;
    int total;
    int off = block_excl_scan(cnt, &total, s_w);
    for (int64_t i = lo; i < hi; ++i)
      if (g[i] != 0.f) out[off++] = (int)i;
    if (threadIdx.x == 0) counts[side] = total;
    both += total;
  }
  if (threadIdx.x == 0) counts[2] = both;
}

// ---------------------------------------------------------------------------------------------------------------------
// weighted BCE (:79-97)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int BCE_MAX_BLOCKS = 256;
constexpr int BCE_Q = 6;   // sum gt, loss over positives, loss over negatives, tp, fp, fn

__device__ inline int bce_n(int64_t n, const int* n_dev) {
  if (!n_dev) return (int)n;
  const int v = *n_dev;
  return v < 0 ? 0 : (v < n ? v : (int)n);
}

__global__ __launch_bounds__(256) void k_bce_partial(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     int64_t n_max, const int* __restrict__ n_dev,
                                                     double* __restrict__ partial /*[gridDim.x][6]*/) {
  __shared__ double s_p[4][BCE_Q];
  const int n = bce_n(n_max, n_dev);
  double v[BCE_Q] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double p = pred[i], g = gt[i];
    // nn.BCELoss clamps each log at -100
    const double l = -(g * fmax(log(p), -100.0) + (1.0 - g) * fmax(log(1.0 - p), -100.0));
    const bool pos = g >= 0.5, hat = pred[i] > 0.5f;          // round() is half-to-even: 0.5 predicts 0
    v[0] += g;
    v[1] += pos ? l : 0.0;
    v[2] += pos ? 0.0 : l;
    v[3] += (pos && hat);
    v[4] += (!pos && hat);
    v[5] += (pos && !hat);
  }
#pragma unroll
  for (int k = 0; k < BCE_Q; ++k) {
    double s = v[k];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) s_p[threadIdx.x >> 6][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < BCE_Q)
    partial[blockIdx.x * BCE_Q + threadIdx.x] =
        ((s_p[0][threadIdx.x] + s_p[1][threadIdx.x]) + s_p[2][threadIdx.x]) + s_p[3][threadIdx.x];
}

__global__ void k_bce_final(const double* __restrict__ partial, int nblocks, int64_t n_max, const int* __restrict__ n_dev,
                            float* __restrict__ out /*[8]*/) {
  if (threadIdx.x != 0) return;
  double s[BCE_Q] = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < nblocks; ++b)
    for (int k = 0; k < BCE_Q; ++k) s[k] += partial[b * BCE_Q + k];
  const double n = (double)bce_n(n_max, n_dev);
  const double w_neg = s[0] / n, w_pos = 1.0 - w_neg;            // :85-86
  out[0] = (float)((w_pos * s[1] + w_neg * s[2]) / n);          // mean of nothing: NaN, as torch.mean
  out[1] = (float)w_neg;
  out[2] = (s[3] + s[4]) > 0 ? (float)(s[3] / (s[3] + s[4])) : 0.f;   // precision, zero denominator -> 0 (sklearn)
  out[3] = (s[3] + s[5]) > 0 ? (float)(s[3] / (s[3] + s[5])) : 0.f;   // recall
  out[4] = (float)s[3];
  out[5] = (float)s[4];
  out[6] = (float)s[5];
  out[7] = (float)n;
}

__global__ void k_bce_backward(const float* __restrict__ pred, const float* __restrict__ gt, int64_t n_max,
                               const int* __restrict__ n_dev, const float* __restrict__ out8,
                               const float* __restrict__ grad_out, const int* __restrict__ scatter_pos,
                               float* __restrict__ dpred) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int n = bce_n(n_max, n_dev);
  if (i >= n) return;
  const double p = pred[i], g = gt[i];
  const double w_neg = out8[1], w = g >= 0.5 ? 1.0 - w_neg : w_neg;
  // binary_cross_entropy_backward: (p - g) / max((1 - p) p, 1e-12)
  const double d = (double)grad_out[0] * w / (double)n * (p - g) / fmax((1.0 - p) * p, 1e-12);
  dpred[scatter_pos ? scatter_pos[i] : i] = (float)d;
}

// ---------------------------------------------------------------------------------------------------------------------
// mutual arg-max of inner products over gathered rows (:132-138), one direction
// ---------------------------------------------------------------------------------------------------------------------
// A workgroup of 4 waves owns 64 gathered rows of `a` (16 per wave, held as the MFMA A operand: lane l carries
// a[row l & 15][4 j + (l >> 4)], j = 0..7) and sweeps every gathered row of `b` in blocks of 64 staged through LDS
// (row stride 36 floats: the 16 x 4 operand read of a k-step touches 32 distinct banks per half wave).  A lane ends a
// block with the scores of rows 4 (l >> 4) + r, column l & 15 of each of the four 16-column tiles; it keeps its running
// maximum with a strict >, so the lowest column wins among equals, and the 16 lanes of a row group settle the row with
// the same rule at the end.
constexpr int AM_LD = 36;

__global__ __launch_bounds__(256) void k_gathered_argmax(const float* __restrict__ a, const int* __restrict__ a_idx,
                                                         const int* __restrict__ na_dev, int na_max,
                                                         const float* __restrict__ b, const int* __restrict__ b_idx,
                                                         const int* __restrict__ nb_dev, int nb_max,
                                                         int* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float s_b[64 * AM_LD];
  int na = *na_dev, nb = *nb_dev;
  na = na < na_max ? na : na_max;
  nb = nb < nb_max ? nb : nb_max;
  const int row0 = blockIdx.x * 64;
  if (row0 >= na) return;                                     // uniform over the block
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kq = lane >> 4, c16 = lane & 15;
  float av[ML_D / 4];
  {
    const int r = row0 + w * 16 + c16;
    const bool ok = r < na;
    const float* ar = a + (int64_t)(ok ? a_idx[r] : 0) * ML_D;
#pragma unroll
    for (int j = 0; j < ML_D / 4; ++j) av[j] = ok ? ar[4 * j + kq] : 0.f;
  }
  float bestv[4];
  int besti[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bestv[r] = -INFINITY, besti[r] = 0x7fffffff;
  for (int c0 = 0; c0 < nb; c0 += 64) {
    __syncthreads();
    {
      const int col = tid >> 2, part = tid & 3, c = c0 + col;
      float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
      if (c < nb) {
        const float4* p = (const float4*)(b + (int64_t)b_idx[c] * ML_D + part * 8);
        v0 = p[0];
        v1 = p[1];
      }
      float* d = s_b + col * AM_LD + part * 8;
      *(float4*)d = v0;
      *(float4*)(d + 4) = v1;
    }
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const float* bp = s_b + (cb * 16 + c16) * AM_LD + kq;
#pragma unroll
      for (int j = 0; j < ML_D / 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bp[4 * j], acc, 0, 0, 0);
      const int c = c0 + cb * 16 + c16;
      if (c < nb) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (acc[r] > bestv[r]) bestv[r] = acc[r], besti[r] = c;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = bestv[r];
    int i = besti[r];
    for (int d = 1; d < 16; d <<= 1) {
      const float ov = __shfl_xor(v, d);
      const int oi = __shfl_xor(i, d);
      if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
    }
    const int row = row0 + w * 16 + kq * 4 + r;
    if (c16 == 0 && row < na) out[row] = i == 0x7fffffff ? 0 : i;
  }
}

// saliency labels (:136-140) and the gathered saliency scores (:142-144)
__global__ void k_saliency_labels(const float* __restrict__ src_pcd, const float* __restrict__ tgt_pcd,
                                  const float* __restrict__ rot, const float* __restrict__ trans,
                                  const int* __restrict__ src_idx, const int* __restrict__ tgt_idx,
                                  const int* __restrict__ counts, const int* __restrict__ row_arg,
                                  const int* __restrict__ col_arg, const float* __restrict__ scores_saliency, int64_t n_src,
                                  int64_t n_tgt, float radius, float* __restrict__ labels, float* __restrict__ sel_scores,
                                  int* __restrict__ pos, float* __restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int ns = counts[0], nt = counts[1];
  ns = ns < n_src ? ns : (int)n_src;
  nt = nt < n_tgt ? nt : (int)n_tgt;
  if (i >= ns + nt) return;
  int s, t, where;
  if (i < ns) {
    int j = row_arg[i];
    j = j < nt ? j : nt - 1;
    s = src_idx[i], t = tgt_idx[j < 0 ? 0 : j], where = s;
  } else {
    int j = col_arg[i - ns];
    j = j < ns ? j : ns - 1;
    s = src_idx[j < 0 ? 0 : j], t = tgt_idx[i - ns], where = (int)n_src + t;
  }
  float p[3];
  rigid(rot, trans, src_pcd + 3 * (int64_t)s, p);
  const float dx = p[0] - tgt_pcd[3 * (int64_t)t], dy = p[1] - tgt_pcd[3 * (int64_t)t + 1],
              dz = p[2] - tgt_pcd[3 * (int64_t)t + 2];
  const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
  dist[i] = d;
  labels[i] = d < radius ? 1.f : 0.f;
  sel_scores[i] = scores_saliency[where];
  pos[i] = where;
}

// ---------------------------------------------------------------------------------------------------------------------
// circle loss + recall (:34-77, :153-167)
// ---------------------------------------------------------------------------------------------------------------------
// correspondences with c_dist < pos_radius - 0.001 (:153-155), compacted in their own order
__global__ __launch_bounds__(1024) void k_circle_select(const long long* __restrict__ corr, int64_t n_corr,
                                                        const float* __restrict__ src_pcd, int64_t n_src,
                                                        const float* __restrict__ tgt_pcd, int64_t n_tgt,
                                                        const float* __restrict__ rot, const float* __restrict__ trans,
                                                        float thresh, int* __restrict__ filt, int* __restrict__ count) {
  __shared__ int s_w[16];
  const int64_t per = (n_corr + blockDim.x - 1) / blockDim.x;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < n_corr ? lo + per : n_corr;
  auto keep = [&](int64_t i) {
    const long long s = corr[2 * i], t = corr[2 * i + 1];
    if (s < 0 || s >= n_src || t < 0 || t >= n_tgt) return false;
    float p[3];
    rigid(rot, trans, src_pcd + 3 * s, p);
    const float dx = p[0] - tgt_pcd[3 * t], dy = p[1] - tgt_pcd[3 * t + 1], dz = p[2] - tgt_pcd[3 * t + 2];
    return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) < thresh;
  };
  int cnt = 0;
  for (int64_t i = lo; i < hi; ++i) cnt += keep(i);
  int total;
  int off = block_excl_scan(cnt, &total, s_w);
  for (int64_t i = lo; i < hi; ++i)
    if (keep(i)) filt[off++] = (int)i;
  if (threadIdx.x == 0) *count = total;
}

// anchors = filtered[choice] (:156-162); a choice outside the filtered list leaves an absent anchor (row -1)
__global__ void k_circle_gather(const long long* __restrict__ corr, const int* __restrict__ filt,
                                const int* __restrict__ count, const long long* __restrict__ choice, int P,
                                const float* __restrict__ src_pcd, const float* __restrict__ tgt_pcd,
                                const float* __restrict__ src_feats, const float* __restrict__ tgt_feats,
                                const float* __restrict__ rot, const float* __restrict__ trans, int* __restrict__ a_row,
                                int* __restrict__ b_row, float* __restrict__ aP, float* __restrict__ bP,
                                float* __restrict__ aF, float* __restrict__ bF) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = g / ML_D, k = g % ML_D;
  if (p >= P) return;
  const long long c = choice[p];
  const bool ok = c >= 0 && c < *count;
  long long s = 0, t = 0;
  if (ok) {
    const int ci = filt[c];
    s = corr[2 * (int64_t)ci], t = corr[2 * (int64_t)ci + 1];
  }
  aF[p * ML_D + k] = ok ? src_feats[s * ML_D + k] : 0.f;
  bF[p * ML_D + k] = ok ? tgt_feats[t * ML_D + k] : 0.f;
  if (k == 0) {
    a_row[p] = ok ? (int)s : -1;
    b_row[p] = ok ? (int)t : -1;
    float q[3] = {0.f, 0.f, 0.f};
    if (ok) rigid(rot, trans, src_pcd + 3 * s, q);
    for (int r = 0; r < 3; ++r) aP[3 * p + r] = q[r], bP[3 * p + r] = ok ? tgt_pcd[3 * t + r] : 0.f;
  }
}

struct CircleParams {
  float pos_radius, safe_radius, pos_optimal, neg_optimal, pos_margin, neg_margin, log_scale;
};

constexpr int CL_LD = ML_D + 1;      // LDS row stride of the staged features: lane j reads row j, conflict-free
constexpr int CL_ROWS = 16;          // anchor rows (waves) per workgroup
constexpr int CL_T = ML_MAXP / 64;   // columns per lane
constexpr int CL_ST = 8;             // per-row record: lse_pos, lse_neg, loss, sel, has_pos, hit, sigmoid, -
static size_t circle_lds_bytes(int nb) { return (size_t)nb * (CL_LD + 3 + 1) * sizeof(float); }

// the other side's features, points and presence flags -> LDS
__device__ inline void circle_stage(const float* __restrict__ bF, const float* __restrict__ bP,
                                    const int* __restrict__ b_row, int nb, float* s_f, float* s_p, int* s_v) {
  for (int e = threadIdx.x; e < nb * ML_D; e += blockDim.x) s_f[(e / ML_D) * CL_LD + (e % ML_D)] = bF[e];
  for (int e = threadIdx.x; e < nb * 3; e += blockDim.x) s_p[e] = bP[e];
  for (int e = threadIdx.x; e < nb; e += blockDim.x) s_v[e] = b_row ? b_row[e] >= 0 : 1;
  __syncthreads();
}

// One entry (i, j): coordinate distance, feature distance (sqrt(clamp(., 1e-12)), lib/utils.py:78-98), the detached
// weights and the two exponents (:38-58).  An entry outside a mask has weight 0, i.e. exponent 0: it still adds exp(0)
// to its log-sum-exp, as in the reference.
struct CircleEntry {
  float cd, fd, s, pw, nw, ap, an;
  bool pos, neg;
};

template <bool DENSE>
__device__ inline CircleEntry circle_entry(int i, int j, const float* af, const float* ap3, const float* s_f,
                                           const float* s_p, const float* __restrict__ cdm,
                                           const float* __restrict__ fdm, int64_t si, int64_t sj, const CircleParams& q) {
  CircleEntry e;
  if (DENSE) {
    e.cd = cdm[i * si + j * sj];
    e.fd = fdm[i * si + j * sj];
    e.s = 0.f;
  } else {
    const float dx = ap3[0] - s_p[3 * j], dy = ap3[1] - s_p[3 * j + 1], dz = ap3[2] - s_p[3 * j + 2];
    e.cd = sqrtf(fmaxf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)), 1e-12f));
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < ML_D; ++k) s = fmaf(af[k], s_f[j * CL_LD + k], s);
    e.s = s;
    e.fd = sqrtf(fmaxf(2.f - 2.f * s, 1e-12f));
  }
  e.pos = e.cd < q.pos_radius;
  e.neg = e.cd > q.safe_radius;
  e.pw = fmaxf(0.f, (e.fd - (e.pos ? 0.f : 1e5f)) - q.pos_optimal);
  e.nw = fmaxf(0.f, q.neg_optimal - (e.fd + (e.neg ? 0.f : 1e5f)));
  e.ap = q.log_scale * (e.fd - q.pos_margin) * e.pw;
  e.an = q.log_scale * (q.neg_margin - e.fd) * e.nw;
  return e;
}

__device__ inline float wave_max(float v) {
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
__device__ inline float wave_sum(float v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// forward of one direction: wave = anchor row i of side a, lanes = the anchors of side b
template <bool DENSE>
__global__ __launch_bounds__(64 * CL_ROWS) void k_circle_rows(
    const float* __restrict__ aF, const float* __restrict__ aP, const int* __restrict__ a_row, int na,
    const float* __restrict__ bF, const float* __restrict__ bP, const int* __restrict__ b_row, int nb,
    const float* __restrict__ cdm, const float* __restrict__ fdm, int64_t si, int64_t sj, CircleParams q,
    float* __restrict__ st /*[na][CL_ST]*/, int* __restrict__ nn /*[na] or NULL*/) {
  extern __shared__ __attribute__((aligned(16))) float s_raw[];
  float* s_f = s_raw;
  float* s_p = s_f + (DENSE ? 0 : nb * CL_LD);
  int* s_v = (int*)(s_p + (DENSE ? 0 : nb * 3));
  if (!DENSE) circle_stage(bF, bP, b_row, nb, s_f, s_p, s_v);
  const int lane = threadIdx.x & 63, i = blockIdx.x * CL_ROWS + (threadIdx.x >> 6);
  if (i >= na) return;
  float* rec = st + (int64_t)i * CL_ST;
  if (!DENSE && a_row && a_row[i] < 0) {
    if (lane < CL_ST) rec[lane] = 0.f;
    if (nn && lane == 0) nn[i] = 0;
    return;
  }
  float af[ML_D], ap3[3] = {0.f, 0.f, 0.f};
  if (!DENSE) {
#pragma unroll
    for (int k = 0; k < ML_D; ++k) af[k] = aF[i * ML_D + k];
    for (int k = 0; k < 3; ++k) ap3[k] = aP[3 * i + k];
  }
  float ap[CL_T], an[CL_T];
  float mp = -INFINITY, mn = -INFINITY, bestd = INFINITY, bestcd = 0.f;
  int bestj = 0x7fffffff, anyp = 0, anyn = 0;
#pragma unroll
  for (int t = 0; t < CL_T; ++t) {
    const int j = lane + 64 * t;
    ap[t] = an[t] = -INFINITY;
    if (j < nb && (DENSE || s_v[j])) {
      const CircleEntry e = circle_entry<DENSE>(i, j, af, ap3, s_f, s_p, cdm, fdm, si, sj, q);
      ap[t] = e.ap, an[t] = e.an;
      mp = fmaxf(mp, e.ap), mn = fmaxf(mn, e.an);
      anyp |= e.pos, anyn |= e.neg;
      if (e.fd < bestd) bestd = e.fd, bestj = j, bestcd = e.cd;
    }
  }
  mp = wave_max(mp), mn = wave_max(mn);
  float sp = 0.f, sn = 0.f;
#pragma unroll
  for (int t = 0; t < CL_T; ++t) {
    sp += ap[t] == -INFINITY ? 0.f : expf(ap[t] - mp);
    sn += an[t] == -INFINITY ? 0.f : expf(an[t] - mn);
  }
  sp = wave_sum(sp), sn = wave_sum(sn);
  anyp = __any(anyp), anyn = __any(anyn);
  for (int d = 32; d >= 1; d >>= 1) {                          // torch.min: the lowest index among equals
    const float od = __shfl_xor(bestd, d), oc = __shfl_xor(bestcd, d);
    const int oj = __shfl_xor(bestj, d);
    if (od < bestd || (od == bestd && oj < bestj)) bestd = od, bestj = oj, bestcd = oc;
  }
  if (lane == 0) {
    const float lp = mp + logf(sp), ln = mn + logf(sn), z = lp + ln;
    rec[0] = lp;
    rec[1] = ln;
    rec[2] = (z > 20.f ? z : log1pf(expf(z))) / q.log_scale;    // F.softplus, threshold 20
    rec[3] = (anyp && anyn) ? 1.f : 0.f;
    rec[4] = anyp ? 1.f : 0.f;
    rec[5] = (anyp && bestcd < q.pos_radius) ? 1.f : 0.f;
    rec[6] = 1.f / (1.f + expf(-z));
    rec[7] = 0.f;
    if (nn) nn[i] = bestj == 0x7fffffff ? 0 : bestj;
  }
}

// means over the selected rows / columns (:63), recall (:72-76); out = circle, recall, #row_sel, #col_sel
__global__ void k_circle_final(const float* __restrict__ stA, int na, const float* __restrict__ stB, int nb,
                               float* __restrict__ out /*[4]*/) {
  const int lane = threadIdx.x;
  double v[6] = {0, 0, 0, 0, 0, 0};     // row loss, #row_sel, col loss, #col_sel, #has_pos, #hit
  for (int i = lane; i < na; i += 64) {
    const float* r = stA + (int64_t)i * CL_ST;
    if (r[3] != 0.f) v[0] += r[2], v[1] += 1.0;
    v[4] += r[4], v[5] += r[5];
  }
  for (int j = lane; j < nb; j += 64) {
    const float* r = stB + (int64_t)j * CL_ST;
    if (r[3] != 0.f) v[2] += r[2], v[3] += 1.0;
  }
  for (int k = 0; k < 6; ++k)
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
  if (lane == 0) {
    out[0] = (float)((v[0] / v[1] + v[2] / v[3]) / 2.0);       // an empty selection: 0 / 0 = NaN, as mean() of nothing
    out[1] = (float)(v[5] / (v[4] + 1e-12));
    out[2] = (float)v[1];
    out[3] = (float)v[3];
  }
}

// backward of one direction: d loss / d (features of side a), or d loss / d feats_dist for dense inputs.  Every entry
// carries its row term and its column term, so one launch per side sees the whole gradient of its anchors.
template <bool DENSE>
__global__ __launch_bounds__(64 * CL_ROWS) void k_circle_bwd_rows(
    const float* __restrict__ aF, const float* __restrict__ aP, const int* __restrict__ a_row, int na,
    const float* __restrict__ bF, const float* __restrict__ bP, const int* __restrict__ b_row, int nb,
    const float* __restrict__ cdm, const float* __restrict__ fdm, int64_t si, int64_t sj, CircleParams q,
    const float* __restrict__ stA, const float* __restrict__ stB, const float* __restrict__ fin, int ia, int ib,
    const float* __restrict__ grad_out, float* __restrict__ dA /*[na][D]*/, float* __restrict__ dfd /*dense*/) {
  extern __shared__ __attribute__((aligned(16))) float s_raw[];
  float* s_f = s_raw;
  float* s_p = s_f + (DENSE ? 0 : nb * CL_LD);
  int* s_v = (int*)(s_p + (DENSE ? 0 : nb * 3));
  if (!DENSE) circle_stage(bF, bP, b_row, nb, s_f, s_p, s_v);
  const int lane = threadIdx.x & 63, i = blockIdx.x * CL_ROWS + (threadIdx.x >> 6);
  if (i >= na) return;
  float acc[ML_D];
#pragma unroll
  for (int k = 0; k < ML_D; ++k) acc[k] = 0.f;
  const bool present = DENSE || !a_row || a_row[i] >= 0;
  if (present) {
    float af[ML_D], ap3[3] = {0.f, 0.f, 0.f};
    if (!DENSE) {
#pragma unroll
      for (int k = 0; k < ML_D; ++k) af[k] = aF[i * ML_D + k];
      for (int k = 0; k < 3; ++k) ap3[k] = aP[3 * i + k];
    }
    const float* ra = stA + (int64_t)i * CL_ST;
    const float g = 0.5f * grad_out[0];
    const float nA = fin[ia], nB = fin[ib];
    const float ca = (ra[3] != 0.f && nA > 0.f) ? g * ra[6] / nA : 0.f;
    const float lpa = ra[0], lna = ra[1];
    for (int t = 0; t < CL_T; ++t) {
      const int j = lane + 64 * t;
      if (j >= nb) break;
      float G = 0.f;
      if (DENSE || s_v[j]) {
        const CircleEntry e = circle_entry<DENSE>(i, j, af, ap3, s_f, s_p, cdm, fdm, si, sj, q);
        const float* rb = stB + (int64_t)j * CL_ST;
        const float cb = (rb[3] != 0.f && nB > 0.f) ? g * rb[6] / nB : 0.f;
        G = ca * (expf(e.ap - lpa) * e.pw - expf(e.an - lna) * e.nw) +
            cb * (expf(e.ap - rb[0]) * e.pw - expf(e.an - rb[1]) * e.nw);
        if (!DENSE) {
          const float Gs = (2.f - 2.f * e.s > 1e-12f) ? -G / e.fd : 0.f;   // clamp: zero gradient where it binds
#pragma unroll
          for (int k = 0; k < ML_D; ++k) acc[k] = fmaf(Gs, s_f[j * CL_LD + k], acc[k]);
        }
      }
      if (DENSE) dfd[i * si + j * sj] = G;
    }
  }
  if (!DENSE) {
#pragma unroll
    for (int k = 0; k < ML_D; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < ML_D; ++k) dA[i * ML_D + k] = acc[k];
    }
  }
}

// d loss / d full rows: anchors that share a row are added in ascending anchor order by the first of them
__global__ void k_circle_scatter(const float* __restrict__ dA, const int* __restrict__ a_row, int P,
                                 float* __restrict__ dfull, int64_t n_rows) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = g / ML_D, k = g % ML_D;
  if (p >= P) return;
  const int row = a_row[p];
  if (row < 0 || row >= n_rows) return;
  for (int qx = 0; qx < p; ++qx)
    if (a_row[qx] == row) return;
  float s = dA[p * ML_D + k];
  for (int qx = p + 1; qx < P; ++qx)
    if (a_row[qx] == row) s += dA[qx * ML_D + k];
  dfull[(int64_t)row * ML_D + k] = s;
}

int circle_params(const float* h, CircleParams* q) {
  APR_CHECK_ARG(h != nullptr, "circle loss: params_host is NULL");
  q->pos_radius = h[0], q->safe_radius = h[1], q->pos_optimal = h[2], q->neg_optimal = h[3];
  q->pos_margin = h[4], q->neg_margin = h[5], q->log_scale = h[6];
  return APR_OK;
}

// more than 64 KB of dynamic LDS has to be asked for once per kernel and device
template <typename K>
int circle_lds_attr(K kernel, size_t bytes) {
  static bool granted[64] = {};
  if (bytes <= 64 * 1024) return APR_OK;
  int dev = 0;
  APR_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && granted[dev]) return APR_OK;
  APR_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)circle_lds_bytes(ML_MAXP)));
  if (dev >= 0 && dev < 64) granted[dev] = true;
  return APR_OK;
}

}  // namespace

APR_API int apr_overlap_labels(const int64_t* corr, int64_t n_corr, int64_t n_src, int64_t n_tgt, float* gt,
                               int32_t* src_idx, int32_t* tgt_idx, int32_t* counts3, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_corr >= 0 && n_src > 0 && n_tgt > 0 && n_src + n_tgt < (1ll << 31), "apr_overlap_labels: bad sizes");
  hipLaunchKernelGGL(k_labels_clear, dim3((unsigned)cdiv64(n_src + n_tgt, 256)), dim3(256), 0, st, n_src, n_tgt, gt);
  if (n_corr > 0)
    hipLaunchKernelGGL(k_labels_set, dim3((unsigned)cdiv64(n_corr, 256)), dim3(256), 0, st, (const long long*)corr,
                       n_corr, n_src, n_tgt, gt);
  hipLaunchKernelGGL(k_labels_compact, dim3(1), dim3(1024), 0, st, gt, n_src, n_tgt, src_idx, tgt_idx, counts3);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API size_t apr_weighted_bce_scratch_bytes(void) { return (size_t)BCE_MAX_BLOCKS * BCE_Q * sizeof(double); }

APR_API int apr_weighted_bce_forward(const float* pred, const float* gt, int64_t n, const int32_t* n_dev, float* out8,
                                     void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n >= 0 && n < (1ll << 31), "apr_weighted_bce_forward: bad size");
  APR_CHECK_ARG(scratch_bytes >= apr_weighted_bce_scratch_bytes(), "apr_weighted_bce_forward: scratch too small");
  int nblocks = (int)cdiv64(n, 256);
  nblocks = nblocks < 1 ? 1 : (nblocks > BCE_MAX_BLOCKS ? BCE_MAX_BLOCKS : nblocks);
  hipLaunchKernelGGL(k_bce_partial, dim3(nblocks), dim3(256), 0, st, pred, gt, n, (const int*)n_dev, (double*)scratch);
  hipLaunchKernelGGL(k_bce_final, dim3(1), dim3(64), 0, st, (const double*)scratch, nblocks, n, (const int*)n_dev, out8);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_weighted_bce_backward(const float* pred, const float* gt, int64_t n, const int32_t* n_dev,
                                      const float* out8, const float* grad_out, const int32_t* scatter_pos, float* dpred,
                                      void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n >= 0 && n < (1ll << 31), "apr_weighted_bce_backward: bad size");
  if (n == 0) return APR_OK;
  hipLaunchKernelGGL(k_bce_backward, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, pred, gt, n, (const int*)n_dev,
                     out8, grad_out, (const int*)scatter_pos, dpred);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_gathered_argmax(const float* a, const int32_t* a_idx, const int32_t* na_dev, int64_t na_max, const float* b,
                                const int32_t* b_idx, const int32_t* nb_dev, int64_t nb_max, int32_t d, int32_t* row_arg,
                                int32_t* col_arg, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(d == ML_D, "apr_gathered_argmax: feature width %d is not covered (need %d)", d, ML_D);
  APR_CHECK_ARG(na_max > 0 && nb_max > 0 && na_max < (1ll << 31) && nb_max < (1ll << 31), "apr_gathered_argmax: bad sizes");
  APR_CHECK_ARG(a && b && a_idx && b_idx && na_dev && nb_dev && row_arg && col_arg, "apr_gathered_argmax: NULL argument");
  APR_CHECK_ARG(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0, "apr_gathered_argmax: rows must be 16-byte aligned");
  hipLaunchKernelGGL(k_gathered_argmax, dim3((unsigned)cdiv64(na_max, 64)), dim3(256), 0, st, a, (const int*)a_idx,
                     (const int*)na_dev, (int)na_max, b, (const int*)b_idx, (const int*)nb_dev, (int)nb_max, row_arg);
  hipLaunchKernelGGL(k_gathered_argmax, dim3((unsigned)cdiv64(nb_max, 64)), dim3(256), 0, st, b, (const int*)b_idx,
                     (const int*)nb_dev, (int)nb_max, a, (const int*)a_idx, (const int*)na_dev, (int)na_max, col_arg);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_saliency_labels(const float* src_pcd, const float* tgt_pcd, const float* rot9, const float* trans3,
                                const int32_t* src_idx, const int32_t* tgt_idx, const int32_t* counts3,
                                const int32_t* row_arg, const int32_t* col_arg, const float* scores_saliency, int64_t n_src,
                                int64_t n_tgt, float radius, float* labels, float* sel_scores, int32_t* pos, float* dist,
                                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_src > 0 && n_tgt > 0 && n_src + n_tgt < (1ll << 31), "apr_saliency_labels: bad sizes");
  hipLaunchKernelGGL(k_saliency_labels, dim3((unsigned)cdiv64(n_src + n_tgt, 256)), dim3(256), 0, st, src_pcd, tgt_pcd, rot9,
                     trans3, (const int*)src_idx, (const int*)tgt_idx, (const int*)counts3, (const int*)row_arg,
                     (const int*)col_arg, scores_saliency, n_src, n_tgt, radius, labels, sel_scores, (int*)pos, dist);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_circle_select(const int64_t* corr, int64_t n_corr, const float* src_pcd, int64_t n_src, const float* tgt_pcd,
                              int64_t n_tgt, const float* rot9, const float* trans3, float thresh, int32_t* filt,
                              int32_t* count, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_corr >= 0 && n_corr < (1ll << 31) && n_src > 0 && n_tgt > 0, "apr_circle_select: bad sizes");
  hipLaunchKernelGGL(k_circle_select, dim3(1), dim3(1024), 0, st, (const long long*)corr, n_corr, src_pcd, n_src, tgt_pcd,
                     n_tgt, rot9, trans3, thresh, (int*)filt, (int*)count);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_circle_gather(const int64_t* corr, const int32_t* filt, const int32_t* count, const int64_t* choice,
                              int32_t p, const float* src_pcd, const float* tgt_pcd, const float* src_feats,
                              const float* tgt_feats, int32_t d, const float* rot9, const float* trans3, int32_t* a_row,
                              int32_t* b_row, float* a_pts, float* b_pts, float* a_feats, float* b_feats, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(d == ML_D, "apr_circle_gather: feature width %d is not covered (need %d)", d, ML_D);
  APR_CHECK_ARG(p > 0 && p <= ML_MAXP, "apr_circle_gather: %d anchors (1 .. %d covered)", p, ML_MAXP);
  hipLaunchKernelGGL(k_circle_gather, dim3((unsigned)cdiv64((int64_t)p * ML_D, 256)), dim3(256), 0, st,
                     (const long long*)corr, (const int*)filt, (const int*)count, (const long long*)choice, p, src_pcd,
                     tgt_pcd, src_feats, tgt_feats, rot9, trans3, (int*)a_row, (int*)b_row, a_pts, b_pts, a_feats, b_feats);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_circle_forward(const float* a_feats, const float* a_pts, const int32_t* a_row, int32_t na,
                               const float* b_feats, const float* b_pts, const int32_t* b_row, int32_t nb,
                               const float* coords_dist, const float* feats_dist, const float* params_host, float* st_a,
                               float* st_b, float* out4, int32_t* nn, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CircleParams q;
  if (int rc = circle_params(params_host, &q)) return rc;
  APR_CHECK_ARG(na > 0 && nb > 0 && na <= ML_MAXP && nb <= ML_MAXP, "apr_circle_forward: %d x %d anchors (1 .. %d covered)",
                na, nb, ML_MAXP);
  const bool dense = coords_dist != nullptr;
  APR_CHECK_ARG(dense ? feats_dist != nullptr : (a_feats && b_feats && a_pts && b_pts),
                "apr_circle_forward: give the two distance matrices or the gathered anchors");
  const dim3 blk(64 * CL_ROWS);
  if (dense) {
    hipLaunchKernelGGL(k_circle_rows<true>, dim3((unsigned)cdiv64(na, CL_ROWS)), blk, 0, st, nullptr, nullptr, nullptr, na,
                       nullptr, nullptr, nullptr, nb, coords_dist, feats_dist, (int64_t)nb, (int64_t)1, q, st_a, (int*)nn);
    hipLaunchKernelGGL(k_circle_rows<true>, dim3((unsigned)cdiv64(nb, CL_ROWS)), blk, 0, st, nullptr, nullptr, nullptr, nb,
                       nullptr, nullptr, nullptr, na, coords_dist, feats_dist, (int64_t)1, (int64_t)nb, q, st_b,
                       (int*)nullptr);
  } else {
    if (int rc = circle_lds_attr(k_circle_rows<false>, circle_lds_bytes(na > nb ? na : nb))) return rc;
    hipLaunchKernelGGL(k_circle_rows<false>, dim3((unsigned)cdiv64(na, CL_ROWS)), blk, circle_lds_bytes(nb), st, a_feats,
                       a_pts, (const int*)a_row, na, b_feats, b_pts, (const int*)b_row, nb, nullptr, nullptr, (int64_t)0,
                       (int64_t)0, q, st_a, (int*)nn);
    hipLaunchKernelGGL(k_circle_rows<false>, dim3((unsigned)cdiv64(nb, CL_ROWS)), blk, circle_lds_bytes(na), st, b_feats,
                       b_pts, (const int*)b_row, nb, a_feats, a_pts, (const int*)a_row, na, nullptr, nullptr, (int64_t)0,
                       (int64_t)0, q, st_b, (int*)nullptr);
  }
  hipLaunchKernelGGL(k_circle_final, dim3(1), dim3(64), 0, st, st_a, na, st_b, nb, out4);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_circle_backward(const float* a_feats, const float* a_pts, const int32_t* a_row, int32_t na,
                                const float* b_feats, const float* b_pts, const int32_t* b_row, int32_t nb,
                                const float* coords_dist, const float* feats_dist, const float* params_host,
                                const float* st_a, const float* st_b, const float* out4, const float* grad_out, float* d_a,
                                float* d_b, float* d_feats_dist, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CircleParams q;
  if (int rc = circle_params(params_host, &q)) return rc;
  APR_CHECK_ARG(na > 0 && nb > 0 && na <= ML_MAXP && nb <= ML_MAXP, "apr_circle_backward: %d x %d anchors (1 .. %d covered)",
                na, nb, ML_MAXP);
  const bool dense = coords_dist != nullptr;
  APR_CHECK_ARG(dense ? (feats_dist && d_feats_dist) : (a_feats && b_feats && a_pts && b_pts && d_a && d_b),
                "apr_circle_backward: give the two distance matrices or the gathered anchors");
  const dim3 blk(64 * CL_ROWS);
  if (dense) {
    hipLaunchKernelGGL(k_circle_bwd_rows<true>, dim3((unsigned)cdiv64(na, CL_ROWS)), blk, 0, st, nullptr, nullptr, nullptr,
                       na, nullptr, nullptr, nullptr, nb, coords_dist, feats_dist, (int64_t)nb, (int64_t)1, q, st_a, st_b,
                       out4, 2, 3, grad_out, (float*)nullptr, d_feats_dist);
  } else {
    if (int rc = circle_lds_attr(k_circle_bwd_rows<false>, circle_lds_bytes(na > nb ? na : nb))) return rc;
    hipLaunchKernelGGL(k_circle_bwd_rows<false>, dim3((unsigned)cdiv64(na, CL_ROWS)), blk, circle_lds_bytes(nb), st,
                       a_feats, a_pts, (const int*)a_row, na, b_feats, b_pts, (const int*)b_row, nb, nullptr, nullptr,
                       (int64_t)0, (int64_t)0, q, st_a, st_b, out4, 2, 3, grad_out, d_a, (float*)nullptr);
    hipLaunchKernelGGL(k_circle_bwd_rows<false>, dim3((unsigned)cdiv64(nb, CL_ROWS)), blk, circle_lds_bytes(na), st,
                       b_feats, b_pts, (const int*)b_row, nb, a_feats, a_pts, (const int*)a_row, na, nullptr, nullptr,
                       (int64_t)0, (int64_t)0, q, st_b, st_a, out4, 3, 2, grad_out, d_b, (float*)nullptr);
  }
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_circle_scatter(const float* d_anchor, const int32_t* row, int32_t p, int32_t d, float* d_full,
                               int64_t n_rows, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(d == ML_D && p > 0 && p <= ML_MAXP && n_rows > 0, "apr_circle_scatter: bad arguments");
  hipLaunchKernelGGL(k_circle_scatter, dim3((unsigned)cdiv64((int64_t)p * ML_D, 256)), dim3(256), 0, st, d_anchor,
                     (const int*)row, p, d_full, n_rows);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

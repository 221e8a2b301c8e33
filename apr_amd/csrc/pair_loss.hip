// Pair-list losses of the FCGF trainers: random-negative contrastive, triplet and hardest triplet.
//
// Reference: FCGF_APR/lib/trainer.py:254-267 (ContrastiveLossTrainer), :532-579 (TripletLossTrainer.triplet_loss),
// :658-731 (HardestTripletLossTrainer.triplet_loss).  All three are sums over cross-cloud row pairs (r0[t], r1[t]) of a
// function of d_t = |F0[r0] - F1[r1]|^2 or sqrt(d_t + eps); a triplet term is two such pairs.  The reference copies arg-min
// indices to the host, filters with np.isin on int64 keys and indexes with host-known sizes.  Here:
//   apr_pair_rows_from_nn  packed apr_feature_nn results -> rows of the full cloud (the mined pairs of the list);
//   apr_pair_dist          one distance per pair, difference-square form (lib/metrics.py:22-29);
//   apr_pair_terms_reduce  key filter (binary search in the sorted positive keys), hinge per term, sums and counts per group
//                          in a fixed order, and per pair the coefficient of (F0[r0] - F1[r1]) in the gradient;
//   apr_pair_grad          dF0[r] = sum over the pairs with r0 = r, in list order, of coef * scale * (F0[r] - F1[r1]), and
//                          the mirrored sum for dF1, through the reverse table of revtable.hip: no float atomics.
// Nothing comes back to the host: the 1 / count of every mean is read from device memory by apr_pair_grad.
#include <math.h>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLanes = 8;      // lanes that share one pair's row: 4 channels each per step
constexpr int kBlock = 256;

__global__ void k_rows_from_nn(const unsigned long long* __restrict__ best, int64_t p, const long long* __restrict__ sel, int64_t m,
                               int* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p) return;
  const unsigned long long j = best[i] & 0xffffffffull;
  rows[i] = j < (unsigned long long)m ? (int)sel[j] : -1;      // -1: a row of no cloud, its distance becomes NaN
}

// kLanes lanes per pair; lane l takes the channels 4 * (l + kLanes * k), then a butterfly over the kLanes lanes
__global__ void k_pair_dist(const float* __restrict__ F0, int64_t N0, const float* __restrict__ F1, int64_t N1, int c,
                            const int* __restrict__ r0, const int* __restrict__ r1, int64_t n, int64_t n_plain, float eps,
                            float* __restrict__ d, float* __restrict__ coef, int* __restrict__ grp) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pair = gid / kLanes;
  const int lane = (int)(gid % kLanes);
  const bool ok = pair < n;
  const int64_t a = ok ? r0[pair] : -1, b = ok ? r1[pair] : -1;
  const bool in = a >= 0 && a < N0 && b >= 0 && b < N1;
  float acc = 0.f;
  if (in) {
    const float* x = F0 + a * c;
    const float* y = F1 + b * c;
    for (int col = lane * 4; col < c; col += kLanes * 4) {
      const f32x4 e = *reinterpret_cast<const f32x4*>(x + col) - *reinterpret_cast<const f32x4*>(y + col);
      acc = fmaf(e.x, e.x, acc);
      acc = fmaf(e.y, e.y, acc);
      acc = fmaf(e.z, e.z, acc);
      acc = fmaf(e.w, e.w, acc);
    }
  }
  for (int dd = 1; dd < kLanes; dd <<= 1) acc += __shfl_xor(acc, dd);
  if (ok && lane == 0) {
    d[pair] = !in ? NAN : (pair < n_plain ? acc : sqrtf(acc + eps));
    coef[pair] = 0.f;
    grp[pair] = 0;
  }
}

__device__ inline bool key_in_sorted(const long long* __restrict__ keys, int64_t n, long long k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo < n && keys[lo] == k;
}

// term = (pa, pb, kp, kind | group << 8).  One thread per term; per group the block's sum and count in a fixed order: a
// butterfly inside every wave, then the waves in ascending order.
__global__ void k_pair_terms(const float* __restrict__ d, const int* __restrict__ r0, const int* __restrict__ r1, int64_t n,
                             const int4* __restrict__ terms, int64_t T, const long long* __restrict__ keys, int64_t nkeys,
                             long long hash_seed, float margin, int G, float* __restrict__ coef, int* __restrict__ grp,
                             unsigned char* __restrict__ kept, double* __restrict__ partial) {
  __shared__ double sh[kBlock / 64][2 * APR_PAIR_MAX_GROUPS];
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  float v = 0.f;
  int g = -1;
  if (t < T) {
    const int4 tm = terms[t];
    const int kind = tm.w & 0xff;
    const int tg = tm.w >> 8;
    const bool pa_ok = tm.x >= 0 && tm.x < n, pb_ok = tm.y >= 0 && tm.y < n;
    const bool shaped = tg >= 0 && tg < G &&
                        (kind == APR_PAIR_TERM_STAT || kind == APR_PAIR_TERM_SQ ? pa_ok
                         : kind == APR_PAIR_TERM_NEG ? pb_ok : kind == APR_PAIR_TERM_TRIPLET ? (pa_ok && pb_ok) : false);
    bool keep = shaped;
    if (keep && tm.z >= 0) keep = tm.z < n && !key_in_sorted(keys, nkeys, (long long)r0[tm.z] + (long long)r1[tm.z] * hash_seed);
    if (keep) {
      g = tg;
      if (kind == APR_PAIR_TERM_STAT) {
        v = d[tm.x];
      } else if (kind == APR_PAIR_TERM_SQ) {
        v = d[tm.x];
        coef[tm.x] = 2.f;
        grp[tm.x] = g;
      } else if (kind == APR_PAIR_TERM_NEG) {
        const float dn = d[tm.y];
        const float r = fmaxf(margin - dn, 0.f);
        v = dn != dn ? dn : r * r;
        if (r > 0.f) {
          coef[tm.y] = -2.f * r / dn;
          grp[tm.y] = g;
        }
      } else {
        const float dp = d[tm.x], dn = d[tm.y];
        const float h = dp + margin - dn;
        v = h != h ? h : fmaxf(h, 0.f);
        if (h > 0.f) {
          coef[tm.x] = 1.f / dp;
          coef[tm.y] = -1.f / dn;
          grp[tm.x] = g;
          grp[tm.y] = g;
        }
      }
    }
    if (kept) kept[t] = keep ? 1 : 0;
  }
  const int wave = threadIdx.x >> 6;
  for (int k = 0; k < G; ++k) {
    double s = g == k ? (double)v : 0.0, m = g == k ? 1.0 : 0.0;
    for (int dd = 32; dd >= 1; dd >>= 1) {
      s += __shfl_xor(s, dd);
      m += __shfl_xor(m, dd);
    }
    if ((threadIdx.x & 63) == 0) {
      sh[wave][2 * k] = s;
      sh[wave][2 * k + 1] = m;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * G) {
    double s = sh[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) s += sh[w][threadIdx.x];
    partial[(int64_t)blockIdx.x * 2 * APR_PAIR_MAX_GROUPS + threadIdx.x] = s;
  }
}

// one block: the blocks' partial sums in ascending block order; red = {sum, count} per group, mean = sum / count (NaN for
// an empty group, as torch.mean of an empty tensor)
__global__ void k_pair_terms_finish(const double* __restrict__ partial, int64_t nblk, int G, double* __restrict__ red,
                                    float* __restrict__ mean) {
  __shared__ double sh[2 * APR_PAIR_MAX_GROUPS];
  if (threadIdx.x < 2 * G) {
    double s = 0.0;
    for (int64_t b = 0; b < nblk; ++b) s += partial[b * 2 * APR_PAIR_MAX_GROUPS + threadIdx.x];
    sh[threadIdx.x] = s;
    red[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x < G) mean[threadIdx.x] = (float)(sh[2 * threadIdx.x] / sh[2 * threadIdx.x + 1]);
}

// thread = (destination row s of Fa, 4 channels): the row's pairs in list order.  A pair whose coefficient is exactly 0
// (inactive hinge, filtered term, statistic only) adds nothing -- not 0 * scale, which is NaN for an empty group.
__global__ void k_pair_grad(const float* __restrict__ Fa, int64_t Na, const float* __restrict__ Fb, int64_t Nb, int c,
                            const int* __restrict__ rb, const int* __restrict__ rev_t, const int* __restrict__ start,
                            const float* __restrict__ coef, const int* __restrict__ grp, const double* __restrict__ red,
                            const float* __restrict__ gout, int n_gout, float* __restrict__ out) {
  const int c4 = c >> 2;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= Na * c4) return;
  const int64_t s = tid / c4;
  const int col = (int)(tid - s * c4) * 4;
  const int e0 = start[s], e1 = start[s + 1];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (e0 < e1) {
    float scale[APR_PAIR_MAX_GROUPS];
#pragma unroll
    for (int k = 0; k < APR_PAIR_MAX_GROUPS; ++k) scale[k] = k < n_gout ? (float)((double)gout[k] / red[2 * k + 1]) : 0.f;
    const f32x4 x = *reinterpret_cast<const f32x4*>(Fa + s * c + col);
    for (int e = e0; e < e1; ++e) {
      const int t = rev_t[e];
      const float cf = coef[t];
      const int64_t j = rb[t];
      const int g = grp[t];
      if (cf != 0.f && j >= 0 && j < Nb && g >= 0 && g < n_gout) {
        float sc = scale[0];
#pragma unroll
        for (int k = 1; k < APR_PAIR_MAX_GROUPS; ++k) sc = g == k ? scale[k] : sc;
        const f32x4 y = *reinterpret_cast<const f32x4*>(Fb + j * c + col);
        acc += (cf * sc) * (x - y);
      }
    }
  }
  *reinterpret_cast<f32x4*>(out + s * c + col) = acc;
}

bool feat_ok(const float* F0, const float* F1, int32_t c) {
  return F0 && F1 && c > 0 && c % 4 == 0 && c <= 256 && ((((uintptr_t)F0) | ((uintptr_t)F1)) & 15) == 0;
}

struct TermScratch {
  double* partial;   // [nblk][2 * APR_PAIR_MAX_GROUPS]
  int64_t nblk;
};
TermScratch walk_terms(AprArena& a, int64_t T) {
  TermScratch s;
  s.nblk = cdiv64(T, kBlock);
  s.partial = a.take<double>((size_t)s.nblk * 2 * APR_PAIR_MAX_GROUPS);
  return s;
}

struct GradScratch {
  int *rev0, *start0, *rev1, *start1;
  void* rev;          // revtable.hip's own scratch, used for one table after the other
  size_t rev_bytes;
};
GradScratch walk_grad(AprArena& a, int64_t n, int64_t N0, int64_t N1) {
  GradScratch s;
  s.rev0 = a.take<int>(n);
  s.start0 = a.take<int>(N0 + 1);
  s.rev1 = a.take<int>(n);
  s.start1 = a.take<int>(N1 + 1);
  const size_t b0 = apr_reverse_table_scratch_bytes(n, 1, N0), b1 = apr_reverse_table_scratch_bytes(n, 1, N1);
  s.rev_bytes = b0 > b1 ? b0 : b1;
  s.rev = a.take<char>(s.rev_bytes);
  return s;
}

}  // namespace

APR_API int apr_pair_rows_from_nn(const uint64_t* best, int64_t p, const int64_t* sel, int64_t m, int32_t* rows, void* stream) {
  APR_CHECK_ARG(best && sel && rows && p > 0 && m > 0, "apr_pair_rows_from_nn: bad arguments");
  hipLaunchKernelGGL(k_rows_from_nn, dim3((unsigned)cdiv64(p, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     (const unsigned long long*)best, p, (const long long*)sel, m, rows);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_pair_dist(const float* F0, int64_t N0, const float* F1, int64_t N1, int32_t c, const int32_t* r0, const int32_t* r1,
                          int64_t n, int64_t n_plain, float eps, float* d, float* coef, int32_t* grp, void* stream) {
  APR_CHECK_ARG(feat_ok(F0, F1, c), "apr_pair_dist: needs 16-byte aligned fp32 rows with c %% 4 == 0 and c <= 256, got c=%d", c);
  APR_CHECK_ARG(r0 && r1 && d && coef && grp && N0 > 0 && N1 > 0 && n > 0 && n < (1ll << 31) && n_plain >= 0 && eps >= 0.f,
                "apr_pair_dist: bad arguments");
  hipLaunchKernelGGL(k_pair_dist, dim3((unsigned)cdiv64(n * kLanes, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, F0, N0, F1, N1,
                     c, r0, r1, n, n_plain, eps, d, coef, grp);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API size_t apr_pair_terms_scratch_bytes(int64_t n_terms) {
  if (n_terms <= 0) return 0;
  AprArena a(nullptr);
  walk_terms(a, n_terms);
  return a.bytes();
}

APR_API int apr_pair_terms_reduce(const float* d, const int32_t* r0, const int32_t* r1, int64_t n, const int32_t* terms,
                                  int64_t n_terms, const int64_t* sorted_pos_keys, int64_t n_keys, int64_t hash_seed,
                                  float margin, int32_t n_groups, double* red, float* mean, float* coef, int32_t* grp,
                                  uint8_t* kept, void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(d && r0 && r1 && terms && red && mean && coef && grp && scratch && n > 0 && n < (1ll << 31) && n_terms > 0 &&
                    n_terms < (1ll << 31) && n_keys >= 0 && (n_keys == 0 || sorted_pos_keys) && n_groups > 0 &&
                    n_groups <= APR_PAIR_MAX_GROUPS && (((uintptr_t)terms) & 15) == 0,
                "apr_pair_terms_reduce: bad arguments");
  AprArena arena(scratch);
  TermScratch s = walk_terms(arena, n_terms);
  APR_CHECK_ARG(arena.fits(scratch_bytes), "apr_pair_terms_reduce: scratch too small");
  hipLaunchKernelGGL(k_pair_terms, dim3((unsigned)s.nblk), dim3(kBlock), 0, st, d, r0, r1, n, (const int4*)terms, n_terms,
                     (const long long*)sorted_pos_keys, n_keys, (long long)hash_seed, margin, n_groups, coef, grp, kept, s.partial);
  hipLaunchKernelGGL(k_pair_terms_finish, dim3(1), dim3(64), 0, st, (const double*)s.partial, s.nblk, n_groups, red, mean);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API size_t apr_pair_grad_scratch_bytes(int64_t n, int64_t N0, int64_t N1) {
  if (n <= 0 || N0 <= 0 || N1 <= 0) return 0;
  AprArena a(nullptr);
  walk_grad(a, n, N0, N1);
  return a.bytes();
}

APR_API int apr_pair_grad(const float* F0, int64_t N0, const float* F1, int64_t N1, int32_t c, const int32_t* r0, const int32_t* r1,
                          int64_t n, const float* coef, const int32_t* grp, const double* red, const float* gout, int32_t n_gout,
                          float* dF0, float* dF1, void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(feat_ok(F0, F1, c) && feat_ok(dF0, dF1, c),
                "apr_pair_grad: needs 16-byte aligned fp32 rows with c %% 4 == 0 and c <= 256, got c=%d", c);
  APR_CHECK_ARG(r0 && r1 && coef && grp && red && gout && scratch && N0 > 0 && N1 > 0 && N0 < (1ll << 30) && N1 < (1ll << 30) &&
                    n > 0 && n < (1ll << 31) && n_gout > 0 && n_gout <= APR_PAIR_MAX_GROUPS,
                "apr_pair_grad: bad arguments");
  AprArena arena(scratch);
  GradScratch s = walk_grad(arena, n, N0, N1);
  APR_CHECK_ARG(arena.fits(scratch_bytes), "apr_pair_grad: scratch too small");
  int rc = apr_reverse_table_build(r0, n, 1, N0, s.rev0, s.start0, s.rev, s.rev_bytes, stream);
  if (rc != APR_OK) return rc;
  hipLaunchKernelGGL(k_pair_grad, dim3((unsigned)cdiv64(N0 * (c / 4), kBlock)), dim3(kBlock), 0, st, F0, N0, F1, N1, c, r1,
                     (const int*)s.rev0, (const int*)s.start0, coef, grp, red, gout, n_gout, dF0);
  rc = apr_reverse_table_build(r1, n, 1, N1, s.rev1, s.start1, s.rev, s.rev_bytes, stream);
  if (rc != APR_OK) return rc;
  hipLaunchKernelGGL(k_pair_grad, dim3((unsigned)cdiv64(N1 * (c / 4), kBlock)), dim3(kBlock), 0, st, F1, N1, F0, N0, c, r0,
                     (const int*)s.rev1, (const int*)s.start1, coef, grp, red, gout, n_gout, dF1);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

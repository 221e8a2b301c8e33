// Geometric cross attention of Predator's overlap-attention module ('cross_cat': MultiHeadedAttentionCat, gcn.py:131-156).
// Per head h and query i, with P = softmax_j(<q_i, k_j>_h / sqrt(dim)) over the OTHER cloud (the scale uses dim, not dim + 3):
//   feat[d] = sum_j P_ij v[j, d, h]      soft[a] = sum_j P_ij c1[j, a]      aug1 = soft - c0[i]      aug2 = ||aug1||_2
// written as one row y[i, e * heads + h], e in [0, dim + 7): feat | soft | aug1 | aug2, leading dimension ldy (columns from
// (dim + 7) * heads on are the caller's: a caller that pads the row to the GEMM's granule zeroes them once).  The three
// coordinate columns ride beside the value columns; no concatenated value tensor exists.  Inference: k_mha_cat_mfma, the
// sibling of k_mha_mfma (attention.hip).  Training: P from k_mha_probs, the rows from it; backward from P, y and dy with
// every sum in a fixed order (no float atomics: the same bits every run).  Coordinates take no gradient.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// k_mha_mfma (attention.hip) with three more columns: q / k / v HEAD-MAJOR (channel h * 64 + d), a workgroup owns 16 queries
// of ONE head, its 4 waves walk the 16-key tiles in turn with an online softmax.  Lane (r16, q) holds the probabilities of
// keys 4q .. 4q+3 against ITS query r16, so the coordinate sums are three fused multiply-adds per key on the lane's own
// values, rescaled by the same per-lane factor as the value accumulators and reduced over the query's 4 q-lanes where the
// denominator is; the 4 waves' partials are merged in the same fixed order.  The epilogue forms aug1 / aug2 and writes the
// whole y row.  Keys past m read row m - 1 with probability exp(-inf) = 0.
__global__ __launch_bounds__(256) void k_mha_cat_mfma(const float* __restrict__ qm, const float* __restrict__ km,
                                                      const float* __restrict__ vm, const float* __restrict__ c0,
                                                      const float* __restrict__ c1, int n, int m, int heads, float scl,
                                                      float* __restrict__ y, int64_t ldy) {
  constexpr int DIM = 64;
  __shared__ float s_o[4][16][DIM + 1];      // [wave][query][d]
  __shared__ float s_c[4][16][4];            // [wave][query][axis]
  __shared__ float s_mx[4][16], s_den[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int nqb = (n + 15) >> 4;
  const int qb = blockIdx.x % nqb, h = blockIdx.x / nqb;
  const int i0 = qb * 16, c = DIM * heads;
  const float* qrow = qm + (int64_t)min(i0 + r16, n - 1) * c + h * DIM + 4 * q;
  f32x4 qa[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qa[s] = *reinterpret_cast<const f32x4*>(qrow + 16 * s);
  const float* kbase = km + h * DIM + 4 * q;     // + key * c + 16 s   (key = tile * 16 + r16)
  const float* vbase = vm + h * DIM + 4 * r16;   // + key * c          (key = tile * 16 + 4 q + i)
  const int ntile = (m + 15) >> 4;
  f32x4 kb[4], vv[4], kn[4], vn[4];
  float cc[4][3], cn[4][3];                      // c1[key = tile * 16 + 4 q + i][axis]
  auto load_tile = [&](int t, f32x4* kd, f32x4* vd, float (*cd)[3]) {
    const float* krow = kbase + (int64_t)min(t * 16 + r16, m - 1) * c;
#pragma unroll
    for (int s = 0; s < 4; ++s) kd[s] = *reinterpret_cast<const f32x4*>(krow + 16 * s);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t key = min(t * 16 + 4 * q + i, m - 1);
      vd[i] = *reinterpret_cast<const f32x4*>(vbase + key * c);
#pragma unroll
      for (int a = 0; a < 3; ++a) cd[i][a] = c1[key * 3 + a];
    }
  };
  if (wave < ntile) load_tile(wave, kb, vv, cc);
  float mx = -__builtin_inff(), den = 0.f;
  float cs[3] = {0.f, 0.f, 0.f};
  f32x4 o[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = wave; t < ntile; t += 4) {
    if (t + 4 < ntile) load_tile(t + 4, kn, vn, cn);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[s][e], qa[s][e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(kb[s][e + 1], qa[s][e + 1], acc1, 0, 0, 0);
      }
    }
    float sc[4], tmx = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sc[i] = t * 16 + 4 * q + i < m ? (acc0[i] + acc1[i]) * scl : -__builtin_inff();
      tmx = fmaxf(tmx, sc[i]);
    }
    tmx = fmaxf(tmx, __shfl_xor(tmx, 16));
    tmx = fmaxf(tmx, __shfl_xor(tmx, 32));      // the tile holds at least one key: finite
    const float mnew = fmaxf(mx, tmx);
    const float f = expf(mx - mnew);            // 0 on the first tile
    mx = mnew;
    float p[4], ps = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = expf(sc[i] - mnew);                // exp(-inf) = 0 for the keys past m
      ps += p[i];
    }
    den = fmaf(den, f, ps);
#pragma unroll
    for (int a = 0; a < 3; ++a) cs[a] *= f;
#pragma unroll
    for (int b = 0; b < 4; ++b) o[b] *= f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int a = 0; a < 3; ++a) cs[a] = fmaf(p[i], cc[i][a], cs[a]);
#pragma unroll
      for (int b = 0; b < 4; ++b) o[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv[i][b], p[i], o[b], 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      kb[s] = kn[s];
      vv[s] = vn[s];
#pragma unroll
      for (int a = 0; a < 3; ++a) cc[s][a] = cn[s][a];
    }
  }
  den += __shfl_xor(den, 16);
  den += __shfl_xor(den, 32);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] += __shfl_xor(cs[a], 16);
    cs[a] += __shfl_xor(cs[a], 32);
  }
  if (q == 0) {
    s_mx[wave][r16] = mx;
    s_den[wave][r16] = den;
#pragma unroll
    for (int a = 0; a < 3; ++a) s_c[wave][r16][a] = cs[a];
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s_o[wave][r16][4 * (4 * q + i) + b] = o[b][i];
  }
  __syncthreads();
  // thread -> (query = tid / 16, d = tid % 16 + 16 j): waves that saw no tile carry den = 0
  const int qi = threadIdx.x >> 4, d0 = threadIdx.x & 15;
  if (i0 + qi < n) {
    float M = -__builtin_inff();
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, s_mx[w][qi]);
    float fw[4], D = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      fw[w] = s_den[w][qi] > 0.f ? expf(s_mx[w][qi] - M) : 0.f;
      D = fmaf(s_den[w][qi], fw[w], D);
    }
    const float inv = 1.f / D;
    float* yrow = y + (int64_t)(i0 + qi) * ldy + h;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int d = d0 + 16 * j;
      float N = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) N = fmaf(s_o[w][qi][d], fw[w], N);
      yrow[d * heads] = N * inv;
    }
    if (d0 == 0) {                               // the query's seven geometric columns
      float a1[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float N = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) N = fmaf(s_c[w][qi][a], fw[w], N);
        const float soft = N * inv;
        a1[a] = soft - c0[(int64_t)(i0 + qi) * 3 + a];
        yrow[(DIM + a) * heads] = soft;
        yrow[(DIM + 3 + a) * heads] = a1[a];
      }
      yrow[(DIM + 6) * heads] = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
    }
  }
}

// training forward, the sums: thread per (i, e, h) with e in [0, dim + 3) -- feat and soft --, the head's row of P walked in j
// order.  One loop for both kinds (the row a thread multiplies by is v's or c1's): the lanes of a wave do not diverge.
__global__ void k_mha_cat_rows(const float* __restrict__ P, const float* __restrict__ v, const float* __restrict__ c1, int n, int m,
                               int dim, int H, float* __restrict__ y, int64_t ldy) {
  const int c = dim * H, cs = (dim + 3) * H;
  const int64_t total = (int64_t)n * cs;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / cs), ch = (int)(t - (int64_t)i * cs), e = ch / H, h = ch - e * H;
    const float* p = P + ((int64_t)h * n + i) * m;
    const float* x = e < dim ? v + ch : c1 + (e - dim);
    const int64_t ldx = e < dim ? c : 3;
    float r = 0.f;
    for (int j = 0; j < m; ++j) r = fmaf(p[j], x[(int64_t)j * ldx], r);
    y[(int64_t)i * ldy + ch] = r;
  }
}

// training forward, the geometry: thread per (i, h) turns the soft it finds in y into aug1 and aug2
__global__ void k_mha_cat_aug(const float* __restrict__ c0, int n, int dim, int H, float* __restrict__ y, int64_t ldy) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n * H) return;
  const int i = (int)(t / H), h = (int)(t - (int64_t)i * H);
  float* yrow = y + (int64_t)i * ldy + h;
  float a1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    a1[a] = yrow[(dim + a) * H] - c0[(int64_t)i * 3 + a];
    yrow[(dim + 3 + a) * H] = a1[a];
  }
  yrow[(dim + 6) * H] = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
}

// dV = P^T g_feat with g_feat the first dim * H columns of the strided dy: thread per (j, channel), i ascending
__global__ void k_mha_cat_dv(const float* __restrict__ P, const float* __restrict__ dy, int64_t ldy, int n, int m, int dim, int H,
                             float* __restrict__ dv) {
  const int c = dim * H;
  const int64_t total = (int64_t)m * c;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(t / c), ch = (int)(t - (int64_t)j * c), h = ch % H;
    const float* a = P + (int64_t)h * n * m + j;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += a[(int64_t)i * m] * dy[(int64_t)i * ldy + ch];
    dv[t] = acc;
  }
}

__device__ inline float cat_block_sum(float v, float* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];      // fixed order
}

// block per (h, i): g_soft = g[soft] + g[aug1] + g[aug2] * aug1 / aug2 (the last term 0 where aug2 == 0, as torch's norm
// has it; aug1, aug2 as the forward stored them), dP_j = <g_feat_i, v_j> + <g_soft_i, c1_j>, D = sum_j P_j dP_j,
// dS_j = P_j (dP_j - D)
__global__ __launch_bounds__(256) void k_mha_cat_ds(const float* __restrict__ P, const float* __restrict__ y,
                                                    const float* __restrict__ dy, int64_t ldy, const float* __restrict__ v,
                                                    const float* __restrict__ c1, int n, int m, int dim, int H,
                                                    float* __restrict__ dS) {
  extern __shared__ float s_g[];      // [dim] g_feat_i's head vector, then 4 reduction slots
  float* s_red = s_g + dim;
  const int h = blockIdx.x % H, i = blockIdx.x / H;
  const int c = dim * H;
  const float* gy = dy + (int64_t)i * ldy + h;
  const float* yy = y + (int64_t)i * ldy + h;
  for (int d = threadIdx.x; d < dim; d += 256) s_g[d] = gy[d * H];
  const float aug2 = yy[(dim + 6) * H], g2 = gy[(dim + 6) * H];
  float gs[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t = aug2 != 0.f ? g2 * (yy[(dim + 3 + a) * H] / aug2) : 0.f;
    gs[a] = (gy[(dim + a) * H] + gy[(dim + 3 + a) * H]) + t;
  }
  __syncthreads();
  const float* p = P + ((int64_t)h * n + i) * m;
  float* ds = dS + ((int64_t)h * n + i) * m;
  float dsum = 0.f;
  for (int j = threadIdx.x; j < m; j += 256) {
    const float* vj = v + (int64_t)j * c + h;
    float acc = 0.f;
    for (int d = 0; d < dim; ++d) acc += s_g[d] * vj[d * H];
#pragma unroll
    for (int a = 0; a < 3; ++a) acc += gs[a] * c1[(int64_t)j * 3 + a];
    ds[j] = acc;                       // dP_j for now
    dsum += p[j] * acc;
  }
  const float D = cat_block_sum(dsum, s_red);
  for (int j = threadIdx.x; j < m; j += 256) ds[j] = p[j] * (ds[j] - D);
}

unsigned cat_blocks(int64_t rows, int64_t ch) {
  const int64_t b = cdiv64(rows * ch, 256);
  return (unsigned)(b > 16384 ? 16384 : b);
}

}  // namespace

APR_API int apr_mha_cat_headmajor(const float* q, const float* k, const float* v, const float* c0, const float* c1, int32_t n,
                                  int32_t m, int32_t dim, int32_t heads, float* y, int64_t ldy, void* stream) {
  APR_CHECK_ARG(n > 0 && m > 0 && heads > 0 && q && k && v && c0 && c1 && y, "apr_mha_cat_headmajor: bad arguments");
  APR_CHECK_ARG(dim == 64, "apr_mha_cat_headmajor: head dimension %d not supported (64 only)", dim);
  APR_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0, "apr_mha_cat_headmajor: q, k, v must be 16-byte aligned");
  APR_CHECK_ARG(ldy >= (int64_t)(dim + 7) * heads, "apr_mha_cat_headmajor: ldy %lld below (dim + 7) * heads", (long long)ldy);
  const unsigned nqb = (unsigned)((n + 15) / 16);
  hipLaunchKernelGGL(k_mha_cat_mfma, dim3(nqb * (unsigned)heads), dim3(256), 0, (hipStream_t)stream, q, k, v, c0, c1, n, m, heads,
                     1.f / sqrtf((float)dim), y, ldy);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_mha_cat_train_forward(const float* q, const float* k, const float* v, const float* c0, const float* c1, int32_t n,
                                      int32_t m, int32_t dim, int32_t heads, float* P, float* y, int64_t ldy, void* stream) {
  APR_CHECK_ARG(n > 0 && m > 0 && dim > 0 && heads > 0 && dim <= 1024 && q && k && v && c0 && c1 && P && y,
                "apr_mha_cat_train_forward: bad arguments");
  APR_CHECK_ARG(ldy >= (int64_t)(dim + 7) * heads, "apr_mha_cat_train_forward: ldy %lld below (dim + 7) * heads", (long long)ldy);
  hipStream_t st = (hipStream_t)stream;
  const int rc = apr_internal_mha_probs(q, k, n, m, dim, heads, P, st);
  if (rc != APR_OK) return rc;
  hipLaunchKernelGGL(k_mha_cat_rows, dim3(cat_blocks(n, (int64_t)(dim + 3) * heads)), dim3(256), 0, st, P, v, c1, n, m, dim, heads, y,
                     ldy);
  APR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mha_cat_aug, dim3((unsigned)cdiv64((int64_t)n * heads, 256)), dim3(256), 0, st, c0, n, dim, heads, y, ldy);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_mha_cat_train_backward(const float* q, const float* k, const float* v, const float* c0, const float* c1,
                                       const float* P, const float* y, const float* dy, int64_t ldy, int32_t n, int32_t m,
                                       int32_t dim, int32_t heads, float* dS, float* dq, float* dk, float* dv, void* stream) {
  APR_CHECK_ARG(n > 0 && m > 0 && dim > 0 && heads > 0 && dim <= 1024 && q && k && v && c0 && c1 && P && y && dy && dS && dq && dk && dv,
                "apr_mha_cat_train_backward: bad arguments");
  APR_CHECK_ARG(ldy >= (int64_t)(dim + 7) * heads, "apr_mha_cat_train_backward: ldy %lld below (dim + 7) * heads", (long long)ldy);
  hipStream_t st = (hipStream_t)stream;
  const float scale = 1.0f / sqrtf((float)dim);
  hipLaunchKernelGGL(k_mha_cat_dv, dim3(cat_blocks(m, (int64_t)dim * heads)), dim3(256), 0, st, P, dy, ldy, n, m, dim, heads, dv);
  APR_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mha_cat_ds, dim3((unsigned)(n * heads)), dim3(256), (size_t)(dim + 4) * 4, st, P, y, dy, ldy, v, c1, n, m, dim,
                     heads, dS);
  APR_LAUNCH_CHECK();
  int rc = apr_internal_mha_rowmat(dS, k, n, m, dim, heads, scale, dq, st);
  if (rc != APR_OK) return rc;
  return apr_internal_mha_colmat(dS, q, n, m, dim, heads, scale, dk, st);
}

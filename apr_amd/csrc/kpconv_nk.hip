// Rigid KPConv for any kernel-point count 1 <= n_kp <= 32 (the reference's `num_kernel_points`; kpconv.hip is built for
// the 15 points of the shipped configs and keeps its launches): step 1 (apr_kpconv_weighted_nk) and the deterministic
// feature gradient (apr_kpconv_dfeat_contrib_nk), every influence and both aggregations.  The contract is kpconv.h's and
// tests/kpconv_nk_oracle.py's with kp [n_kp, 3] and wf[q, k * cin + c] for k < n_kp.
//
// The kernels are kpconv.hip's with the kernel-point count as data: the MFMA correlation carries ONE 16-row tile for
// n_kp <= 16 and TWO for 17..32 (lane r16 owns kernel points r16 and 16 + r16; the gathered B operand feeds both tiles),
// rows k >= n_kp carry w = 0 and are not stored; the feature gradient sizes its LDS influence table and its per-lane dwf
// registers by the tile count.  Neighbours accumulate in slot order, kernel points in ascending order, with the influence
// statements of kpconv.h: at n_kp = 15 the bits of apr_kpconv_weighted_mode / apr_kpconv_dfeat_contrib_mode (dfeat_d2 below).
#include "kpconv_nk.h"      // kMaxKP, closest_kp_nk (shared with kpconv_deform_nk.hip)

namespace {

// Step 1, MFMA form.  One wave per query; cin % 64 == 0; T 16-row tiles of kernel points, NG 64-channel groups per pass
// (T * NG * 16 accumulator registers: <1, 4> and <2, 2> hold 64, the budget of k_kpconv_weighted_mfma<4>).
template <int T, int NG, int INF, bool CLOSEST>
__global__ __launch_bounds__(256) void k_kpconv_weighted_nk_mfma(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ kp, int n_kp, float extent,
    const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf, int nq, int ns, int xcd_swz) {
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_diff[4][kMaxH][3];
  __shared__ unsigned char s_cl[CLOSEST ? 4 : 1][CLOSEST ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = kp_xcd_block(xcd_swz) * 4 + wave;
  if (qi >= nq) return;
  const int cnt = kp_neighbour_stage<false>(q_pts, s_pts, nbr, H, kp, rowsum, qi, ns, lane, s_idx[wave], s_diff[wave], nullptr);
  if constexpr (CLOSEST) {
    for (int h = lane; h < kMaxH; h += 64)      // the lane that staged slot h reads its own centred point back
      s_cl[wave][h] = s_idx[wave][h] >= 0 ? (unsigned char)closest_kp_nk(s_diff[wave][h][0], s_diff[wave][h][1],
                                                                         s_diff[wave][h][2], kp, n_kp, 0.f)
                                          : 0;
  }
  const float inv_num = 1.f / (float)max(cnt, 1);
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  bool kvalid[T];
  float kx[T], ky[T], kz[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int k = 16 * t + r16;
    kvalid[t] = k < n_kp;
    kx[t] = kvalid[t] ? kp[3 * k] : 0.f;
    ky[t] = kvalid[t] ? kp[3 * k + 1] : 0.f;
    kz[t] = kvalid[t] ? kp[3 * k + 2] : 0.f;
  }
  const int nsteps = (H + 3) >> 2;
  for (int g0 = 0; g0 < cin / 64; g0 += NG) {
    f32x4 acc[T][NG][4];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[t][g][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nsteps; ++st) {
      const int h = st * 4 + qd;
      const int idx = s_idx[wave][h];
      float w[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        w[t] = 0.f;
        if (kvalid[t] && idx >= 0) {
          w[t] = kpmode::influence<INF>(kp_d2(s_diff[wave][h][0], s_diff[wave][h][1], s_diff[wave][h][2], kx[t], ky[t], kz[t]),
                                        inv_extent, gden);
          if constexpr (CLOSEST) w[t] = (int)(s_cl[wave][h] & 31) == 16 * t + r16 ? w[t] : 0.f;
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f32x4 b = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (idx >= 0 && g0 + g < cin / 64)
          b = *reinterpret_cast<const f32x4*>(x + (int64_t)idx * ldx + (g0 + g) * 64 + r16 * 4);
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) acc[t][g][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], b[cb], acc[t][g][cb], 0, 0, 0);
      }
    }
    // D[k = 16 t + 4 qd + i][col r16 of block cb] <-> channel (g0+g)*64 + 4*r16 + cb
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g0 + g >= cin / 64) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 16 * t + qd * 4 + i;
          if (k < n_kp) {
            f32x4 v = {acc[t][g][0][i] * inv_num, acc[t][g][1][i] * inv_num, acc[t][g][2][i] * inv_num,
                       acc[t][g][3][i] * inv_num};
            *reinterpret_cast<f32x4*>(wf + (int64_t)qi * ldwf + (int64_t)k * cin + (g0 + g) * 64 + r16 * 4) = v;
          }
        }
      }
  }
}

// Step 1, VALU form for any cin and alignment.  One thread per (query, kernel point).
template <int INF, bool CLOSEST>
__global__ void k_kpconv_weighted_nk_generic(const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                             const int* __restrict__ nbr, int H, const float* __restrict__ x, int64_t ldx,
                                             int cin, const float* __restrict__ kp, int n_kp, float extent,
                                             const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf,
                                             int nq, int ns) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nq * n_kp) return;
  const int qi = (int)(t / n_kp), k = (int)(t - (int64_t)qi * n_kp);
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  const float kx = kp[3 * k], ky = kp[3 * k + 1], kz = kp[3 * k + 2];
  const float inv_extent = 1.f / extent;
  int cnt = 0;
  for (int h = 0; h < H; ++h) {
    const int idx = nbr[(int64_t)qi * H + h];
    if (idx >= 0 && idx < ns && rowsum[idx] > 0.f) ++cnt;
  }
  const float inv_num = 1.f / (float)max(cnt, 1);
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  for (int c0 = 0; c0 < cin; c0 += 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nc = min(8, cin - c0);
    for (int h = 0; h < H; ++h) {
      const int idx = nbr[(int64_t)qi * H + h];
      if (idx < 0 || idx >= ns) continue;
      const float dx = s_pts[3 * (int64_t)idx] - qx, dy = s_pts[3 * (int64_t)idx + 1] - qy,
                  dz = s_pts[3 * (int64_t)idx + 2] - qz;
      float w = kpmode::influence<INF>(kp_d2(dx, dy, dz, kx, ky, kz), inv_extent, gden);
      if constexpr (CLOSEST) w = (closest_kp_nk(dx, dy, dz, kp, n_kp, 0.f) & 31) == k ? w : 0.f;
      if (w == 0.f) continue;
      for (int c = 0; c < nc; ++c) acc[c] = fmaf(w, x[(int64_t)idx * ldx + c0 + c], acc[c]);
    }
    for (int c = 0; c < nc; ++c) wf[(int64_t)qi * ldwf + (int64_t)k * cin + c0 + c] = acc[c] * inv_num;
  }
}

// The squared distance behind the gradient's influences, spelled out.  kpconv.h's kp_d2 leaves its contraction to the
// compiler, and in k_kpconv_dfeat (kpconv.hip) today's compiler makes of it
//   fma(ez, ez, fma(ex, ex, ey ey))   without CLOSEST, and with CLOSEST for kernel point 14,
//   fma(ey, ey, ex ex) + ez ez        with CLOSEST for kernel points 0 .. 13 (ex ex is closest_kp's product, the two squares
//                                     of a kernel point share a packed multiply)
// (read from the ISA of kpconv.hip).  These are those forms, contraction off, so that n_kp = 15 gives the bits of
// apr_kpconv_dfeat_contrib_mode in every mode; tests/test_kpconv_nk_gpu.py holds them to that.  The price: this mirrors what a
// compiler chose in another translation unit -- a compiler change, or any edit of k_kpconv_dfeat, can part the two and that
// test then fails.  The durable statement is one explicit d2 in kpconv.h shared by both kernels; it changes the existing
// kernels' code and was left out of this file's change on purpose.  For n_kp != 15 either form is inside the oracle's bound.
template <bool CLOSEST>
__device__ inline float dfeat_d2(float ex, float ey, float ez, int k) {
#pragma clang fp contract(off)
  const float sum_form = __builtin_fmaf(ez, ez, __builtin_fmaf(ex, ex, ey * ey));
  if constexpr (!CLOSEST) return sum_form;
  const float pair_form = __builtin_fmaf(ey, ey, ex * ex) + ez * ez;
  return k == 14 ? sum_form : pair_form;
}

// The deterministic feature gradient: row (q, h) of contrib [nq * H, cin] = (1 / num_q) sum_k w[q,k,h] dwf[q, k cin + c], the
// k-sum an ascending fmaf chain (k_kpconv_dfeat's contrib form).  One wave per query, WPB waves per block; KT = 16 or 32
// sizes the LDS influence table s_w[.][h][KT] and the lane's dwf registers g[CPL][KT].  Columns k >= n_kp hold w = -0 and
// g = +0: fmaf(-0, +0, acc) = acc + (-0) = acc for every acc, a zero of either sign included, so the chain is the n_kp-term
// one.  Channels go in passes of 64 CPL.
template <int CPL, int KT, int INF, bool CLOSEST>
__global__ __launch_bounds__(KT == 16 ? 256 : 128) void k_kpconv_dfeat_contrib_nk(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ dwf, int64_t lddwf, int cin, const float* __restrict__ kp, int n_kp, float extent,
    const float* __restrict__ rowsum, int nq, int ns, float* __restrict__ contrib) {
  constexpr int WPB = KT == 16 ? 4 : 2;      // 32 KB of influences per block either way
  __shared__ int s_idx[WPB][kMaxH];
  __shared__ float s_w[WPB][kMaxH][KT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * WPB + wave;
  if (qi >= nq) return;
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  int cnt = 0;
  for (int h = lane; h < H; h += 64) {
    int idx = nbr[(int64_t)qi * H + h];
    if (idx < 0 || idx >= ns) idx = -1;
    s_idx[wave][h] = idx;
    if (idx >= 0) {
      cnt += rowsum[idx] > 0.f ? 1 : 0;
      const float dx_ = s_pts[3 * (int64_t)idx] - qx, dy_ = s_pts[3 * (int64_t)idx + 1] - qy,
                  dz_ = s_pts[3 * (int64_t)idx + 2] - qz;
      const int cl = CLOSEST ? (closest_kp_nk(dx_, dy_, dz_, kp, n_kp, 0.f) & 31) : -1;
      for (int k = 0; k < n_kp; ++k) {
        const float ex = dx_ - kp[3 * k], ey = dy_ - kp[3 * k + 1], ez = dz_ - kp[3 * k + 2];
        const float w = kpmode::influence<INF>(dfeat_d2<CLOSEST>(ex, ey, ez, k), inv_extent, gden);
        s_w[wave][h][k] = (!CLOSEST || k == cl) ? w : 0.f;
      }
      for (int k = n_kp; k < KT; ++k) s_w[wave][h][k] = -0.f;
    }
  }
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  const float inv_num = 1.f / (float)max(cnt, 1);
  // (the wave's LDS writes are read back by other lanes of the same wave: in-order LDS queue, no barrier needed)
  for (int c0 = 0; c0 < cin; c0 += 64 * CPL) {
    float g[CPL][KT];
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = c0 + lane + 64 * u;
#pragma unroll
      for (int k = 0; k < KT; ++k)
        g[u][k] = (c < cin && k < n_kp) ? dwf[(int64_t)qi * lddwf + (int64_t)k * cin + c] * inv_num : 0.f;
    }
    for (int h = 0; h < H; ++h) {
      const int idx = s_idx[wave][h];      // wave-uniform
      if (idx < 0) continue;
      float w[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) w[k] = s_w[wave][h][k];
#pragma unroll
      for (int u = 0; u < CPL; ++u) {
        const int c = c0 + lane + 64 * u;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) acc = fmaf(w[k], g[u][k], acc);
        if (c < cin) contrib[((int64_t)qi * H + h) * cin + c] = acc;
      }
    }
  }
}

template <int INF, bool CLOSEST>
int kpconv_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                       const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp, float extent,
                       const float* rowsum, float* wf, int64_t ldwf, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool vec = cin % 64 == 0 && H <= kMaxH && ldx % 4 == 0 && ldwf % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)wf)) & 15) == 0;
  if (vec) {
    const unsigned grid = (unsigned)cdiv64(nq, 4);
    const int s_xcd = kpconv_xcd();
#define APR_NK(T, NG)                                                                                                       \
  hipLaunchKernelGGL((k_kpconv_weighted_nk_mfma<T, NG, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, \
                     ldx, cin, kernel_points, n_kp, extent, rowsum, wf, ldwf, (int)nq, (int)ns, s_xcd)
    if (n_kp <= 16) {      // the channel groups per pass of apr_kpconv_weighted_mode
      if (cin >= 256) APR_NK(1, 4);
      else if (cin == 128) APR_NK(1, 2);
      else APR_NK(1, 1);
    } else {               // two tiles: half the groups per pass, the same accumulator registers
      if (cin >= 128) APR_NK(2, 2);
      else APR_NK(2, 1);
    }
#undef APR_NK
  } else {
    hipLaunchKernelGGL((k_kpconv_weighted_nk_generic<INF, CLOSEST>), dim3((unsigned)cdiv64(nq * n_kp, 256)), dim3(256), 0, st,
                       q_pts, s_pts, nbr, H, x, ldx, cin, kernel_points, n_kp, extent, rowsum, wf, ldwf, (int)nq, (int)ns);
  }
  APR_LAUNCH_CHECK();
  return APR_OK;
}

template <int INF, bool CLOSEST>
int kpconv_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                            const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                            float extent, const float* rowsum, float* contrib, void* stream) {
  hipStream_t st = (hipStream_t)stream;
#define APR_DF(N, KT)                                                                                                        \
  hipLaunchKernelGGL((k_kpconv_dfeat_contrib_nk<N, KT, INF, CLOSEST>), dim3((unsigned)cdiv64(nq, KT == 16 ? 4 : 2)),          \
                     dim3(KT == 16 ? 256 : 128), 0, st, q_pts, s_pts, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent, \
                     rowsum, (int)nq, (int)ns, contrib)
  if (n_kp <= 16) {        // one pass, the registers of k_kpconv_dfeat
    if (cin <= 64) APR_DF(1, 16);
    else if (cin <= 128) APR_DF(2, 16);
    else if (cin <= 256) APR_DF(4, 16);
    else APR_DF(8, 16);
  } else {                 // 32 dwf registers per channel: at most 4 channels per lane and pass
    if (cin <= 64) APR_DF(1, 32);
    else if (cin <= 128) APR_DF(2, 32);
    else APR_DF(4, 32);
  }
#undef APR_DF
  APR_LAUNCH_CHECK();
  return APR_OK;
}

}  // namespace

// apr_kpconv_weighted_mode for 1 <= n_kp <= 32 kernel points (kernel_points f32 [n_kp, 3], wf[q, k * cin + c], k < n_kp).
APR_API int apr_kpconv_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                   int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                                   int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf,
                                   int32_t influence, int32_t closest, void* stream) {
  APR_CHECK_ARG(n_kp >= 1 && n_kp <= kMaxKP, "apr_kpconv_weighted_nk: 1 <= n_kp <= %d, got %d", kMaxKP, n_kp);
  APR_CHECK_ARG(kpmode::valid(influence, closest),
                "apr_kpconv_weighted_nk: influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d", influence, closest);
  APR_CHECK_ARG(nq >= 0 && nq <= INT32_MAX - 4 && ns > 0 && ns <= INT32_MAX && H > 0 && cin > 0 && extent > 0.f,
                "apr_kpconv_weighted_nk: bad arguments (nq %lld, ns %lld, H %d, cin %d)", (long long)nq, (long long)ns, H, cin);
  APR_CHECK_ARG(ldx >= cin && ldwf >= (int64_t)n_kp * cin, "apr_kpconv_weighted_nk: leading dimension too small");
  if (nq == 0) return APR_OK;
  APR_CHECK_ARG(q_pts && s_pts && nbr && x && kernel_points && rowsum && wf, "apr_kpconv_weighted_nk: null pointer");
  APR_KP_MODE_DISPATCH(kpconv_weighted_nk, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, kernel_points, n_kp, extent, rowsum, wf,
                       ldwf, stream)
}

// apr_kpconv_dfeat_contrib_mode for 1 <= n_kp <= 32 kernel points: rows (q, h) of contrib f32 [nq * H, cin] (the rows of
// padding neighbours are left untouched); apr_reverse_gather sums them.  H <= 128, cin <= 512.
APR_API int apr_kpconv_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                        int32_t H, const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points,
                                        int32_t n_kp, float extent, const float* rowsum, float* contrib, int32_t influence,
                                        int32_t closest, void* stream) {
  APR_CHECK_ARG(n_kp >= 1 && n_kp <= kMaxKP, "apr_kpconv_dfeat_contrib_nk: 1 <= n_kp <= %d, got %d", kMaxKP, n_kp);
  APR_CHECK_ARG(kpmode::valid(influence, closest),
                "apr_kpconv_dfeat_contrib_nk: influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d", influence, closest);
  APR_CHECK_ARG(nq >= 0 && nq <= INT32_MAX - 4 && ns > 0 && ns <= INT32_MAX && H > 0 && H <= kMaxH && cin > 0 && cin <= 512 &&
                    extent > 0.f,
                "apr_kpconv_dfeat_contrib_nk: bad arguments (H <= %d, cin <= 512; nq %lld, ns %lld, H %d, cin %d)", kMaxH,
                (long long)nq, (long long)ns, H, cin);
  APR_CHECK_ARG(lddwf >= (int64_t)n_kp * cin, "apr_kpconv_dfeat_contrib_nk: leading dimension too small");
  APR_CHECK_ARG(contrib != nullptr, "apr_kpconv_dfeat_contrib_nk: null contribution buffer");
  if (nq == 0) return APR_OK;
  APR_CHECK_ARG(q_pts && s_pts && nbr && dwf && kernel_points && rowsum, "apr_kpconv_dfeat_contrib_nk: null pointer");
  APR_KP_MODE_DISPATCH(kpconv_dfeat_contrib_nk, q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent,
                       rowsum, contrib, stream)
}

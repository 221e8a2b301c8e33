// KPConv encoder kernels: the rigid correlation, its feature gradient and the gather pools.
//
// KPConv (Predator_APR/models/blocks.py:229-374, rigid / linear influence / sum aggregation):
//   out[q] = ( sum_k ( sum_h w[q,k,h] * x[nbr[q,h]] ) @ W[k] ) / max(#{h : sum_c x[nbr[q,h],c] > 0}, 1)
//   w[q,k,h] = max(0, 1 - |s[nbr[q,h]] - q - kp[k]| / extent)
// The reference materialises [N,H,15,3] differences and two batched matmuls.  Here step 1 (the
// kernel-point correlation) is one wave per query on the fp32 MFMA: A = w[k][h] computed on the
// fly in registers (M = 16 >= 15 kernel points, K = neighbours), B = neighbour features gathered
// straight from HBM with one 16-B load per lane (channel permutation c = 4*r + cb makes every
// gathered row a single 256-B coalesced read AND every output row a 16-B store), already
// divided by the neighbour count.  Step 2 is the dense [Nq, 15*Cin] x [15*Cin, Cout] GEMM on the
// sparse-conv MFMA kernel (identity map).  The remaining kernels are the small gather / reduce
// ops of the blocks (the overlap-attention module's are in attention.hip).
// The influence function (linear, constant, gaussian) and the aggregation (sum, `closest`; blocks.py:61-68, 320-345) are
// compile-time parameters of the correlation kernels and of the deterministic feature gradient: one influence statement
// per kernel (kpmode::influence of kp_d2) and one neighbour stage for the MFMA correlations (kp_neighbour_stage), in kpconv.h.
#include "kpconv.h"

namespace {

__global__ void k_row_sums(const float* __restrict__ x, int64_t ld, int64_t n, int c, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  float s = 0.f;
  for (int j = lane; j < c; j += 64) s += x[row * ld + j];
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) out[row] = s;
}

// Step 1, MFMA form.  One wave per query; Cin % 64 == 0; NG = 64-channel groups per pass.
// INF / CLOSEST: the influence function and the aggregation (blocks.py:320-345) as compile-time parameters.  With CLOSEST
// the lane that stages slot h -- it holds the centred point -- records the neighbour's closest kernel point
// (kpmode::closest_kp), and the A operand of every other kernel point is 0.
template <int NG, int INF = kpmode::kLinear, bool CLOSEST = false>
__global__ __launch_bounds__(256) void k_kpconv_weighted_mfma(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ kp, float extent,
    const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf, int nq, int ns, int xcd_swz) {
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_diff[4][kMaxH][3];
  __shared__ unsigned char s_cl[CLOSEST ? 4 : 1][CLOSEST ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = kp_xcd_block(xcd_swz) * 4 + wave;
  if (qi >= nq) return;
  const int cnt = kp_neighbour_stage<CLOSEST>(q_pts, s_pts, nbr, H, kp, rowsum, qi, ns, lane, s_idx[wave], s_diff[wave],
                                              s_cl[CLOSEST ? wave : 0]);
  const float inv_num = 1.f / (float)max(cnt, 1);
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  const bool kvalid = r16 < kKP;
  const float kx = kvalid ? kp[3 * r16] : 0.f, ky = kvalid ? kp[3 * r16 + 1] : 0.f, kz = kvalid ? kp[3 * r16 + 2] : 0.f;
  const int nsteps = (H + 3) >> 2;
  for (int g0 = 0; g0 < cin / 64; g0 += NG) {
    f32x4 acc[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[g][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nsteps; ++st) {
      const int h = st * 4 + qd;
      const int idx = s_idx[wave][h];
      float w = 0.f;
      if (kvalid && idx >= 0) {
        w = kpmode::influence<INF>(kp_d2(s_diff[wave][h][0], s_diff[wave][h][1], s_diff[wave][h][2], kx, ky, kz), inv_extent, gden);
        if constexpr (CLOSEST) w = (int)s_cl[wave][h] == r16 ? w : 0.f;
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f32x4 b = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (idx >= 0 && g0 + g < cin / 64)
          b = *reinterpret_cast<const f32x4*>(x + (int64_t)idx * ldx + (g0 + g) * 64 + r16 * 4);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[g][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[cb], acc[g][cb], 0, 0, 0);
      }
    }
    // D[k = 4*qd + i][col r16 of block cb] <-> channel (g0+g)*64 + 4*r16 + cb
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g0 + g >= cin / 64) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = qd * 4 + i;
        if (k < kKP) {
          f32x4 v = {acc[g][0][i] * inv_num, acc[g][1][i] * inv_num, acc[g][2][i] * inv_num, acc[g][3][i] * inv_num};
          *reinterpret_cast<f32x4*>(wf + (int64_t)qi * ldwf + (int64_t)k * cin + (g0 + g) * 64 + r16 * 4) = v;
        }
      }
    }
  }
}

// Step 1, MFMA form for Cin = 32 (the first layer of the symmetric generator KPFCNNDecoder reads the encoder's 32-d
// descriptors on the FINEST level; linear influence, sum aggregation).  k_kpconv_weighted_mfma with a 128-byte feature row:
// one wave per query, lane r16 gathers the float2 of channels 2 r16, 2 r16 + 1 (the 16 lanes of a k-slot read one row, the
// four k-slots four neighbours), two column blocks cb <-> channel 2 r16 + cb, and D[k = 4 qd + i][col r16] leaves as one
// float2 per kernel point.  The next step's two operands (index, centred point from LDS; the row from memory) are fetched
// before the current step's MFMAs are issued.
__global__ __launch_bounds__(256) void k_kpconv_weighted_c32(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ kp, float extent,
    const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf, int nq, int ns, int xcd_swz) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int kC = 32;
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_diff[4][kMaxH][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = kp_xcd_block(xcd_swz) * 4 + wave;
  if (qi >= nq) return;
  const int cnt = kp_neighbour_stage<false>(q_pts, s_pts, nbr, H, kp, rowsum, qi, ns, lane, s_idx[wave], s_diff[wave], nullptr);
  const float inv_num = 1.f / (float)max(cnt, 1);
  const float inv_extent = 1.f / extent;
  const bool kvalid = r16 < kKP;
  const float kx = kvalid ? kp[3 * r16] : 0.f, ky = kvalid ? kp[3 * r16 + 1] : 0.f, kz = kvalid ? kp[3 * r16 + 2] : 0.f;
  const int nsteps = (H + 3) >> 2;      // 4 * nsteps <= kMaxH: every slot read below was staged above
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int st, int& idx, f32x2& b) {
    idx = s_idx[wave][st * 4 + qd];
    b = (f32x2){0.f, 0.f};
    if (idx >= 0) b = *reinterpret_cast<const f32x2*>(x + (int64_t)idx * ldx + r16 * 2);
  };
  int idx;
  f32x2 b;
  fetch(0, idx, b);
  for (int st = 0; st < nsteps; ++st) {
    int idx_n = -1;
    f32x2 b_n = {0.f, 0.f};
    if (st + 1 < nsteps) fetch(st + 1, idx_n, b_n);
    const int h = st * 4 + qd;
    float w = 0.f;
    if (kvalid && idx >= 0)
      w = kpmode::influence<kpmode::kLinear>(kp_d2(s_diff[wave][h][0], s_diff[wave][h][1], s_diff[wave][h][2], kx, ky, kz),
                                             inv_extent, 0.f);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[1], acc1, 0, 0, 0);
    idx = idx_n;
    b = b_n;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = qd * 4 + i;
    if (k < kKP) {
      const f32x2 v = {acc0[i] * inv_num, acc1[i] * inv_num};
      *reinterpret_cast<f32x2*>(wf + (int64_t)qi * ldwf + (int64_t)k * kC + r16 * 2) = v;
    }
  }
}

// Step 1, VALU form for any Cin (the first layer has Cin = 1).  One thread per (query, kernel point).  With CLOSEST every
// thread finds the neighbour's closest kernel point itself (the one statement of it, kpmode::closest_kp).
template <int INF = kpmode::kLinear, bool CLOSEST = false>
__global__ void k_kpconv_weighted_generic(const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                          const int* __restrict__ nbr, int H, const float* __restrict__ x, int64_t ldx,
                                          int cin, const float* __restrict__ kp, float extent,
                                          const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf,
                                          int nq, int ns) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nq * kKP) return;
  const int qi = (int)(t / kKP), k = (int)(t - (int64_t)qi * kKP);
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
      if constexpr (CLOSEST) w = (kpmode::closest_kp(dx, dy, dz, kp, 0.f) & 15) == k ? w : 0.f;
      if (w == 0.f) continue;
      for (int c = 0; c < nc; ++c) acc[c] = fmaf(w, x[(int64_t)idx * ldx + c0 + c], acc[c]);
    }
    for (int c = 0; c < nc; ++c) wf[(int64_t)qi * ldwf + (int64_t)k * cin + c0 + c] = acc[c] * inv_num;
  }
}

// Backward of step 1 with respect to the neighbour features (Predator side):
//   dx[nbr[q,h], c] += (1 / num_q) * sum_k w[q,k,h] * dwf[q, k*cin + c]
// (the neighbour count num_q and the influences w depend on the geometry and on the SIGN of the feature sums only:
// piecewise constant in x, no gradient through them - the same graph torch builds for blocks.py:326-374).
// One wave per query: the 15 x H influences go to LDS once, a lane keeps the 15 values dwf[q, :, c] of its channel
// in registers and walks the neighbours; the sums leave through float atomics (a support point is the neighbour of
// ~H queries: the transposed table is not available, and torch's own index backward adds atomically as well).
// INF / CLOSEST as in k_kpconv_weighted_mfma; the modes other than <kLinear, false> exist in the deterministic `contrib`
// form only (the host launches nothing else).
template <int CPL, int INF = kpmode::kLinear, bool CLOSEST = false>   // channels per lane: cin <= 64 * CPL
__global__ __launch_bounds__(256) void k_kpconv_dfeat(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ dwf, int64_t lddwf, int cin, const float* __restrict__ kp, float extent,
    const float* __restrict__ rowsum, float* __restrict__ dx, int64_t lddx, int nq, int ns,
    float* __restrict__ contrib) {      // non-NULL: the deterministic form -- row (q, h) of contrib instead of an atomic add
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_w[4][kMaxH][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * 4 + wave;
  if (qi >= nq) return;
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  // kp_neighbour_stage's slot with the 15 influences in place of the centred point, and only the slots below H (the stage
  // itself, templated on that, changed this kernel's register counts: DESIGN 36)
  int cnt = 0;
  for (int h = lane; h < H; h += 64) {
    int idx = nbr[(int64_t)qi * H + h];
    if (idx < 0 || idx >= ns) idx = -1;
    s_idx[wave][h] = idx;
    if (idx >= 0) {
      cnt += rowsum[idx] > 0.f ? 1 : 0;
      const float dx_ = s_pts[3 * (int64_t)idx] - qx, dy_ = s_pts[3 * (int64_t)idx + 1] - qy,
                  dz_ = s_pts[3 * (int64_t)idx + 2] - qz;
      const int cl = CLOSEST ? (kpmode::closest_kp(dx_, dy_, dz_, kp, 0.f) & 15) : -1;
#pragma unroll
      for (int k = 0; k < kKP; ++k) {
        const float w = kpmode::influence<INF>(kp_d2(dx_, dy_, dz_, kp[3 * k], kp[3 * k + 1], kp[3 * k + 2]), inv_extent, gden);
        s_w[wave][h][k] = (!CLOSEST || k == cl) ? w : 0.f;
      }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  const float inv_num = 1.f / (float)max(cnt, 1);
  // (the wave's LDS writes are read back by other lanes of the same wave: in-order LDS queue, no barrier needed)
  float g[CPL][kKP];
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const int c = lane + 64 * u;
#pragma unroll
    for (int k = 0; k < kKP; ++k)
      g[u][k] = c < cin ? dwf[(int64_t)qi * lddwf + (int64_t)k * cin + c] * inv_num : 0.f;
  }
  for (int h = 0; h < H; ++h) {
    const int idx = s_idx[wave][h];      // wave-uniform
    if (idx < 0) continue;
    float w[kKP];
#pragma unroll
    for (int k = 0; k < kKP; ++k) w[k] = s_w[wave][h][k];
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = lane + 64 * u;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < kKP; ++k) acc = fmaf(w[k], g[u][k], acc);
      if (c < cin) {
        if (contrib) contrib[((int64_t)qi * H + h) * cin + c] = acc;
        else atomicAdd(dx + (int64_t)idx * lddx + c, acc);
      }
    }
  }
}

// out[q,:] = max_h x_pad[inds[q,h],:]  (x_pad = x plus a zero shadow row; blocks.py:86-102)
// mode 1: out[q,:] = x_pad[inds[q,0],:]  (closest_pool, blocks.py:71-83)
// 16-B form: thread = (query, 4 channels); rows of x / out 16-byte aligned, c % 4 == 0
__global__ void k_gather_pool4(const float* __restrict__ x, int64_t ldx, int ns, int c, const int* __restrict__ inds,
                               int H, int64_t nq, int mode, float* __restrict__ out, int64_t ldo) {
  const int c4 = c >> 2;
  const int64_t total = nq * c4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 ninf = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t qi = t / c4;
    const int col = (int)(t - qi * c4) * 4;
    f32x4 m;
    if (mode == 1) {
      const int idx = inds[qi * H];
      m = (idx >= 0 && idx < ns) ? *reinterpret_cast<const f32x4*>(x + (int64_t)idx * ldx + col) : zero;
    } else {
      m = ninf;
      for (int h0 = 0; h0 < H; h0 += 8) {
        int idx[8];
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) idx[u] = (h0 + u < H) ? inds[qi * H + h0 + u] : -2;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = (idx[u] >= 0 && idx[u] < ns) ? *reinterpret_cast<const f32x4*>(x + (int64_t)idx[u] * ldx + col)
                                              : (idx[u] == -2 ? ninf : zero);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[u][e]);
      }
    }
    *reinterpret_cast<f32x4*>(out + qi * ldo + col) = m;
  }
}

__global__ void k_gather_pool(const float* __restrict__ x, int64_t ldx, int ns, int c, const int* __restrict__ inds,
                              int H, int64_t nq, int mode, float* __restrict__ out, int64_t ldo) {
  const int64_t total = nq * c;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t qi = t / c;
    const int col = (int)(t - qi * c);
    float m;
    if (mode == 1) {
      const int idx = inds[qi * H];
      m = (idx >= 0 && idx < ns) ? x[(int64_t)idx * ldx + col] : 0.f;
    } else {
      m = -__builtin_inff();
      for (int h0 = 0; h0 < H; h0 += 8) {     // 8 index loads, then 8 gathers in flight (not 2 dependent trips per h)
        int idx[8];
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) idx[u] = (h0 + u < H) ? inds[qi * H + h0 + u] : -2;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          v[u] = (idx[u] >= 0 && idx[u] < ns) ? x[(int64_t)idx[u] * ldx + col] : (idx[u] == -2 ? -__builtin_inff() : 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u) m = fmaxf(m, v[u]);
      }
    }
    out[qi * ldo + col] = m;
  }
}

// max_pool with the position of the maximum: amax[q, c] = the FIRST h whose x_pad[inds[q,h], c] equals the maximum (what
// the backward routes the gradient to, as torch.max(dim) does); thread = (query, channel)
__global__ void k_gather_pool_argmax(const float* __restrict__ x, int64_t ldx, int ns, int c, const int* __restrict__ inds,
                                     int H, int64_t nq, float* __restrict__ out, int64_t ldo,
                                     unsigned char* __restrict__ amax) {
  const int64_t total = nq * c;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t qi = t / c;
    const int col = (int)(t - qi * c);
    float m = -__builtin_inff();
    int best = 0;
    for (int h0 = 0; h0 < H; h0 += 8) {
      int idx[8];
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) idx[u] = (h0 + u < H) ? inds[qi * H + h0 + u] : -2;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = (idx[u] >= 0 && idx[u] < ns) ? x[(int64_t)idx[u] * ldx + col] : (idx[u] == -2 ? -__builtin_inff() : 0.f);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (v[u] > m) {
          m = v[u];
          best = h0 + u;
        }
    }
    out[qi * ldo + col] = m;
    amax[qi * c + col] = (unsigned char)best;
  }
}

// Backward of max_pool / closest_pool as a GATHER over the reverse neighbour table (revtable.hip): dx[s, c] = sum of
// dout[q, c] over the entries (q, h) of row s's run with h == amax[q, c] (mode 0) or h == 0 (mode 1), in run order:
// deterministic, no float atomics, no contribution buffer.  thread = (support row, channel)
__global__ void k_gather_pool_bwd(const float* __restrict__ dout, int64_t lddo, int c, const int* __restrict__ rev_t,
                                  const int* __restrict__ start, int64_t ns, int H, const unsigned char* __restrict__ amax,
                                  int mode, float* __restrict__ dx, int64_t lddx) {
  const int64_t total = ns * c;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = t / c;
    const int col = (int)(t - s * c);
    float acc = 0.f;
    for (int e = start[s]; e < start[s + 1]; ++e) {
      const int pos = rev_t[e];
      const int q = pos / H, h = pos - q * H;
      const bool mine = mode == 1 ? h == 0 : (int)amax[(int64_t)q * c + col] == h;
      if (mine) acc += dout[(int64_t)q * lddo + col];
    }
    dx[s * lddx + col] = acc;
  }
}

}  // namespace

APR_API int apr_row_sums(const float* x, int64_t ld, int64_t n, int32_t c, float* out, void* stream) {
  APR_CHECK_ARG(n >= 0 && c > 0 && ld >= c, "apr_row_sums: bad shape");
  if (n == 0) return APR_OK;
  hipLaunchKernelGGL(k_row_sums, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, (hipStream_t)stream, x, ld, n, c, out);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

template <int INF, bool CLOSEST>
static int kpconv_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                           const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp,
                           float extent, const float* rowsum, float* wf, int64_t ldwf, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_kp == kKP, "apr_kpconv_weighted: built for %d kernel points, got %d", kKP, n_kp);
  APR_CHECK_ARG(nq >= 0 && ns > 0 && H > 0 && cin > 0 && extent > 0.f, "apr_kpconv_weighted: bad arguments");
  APR_CHECK_ARG(ldx >= cin && ldwf >= (int64_t)kKP * cin, "apr_kpconv_weighted: leading dimension too small");
  if (nq == 0) return APR_OK;
  const bool vec = cin % 64 == 0 && H <= kMaxH && ldx % 4 == 0 && ldwf % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)wf)) & 15) == 0;
  if (vec) {
    const unsigned grid = (unsigned)cdiv64(nq, 4);
    const int s_xcd = kpconv_xcd();
    if (cin >= 256)
      hipLaunchKernelGGL((k_kpconv_weighted_mfma<4, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, ldx,
                         cin, kernel_points, extent, rowsum, wf, ldwf, (int)nq, (int)ns, s_xcd);
    else if (cin == 128)
      hipLaunchKernelGGL((k_kpconv_weighted_mfma<2, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, ldx,
                         cin, kernel_points, extent, rowsum, wf, ldwf, (int)nq, (int)ns, s_xcd);
    else
      hipLaunchKernelGGL((k_kpconv_weighted_mfma<1, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, ldx,
                         cin, kernel_points, extent, rowsum, wf, ldwf, (int)nq, (int)ns, s_xcd);
  } else {
    hipLaunchKernelGGL((k_kpconv_weighted_generic<INF, CLOSEST>), dim3((unsigned)cdiv64(nq * kKP, 256)), dim3(256), 0, st,
                       q_pts, s_pts, nbr, H, x, ldx, cin, kernel_points, extent, rowsum, wf, ldwf, (int)nq, (int)ns);
  }
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Step 1 with the influence function (0 constant, 1 linear, 2 gaussian: blocks.py:320-337, 61-68) and the aggregation
// (closest = 1: only the kernel point nearest to a neighbour keeps its influence, blocks.py:339-345).
APR_API int apr_kpconv_weighted_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                     int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                                     int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf,
                                     int32_t influence, int32_t closest, void* stream) {
  APR_CHECK_ARG(kpmode::valid(influence, closest),
                "apr_kpconv_weighted_mode: influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d", influence, closest);
  APR_KP_MODE_DISPATCH(kpconv_weighted, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, kernel_points, n_kp, extent, rowsum, wf,
                       ldwf, stream)
}

// linear influence, sum aggregation
APR_API int apr_kpconv_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                                int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf, void* stream) {
  return apr_kpconv_weighted_mode(q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, kernel_points, n_kp, extent, rowsum, wf, ldwf,
                                  kpmode::kLinear, 0, stream);
}

// apr_kpconv_weighted for cin = 32 on the fp32 MFMA (k_kpconv_weighted_c32; linear influence, sum aggregation).  Unlike
// apr_kpconv_weighted it has no other route: anything the kernel does not take is refused, and a refused call writes
// nothing.
APR_API int apr_kpconv_weighted_c32(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                    int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                                    int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf, void* stream) {
  APR_CHECK_ARG(n_kp == kKP, "apr_kpconv_weighted_c32: built for %d kernel points, got %d", kKP, n_kp);
  APR_CHECK_ARG(cin == 32, "apr_kpconv_weighted_c32: built for 32 input channels, got %d", cin);
  APR_CHECK_ARG(H > 0 && H <= kMaxH, "apr_kpconv_weighted_c32: 1 <= H <= %d, got %d", kMaxH, H);
  APR_CHECK_ARG(nq >= 0 && nq <= INT32_MAX - 4 && ns > 0 && ns <= INT32_MAX && extent > 0.f,
                "apr_kpconv_weighted_c32: bad arguments");
  APR_CHECK_ARG(ldx >= cin && ldwf >= (int64_t)kKP * cin, "apr_kpconv_weighted_c32: leading dimension too small");
  if (nq == 0) return APR_OK;
  APR_CHECK_ARG(q_pts && s_pts && nbr && x && kernel_points && rowsum && wf, "apr_kpconv_weighted_c32: null pointer");
  APR_CHECK_ARG(ldx % 2 == 0 && ldwf % 2 == 0 && ((((uintptr_t)x) | ((uintptr_t)wf)) & 7) == 0,
                "apr_kpconv_weighted_c32: the rows of x and wf must start on 8-byte boundaries");
  hipLaunchKernelGGL(k_kpconv_weighted_c32, dim3((unsigned)cdiv64(nq, 4)), dim3(256), 0, (hipStream_t)stream, q_pts, s_pts,
                     nbr, H, x, ldx, kernel_points, extent, rowsum, wf, ldwf, (int)nq, (int)ns, kpconv_xcd());
  APR_LAUNCH_CHECK();
  return APR_OK;
}

template <int INF, bool CLOSEST>
static int kpconv_dfeat(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                        const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                        float extent, const float* rowsum, float* dx, int64_t lddx, float* contrib, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(n_kp == kKP, "apr_kpconv_dfeat: built for %d kernel points, got %d", kKP, n_kp);
  APR_CHECK_ARG(nq >= 0 && ns > 0 && H > 0 && H <= kMaxH && cin > 0 && cin <= 512 && extent > 0.f,
                "apr_kpconv_dfeat: bad arguments (H <= %d, cin <= 512)", kMaxH);
  APR_CHECK_ARG(lddx >= cin && lddwf >= (int64_t)kKP * cin, "apr_kpconv_dfeat: leading dimension too small");
  if (nq == 0) return APR_OK;
  const unsigned grid = (unsigned)cdiv64(nq, 4);
#define APR_DF(N)                                                                                                     \
  hipLaunchKernelGGL((k_kpconv_dfeat<N, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, dwf, lddwf, cin, \
                     kernel_points, extent, rowsum, dx, lddx, (int)nq, (int)ns, contrib)
  if (cin <= 64) APR_DF(1);
  else if (cin <= 128) APR_DF(2);
  else if (cin <= 256) APR_DF(4);
  else APR_DF(8);
#undef APR_DF
  APR_LAUNCH_CHECK();
  return APR_OK;
}

template <int INF, bool CLOSEST>
static int kpconv_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                                float extent, const float* rowsum, float* contrib, void* stream) {
  APR_CHECK_ARG(contrib != nullptr, "apr_kpconv_dfeat_contrib: null contribution buffer");
  return kpconv_dfeat<INF, CLOSEST>(q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent, rowsum, contrib,
                                    cin, contrib, stream);
}

APR_API int apr_kpconv_dfeat(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                             const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                             float extent, const float* rowsum, float* dx, int64_t lddx, void* stream) {
  return kpconv_dfeat<kpmode::kLinear, false>(q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent,
                                              rowsum, dx, lddx, nullptr, stream);
}

// The deterministic form: the per-(query, neighbour) contributions go to contrib f32 [nq * H, cin] (rows of padding
// neighbours are left untouched and never read); apr_reverse_gather then sums every support point's rows in the order of
// the reverse table (apr_reverse_table_build): a fixed order, no float atomics.  Influence function and aggregation as in
// apr_kpconv_weighted_mode (blocks.py:320-345: d x flows through whichever influences the forward used; the closest kernel
// point is the forward's, kpmode::closest_kp).
APR_API int apr_kpconv_dfeat_contrib_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                          int32_t H, const float* dwf, int64_t lddwf, int32_t cin,
                                          const float* kernel_points, int32_t n_kp, float extent, const float* rowsum,
                                          float* contrib, int32_t influence, int32_t closest, void* stream) {
  APR_CHECK_ARG(kpmode::valid(influence, closest),
                "apr_kpconv_dfeat_contrib_mode: influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d", influence, closest);
  APR_KP_MODE_DISPATCH(kpconv_dfeat_contrib, q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent, rowsum,
                       contrib, stream)
}

// linear influence, sum aggregation
APR_API int apr_kpconv_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                     int32_t H, const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points,
                                     int32_t n_kp, float extent, const float* rowsum, float* contrib, void* stream) {
  return apr_kpconv_dfeat_contrib_mode(q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, kernel_points, n_kp, extent, rowsum,
                                       contrib, kpmode::kLinear, 0, stream);
}

APR_API int apr_gather_pool(const float* x, int64_t ldx, int64_t ns, int32_t c, const int32_t* inds, int32_t H,
                            int64_t nq, int32_t mode, float* out, int64_t ldo, void* stream) {
  APR_CHECK_ARG(nq >= 0 && ns >= 0 && c > 0 && H > 0 && ldx >= c && ldo >= c && (mode == 0 || mode == 1),
                "apr_gather_pool: bad arguments");
  if (nq == 0) return APR_OK;
  const bool vec = (c & 3) == 0 && (ldx & 3) == 0 && (ldo & 3) == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
  int64_t nblk = cdiv64(nq * (vec ? c / 4 : c), 256);
  if (nblk > 16384) nblk = 16384;
  if (vec)
    hipLaunchKernelGGL(k_gather_pool4, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)ns, c, inds,
                       H, nq, mode, out, ldo);
  else
    hipLaunchKernelGGL(k_gather_pool, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)ns, c, inds, H,
                       nq, mode, out, ldo);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// max_pool (blocks.py:86-102) with the arg-max kept for the backward: amax u8 [nq, c] (H <= 255).
APR_API int apr_gather_pool_argmax(const float* x, int64_t ldx, int64_t ns, int32_t c, const int32_t* inds, int32_t H,
                                   int64_t nq, float* out, int64_t ldo, uint8_t* amax, void* stream) {
  APR_CHECK_ARG(nq >= 0 && ns >= 0 && c > 0 && H > 0 && H <= 255 && ldx >= c && ldo >= c && x && inds && out && amax,
                "apr_gather_pool_argmax: bad arguments (H <= 255)");
  if (nq == 0) return APR_OK;
  int64_t nblk = cdiv64(nq * c, 256);
  if (nblk > 16384) nblk = 16384;
  hipLaunchKernelGGL(k_gather_pool_argmax, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)ns, c, inds, H,
                     nq, out, ldo, amax);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Input gradient of max_pool (mode 0, amax from apr_gather_pool_argmax) / closest_pool (mode 1, amax unused) over the
// reverse table of the SAME index tensor (apr_reverse_table_build(inds, nq, H, ns)): dx f32 [ns, c], every row written.
APR_API int apr_gather_pool_backward(const float* dout, int64_t lddo, int32_t c, const int32_t* rev_t, const int32_t* start,
                                     int64_t ns, int32_t H, const uint8_t* amax, int32_t mode, float* dx, int64_t lddx,
                                     void* stream) {
  APR_CHECK_ARG(dout && rev_t && start && dx && ns > 0 && c > 0 && H > 0 && lddo >= c && lddx >= c && (mode == 1 || amax) &&
                    (mode == 0 || mode == 1),
                "apr_gather_pool_backward: bad arguments");
  int64_t nblk = cdiv64(ns * c, 256);
  if (nblk > 16384) nblk = 16384;
  hipLaunchKernelGGL(k_gather_pool_bwd, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, dout, lddo, c, rev_t, start, ns,
                     H, amax, mode, dx, lddx);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Deformable / modulated KPConv (Predator_APR/models/blocks.py:229-374 with deformable=True): the kernel-point
// correlation with PER-QUERY kernel points, its feature gradient and its geometry gradient.
//
//   dkp[q, k]  = kernel_points[k] + extent * offsets[q, k]          (blocks.py:258, 279; built by the caller)
//   mod[q, k]  = 2 sigmoid(offset_features[q, 45 + k]), or 1        (blocks.py:247)
//   diff       = s[nbr[q, h]] - q - dkp[q, k],  d2 = |diff|^2,  w = max(0, 1 - sqrt(d2) / extent)   (real neighbours)
//   min_d2[q,k]= min over ALL H slots of d2, a padding slot entering as the point (1e6, 1e6, 1e6)     (blocks.py:295)
//   in_range[q, h] = real and d2 < extent^2 for some k                                                (blocks.py:298)
//   num[q]     = max(1, #{h : in_range and rowsum[nbr[q, h]] > 0})                                    (blocks.py:369-371)
//   wf[q, k * cin + c] = mod[q, k] / num[q] * sum_h w[q, k, h] x[nbr[q, h], c]                       (blocks.py:354-358)
// The reference re-gathers the in-range neighbours with a topk (blocks.py:301-316); w = 0 outside every ball, so the
// influences are the same without it and only the count sees the difference: a support beyond every DEFORMED kernel
// point does not count (the rigid kernel counts it).
//
// Backward (num and in_range are constants, as in the graph torch builds), dwf = d_out @ W^T:
//   contrib[(q, h), c] = sum_k mod[q, k] w[q, k, h] dwf[q, k * cin + c] / num[q]     real neighbours; padding rows untouched
//   P[h, k]     = <x[nbr[q, h], :], dwf[q, k, :]>
//   d_mod[q, k] = sum_h w[q, k, h] P[h, k] / num[q]
//   d_dkp[q, k] = mod[q, k] / num[q] * sum_{h real, 0 < d < extent} diff / (d * extent) * P[h, k]
// DEVIATION from the reference: a neighbour exactly on a deformed kernel point (d = 0) contributes 0 to d_dkp; the
// reference's graph gives NaN there (the derivative of sqrt at 0 times 0).
//
// All three kernels: one wave per query, 4 per block, n_kp = 15, cin % 64 == 0, cin <= 512, 1 <= H <= 128, 16-byte
// aligned rows; every sum in a fixed order (no atomics): the same bits on every run.
//
// Influence and aggregation (blocks.py:320-345) are compile-time parameters INF / CLOSEST of all three kernels; <kLinear,
// false> gives the formulas above.  For the constant and the gaussian influence the reference's re-gather DOES matter: a real
// neighbour outside every deformed ball contributes nothing (in_range masks w), one inside a ball carries its influence to
// all 15 kernel points, or with CLOSEST to its nearest one alone (kpmode::closest_kp, the same statement in every kernel).
//   gaussian: w = exp(-d2 / (2 sigma^2 + 1e-9)), sigma = 0.3 extent;  d_dkp = mod / num * sum_{h in range} w 2 diff / (2 sigma^2 + 1e-9) P
//   constant: w = 1;  d_dkp = 0
#include "kpconv.h"

namespace {

constexpr float kShadow = 1e6f;

// Step 1.  The MFMA form of k_kpconv_weighted_mfma (kpconv.hip): A = w[k = r16][h = qd] on the fly from the lane's own
// dkp[q, r16], B = one 16-byte gather per lane.  New: a geometry pass before the channel passes gives, per step of 4
// neighbours, the in-range flags (one ballot: the 16 lanes of a k-slot hold the 15 kernel points of its neighbour), the
// count from them, and the running minimum of d2 per kernel point (reduced over the four k-slot lane groups at the end).
// With a mode other than <kLinear, false> the lane that stages slot h also records the slot's mode byte (closest kernel
// point, in-range flag) for the channel passes.
template <int NG, int INF = kpmode::kLinear, bool CLOSEST = false>
__global__ __launch_bounds__(256) void k_kpconv_deform_weighted(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ dkp, const float* __restrict__ mod,
    float extent, const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf, float* __restrict__ min_d2,
    int nq, int ns, int xcd_swz) {
  __shared__ int s_idx[4][kMaxH];          // >= 0: support row; -1: padding; bit 30 of a real row: positive feature sum
  __shared__ float s_diff[4][kMaxH][3];
  constexpr bool MODE = CLOSEST || INF != kpmode::kLinear;
  __shared__ unsigned char s_cl[MODE ? 4 : 1][MODE ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = kp_xcd_block(xcd_swz) * 4 + wave;
  if (qi >= nq) return;
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  for (int h = lane; h < kMaxH; h += 64) {
    int idx = -1;
    float dx = kShadow - qx, dy = kShadow - qy, dz = kShadow - qz;      // the shadow point, centred as the reference does
    if (h < H) {
      const int v = nbr[(int64_t)qi * H + h];
      if (v >= 0 && v < ns) {
        idx = v | (rowsum[v] > 0.f ? (1 << 30) : 0);
        dx = s_pts[3 * (int64_t)v] - qx;
        dy = s_pts[3 * (int64_t)v + 1] - qy;
        dz = s_pts[3 * (int64_t)v + 2] - qz;
      }
    }
    s_idx[wave][h] = idx;
    s_diff[wave][h][0] = dx; s_diff[wave][h][1] = dy; s_diff[wave][h][2] = dz;
    if constexpr (MODE)
      s_cl[wave][h] = idx >= 0 ? (unsigned char)kpmode::closest_kp(dx, dy, dz, dkp + (int64_t)qi * kKP * 3, extent * extent) : 0;
  }
  // (the wave's LDS writes are read back by other lanes of the same wave: in-order LDS queue, no barrier needed)
  const float inv_extent = 1.f / extent, ext2 = extent * extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  const bool kvalid = r16 < kKP;
  const float* kq = dkp + ((int64_t)qi * kKP + (kvalid ? r16 : 0)) * 3;
  const float kx = kq[0], ky = kq[1], kz = kq[2];
  const int nsteps = (H + 3) >> 2;
  int cnt = 0;
  float mn = __builtin_inff();
  for (int st = 0; st < nsteps; ++st) {
    const int h = st * 4 + qd;
    const int idx = s_idx[wave][h];
    const float ex = s_diff[wave][h][0] - kx, ey = s_diff[wave][h][1] - ky, ez = s_diff[wave][h][2] - kz;
    const float d2 = ex * ex + ey * ey + ez * ez;
    if (kvalid && h < H) mn = fminf(mn, d2);
    const unsigned long long m = __ballot(kvalid && idx >= 0 && d2 < ext2);
    const bool counted = ((m >> (16 * qd)) & 0xffffull) != 0 && idx >= 0 && (idx & (1 << 30)) && r16 == 0;
    cnt += __popcll(__ballot(counted));
  }
  mn = fminf(mn, __shfl_xor(mn, 16));
  mn = fminf(mn, __shfl_xor(mn, 32));
  if (min_d2 && qd == 0 && kvalid) min_d2[(int64_t)qi * kKP + r16] = mn;
  const float inv_num = 1.f / (float)max(cnt, 1);
  float sc[4];      // the epilogue's factor of output row k = 4 qd + i: mod / num
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = qd * 4 + i;
    sc[i] = (mod && k < kKP) ? mod[(int64_t)qi * kKP + k] * inv_num : inv_num;
  }
  for (int g0 = 0; g0 < cin / 64; g0 += NG) {
    f32x4 acc[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[g][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < nsteps; ++st) {
      const int h = st * 4 + qd;
      const int raw = s_idx[wave][h];
      const int idx = raw & ~(1 << 30);
      float w = 0.f;
      if (kvalid && raw >= 0) {
        // constant, gaussian: only the neighbours inside some deformed ball take part (blocks.py:298-316)
        const float ex = s_diff[wave][h][0] - kx, ey = s_diff[wave][h][1] - ky, ez = s_diff[wave][h][2] - kz;
        const bool part = INF == kpmode::kLinear || (s_cl[wave][h] & kpmode::kInRange);
        w = part ? kpmode::influence<INF>(ex * ex + ey * ey + ez * ez, inv_extent, gden) : 0.f;
        if constexpr (CLOSEST) w = (s_cl[wave][h] & 15) == r16 ? w : 0.f;
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f32x4 b = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (raw >= 0 && g0 + g < cin / 64)
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
          f32x4 v = {acc[g][0][i] * sc[i], acc[g][1][i] * sc[i], acc[g][2][i] * sc[i], acc[g][3][i] * sc[i]};
          *reinterpret_cast<f32x4*>(wf + (int64_t)qi * ldwf + (int64_t)k * cin + (g0 + g) * 64 + r16 * 4) = v;
        }
      }
    }
  }
}

// The index stage the two backward kernels share: lane h of the wave fills slot h (idx, centred point, and for the
// feature gradient the 15 influences) and the wave's in-range count comes back.  dkp[q] is read at wave-uniform
// addresses.
// With a mode other than <kLinear, false>: the influences kept are the mode's (masked by the in-range flag unless linear,
// and by the closest kernel point with CLOSEST); the geometry gradient gets the slot's mode byte in s_cl instead.
template <bool KEEP_W, int INF = kpmode::kLinear, bool CLOSEST = false>
__device__ inline int deform_index_stage(const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                         const int* __restrict__ nbr, int H, const float* __restrict__ kq, float extent,
                                         const float* __restrict__ rowsum, int qi, int ns, int lane, int* s_idx,
                                         float (*s_diff)[3], float (*s_w)[16], unsigned char* s_cl = nullptr) {
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  constexpr bool MODE = CLOSEST || INF != kpmode::kLinear;
  [[maybe_unused]] const float inv_extent = 1.f / extent;
  const float ext2 = extent * extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  int cnt = 0;
  for (int h = lane; h < kMaxH; h += 64) {
    int idx = -1;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (h < H) {
      idx = nbr[(int64_t)qi * H + h];
      if (idx < 0 || idx >= ns) idx = -1;
    }
    if (idx >= 0) {
      dx = s_pts[3 * (int64_t)idx] - qx;
      dy = s_pts[3 * (int64_t)idx + 1] - qy;
      dz = s_pts[3 * (int64_t)idx + 2] - qz;
      // in range: a mode takes the flag from the closest kernel point's statement, <kLinear, false> from the influences' d2
      const int cl = MODE ? kpmode::closest_kp(dx, dy, dz, kq, ext2) : 0;
      bool inr = (cl & kpmode::kInRange) != 0;
      if constexpr (KEEP_W || !MODE) {
#pragma unroll
        for (int k = 0; k < kKP; ++k) {
          const float ex = dx - kq[3 * k], ey = dy - kq[3 * k + 1], ez = dz - kq[3 * k + 2];
          const float d2 = ex * ex + ey * ey + ez * ez;
          if constexpr (!MODE) inr = inr || d2 < ext2;
          if constexpr (KEEP_W) {
            const float w = (INF == kpmode::kLinear || inr) ? kpmode::influence<INF>(d2, inv_extent, gden) : 0.f;
            s_w[h][k] = (!CLOSEST || k == (cl & 15)) ? w : 0.f;
          }
        }
      }
      if constexpr (!KEEP_W && MODE) s_cl[h] = (unsigned char)cl;
      cnt += (inr && rowsum[idx] > 0.f) ? 1 : 0;
    }
    s_idx[h] = idx;
    if (!KEEP_W) { s_diff[h][0] = dx; s_diff[h][1] = dy; s_diff[h][2] = dz; }
  }
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  return cnt;
}

// Feature gradient, contribution rows: k_kpconv_dfeat (kpconv.hip) with the query's own kernel points, mod folded into
// the 15 register values of a lane's channel, and the in-range count.
template <int CPL, int INF = kpmode::kLinear, bool CLOSEST = false>   // channels per lane: cin <= 64 * CPL
__global__ __launch_bounds__(256) void k_kpconv_deform_dfeat(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ dwf, int64_t lddwf, int cin, const float* __restrict__ dkp, const float* __restrict__ mod,
    float extent, const float* __restrict__ rowsum, int nq, int ns, float* __restrict__ contrib) {
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_w[4][kMaxH][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * 4 + wave;
  if (qi >= nq) return;
  const int cnt = deform_index_stage<true, INF, CLOSEST>(q_pts, s_pts, nbr, H, dkp + (int64_t)qi * kKP * 3, extent, rowsum, qi,
                                                         ns, lane, s_idx[wave], nullptr, s_w[wave]);
  const float inv_num = 1.f / (float)max(cnt, 1);
  float g[CPL][kKP];
#pragma unroll
  for (int k = 0; k < kKP; ++k) {
    const float f = mod ? mod[(int64_t)qi * kKP + k] * inv_num : inv_num;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = lane + 64 * u;
      g[u][k] = c < cin ? dwf[(int64_t)qi * lddwf + (int64_t)k * cin + c] * f : 0.f;
    }
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
      if (c < cin) contrib[((int64_t)qi * H + h) * cin + c] = acc;
    }
  }
}

// Geometry gradient.  P[h, k] = <x[nbr[q, h], :], dwf[q, k, :]> is an [H, cin] x [cin, 16] product on the fp32 MFMA:
// rows = 16 neighbours of a tile, columns = kernel points, contraction over channels.  A dot product does not care in
// which order the channels meet, so BOTH operands come straight from memory as 16-byte loads with the same channel map
// (k-slot qd of step 4 j + e of a 64-channel chunk <-> channel 16 qd + 4 j + e): lane (r16, qd) loads 64 contiguous bytes
// of x row h = 16 t + r16 (A) and of dwf[q, k = r16] (B); the four k-slot lanes of a row read one 256-byte line.  dwf[q]
// is the stationary operand: 16 registers per chunk, loaded once; the <= 8 neighbour tiles stream under it into 8
// accumulators, so every gathered row is read once.  LDS holds only the index stage's [128] rows and [128][3] centred
// points per wave: written at stride 3 words by 64 lanes (3 is odd: conflict free), read with 4 distinct rows per
// instruction (broadcast within each k-slot group).
// The accumulator leaves lane (k = r16, qd) with P[h = 16 t + 4 qd + i][k]: it combines them with ITS kernel point's
// diff / (d extent) and w in ascending (t, i), the four qd groups meet by two shuffles: a fixed order.
// Modes: the term of (h, k) exists for the neighbours in range (and, with CLOSEST, for the neighbour's closest kernel point
// alone: the one-hot mask is a constant of the graph).  gaussian: d_mod += w P, d_dkp += w 2 diff / (2 sigma^2 + 1e-9) P -- no
// singularity at d = 0, so no term is left out there; constant: d_mod += P, d_dkp = 0 exactly.
template <int INF = kpmode::kLinear, bool CLOSEST = false>
__global__ __launch_bounds__(256) void k_kpconv_deform_dgeom(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ dwf, int64_t lddwf,
    const float* __restrict__ dkp, const float* __restrict__ mod, float extent, const float* __restrict__ rowsum,
    float* __restrict__ d_dkp, float* __restrict__ d_mod, int nq, int ns) {
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_diff[4][kMaxH][3];
  constexpr bool MODE = CLOSEST || INF != kpmode::kLinear;
  __shared__ unsigned char s_cl[MODE ? 4 : 1][MODE ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = blockIdx.x * 4 + wave;
  if (qi >= nq) return;
  const float* kq = dkp + (int64_t)qi * kKP * 3;
  const int cnt = deform_index_stage<false, INF, CLOSEST>(q_pts, s_pts, nbr, H, kq, extent, rowsum, qi, ns, lane, s_idx[wave],
                                                          s_diff[wave], nullptr, s_cl[MODE ? wave : 0]);
  const float inv_num = 1.f / (float)max(cnt, 1);
  const bool kvalid = r16 < kKP;
  const int ntile = (H + 15) >> 4;
  int arow[8];      // the x row of this lane's A operand per tile, -1: a zero row
#pragma unroll
  for (int t = 0; t < 8; ++t) arow[t] = t < ntile ? s_idx[wave][t * 16 + r16] : -1;
  f32x4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* brow = dwf + (int64_t)qi * lddwf + (int64_t)(kvalid ? r16 : 0) * cin + 16 * qd;
  for (int c0 = 0; c0 < cin; c0 += 64) {
    f32x4 b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      b[j] = kvalid ? *reinterpret_cast<const f32x4*>(brow + c0 + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (t < ntile) {      // wave-uniform
        f32x4 a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          a[j] = arow[t] >= 0 ? *reinterpret_cast<const f32x4*>(x + (int64_t)arow[t] * ldx + c0 + 16 * qd + 4 * j)
                              : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[j][e], acc[t], 0, 0, 0);
      }
    }
  }
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  const float kx = kvalid ? kq[3 * r16] : 0.f, ky = kvalid ? kq[3 * r16 + 1] : 0.f, kz = kvalid ? kq[3 * r16 + 2] : 0.f;
  float gx = 0.f, gy = 0.f, gz = 0.f, gm = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t < ntile) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = t * 16 + 4 * qd + i;
        if (s_idx[wave][h] >= 0) {      // real (slots behind H hold -1)
          const float ex = s_diff[wave][h][0] - kx, ey = s_diff[wave][h][1] - ky, ez = s_diff[wave][h][2] - kz;
          if constexpr (INF == kpmode::kLinear) {
            const float d = sqrtf(ex * ex + ey * ey + ez * ez);
            const float w = 1.f - d * inv_extent;
            bool live = w > 0.f;
            if constexpr (CLOSEST) live = live && (s_cl[wave][h] & 15) == r16;
            if (live) {
              const float p = acc[t][i];
              gm = fmaf(w, p, gm);
              if (d > 0.f) {
                const float f = p / (d * extent);
                gx = fmaf(ex, f, gx); gy = fmaf(ey, f, gy); gz = fmaf(ez, f, gz);
              }
            }
          } else {
            const int cl = s_cl[wave][h];
            bool live = (cl & kpmode::kInRange) != 0;
            if constexpr (CLOSEST) live = live && (cl & 15) == r16;
            if (live) {
              const float p = acc[t][i];
              if constexpr (INF == kpmode::kGaussian) {
                const float w = kpmode::influence<INF>(ex * ex + ey * ey + ez * ez, inv_extent, gden);
                gm = fmaf(w, p, gm);
                const float f = w * (2.f / gden) * p;
                gx = fmaf(ex, f, gx); gy = fmaf(ey, f, gy); gz = fmaf(ez, f, gz);
              } else {
                gm += p;      // constant influence: no dependence on the kernel point's position
              }
            }
          }
        }
      }
    }
  }
  gx += __shfl_xor(gx, 16); gy += __shfl_xor(gy, 16); gz += __shfl_xor(gz, 16); gm += __shfl_xor(gm, 16);
  gx += __shfl_xor(gx, 32); gy += __shfl_xor(gy, 32); gz += __shfl_xor(gz, 32); gm += __shfl_xor(gm, 32);
  if (qd == 0 && kvalid) {
    const float f = mod ? mod[(int64_t)qi * kKP + r16] * inv_num : inv_num;
    float* o = d_dkp + ((int64_t)qi * kKP + r16) * 3;
    o[0] = gx * f; o[1] = gy * f; o[2] = gz * f;
    d_mod[(int64_t)qi * kKP + r16] = gm * inv_num;
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

#define APR_DEFORM_SHAPE(fn)                                                                                           \
  APR_CHECK_ARG(n_kp == kKP, fn ": built for %d kernel points, got %d", kKP, n_kp);                                    \
  APR_CHECK_ARG(nq >= 0 && ns > 0 && ns < (1 << 30) && H >= 1 && H <= kMaxH && cin >= 64 && cin <= 512 && cin % 64 == 0 && extent > 0.f, \
                fn ": needs cin %% 64 == 0, cin <= 512, 1 <= H <= %d, ns > 0, extent > 0", kMaxH);                     \
  APR_CHECK_ARG(q_pts && s_pts && nbr && dkp && rowsum, fn ": null argument")

// One body per operation; the entry points without a mode are the _mode ones at (linear, sum).
template <int INF, bool CLOSEST>
static int deform_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                           const float* x, int64_t ldx, int32_t cin, const float* dkp, const float* mod, int32_t n_kp,
                           float extent, const float* rowsum, float* wf, int64_t ldwf, float* min_d2, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_DEFORM_SHAPE("apr_kpconv_deform_weighted");
  APR_CHECK_ARG(x && wf && ldx >= cin && ldwf >= (int64_t)kKP * cin && ldx % 4 == 0 && ldwf % 4 == 0 && aligned16(x) &&
                    aligned16(wf),
                "apr_kpconv_deform_weighted: x / wf rows must be 16-byte aligned and at least cin / 15 cin wide");
  if (nq == 0) return APR_OK;
  const unsigned grid = (unsigned)cdiv64(nq, 4);
  const int s_xcd = kpconv_xcd();
#define APR_DW(N)                                                                                                       \
  hipLaunchKernelGGL((k_kpconv_deform_weighted<N, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, ldx, \
                     cin, dkp, mod, extent, rowsum, wf, ldwf, min_d2, (int)nq, (int)ns, s_xcd)
  if (cin >= 256) APR_DW(4);
  else if (cin == 128) APR_DW(2);
  else APR_DW(1);
#undef APR_DW
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_kpconv_deform_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                       int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dkp,
                                       const float* mod, int32_t n_kp, float extent, const float* rowsum, float* wf,
                                       int64_t ldwf, float* min_d2, void* stream) {
  return apr_kpconv_deform_weighted_mode(q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dkp, mod, n_kp, extent, rowsum, wf, ldwf,
                                         min_d2, kpmode::kLinear, 0, stream);
}

#define APR_DEFORM_MODE(fn)                                                                                            \
  APR_CHECK_ARG(kpmode::valid(influence, closest), fn ": influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d", \
                influence, closest)

// apr_kpconv_deform_weighted with the influence function (0 constant, 1 linear, 2 gaussian: blocks.py:320-337, 61-68) and
// the aggregation (closest = 1: blocks.py:339-345).  For the constant and the gaussian influence only the neighbours inside
// some deformed ball take part (the re-gather of blocks.py:298-316).  (1, 0) launches what apr_kpconv_deform_weighted
// launches: the same bits.
APR_API int apr_kpconv_deform_weighted_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                            int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dkp,
                                            const float* mod, int32_t n_kp, float extent, const float* rowsum, float* wf,
                                            int64_t ldwf, float* min_d2, int32_t influence, int32_t closest, void* stream) {
  APR_DEFORM_MODE("apr_kpconv_deform_weighted_mode");
  APR_KP_MODE_DISPATCH(deform_weighted, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dkp, mod, n_kp, extent, rowsum, wf, ldwf,
                       min_d2, stream)
}

template <int INF, bool CLOSEST>
static int deform_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                const float* dwf, int64_t lddwf, int32_t cin, const float* dkp, const float* mod,
                                int32_t n_kp, float extent, const float* rowsum, float* contrib, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_DEFORM_SHAPE("apr_kpconv_deform_dfeat_contrib");
  APR_CHECK_ARG(dwf && contrib && lddwf >= (int64_t)kKP * cin,
                "apr_kpconv_deform_dfeat_contrib: null buffer or leading dimension too small");
  if (nq == 0) return APR_OK;
  const unsigned grid = (unsigned)cdiv64(nq, 4);
#define APR_DF(N)                                                                                                       \
  hipLaunchKernelGGL((k_kpconv_deform_dfeat<N, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, dwf, lddwf, \
                     cin, dkp, mod, extent, rowsum, (int)nq, (int)ns, contrib)
  if (cin <= 64) APR_DF(1);
  else if (cin <= 128) APR_DF(2);
  else if (cin <= 256) APR_DF(4);
  else APR_DF(8);
#undef APR_DF
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_kpconv_deform_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                            const int32_t* nbr, int32_t H, const float* dwf, int64_t lddwf, int32_t cin,
                                            const float* dkp, const float* mod, int32_t n_kp, float extent,
                                            const float* rowsum, float* contrib, void* stream) {
  return apr_kpconv_deform_dfeat_contrib_mode(q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, dkp, mod, n_kp, extent, rowsum,
                                              contrib, kpmode::kLinear, 0, stream);
}

// apr_kpconv_deform_dfeat_contrib with the mode of apr_kpconv_deform_weighted_mode: d x flows through the influences the
// forward used (blocks.py:320-358), in-range filter and closest kernel point included.  (1, 0): the same bits as the old entry.
APR_API int apr_kpconv_deform_dfeat_contrib_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                                 const int32_t* nbr, int32_t H, const float* dwf, int64_t lddwf, int32_t cin,
                                                 const float* dkp, const float* mod, int32_t n_kp, float extent,
                                                 const float* rowsum, float* contrib, int32_t influence, int32_t closest,
                                                 void* stream) {
  APR_DEFORM_MODE("apr_kpconv_deform_dfeat_contrib_mode");
  APR_KP_MODE_DISPATCH(deform_dfeat_contrib, q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, dkp, mod, n_kp, extent, rowsum,
                       contrib, stream)
}

template <int INF, bool CLOSEST>
static int deform_dgeom(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                        const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf, const float* dkp,
                        const float* mod, int32_t n_kp, float extent, const float* rowsum, float* d_dkp, float* d_mod,
                        void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_DEFORM_SHAPE("apr_kpconv_deform_dgeom");
  APR_CHECK_ARG(x && dwf && d_dkp && d_mod && ldx >= cin && lddwf >= (int64_t)kKP * cin && ldx % 4 == 0 && lddwf % 4 == 0 &&
                    aligned16(x) && aligned16(dwf),
                "apr_kpconv_deform_dgeom: x / dwf rows must be 16-byte aligned and at least cin / 15 cin wide");
  if (nq == 0) return APR_OK;
  hipLaunchKernelGGL((k_kpconv_deform_dgeom<INF, CLOSEST>), dim3((unsigned)cdiv64(nq, 4)), dim3(256), 0, st, q_pts, s_pts, nbr,
                     H, x, ldx, cin, dwf, lddwf, dkp, mod, extent, rowsum, d_dkp, d_mod, (int)nq, (int)ns);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_kpconv_deform_dgeom(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                    int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf,
                                    const float* dkp, const float* mod, int32_t n_kp, float extent, const float* rowsum,
                                    float* d_dkp, float* d_mod, void* stream) {
  return apr_kpconv_deform_dgeom_mode(q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dwf, lddwf, dkp, mod, n_kp, extent, rowsum,
                                      d_dkp, d_mod, kpmode::kLinear, 0, stream);
}

// apr_kpconv_deform_dgeom with the mode of apr_kpconv_deform_weighted_mode (the graph of blocks.py:284-358 differentiated
// with respect to deformed_KP and the modulations): linear as the old entry, masked by the closest kernel point's one-hot
// when closest; gaussian d_dkp = mod / num * sum_{h in range} w 2 diff / (2 sigma^2 + 1e-9) P; constant d_dkp = 0 exactly;
// d_mod = sum_h w P / num with the mode's w.  (1, 0): the same bits as the old entry.
APR_API int apr_kpconv_deform_dgeom_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                         int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf,
                                         const float* dkp, const float* mod, int32_t n_kp, float extent, const float* rowsum,
                                         float* d_dkp, float* d_mod, int32_t influence, int32_t closest, void* stream) {
  APR_DEFORM_MODE("apr_kpconv_deform_dgeom_mode");
  APR_KP_MODE_DISPATCH(deform_dgeom, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dwf, lddwf, dkp, mod, n_kp, extent, rowsum,
                       d_dkp, d_mod, stream)
}

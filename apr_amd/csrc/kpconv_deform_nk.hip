// Deformable / modulated KPConv for any kernel-point count 1 <= n_kp <= 32 (the reference's `num_kernel_points` on a
// deformable block; kpconv_deform.hip is built for the 15 points of the shipped configs and keeps its launches): the
// correlation with PER-QUERY kernel points (apr_kpconv_deform_weighted_nk), its feature gradient
// (apr_kpconv_deform_dfeat_contrib_nk) and its geometry gradient (apr_kpconv_deform_dgeom_nk), every influence and both
// aggregations.  The contract is kpconv_deform.hip's header and tests/kpconv_deform_nk_oracle.py's with dkp [nq, n_kp, 3],
// mod / min_d2 / d_mod [nq, n_kp], d_dkp [nq, n_kp, 3] and wf[q, k * cin + c] for k < n_kp.
//
// The kernels are kpconv_deform.hip's with the kernel-point count as data, tiled as kpconv_nk.hip tiles the rigid ones: the
// MFMA kernels carry ONE 16-row tile of kernel points for n_kp <= 16 and TWO for 17..32 (lane r16 owns kernel points r16
// and 16 + r16 of dkp[q]); rows k >= n_kp carry w = 0 (a zero B operand in the geometry gradient) and are neither stored
// nor counted.  One wave per query, cin % 64 == 0, 64 <= cin <= 512, 1 <= H <= 128, 16-byte aligned rows; no atomics, every
// sum in a fixed order: the same bits on every run.  The closest kernel point and, for a mode other than (linear, sum), the
// in-range flag come from closest_kp_nk (kpconv_nk.h) on dkp[q] with extent^2 in all three kernels.
#include "kpconv_nk.h"

namespace {

constexpr float kShadow = 1e6f;

// Step 1: k_kpconv_deform_weighted with T tiles of kernel points and NG 64-channel groups per pass (T * NG * 16 accumulator
// registers: <1, 4> and <2, 2> hold 64).  One gathered B operand feeds both tiles.  The geometry pass: a slot's in-range
// flag is the OR over the lane's T kernel points BEFORE the ballot (the 16 lanes of a k-slot then hold all n_kp kernel
// points of its neighbour), the count comes from that flag, the running minimum of d2 is kept per tile and stored for all
// n_kp rows.
template <int T, int NG, int INF, bool CLOSEST>
__global__ __launch_bounds__(256) void k_kpconv_deform_weighted_nk(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ dkp, const float* __restrict__ mod, int n_kp,
    float extent, const float* __restrict__ rowsum, float* __restrict__ wf, int64_t ldwf, float* __restrict__ min_d2, int nq,
    int ns, int xcd_swz) {
  __shared__ int s_idx[4][kMaxH];          // >= 0: support row; -1: padding; bit 30 of a real row: positive feature sum
  __shared__ float s_diff[4][kMaxH][3];
  constexpr bool MODE = CLOSEST || INF != kpmode::kLinear;
  __shared__ unsigned char s_cl[MODE ? 4 : 1][MODE ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = kp_xcd_block(xcd_swz) * 4 + wave;
  if (qi >= nq) return;
  const float* kq = dkp + (int64_t)qi * n_kp * 3;
  const float ext2 = extent * extent;
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
    if constexpr (MODE) s_cl[wave][h] = idx >= 0 ? (unsigned char)closest_kp_nk(dx, dy, dz, kq, n_kp, ext2) : 0;
  }
  // (the wave's LDS writes are read back by other lanes of the same wave: in-order LDS queue, no barrier needed)
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
  bool kvalid[T];
  float kx[T], ky[T], kz[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int k = 16 * t + r16;
    kvalid[t] = k < n_kp;
    kx[t] = kvalid[t] ? kq[3 * k] : 0.f;
    ky[t] = kvalid[t] ? kq[3 * k + 1] : 0.f;
    kz[t] = kvalid[t] ? kq[3 * k + 2] : 0.f;
  }
  const int nsteps = (H + 3) >> 2;
  int cnt = 0;
  float mn[T];
#pragma unroll
  for (int t = 0; t < T; ++t) mn[t] = __builtin_inff();
  for (int st = 0; st < nsteps; ++st) {
    const int h = st * 4 + qd;
    const int idx = s_idx[wave][h];
    bool inr = false;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const float d2 = kp_d2(s_diff[wave][h][0], s_diff[wave][h][1], s_diff[wave][h][2], kx[t], ky[t], kz[t]);
      if (kvalid[t] && h < H) mn[t] = fminf(mn[t], d2);
      inr = inr || (kvalid[t] && idx >= 0 && d2 < ext2);
    }
    const unsigned long long m = __ballot(inr);
    const bool counted = ((m >> (16 * qd)) & 0xffffull) != 0 && idx >= 0 && (idx & (1 << 30)) && r16 == 0;
    cnt += __popcll(__ballot(counted));
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    mn[t] = fminf(mn[t], __shfl_xor(mn[t], 16));
    mn[t] = fminf(mn[t], __shfl_xor(mn[t], 32));
    if (min_d2 && qd == 0 && kvalid[t]) min_d2[(int64_t)qi * n_kp + 16 * t + r16] = mn[t];
  }
  const float inv_num = 1.f / (float)max(cnt, 1);
  float sc[T][4];      // the epilogue's factor of output row k = 16 t + 4 qd + i: mod / num
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 16 * t + qd * 4 + i;
      sc[t][i] = (mod && k < n_kp) ? mod[(int64_t)qi * n_kp + k] * inv_num : inv_num;
    }
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
      const int raw = s_idx[wave][h];
      const int idx = raw & ~(1 << 30);
      float w[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        w[t] = 0.f;
        if (kvalid[t] && raw >= 0) {
          // constant, gaussian: only the neighbours inside some deformed ball take part (blocks.py:298-316)
          bool part = true;
          if constexpr (INF != kpmode::kLinear) part = (s_cl[wave][h] & kpmode::kInRange) != 0;
          w[t] = part ? kpmode::influence<INF>(kp_d2(s_diff[wave][h][0], s_diff[wave][h][1], s_diff[wave][h][2], kx[t], ky[t],
                                                     kz[t]),
                                               inv_extent, gden)
                      : 0.f;
          if constexpr (CLOSEST) w[t] = (int)(s_cl[wave][h] & 31) == 16 * t + r16 ? w[t] : 0.f;
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        f32x4 b = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (raw >= 0 && g0 + g < cin / 64)
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
            const float f = sc[t][i];
            f32x4 v = {acc[t][g][0][i] * f, acc[t][g][1][i] * f, acc[t][g][2][i] * f, acc[t][g][3][i] * f};
            *reinterpret_cast<f32x4*>(wf + (int64_t)qi * ldwf + (int64_t)k * cin + (g0 + g) * 64 + r16 * 4) = v;
          }
        }
      }
  }
}

// The index stage the two backward kernels share (deform_index_stage of kpconv_deform.hip with n_kp as data): lane h of the
// wave fills slot h -- idx, and either the KT influences of the slot (KEEP_W; columns k >= n_kp hold -0) or the centred
// point and, for a mode, the slot's mode byte -- and the wave's in-range count comes back.  kq = dkp[q] is read at
// wave-uniform addresses.  In range: a mode takes the flag from closest_kp_nk, <kLinear, false> from the influences' d2.
template <bool KEEP_W, int KT, int INF, bool CLOSEST>
__device__ inline int deform_index_stage_nk(const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                            const int* __restrict__ nbr, int H, const float* __restrict__ kq, int n_kp,
                                            float extent, const float* __restrict__ rowsum, int qi, int ns, int lane, int* s_idx,
                                            float (*s_diff)[3], float (*s_w)[KT], unsigned char* s_cl) {
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
      const int cl = MODE ? closest_kp_nk(dx, dy, dz, kq, n_kp, ext2) : 0;
      bool inr = (cl & kpmode::kInRange) != 0;
      if constexpr (KEEP_W || !MODE) {
        for (int k = 0; k < n_kp; ++k) {
          const float d2 = kp_d2(dx, dy, dz, kq[3 * k], kq[3 * k + 1], kq[3 * k + 2]);
          if constexpr (!MODE) inr = inr || d2 < ext2;
          if constexpr (KEEP_W) {
            const float w = (INF == kpmode::kLinear || inr) ? kpmode::influence<INF>(d2, inv_extent, gden) : 0.f;
            s_w[h][k] = (!CLOSEST || k == (cl & 31)) ? w : 0.f;
          }
        }
        if constexpr (KEEP_W)
          for (int k = n_kp; k < KT; ++k) s_w[h][k] = -0.f;
      }
      if constexpr (!KEEP_W && MODE) s_cl[h] = (unsigned char)cl;
      cnt += (inr && rowsum[idx] > 0.f) ? 1 : 0;
    }
    s_idx[h] = idx;
    if constexpr (!KEEP_W) { s_diff[h][0] = dx; s_diff[h][1] = dy; s_diff[h][2] = dz; }
  }
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  return cnt;
}

// Feature gradient, contribution rows: the layout of k_kpconv_dfeat_contrib_nk (kpconv_nk.hip) -- KT = 16 or 32 sizes the
// LDS influence table and the lane's g[CPL][KT]; KT = 32 runs two waves per block and channel passes of 64 CPL <= 256 --
// with the query's own kernel points and mod / num folded into g.  The k-sum is an ascending fmaf chain; columns k >= n_kp
// hold w = -0 and g = +0: fmaf(-0, +0, acc) = acc for every acc, a zero of either sign included.
template <int CPL, int KT, int INF, bool CLOSEST>
__global__ __launch_bounds__(KT == 16 ? 256 : 128) void k_kpconv_deform_dfeat_nk(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ dwf, int64_t lddwf, int cin, const float* __restrict__ dkp, const float* __restrict__ mod,
    int n_kp, float extent, const float* __restrict__ rowsum, int nq, int ns, float* __restrict__ contrib) {
  constexpr int WPB = KT == 16 ? 4 : 2;      // 32 KB of influences per block either way
  __shared__ int s_idx[WPB][kMaxH];
  __shared__ float s_w[WPB][kMaxH][KT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * WPB + wave;
  if (qi >= nq) return;
  const int cnt = deform_index_stage_nk<true, KT, INF, CLOSEST>(q_pts, s_pts, nbr, H, dkp + (int64_t)qi * n_kp * 3, n_kp, extent,
                                                                rowsum, qi, ns, lane, s_idx[wave], nullptr, s_w[wave], nullptr);
  const float inv_num = 1.f / (float)max(cnt, 1);
  for (int c0 = 0; c0 < cin; c0 += 64 * CPL) {
    float g[CPL][KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const float f = (mod && k < n_kp) ? mod[(int64_t)qi * n_kp + k] * inv_num : inv_num;
#pragma unroll
      for (int u = 0; u < CPL; ++u) {
        const int c = c0 + lane + 64 * u;
        g[u][k] = (c < cin && k < n_kp) ? dwf[(int64_t)qi * lddwf + (int64_t)k * cin + c] * f : 0.f;
      }
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

// Geometry gradient: k_kpconv_deform_dgeom with T tiles of kernel points.  P[h, k] = <x[nbr[q, h], :], dwf[q, k, :]> on the
// fp32 MFMA, rows = 16 neighbours of a tile, columns = the 16 kernel points of a k-tile, both operands straight from
// memory with the same channel map.  dwf[q, k] is the stationary B operand, one set per k-tile (k = r16 and 16 + r16; 16
// registers per set and 64-channel chunk, zero for k >= n_kp); the <= 8 neighbour tiles stream under them into T x 8
// accumulators, so every gathered row of x is still read once.  The accumulator of k-tile t leaves lane (r16, qd) with
// P[h = 16 nt + 4 qd + i][k = 16 t + r16]: the lane combines them with THAT kernel point's diff and w in ascending (nt, i),
// per k-tile, and the four qd groups meet by the same two shuffles: a fixed order.
template <int T, int INF, bool CLOSEST>
__global__ __launch_bounds__(256) void k_kpconv_deform_dgeom_nk(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ dwf, int64_t lddwf,
    const float* __restrict__ dkp, const float* __restrict__ mod, int n_kp, float extent, const float* __restrict__ rowsum,
    float* __restrict__ d_dkp, float* __restrict__ d_mod, int nq, int ns) {
  __shared__ int s_idx[4][kMaxH];
  __shared__ float s_diff[4][kMaxH][3];
  constexpr bool MODE = CLOSEST || INF != kpmode::kLinear;
  __shared__ unsigned char s_cl[MODE ? 4 : 1][MODE ? kMaxH : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qd = lane >> 4;
  const int qi = blockIdx.x * 4 + wave;
  if (qi >= nq) return;
  const float* kq = dkp + (int64_t)qi * n_kp * 3;
  const int cnt = deform_index_stage_nk<false, 16, INF, CLOSEST>(q_pts, s_pts, nbr, H, kq, n_kp, extent, rowsum, qi, ns, lane,
                                                                 s_idx[wave], s_diff[wave], nullptr, s_cl[MODE ? wave : 0]);
  const float inv_num = 1.f / (float)max(cnt, 1);
  bool kvalid[T];
#pragma unroll
  for (int t = 0; t < T; ++t) kvalid[t] = 16 * t + r16 < n_kp;
  const int ntile = (H + 15) >> 4;
  int arow[8];      // the x row of this lane's A operand per neighbour tile, -1: a zero row
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) arow[nt] = nt < ntile ? s_idx[wave][nt * 16 + r16] : -1;
  f32x4 acc[T][8];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) acc[t][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* brow[T];
#pragma unroll
  for (int t = 0; t < T; ++t) brow[t] = dwf + (int64_t)qi * lddwf + (int64_t)(kvalid[t] ? 16 * t + r16 : 0) * cin + 16 * qd;
  for (int c0 = 0; c0 < cin; c0 += 64) {
    f32x4 b[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        b[t][j] = kvalid[t] ? *reinterpret_cast<const f32x4*>(brow[t] + c0 + 4 * j) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      if (nt < ntile) {      // wave-uniform
        f32x4 a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          a[j] = arow[nt] >= 0 ? *reinterpret_cast<const f32x4*>(x + (int64_t)arow[nt] * ldx + c0 + 16 * qd + 4 * j)
                               : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[t][j][e], acc[t][nt], 0, 0, 0);
      }
    }
  }
  const float inv_extent = 1.f / extent;
  [[maybe_unused]] const float gden = INF == kpmode::kGaussian ? kpmode::gauss_den(extent) : 0.f;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int kown = 16 * t + r16;
    const float kx = kvalid[t] ? kq[3 * kown] : 0.f, ky = kvalid[t] ? kq[3 * kown + 1] : 0.f,
                kz = kvalid[t] ? kq[3 * kown + 2] : 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f, gm = 0.f;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      if (nt < ntile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int h = nt * 16 + 4 * qd + i;
          if (s_idx[wave][h] >= 0) {      // real (slots behind H hold -1)
            const float ex = s_diff[wave][h][0] - kx, ey = s_diff[wave][h][1] - ky, ez = s_diff[wave][h][2] - kz;
            if constexpr (INF == kpmode::kLinear) {
              const float d = sqrtf(ex * ex + ey * ey + ez * ez);
              const float w = 1.f - d * inv_extent;
              bool live = w > 0.f;
              if constexpr (CLOSEST) live = live && (int)(s_cl[wave][h] & 31) == kown;
              if (live) {
                const float p = acc[t][nt][i];
                gm = fmaf(w, p, gm);
                if (d > 0.f) {      // a neighbour exactly on the kernel point: no contribution (kpconv_deform.hip's rule)
                  const float f = p / (d * extent);
                  gx = fmaf(ex, f, gx); gy = fmaf(ey, f, gy); gz = fmaf(ez, f, gz);
                }
              }
            } else {
              const int cl = s_cl[wave][h];
              bool live = (cl & kpmode::kInRange) != 0;
              if constexpr (CLOSEST) live = live && (cl & 31) == kown;
              if (live) {
                const float p = acc[t][nt][i];
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
    if (qd == 0 && kvalid[t]) {
      const float f = mod ? mod[(int64_t)qi * n_kp + kown] * inv_num : inv_num;
      float* o = d_dkp + ((int64_t)qi * n_kp + kown) * 3;
      o[0] = gx * f; o[1] = gy * f; o[2] = gz * f;
      d_mod[(int64_t)qi * n_kp + kown] = gm * inv_num;
    }
  }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#define APR_DEFORM_NK_SHAPE(fn)                                                                                          \
  APR_CHECK_ARG(n_kp >= 1 && n_kp <= kMaxKP, fn ": 1 <= n_kp <= %d, got %d", kMaxKP, n_kp);                              \
  APR_CHECK_ARG(kpmode::valid(influence, closest), fn ": influence must be 0, 1 or 2 and closest 0 or 1, got %d, %d",    \
                influence, closest);                                                                                     \
  APR_CHECK_ARG(nq >= 0 && nq <= INT32_MAX - 4 && ns > 0 && ns < (1 << 30) && H >= 1 && H <= kMaxH && cin >= 64 &&       \
                    cin <= 512 && cin % 64 == 0 && extent > 0.f,                                                         \
                fn ": needs cin %% 64 == 0, 64 <= cin <= 512, 1 <= H <= %d, ns > 0, extent > 0", kMaxH);                 \
  APR_CHECK_ARG(q_pts && s_pts && nbr && dkp && rowsum, fn ": null argument")

template <int INF, bool CLOSEST>
int deform_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                       const float* x, int64_t ldx, int32_t cin, const float* dkp, const float* mod, int32_t n_kp, float extent,
                       const float* rowsum, float* wf, int64_t ldwf, float* min_d2, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)cdiv64(nq, 4);
  const int s_xcd = kpconv_xcd();
#define APR_DW(T, NG)                                                                                                        \
  hipLaunchKernelGGL((k_kpconv_deform_weighted_nk<T, NG, INF, CLOSEST>), dim3(grid), dim3(256), 0, st, q_pts, s_pts, nbr, H, x, \
                     ldx, cin, dkp, mod, n_kp, extent, rowsum, wf, ldwf, min_d2, (int)nq, (int)ns, s_xcd)
  if (n_kp <= 16) {      // the channel groups per pass of apr_kpconv_deform_weighted_mode
    if (cin >= 256) APR_DW(1, 4);
    else if (cin == 128) APR_DW(1, 2);
    else APR_DW(1, 1);
  } else {               // two tiles: half the groups per pass, the same accumulator registers
    if (cin >= 128) APR_DW(2, 2);
    else APR_DW(2, 1);
  }
#undef APR_DW
  APR_LAUNCH_CHECK();
  return APR_OK;
}

template <int INF, bool CLOSEST>
int deform_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                            const float* dwf, int64_t lddwf, int32_t cin, const float* dkp, const float* mod, int32_t n_kp,
                            float extent, const float* rowsum, float* contrib, void* stream) {
  hipStream_t st = (hipStream_t)stream;
#define APR_DF(N, KT)                                                                                                         \
  hipLaunchKernelGGL((k_kpconv_deform_dfeat_nk<N, KT, INF, CLOSEST>), dim3((unsigned)cdiv64(nq, KT == 16 ? 4 : 2)),            \
                     dim3(KT == 16 ? 256 : 128), 0, st, q_pts, s_pts, nbr, H, dwf, lddwf, cin, dkp, mod, n_kp, extent, rowsum, \
                     (int)nq, (int)ns, contrib)
  if (n_kp <= 16) {        // one pass, the registers of k_kpconv_deform_dfeat
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

template <int INF, bool CLOSEST>
int deform_dgeom_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                    const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf, const float* dkp, const float* mod,
                    int32_t n_kp, float extent, const float* rowsum, float* d_dkp, float* d_mod, void* stream) {
  hipStream_t st = (hipStream_t)stream;
#define APR_DG(T)                                                                                                            \
  hipLaunchKernelGGL((k_kpconv_deform_dgeom_nk<T, INF, CLOSEST>), dim3((unsigned)cdiv64(nq, 4)), dim3(256), 0, st, q_pts, s_pts, \
                     nbr, H, x, ldx, cin, dwf, lddwf, dkp, mod, n_kp, extent, rowsum, d_dkp, d_mod, (int)nq, (int)ns)
  if (n_kp <= 16) APR_DG(1);
  else APR_DG(2);
#undef APR_DG
  APR_LAUNCH_CHECK();
  return APR_OK;
}

}  // namespace

// apr_kpconv_deform_weighted_mode for 1 <= n_kp <= 32 kernel points: dkp f32 [nq, n_kp, 3], mod f32 [nq, n_kp] or null,
// wf[q, k * cin + c] for k < n_kp, min_d2 f32 [nq, n_kp] or null.
APR_API int apr_kpconv_deform_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                          int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dkp,
                                          const float* mod, int32_t n_kp, float extent, const float* rowsum, float* wf,
                                          int64_t ldwf, float* min_d2, int32_t influence, int32_t closest, void* stream) {
  APR_DEFORM_NK_SHAPE("apr_kpconv_deform_weighted_nk");
  APR_CHECK_ARG(x && wf && ldx >= cin && ldwf >= (int64_t)n_kp * cin && ldx % 4 == 0 && ldwf % 4 == 0 && aligned16(x) &&
                    aligned16(wf),
                "apr_kpconv_deform_weighted_nk: x / wf rows must be 16-byte aligned and at least cin / n_kp cin wide");
  if (nq == 0) return APR_OK;
  APR_KP_MODE_DISPATCH(deform_weighted_nk, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dkp, mod, n_kp, extent, rowsum, wf, ldwf,
                       min_d2, stream)
}

// apr_kpconv_deform_dfeat_contrib_mode for 1 <= n_kp <= 32: rows (q, h) of contrib f32 [nq * H, cin], the rows of padding
// neighbours untouched; apr_reverse_gather sums them.
APR_API int apr_kpconv_deform_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns,
                                               const int32_t* nbr, int32_t H, const float* dwf, int64_t lddwf, int32_t cin,
                                               const float* dkp, const float* mod, int32_t n_kp, float extent,
                                               const float* rowsum, float* contrib, int32_t influence, int32_t closest,
                                               void* stream) {
  APR_DEFORM_NK_SHAPE("apr_kpconv_deform_dfeat_contrib_nk");
  APR_CHECK_ARG(dwf && contrib && lddwf >= (int64_t)n_kp * cin,
                "apr_kpconv_deform_dfeat_contrib_nk: null buffer or leading dimension too small");
  if (nq == 0) return APR_OK;
  APR_KP_MODE_DISPATCH(deform_dfeat_contrib_nk, q_pts, nq, s_pts, ns, nbr, H, dwf, lddwf, cin, dkp, mod, n_kp, extent, rowsum,
                       contrib, stream)
}

// apr_kpconv_deform_dgeom_mode for 1 <= n_kp <= 32: d_dkp f32 [nq, n_kp, 3], d_mod f32 [nq, n_kp].
APR_API int apr_kpconv_deform_dgeom_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                       int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf,
                                       const float* dkp, const float* mod, int32_t n_kp, float extent, const float* rowsum,
                                       float* d_dkp, float* d_mod, int32_t influence, int32_t closest, void* stream) {
  APR_DEFORM_NK_SHAPE("apr_kpconv_deform_dgeom_nk");
  APR_CHECK_ARG(x && dwf && d_dkp && d_mod && ldx >= cin && lddwf >= (int64_t)n_kp * cin && ldx % 4 == 0 && lddwf % 4 == 0 &&
                    aligned16(x) && aligned16(dwf),
                "apr_kpconv_deform_dgeom_nk: x / dwf rows must be 16-byte aligned and at least cin / n_kp cin wide");
  if (nq == 0) return APR_OK;
  APR_KP_MODE_DISPATCH(deform_dgeom_nk, q_pts, nq, s_pts, ns, nbr, H, x, ldx, cin, dwf, lddwf, dkp, mod, n_kp, extent, rowsum,
                       d_dkp, d_mod, stream)
}

// Fused rigid KPConv forward: kernel-point correlation and [15 cin] x [15 cin, cout] contraction in ONE kernel.
//
//   out[q, :] = wf[q, :] @ W.reshape(15 cin, cout)
//   wf[q, k cin + c] = (1 / num[q]) * sum_h max(0, 1 - |s[nbr[q,h]] - q - kp[k]| / extent) * x[nbr[q,h], c]
//
// apr_kpconv_weighted + apr_dense_gemm_bf3 write wf [N, 15 cin] to HBM and read it back (42 .. 100 MB per layer on a KITTI
// pair).  Here the [queries, 15 cin] tile lives in LDS and registers only.  A workgroup (4 waves) owns 16 queries and ALL
// cout columns, and walks cin in 32-channel chunks -- one 32-deep step of the weight image per kernel point:
//   A. correlation, fp32 MFMA (the body of k_kpconv_weighted_mfma): a wave takes 4 queries side by side; per 4 neighbours
//      the influences are computed in registers (A operand: row = kernel point, k = neighbour), the neighbours' 32 channels
//      are gathered with one 8-B load per lane (B operand: column r16 of block cb = channel 2 r16 + cb, every gathered row
//      piece one 128-B line), four steps' loads in flight together; the accumulator -- kernel points in its rows, channels
//      on its lanes -- is scaled by 1 / num and written to the LDS tile [query][kernel point][32 channels] (8-B stores);
//   B. contraction, bf16 MFMA in the 3-way split of bf3.h: the tile is read back as an operand whose rows are QUERIES (lane
//      (query r16, quad q) -> 8 consecutive channels of one kernel point: two conflict-free ds_read_b128; the row stride of
//      484 words sends the 16 queries of a hardware lane group to 16 different 16-B slots), split in registers, and
//      multiplied with the weight fragments of the wave's OWN cout / 4 columns.  No two waves need the same fragment, so the
//      weights go straight from global memory into MFMA operand registers (lane (column r16, quad q) -> the 16-B piece of
//      apr_spconv_pack_weights_bf3's image: 1 KB contiguous per 16 columns), two (kernel point, column group) units ahead;
//      no LDS staging, no barrier for them.  The six cross terms in the order of k_dense_gemm_bf3, small terms first.
// The correlation of a query tile is computed once, whatever cout: the accumulators of all its columns (cout / 64 f32x4 per
// lane) stay in registers over the whole cin walk.  The neighbour geometry (difference vector + row index, 16 B per entry)
// is staged once per workgroup in dynamic LDS, sized by H.  A 32-query tile (half the weight traffic per query, 62 KB of
// LDS) measured 1.2 - 1.7x slower at every level of the KITTI pyramid and is not kept.
// No atomics, fixed summation order: the same bits on every run.
#include "kpconv.h"
#include "bf3.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kTileRow = kKP * 32 + 4;      // words per query of the LDS tile (+4: conflict-free operand reads)

template <int NC>   // NC = cout / 64 column groups of 16 per wave
__global__ __launch_bounds__(256) void k_kpconv_fused(
    const float* __restrict__ q_pts, const float* __restrict__ s_pts, const int* __restrict__ nbr, int H,
    const float* __restrict__ x, int64_t ldx, int cin, const float* __restrict__ kp, float extent,
    const float* __restrict__ rowsum, const unsigned char* __restrict__ wp3, float* __restrict__ out, int64_t ldo, int nq,
    int ns) {
  constexpr int QT = 16, NQW = QT / 4, U = 4;      // queries per workgroup / per wave; neighbour steps gathered together
  __shared__ __attribute__((aligned(16))) float s_t[QT * kTileRow];
  __shared__ float s_inv[QT];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];      // [QT][Hp] x {dx, dy, dz, row index}
  i32x4* s_g = reinterpret_cast<i32x4*>(s_dyn);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, qd = lane >> 4;
  const int Hp = (H + 15) & ~15;      // the list padded (index -1) to whole groups of U steps
  const int q0 = blockIdx.x * QT;

  // neighbour geometry of the wave's queries, once per workgroup; absent queries and padding entries: index -1
  // (kp_neighbour_stage's slot, in this kernel's own layout: one 16-B entry per slot, Hp slots, queries past nq staged too)
  for (int i = 0; i < NQW; ++i) {
    const int ql = wave * NQW + i, qi = q0 + ql;
    const bool live = qi < nq;
    const int64_t qr = live ? qi : 0;
    const float qx = q_pts[3 * qr], qy = q_pts[3 * qr + 1], qz = q_pts[3 * qr + 2];
    int cnt = 0;
    for (int h = lane; h < Hp; h += 64) {
      int idx = -1;
      float dx = 1e6f, dy = 1e6f, dz = 1e6f;
      if (live && h < H) {
        idx = nbr[(int64_t)qi * H + h];
        if (idx >= 0 && idx < ns) {
          dx = s_pts[3 * (int64_t)idx] - qx;
          dy = s_pts[3 * (int64_t)idx + 1] - qy;
          dz = s_pts[3 * (int64_t)idx + 2] - qz;
          cnt += rowsum[idx] > 0.f ? 1 : 0;
        } else {
          idx = -1;
        }
      }
      s_g[ql * Hp + h] = (i32x4){__float_as_int(dx), __float_as_int(dy), __float_as_int(dz), idx};
    }
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) s_inv[ql] = 1.f / (float)max(cnt, 1);
  }
  __syncthreads();

  const float inv_extent = 1.f / extent;
  const bool kvalid = r16 < kKP;
  const float kx = kvalid ? kp[3 * r16] : 0.f, ky = kvalid ? kp[3 * r16 + 1] : 0.f, kz = kvalid ? kp[3 * r16 + 2] : 0.f;
  const int nsteps = Hp >> 2;
  float inv_num[NQW];
#pragma unroll
  for (int i = 0; i < NQW; ++i) inv_num[i] = s_inv[wave * NQW + i];

  // weight fragments of this lane: column (wave NC + j) 16 + r16, 16-B piece q (q ^ 3 in the columns with bit 3 set); the
  // column group's part of the address is wave-uniform
  const int64_t plane_bytes = (int64_t)((kKP * cin) >> 5) * 4096;
  const unsigned char* wlane = wp3 + r16 * 64 + (((r16 & 8) ? (qd ^ 3) : qd) << 4);

  f32x4 acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < cin; c0 += 32) {
    // ---- A. correlation of the wave's NQW queries over channels c0 .. c0 + 31
    {
      f32x4 ca[NQW][2];
#pragma unroll
      for (int i = 0; i < NQW; ++i) ca[i][0] = ca[i][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* xc = x + c0 + 2 * r16;
      // U steps of 4 neighbours at a time: the U * NQW row pieces are all in flight before the first MFMA needs one (one
      // step at a time is a chain of LDS read -> gather -> MFMA per step: a full memory latency each)
      for (int st = 0; st < nsteps; st += U) {
        i32x4 gm[U][NQW];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < NQW; ++i) gm[u][i] = s_g[(wave * NQW + i) * Hp + (st + u) * 4 + qd];
        f32x2 b[U][NQW];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < NQW; ++i) {
            b[u][i] = (f32x2){0.f, 0.f};
            if (gm[u][i][3] >= 0) b[u][i] = *reinterpret_cast<const f32x2*>(xc + (int64_t)gm[u][i][3] * ldx);
          }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int i = 0; i < NQW; ++i) {
            float w = 0.f;
            if (kvalid && gm[u][i][3] >= 0)
              w = kpmode::influence<kpmode::kLinear>(
                  kp_d2(__int_as_float(gm[u][i][0]), __int_as_float(gm[u][i][1]), __int_as_float(gm[u][i][2]), kx, ky, kz),
                  inv_extent, 0.f);
            ca[i][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[u][i][0], ca[i][0], 0, 0, 0);
            ca[i][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w, b[u][i][1], ca[i][1], 0, 0, 0);
          }
      }
      // D[kernel point 4 qd + e][column r16 of block cb] <-> channel c0 + 2 r16 + cb
#pragma unroll
      for (int i = 0; i < NQW; ++i) {
        float* trow = s_t + (wave * NQW + i) * kTileRow + 2 * r16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = qd * 4 + e;
          if (k < kKP)
            *reinterpret_cast<f32x2*>(trow + k * 32) = (f32x2){ca[i][0][e] * inv_num[i], ca[i][1][e] * inv_num[i]};
        }
      }
    }
    __syncthreads();

    // ---- B. contraction of the tile with the 15 weight steps of this chunk
    {
      const int64_t wchunk = (int64_t)(c0 >> 5) * 4096;          // step of (kernel point k, chunk c0): k * (cin / 32) + c0 / 32
      const int64_t wkstep = (int64_t)(cin >> 5) * 4096;
      bf16x8 wf[3][3];
      auto load_w = [&](int k, int j, bf16x8* dst) {
        const int cg = wave * NC + j;      // 16-column group: 64-column block cg / 4, 1 KB per group inside a step
        const unsigned char* p = wlane + (int64_t)(cg >> 2) * 3 * plane_bytes + (cg & 3) * 1024 + wchunk + (int64_t)k * wkstep;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) dst[pl] = *reinterpret_cast<const bf16x8*>(p + pl * plane_bytes);
      };
      load_w(0, 0, wf[0]);
      load_w(NC > 1 ? 0 : 1, NC > 1 ? 1 : 0, wf[1]);
      const float* arow = s_t + r16 * kTileRow + qd * 8;
      for (int k3 = 0; k3 < kKP; k3 += 3) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
          const int k = k3 + kk;
          bf16x8 ah, am, al;
          apr_split3(*reinterpret_cast<const f32x4*>(arow + k * 32), *reinterpret_cast<const f32x4*>(arow + k * 32 + 4), ah, am, al);
#pragma unroll
          for (int j = 0; j < NC; ++j) {
            const int it = kk * NC + j, nx = it + 2;             // unit `it` of this block of three; its successor's successor
            const int kn = k3 + nx / NC, jn = nx % NC;
            if (kn < kKP) load_w(kn, jn, wf[nx % 3]);
            const bf16x8 wh = wf[it % 3][0], wm = wf[it % 3][1], wl = wf[it % 3][2];
            f32x4 t = acc[j];
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl, ah, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, al, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, am, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wm, ah, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, am, t, 0, 0, 0);
            t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh, ah, t, 0, 0, 0);
            acc[j] = t;
          }
        }
      }
    }
    __syncthreads();      // the tile is free for the next chunk
  }

  // lane (query r16, quad q) holds columns (wave NC + j) 16 + 4 q .. + 3 of its row
  const int qi = q0 + r16;
  if (qi >= nq) return;
#pragma unroll
  for (int j = 0; j < NC; ++j) *reinterpret_cast<f32x4*>(out + (int64_t)qi * ldo + (wave * NC + j) * 16 + qd * 4) = acc[j];
}

typedef void (*FusedKernel)(const float*, const float*, const int*, int, const float*, int64_t, int, const float*, float,
                            const float*, const unsigned char*, float*, int64_t, int, int);

FusedKernel fused_kernel(int nc) {
  switch (nc) {
    case 1: return k_kpconv_fused<1>;
    case 2: return k_kpconv_fused<2>;
    case 3: return k_kpconv_fused<3>;
    case 4: return k_kpconv_fused<4>;
    case 5: return k_kpconv_fused<5>;
    case 6: return k_kpconv_fused<6>;
    case 7: return k_kpconv_fused<7>;
    default: return k_kpconv_fused<8>;
  }
}

}  // namespace

APR_API int32_t apr_kpconv_fused_ok(int32_t cin, int32_t cout, int32_t H) {
  return cin >= 64 && cin <= 512 && cin % 64 == 0 && cout >= 64 && cout <= 512 && cout % 64 == 0 && H >= 1 && H <= kMaxH;
}

// 1 where the fused kernel measured faster than apr_kpconv_weighted + apr_dense_gemm_bf3 by more than the spread of the
// alternated medians (scripts/kpconv_fused_bench.py)
APR_API int32_t apr_kpconv_fused_route(int64_t nq, int32_t cin, int32_t cout, int32_t H) {
  if (nq <= 0 || !apr_kpconv_fused_ok(cin, cout, H)) return 0;
  return 0;
}

APR_API int apr_kpconv_fused(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                             const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp, float extent,
                             const float* rowsum, const void* w_bf3, int32_t cout, float* out, int64_t ldo, void* stream) {
  APR_CHECK_ARG(n_kp == kKP, "apr_kpconv_fused: built for %d kernel points, got %d", kKP, n_kp);
  APR_CHECK_ARG(apr_kpconv_fused_ok(cin, cout, H),
                "apr_kpconv_fused: needs cin and cout multiples of 64 in 64 .. 512 and 1 <= H <= %d (cin %d, cout %d, H %d)", kMaxH,
                cin, cout, H);
  APR_CHECK_ARG(nq >= 0 && nq < (1ll << 31) - 64 && ns > 0 && ns < (1ll << 31) && extent > 0.f, "apr_kpconv_fused: bad arguments");
  APR_CHECK_ARG(ldx >= cin && ldo >= cout, "apr_kpconv_fused: leading dimension too small");
  APR_CHECK_ARG(ldx % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)x | (uintptr_t)out | (uintptr_t)w_bf3) & 15) == 0,
                "apr_kpconv_fused: rows of x / out and the weight image must be 16-byte aligned");
  if (nq == 0) return APR_OK;
  APR_CHECK_ARG(q_pts && s_pts && nbr && x && kernel_points && rowsum && w_bf3 && out, "apr_kpconv_fused: null argument");
  // static tile 31 KB + geometry <= 32 KB: inside the 64 KB a kernel gets without opting in
  const int Hp = (H + 15) & ~15;
  hipLaunchKernelGGL(fused_kernel(cout / 64), dim3((unsigned)cdiv64(nq, 16)), dim3(256), (size_t)16 * Hp * 16, (hipStream_t)stream,
                     q_pts, s_pts, nbr, H, x, ldx, cin, kernel_points, extent, rowsum, (const unsigned char*)w_bf3, out, ldo, (int)nq,
                     (int)ns);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

// Sparse convolution forward for 32 < K <= 125 with real channel counts (cin, cout multiples of 32) on gfx950: the
// symmetric recipe's generator conv1 (FCGF_APR/lib/complement_trainer.py:52-60: ResUNetFatBN(128, 12, conv1_kernel_size=5),
// a 5^3 kernel over 128 -> 32 channels) and its input gradient (32 -> 128 over the mirrored offsets).
//
//   out[j,:] = act((sum_o in[nbr[j,o],:] @ W[o]) * scale + shift + residual[j,:])
//
// The pair-compacted, wave-autonomous form of k_spconv_pairs (spconv.hip) carried to 125 offsets:
//   * a workgroup owns 64 output rows x 32 output channels; its slice of the neighbour table (64 x K ints, 32 KB at
//     K = 125) is staged coalesced in the accumulator region, then every offset's (input row, local output row) pairs are
//     compacted by ballot + popcount into LDS lists, and the active offsets are listed in two 64-lane ballot rounds;
//   * work item = (active offset, 32-wide cin chunk), dealt statically to the 4 waves; a wave walks the item's pairs in
//     groups of 16: exact fp32 v_mfma_f32_16x16x4_f32, D^T = W^T . A^T, so a lane ends up with 4 consecutive output
//     channels of one pair and adds them into the wave's PRIVATE accumulator tile in LDS (rows of a group are distinct:
//     no atomics);
//   * weights are read in the plain [K, cin, cout] layout that apr_spconv_pack_weights leaves for K > 32 (and, for the
//     input gradient, that apr_weights_flip_transpose leaves): a B fragment is rows along cout, 16 lanes x 4 B = 64 B
//     contiguous per cin row, straight from L2 (125 x 128 x 32 floats = 2 MB, shared by every tile);
//   * one barrier, then the epilogue sums the 4 private tiles in fixed order and applies scale / shift / residual / ReLU
//     with 16-B row stores.  Static item deal + in-order LDS adds per wave: bit-identical run to run, no global atomics.
// LDS: 4 x 64 x 36 floats of accumulators (36,864 B) + 125 x 64 input rows (32,000 B) + 125 x 64 local rows (8,000 B)
// + 2 x 128 ints of counts / active offsets = 77,892 B: two workgroups per CU.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBigKMax = 125;

template <int TM, int CN, int CK, int NW>
__global__ __launch_bounds__(64 * NW, 2) void k_spconv_bigk(
    const float* __restrict__ in, int64_t ldi, const int* __restrict__ nbr, int n_out, int K, int cin, int cout,
    const float* __restrict__ w, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ residual, int64_t ldr, int relu, float* __restrict__ out, int64_t ldo) {
  constexpr int CB = CN / 16;   // 16-col blocks per wave item
  constexpr int NJ = CK / 16;   // 16-wide cin groups per chunk
  constexpr int LDO = CN + 4;   // accumulator row stride (floats), 16-B aligned rows
  constexpr int NT = 64 * NW;
  static_assert(TM * kBigKMax <= NW * TM * LDO, "nbr staging must fit in the accumulator region");
  static_assert(TM <= 256 && TM % 64 == 0, "local rows are bytes; the compaction walks 64 rows per ballot");

  __shared__ __attribute__((aligned(16))) float s_acc[NW * TM * LDO];
  __shared__ int s_in[kBigKMax * TM];
  __shared__ __attribute__((aligned(4))) unsigned char s_row[kBigKMax * TM];
  __shared__ int s_cnt[128];
  __shared__ int s_act[128];
  __shared__ int s_nact;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;

  // blocks that share an XCD (b % 8) get a contiguous range of tiles (overlapping gathers hit the same L2)
  const int nb = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, loc = bid >> 3;
  const int lin = xcd * (nb >> 3) + min(xcd, nb & 7) + loc;
  const int ncol = cout / CN;
  const int tile_m = lin / ncol, tile_n = lin - tile_m * ncol;
  const int row0 = tile_m * TM;
  const int col0 = tile_n * CN;

  // 1. stage this tile's slice of the neighbour table (coalesced) in the accumulator region
  int* s_stage = reinterpret_cast<int*>(s_acc);
  for (int t = tid; t < TM * K; t += NT) {
    const int r = t / K;
    int v = -1;
    if (row0 + r < n_out) v = nbr[(int64_t)row0 * K + t];
    s_stage[t] = v;
  }
  __syncthreads();
  // 2. per-offset compaction of (input row, local output row) pairs: ballot + popcount
  for (int k = wave; k < K; k += NW) {
    int cnt = 0;
#pragma unroll
    for (int base = 0; base < TM; base += 64) {
      const int r = base + lane;
      const int v = s_stage[r * K + k];
      const unsigned long long m = __ballot(v >= 0);
      if (v >= 0) {
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        s_in[k * TM + pos] = v;
        s_row[k * TM + pos] = (unsigned char)r;
      }
      cnt += __popcll(m);
    }
    if (lane == 0) s_cnt[k] = cnt;
  }
  __syncthreads();
  // 3. active offset list, ascending, in two 64-lane rounds (wave 0) + zero the accumulators (everyone)
  if (wave == 0) {
    int n = 0;
#pragma unroll
    for (int base = 0; base < 128; base += 64) {
      const int k = base + lane;
      const int c = (k < K) ? s_cnt[k] : 0;
      const unsigned long long m = __ballot(c > 0);
      if (c > 0) s_act[n + __popcll(m & ((1ull << lane) - 1ull))] = k;
      n += __popcll(m);
    }
    if (lane == 0) s_nact = n;
  }
  for (int t = tid; t < NW * TM * LDO / 4; t += NT)
    reinterpret_cast<f32x4*>(s_acc)[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  const int nact = s_nact;
  const int nchunk = cin / CK;
  float* my_acc = s_acc + wave * TM * LDO;

  // 4. wave-autonomous main loop, no barriers: a step = (item, 16-pair group); every step issues the loads of the NEXT step
  //    into the other register buffer before its own MFMAs (unrolled by two so the buffers swap by name).
  const int nitems = nact * nchunk;
  struct Desc { int item, g0, k, chunk, cnt; };
  auto decode = [&](Desc& d) {
    const int ai = d.item / nchunk;
    d.chunk = d.item - ai * nchunk;
    d.k = __builtin_amdgcn_readfirstlane(s_act[ai]);
    d.cnt = __builtin_amdgcn_readfirstlane(s_cnt[d.k]);
  };
  // false when there is no further step (d is left unchanged so the dummy loads stay valid)
  auto advance = [&](Desc& d) -> bool {
    if (d.g0 + 16 < d.cnt) {
      d.g0 += 16;
      return true;
    }
    if (d.item + NW >= nitems) return false;
    d.item += NW;
    d.g0 = 0;
    decode(d);
    return true;
  };
  // MFMA k index (j, t) of lane group q is cin channel 16 j + 4 q + t on both operands
  const int lane_w_off = q * 4 * cout + r16;             // floats, lane-constant
  auto load = [&](const Desc& d, float (&bw)[CB][NJ][4], f32x4 (&aw)[NJ]) {
    const float* wb = w + ((int64_t)d.k * cin + d.chunk * CK) * cout + col0 + lane_w_off;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) bw[cb][j][t] = wb[(int64_t)(j * 16 + t) * cout + cb * 16];
    // padded pairs (p >= cnt) gather pair 0's row: their columns of D^T are never written back
    const int p = d.g0 + r16;
    const int idx = s_in[d.k * TM + (p < d.cnt ? p : 0)];
    const float* ab = in + (int64_t)idx * ldi + (d.chunk * CK + q * 4);
#pragma unroll
    for (int j = 0; j < NJ; ++j) aw[j] = *reinterpret_cast<const f32x4*>(ab + j * 16);
  };
  auto compute = [&](const Desc& d, const float (&bw)[CB][NJ][4], const f32x4 (&aw)[NJ]) {
    f32x4 acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[cb][j][t], aw[j][t], acc[cb], 0, 0, 0);
    if (d.g0 + r16 < d.cnt) {
      float* dst = my_acc + (int)s_row[d.k * TM + d.g0 + r16] * LDO + q * 4;
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        f32x4* d4 = reinterpret_cast<f32x4*>(dst + cb * 16);
        *d4 = *d4 + acc[cb];
      }
    }
  };

  if (wave < nitems) {
    float b0[CB][NJ][4], b1[CB][NJ][4];
    f32x4 a0[NJ], a1[NJ];
    Desc d0;
    d0.item = wave;
    d0.g0 = 0;
    decode(d0);
    load(d0, b0, a0);
    while (true) {
      Desc d1 = d0;
      const bool more1 = advance(d1);
      load(d1, b1, a1);          // prefetch (a harmless re-load of d0 when there is no next step)
      compute(d0, b0, a0);
      if (!more1) break;
      d0 = d1;
      const bool more0 = advance(d0);
      load(d0, b0, a0);
      compute(d1, b1, a1);
      if (!more0) break;
    }
  }
  __syncthreads();

  // 5. epilogue: fixed-order sum of the private tiles, fused affine / residual / ReLU, 16-B row stores
  for (int e = tid; e < TM * (CN / 4); e += NT) {
    const int r = e / (CN / 4), c4 = e - r * (CN / 4);
    const int row = row0 + r;
    if (row >= n_out) continue;
    const int col = col0 + c4 * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(&s_acc[(0 * TM + r) * LDO + c4 * 4]);
#pragma unroll
    for (int wv = 1; wv < NW; ++wv) v += *reinterpret_cast<const f32x4*>(&s_acc[(wv * TM + r) * LDO + c4 * 4]);
    if (scale) v *= *reinterpret_cast<const f32x4*>(scale + col);
    if (shift) v += *reinterpret_cast<const f32x4*>(shift + col);
    if (residual) v += *reinterpret_cast<const f32x4*>(residual + (int64_t)row * ldr + col);
    if (relu) {
      v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
    }
    *reinterpret_cast<f32x4*>(out + (int64_t)row * ldo + col) = v;
  }
}

}  // namespace

APR_API int32_t apr_spconv_bigk_supported(int32_t K, int32_t cin, int32_t cout) {
  return (K > 32 && K <= kBigKMax && cin >= 32 && cin % 32 == 0 && cout >= 32 && cout % 32 == 0) ? 1 : 0;
}

bool apr_internal_spconv_bigk_aligned(const apr_spconv_desc& d) {
  return d.nbr != nullptr && d.ldi % 4 == 0 && d.ldo % 4 == 0 &&
         ((((uintptr_t)d.in) | ((uintptr_t)d.out) | ((uintptr_t)d.scale) | ((uintptr_t)d.shift)) & 15) == 0 &&
         (!d.residual || (d.ldr % 4 == 0 && (((uintptr_t)d.residual) & 15) == 0));
}

int apr_internal_spconv_bigk(const apr_spconv_desc& d, hipStream_t st) {
  APR_CHECK_ARG(apr_spconv_bigk_supported(d.K, d.cin, d.cout) && apr_internal_spconv_bigk_aligned(d) && d.n_out > 0 &&
                    d.n_out < (1ll << 31),
                "spconv_bigk: needs 32 < K <= 125, cin and cout multiples of 32, a kernel map and 16-byte aligned rows");
  const int64_t tiles = cdiv64(d.n_out, 64) * (d.cout / 32);
  APR_CHECK_ARG(tiles < (1ll << 31), "spconv_bigk: %lld tiles", (long long)tiles);
  hipLaunchKernelGGL((k_spconv_bigk<64, 32, 32, 4>), dim3((unsigned)tiles), dim3(256), 0, st, d.in, d.ldi, d.nbr, (int)d.n_out,
                     d.K, d.cin, d.cout, d.w_packed, d.scale, d.shift, d.residual, d.ldr, d.relu, d.out, d.ldo);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

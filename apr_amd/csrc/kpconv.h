// What the KPConv translation units (kpconv.hip, kpconv_deform.hip, kpconv_fused.hip) share, so that every kernel of a
// layer -- forward, feature gradient, geometry gradient -- decides the influences, the closest kernel point and the
// neighbour count with the same float32 expressions (Predator_APR/models/blocks.py:61-68, 320-345).
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kKP = 15;
constexpr int kMaxH = 128;

// A/B switch of the XCD-aware query order, read once for every kernel that takes it
inline int kpconv_xcd() {
  static const int s_xcd = env_int("APR_KPCONV_XCD", 1);
  return s_xcd;
}

// The block a workgroup works as: with xcd_swz consecutive queries (they share neighbours) sit behind ONE XCD's L2
__device__ inline int kp_xcd_block(int xcd_swz) {
  int blk = blockIdx.x;
  if (xcd_swz) {
    const int nb = gridDim.x, xcd = blk & 7, loc = blk >> 3;
    blk = xcd * (nb >> 3) + min(xcd, nb & 7) + loc;
  }
  return blk;
}

// |centred neighbour - kernel point|^2: the one statement behind every influence
__device__ inline float kp_d2(float dx, float dy, float dz, float kx, float ky, float kz) {
  const float ex = dx - kx, ey = dy - ky, ez = dz - kz;
  return ex * ex + ey * ey + ez * ez;
}

namespace kpmode {

constexpr int kConstant = 0, kLinear = 1, kGaussian = 2;
constexpr int kInRange = 0x80;      // flag next to the closest index in a slot's mode byte

inline bool valid(int influence, int closest) { return influence >= 0 && influence <= 2 && (closest == 0 || closest == 1); }

// (influence, closest) -> the instantiation fn<INF, CLOSEST> of a host function; the caller has checked valid()
#define APR_KP_MODE_DISPATCH(fn, ...)                                                   \
  switch (influence * 2 + closest) {                                                    \
    case 0: return fn<kpmode::kConstant, false>(__VA_ARGS__);                           \
    case 1: return fn<kpmode::kConstant, true>(__VA_ARGS__);                            \
    case 2: return fn<kpmode::kLinear, false>(__VA_ARGS__);                             \
    case 3: return fn<kpmode::kLinear, true>(__VA_ARGS__);                              \
    case 4: return fn<kpmode::kGaussian, false>(__VA_ARGS__);                           \
    default: return fn<kpmode::kGaussian, true>(__VA_ARGS__);                           \
  }

// 2 sigma^2 + 1e-9 with sigma = 0.3 extent (blocks.py:61-68, 333): evaluated in double as the reference's Python scalars
// are, rounded once to the float32 that divides the float32 d2
__device__ inline float gauss_den(float extent) {
  const double sg = 0.3 * (double)extent;
  return (float)(2.0 * sg * sg + 1e-9);
}

template <int INF>
__device__ inline float influence(float d2, float inv_extent, float gden) {
  if constexpr (INF == kConstant) return 1.f;
  else if constexpr (INF == kLinear) return fmaxf(1.f - sqrtf(d2) * inv_extent, 0.f);
  else return expf(-d2 / gden);      // not clipped at the extent; expf, not a fast intrinsic: its error is bounded
}

// The kernel point closest to the centred neighbour (dx, dy, dz) among kpts[15][3], bits 0..3, and whether the neighbour
// lies inside some ball (d2 < ext2), bit 7.  The ONE statement of the argmin of blocks.py:341: d2 in a fixed evaluation
// order (no contraction left to the compiler), strict <, so the lowest index wins an exact tie as torch.argmin does.
__device__ inline int closest_kp(float dx, float dy, float dz, const float* __restrict__ kpts, float ext2) {
  int best = 0;
  float bd = __builtin_inff();
  bool inr = false;
#pragma unroll
  for (int k = 0; k < 15; ++k) {
    const float ex = dx - kpts[3 * k], ey = dy - kpts[3 * k + 1], ez = dz - kpts[3 * k + 2];
    const float d2 = __fmaf_rn(ez, ez, __fmaf_rn(ey, ey, ex * ex));
    if (d2 < bd) { bd = d2; best = k; }
    inr = inr || d2 < ext2;
  }
  return best | (inr ? kInRange : 0);
}

}  // namespace kpmode

// The neighbour stage of the rigid correlation kernels, one wave per query: lane h fills slots h and h + 64 with the
// support row (-1: padding or out of range -- a shadow neighbour: zero feature row, point at +1e6 => zero influence), the
// support point centred on the query and, with CLOSEST, the neighbour's closest kernel point; returns the wave's count of
// neighbours with a positive feature sum.
// (the wave's LDS writes are read back by other lanes of the same wave: in-order LDS queue, no barrier needed)
template <bool CLOSEST>
__device__ inline int kp_neighbour_stage(const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                         const int* __restrict__ nbr, int H, const float* __restrict__ kp,
                                         const float* __restrict__ rowsum, int qi, int ns, int lane, int* s_idx,
                                         float (*s_diff)[3], unsigned char* s_cl) {
  const float qx = q_pts[3 * (int64_t)qi], qy = q_pts[3 * (int64_t)qi + 1], qz = q_pts[3 * (int64_t)qi + 2];
  int cnt = 0;
  for (int h = lane; h < kMaxH; h += 64) {
    int idx = -1;
    float dx = 1e6f, dy = 1e6f, dz = 1e6f;
    if (h < H) {
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
    s_idx[h] = idx;
    s_diff[h][0] = dx; s_diff[h][1] = dy; s_diff[h][2] = dz;
    if constexpr (CLOSEST) s_cl[h] = idx >= 0 ? (unsigned char)kpmode::closest_kp(dx, dy, dz, kp, 0.f) : 0;
  }
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  return cnt;
}

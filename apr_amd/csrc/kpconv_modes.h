// KPConv influence functions and the closest kernel point (Predator_APR/models/blocks.py:61-68, 320-345), shared by
// kpconv.hip and kpconv_deform.hip so that every kernel of a layer -- forward, feature gradient, geometry gradient --
// decides them with the same float32 expressions.
#pragma once
#include <hip/hip_runtime.h>

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

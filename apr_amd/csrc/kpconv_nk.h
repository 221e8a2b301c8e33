// What the any-kernel-point-count translation units (kpconv_nk.hip: rigid; kpconv_deform_nk.hip: deformable) share.
#pragma once
#include "kpconv.h"

namespace {

constexpr int kMaxKP = 32;

// kpmode::closest_kp for n_kp kernel points: the same float32 statement (d2 in a fixed evaluation order, strict <, the
// lowest index wins an exact tie), the index in bits 0..4, the in-range flag in bit 7.  Forward and backward both call it.
__device__ inline int closest_kp_nk(float dx, float dy, float dz, const float* __restrict__ kpts, int n_kp, float ext2) {
  int best = 0;
  float bd = __builtin_inff();
  bool inr = false;
  for (int k = 0; k < n_kp; ++k) {
    const float ex = dx - kpts[3 * k], ey = dy - kpts[3 * k + 1], ez = dz - kpts[3 * k + 2];
    const float d2 = __fmaf_rn(ez, ez, __fmaf_rn(ey, ey, ex * ex));
    if (d2 < bd) { bd = d2; best = k; }
    inr = inr || d2 < ext2;
  }
  return best | (inr ? kpmode::kInRange : 0);
}

}  // namespace

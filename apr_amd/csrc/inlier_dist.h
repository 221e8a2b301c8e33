// The float32 point arithmetic of Predator_APR's get_inlier_ratio (lib/benchmark_utils.py:246, :252), shared by
// k_inlier_ratio (mutual.hip) and k_predator_test_pair (predator_valid.hip): the same bits in both.
#pragma once
#include "common.h"

namespace {

// benchmark_utils.py:246: (rot @ src.T + trans).T in float32, the products added left to right, every operation rounded
__device__ inline void transform_f32(const float* __restrict__ rot9, const float* __restrict__ trans3, const float* __restrict__ p,
                                     float q[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(rot9[3 * a], p[0]), __fmul_rn(rot9[3 * a + 1], p[1])),
                              __fmul_rn(rot9[3 * a + 2], p[2]));
    q[a] = __fadd_rn(s, trans3[a]);
  }
}

__device__ inline float dist_f32(const float q[3], const float* __restrict__ t) {
  const float dx = __fsub_rn(q[0], t[0]), dy = __fsub_rn(q[1], t[1]), dz = __fsub_rn(q[2], t[2]);
  return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

}  // namespace

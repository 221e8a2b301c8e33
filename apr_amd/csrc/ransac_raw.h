// The raw form of a RANSAC result on the device: the best hypothesis with `total_valid` behind it.  ransac.hip writes it
// (apr_ransac_pose_geometric_async leaves it in `raw_dev`, every batch result slot starts with it), apr_ransac_decode reads
// it on the host and k_predator_test_pair (predator_valid.hip) reads it on the device: one layout, one decoder.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

#include "common.h"

namespace {

struct Hyp {
  double T[12];  // row-major [R | t], 3x4
  long long it;
  int inliers;
  int pad;
  double err2;
};

constexpr size_t kRawBytes = sizeof(Hyp) + 8;      // Hyp, then long long total_valid

// the 20 doubles of a result (apr_ransac_pose's result_host): T 4x4 row-major, inliers, rmse, best iteration, total_valid
__host__ __device__ inline void raw_decode20(const Hyp& hb, long long tv, double* r) {
  for (int k = 0; k < 12; ++k) r[k] = hb.T[k];
  r[12] = 0.0; r[13] = 0.0; r[14] = 0.0; r[15] = 1.0;
  r[16] = (double)(hb.inliers < 0 ? 0 : hb.inliers);
  r[17] = hb.inliers > 0 ? sqrt(hb.err2 / (double)hb.inliers) : 0.0;
  r[18] = (double)hb.it;
  r[19] = (double)tv;
}

}  // namespace

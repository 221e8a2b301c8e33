// est_quad_linear_robust (FCGF_APR/util/transform_estimation.py:89-116) as device code for ONE 1024-thread workgroup:
// 20 IRLS iterations, `par` halved every 5, rot_z * rot_y * rot_x composition.  k_irls (ransac.hip) and k_valid_pair
// (valid.hip) both call irls_run, so the two give the same bits on the same correspondences.
#pragma once
#include "common.h"

__device__ inline void solve6(double M[6][7]) {
  // Gauss-Jordan with partial pivoting on the augmented 6x7 system (thread 0 only)
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double mx = fabs(M[c][c]);
    for (int r = c + 1; r < 6; ++r)
      if (fabs(M[r][c]) > mx) {
        mx = fabs(M[r][c]);
        piv = r;
      }
    if (piv != c)
      for (int k = 0; k < 7; ++k) {
        double tmp = M[c][k];
        M[c][k] = M[piv][k];
        M[piv][k] = tmp;
      }
    double inv = 1.0 / M[c][c];
    for (int k = 0; k < 7; ++k) M[c][k] *= inv;
    for (int r = 0; r < 6; ++r)
      if (r != c) {
        double f = M[r][c];
        for (int k = 0; k < 7; ++k) M[r][k] -= f * M[c][k];
      }
  }
}

// pts0 / pts1 f32[n,3] paired, weight0 f32[n] or NULL; cur f32[3n] and w f32[n] are global scratch.  Every thread of the
// 1024-thread workgroup calls it; on return (after a barrier) s_T[0..15] (shared memory of the caller) holds the
// row-major 4x4 transform.
__device__ inline void irls_run(const float* __restrict__ pts0, const float* __restrict__ pts1,
                                const float* __restrict__ weight0, int64_t n, float* __restrict__ cur,
                                float* __restrict__ w, float* s_T) {
  __shared__ double s_red[16][27];
  __shared__ double s_M[6][7];
  __shared__ float s_Tc[12];  // current step [R|t]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t i = tid; i < n; i += 1024) {
    cur[3 * i] = pts0[3 * i]; cur[3 * i + 1] = pts0[3 * i + 1]; cur[3 * i + 2] = pts0[3 * i + 2];
    w[i] = weight0 ? weight0[i] : 1.f;
  }
  if (tid < 16) s_T[tid] = (tid % 5 == 0) ? 1.f : 0.f;
  __syncthreads();
  float par = 1.0f;
  for (int iter = 0; iter < 20; ++iter) {
    if (iter > 0 && iter % 5 == 0) par *= 0.5f;
    // normal equations: rows a0=[0,z,-y,1,0,0], a1=[-z,0,x,0,1,0], a2=[y,-x,0,0,0,1], all scaled by w
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int64_t i = tid; i < n; i += 1024) {
      double x = cur[3 * i], y = cur[3 * i + 1], z = cur[3 * i + 2];
      double ww = (double)w[i] * (double)w[i];
      double bx = (double)pts1[3 * i] - x, by = (double)pts1[3 * i + 1] - y, bz = (double)pts1[3 * i + 2] - z;
      // AtA upper triangle (21) in row-major order, then Atb (6)
      acc[0] += ww * (z * z + y * y);  // 00
      acc[1] += ww * (-x * y);         // 01
      acc[2] += ww * (-x * z);         // 02
      acc[3] += 0.0;                   // 03
      acc[4] += ww * (-z);             // 04
      acc[5] += ww * (y);              // 05
      acc[6] += ww * (z * z + x * x);  // 11
      acc[7] += ww * (-y * z);         // 12
      acc[8] += ww * (z);              // 13
      acc[9] += 0.0;                   // 14
      acc[10] += ww * (-x);            // 15
      acc[11] += ww * (y * y + x * x); // 22
      acc[12] += ww * (-y);            // 23
      acc[13] += ww * (x);             // 24
      acc[14] += 0.0;                  // 25
      acc[15] += ww;                   // 33
      acc[16] += 0.0;                  // 34
      acc[17] += 0.0;                  // 35
      acc[18] += ww;                   // 44
      acc[19] += 0.0;                  // 45
      acc[20] += ww;                   // 55
      acc[21] += ww * (-z * by + y * bz);
      acc[22] += ww * (z * bx - x * bz);
      acc[23] += ww * (-y * bx + x * by);
      acc[24] += ww * bx;
      acc[25] += ww * by;
      acc[26] += ww * bz;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
      double v = acc[k];
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
      if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double tot[27];
      for (int k = 0; k < 27; ++k) {
        double v = 0.0;
        for (int wv = 0; wv < 16; ++wv) v += s_red[wv][k];
        tot[k] = v;
      }
      int p = 0;
      for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) {
          s_M[r][c] = tot[p];
          s_M[c][r] = tot[p];
          ++p;
        }
      for (int r = 0; r < 6; ++r) s_M[r][6] = tot[21 + r];
      double M[6][7];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 7; ++c) M[r][c] = s_M[r][c];
      solve6(M);
      float x0 = (float)M[0][6], x1 = (float)M[1][6], x2 = (float)M[2][6];
      float cx = cosf(x0), sx = sinf(x0), cy = cosf(x1), sy = sinf(x1), cz = cosf(x2), sz = sinf(x2);
      // R = rot_z(x2) rot_y(x1) rot_x(x0)
      float R[3][3];
      R[0][0] = cz * cy; R[0][1] = cz * sy * sx - sz * cx; R[0][2] = cz * sy * cx + sz * sx;
      R[1][0] = sz * cy; R[1][1] = sz * sy * sx + cz * cx; R[1][2] = sz * sy * cx - cz * sx;
      R[2][0] = -sy;     R[2][1] = cy * sx;                R[2][2] = cy * cx;
      for (int a = 0; a < 3; ++a) {
        s_Tc[a * 4 + 0] = R[a][0]; s_Tc[a * 4 + 1] = R[a][1]; s_Tc[a * 4 + 2] = R[a][2];
        s_Tc[a * 4 + 3] = (float)M[3 + a][6];
      }
      // trans = trans_curr @ trans
      float Tn[12];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) {
          float v = s_Tc[a * 4 + 0] * s_T[0 * 4 + b] + s_Tc[a * 4 + 1] * s_T[1 * 4 + b] + s_Tc[a * 4 + 2] * s_T[2 * 4 + b];
          if (b == 3) v += s_Tc[a * 4 + 3];
          Tn[a * 4 + b] = v;
        }
      for (int k = 0; k < 12; ++k) s_T[k] = Tn[k];
    }
    __syncthreads();
    for (int64_t i = tid; i < n; i += 1024) {
      float x = cur[3 * i], y = cur[3 * i + 1], z = cur[3 * i + 2];
      float nx = s_Tc[0] * x + s_Tc[1] * y + s_Tc[2] * z + s_Tc[3];
      float ny = s_Tc[4] * x + s_Tc[5] * y + s_Tc[6] * z + s_Tc[7];
      float nz = s_Tc[8] * x + s_Tc[9] * y + s_Tc[10] * z + s_Tc[11];
      cur[3 * i] = nx; cur[3 * i + 1] = ny; cur[3 * i + 2] = nz;
      float dx = nx - pts1[3 * i], dy = ny - pts1[3 * i + 1], dz = nz - pts1[3 * i + 2];
      w[i] = par / (sqrtf(dx * dx + dy * dy + dz * dz) + par);
    }
    __syncthreads();
  }
}

// Multiway registration (open3d's get_information_matrix_from_point_clouds + global_optimization with
// GlobalOptimizationLevenbergMarquardt), the default route to the poses of APR's aggregated point cloud:
//   FCGF_APR/lib/complement_data_loader.py:408-516 (pairwise_registration, full_registration, multiway_registration),
//   Predator_APR/datasets/kitti.py:197-297.
// open3d is not part of this build: both kernels implement the restatement of DESIGN section 19.
//
//   apr_information_batch : the evaluation step of apr_icp_batch (same grid, same packed rows, same arithmetic) once, at the
//                           transform handed in; ten fp64 sums over the matched TARGET rows, combined in k_icp_assoc's fixed
//                           order (xor butterfly per wave, (w0 + w1) + (w2 + w3), partial rows of a problem by one workgroup).
//   apr_posegraph_optimize: one workgroup per graph (<= 8 nodes, <= 28 edges), fp64, the damped 48 x 48 system in LDS.  A
//                           thread owns an entry of H / b and walks the edges in ascending order; every scalar decision of
//                           the LM loop is taken by thread 0 and read back by the workgroup.  No atomics.
#include <math.h>

#include "common.h"

namespace {

constexpr int kInfoMaxProblems = 64;   // = the segment limit of the batched search grid
constexpr int kInfoBlock = 256;
constexpr int kInfoSums = 10;          // n, x, y, z, xx, yy, zz, xy, xz, yz


struct InfoBatch {
  int nb;
  int blk0[kInfoMaxProblems + 1];   // first workgroup (= first row of partials) of every problem
  int a0[kInfoMaxProblems + 1];     // source rows
  int tseg[kInfoMaxProblems];       // target segment of every problem
  int b0[kInfoMaxProblems + 1];     // target rows of every SEGMENT
};

// the fp32 distance of apr_icp_batch's contract, every operation rounded: plain operators with contraction switched off for
// the body (the __f*_rn intrinsics are inlined from a header compiled with contraction on and fuse like any other
// expression)
__device__ inline float info_d2(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// one coordinate of T s: ((T0 x + T1 y) + T2 z) + T3 in fp64 with every operation rounded, then rounded to fp32 once
__device__ inline float info_move(const double* __restrict__ t, double x, double y, double z) {
#pragma clang fp contract(off)
  return (float)(((t[0] * x + t[1] * y) + t[2] * z) + t[3]);
}

// sum over the 256 threads in a fixed order: xor butterfly inside each wave, then (w0 + w1) + (w2 + w3)
__device__ inline void info_block_sums(double* v, double (*s_w)[kInfoSums]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) {
    double x = v[k];
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if (lane == 0) s_w[wave][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < kInfoSums) {
    const int k = threadIdx.x;
    v[0] = (s_w[0][k] + s_w[1][k]) + (s_w[2][k] + s_w[3][k]);
  }
}

__global__ __launch_bounds__(kInfoBlock) void k_info_assoc(const float* __restrict__ a, const float4* __restrict__ rows,
                                                           AprSearchGrid g, InfoBatch sg, float r2, const double* __restrict__ Tm,
                                                           int64_t t_stride, double* __restrict__ partial,
                                                           int* __restrict__ corr) {
  __shared__ double s_w[4][kInfoSums];
  int prob = 0;
  while (prob + 1 < sg.nb && (int)blockIdx.x >= sg.blk0[prob + 1]) ++prob;
  if (*g.status != 0) return;                                  // a flagged grid is never searched (k_icp_pack)
  const int seg = sg.tseg[prob];
  const int64_t i = (int64_t)sg.a0[prob] + (int64_t)((int)blockIdx.x - sg.blk0[prob]) * kInfoBlock + threadIdx.x;
  double v[kInfoSums];
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) v[k] = 0.0;
  if (i < sg.a0[prob + 1]) {
    const double* T = Tm + (size_t)prob * t_stride;
    const double sx = a[3 * i], sy = a[3 * i + 1], sz = a[3 * i + 2];
    float p[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = info_move(T + 4 * d, sx, sy, sz);
    int c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = (int)floorf((p[d] - g.mins[3 * seg + d]) / g.cell);   // sub, then IEEE division
    float bd = __builtin_inff();
    unsigned bj = 0xFFFFFFFFu;
    float4 bq = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int o = 0; o < 27; ++o) {
      const int X = c[0] + o % 3 - 1, Y = c[1] + (o / 3) % 3 - 1, Z = c[2] + o / 9 - 1;
      if (!apr_key_in_range(seg, X, Y, Z)) continue;
      const int id = apr_table_lookup(g.keys, g.vals, g.mask, apr_pack_key(seg, X, Y, Z));
      if (id < 0) continue;
      const int e1 = g.start[id + 1];
      for (int e = g.start[id]; e < e1; ++e) {
        const float4 q = rows[e];
        const float d2 = info_d2(p[0], p[1], p[2], q.x, q.y, q.z);
        const unsigned j = (unsigned)__float_as_int(q.w);
        if (d2 < bd || (d2 == bd && j < bj)) {
          bd = d2;
          bj = j;
          bq = q;
        }
      }
    }
    const bool hit = bd < r2;
    if (corr) corr[i] = hit ? (int)bj - sg.b0[seg] : -1;
    if (hit) {
      const double x = bq.x, y = bq.y, z = bq.z;              // the target's own coordinates, products in fp64
      v[0] = 1.0;
      v[1] = x; v[2] = y; v[3] = z;
      v[4] = x * x; v[5] = y * y; v[6] = z * z;                // single products: nothing to fuse with
      v[7] = x * y; v[8] = x * z; v[9] = y * z;
    }
  }
  info_block_sums(v, s_w);
  if (threadIdx.x < kInfoSums) partial[(size_t)blockIdx.x * kInfoSums + threadIdx.x] = v[0];
}

// workgroup per problem: the partial rows in a fixed order, then Lambda = sum G^T G in its closed form
__global__ __launch_bounds__(kInfoBlock) void k_info_reduce(InfoBatch sg, const double* __restrict__ partial,
                                                            const int* __restrict__ grid_status, double* __restrict__ info,
                                                            double* __restrict__ sums) {
  __shared__ double s_w[4][kInfoSums];
  __shared__ double s_tot[kInfoSums];
  const int prob = blockIdx.x;
  if (*grid_status != 0) return;                               // no association ran: the host returns APR_ERANGE
  double v[kInfoSums];
#pragma unroll
  for (int k = 0; k < kInfoSums; ++k) v[k] = 0.0;
  for (int blk = sg.blk0[prob] + (int)threadIdx.x; blk < sg.blk0[prob + 1]; blk += kInfoBlock)
#pragma unroll
    for (int k = 0; k < kInfoSums; ++k) v[k] += partial[(size_t)blk * kInfoSums + k];
  info_block_sums(v, s_w);
  if (threadIdx.x < kInfoSums) {
    s_tot[threadIdx.x] = v[0];
    if (sums) sums[(size_t)prob * kInfoSums + threadIdx.x] = v[0];
  }
  __syncthreads();
  if (threadIdx.x >= 36) return;
  const double n = s_tot[0], x = s_tot[1], y = s_tot[2], z = s_tot[3], xx = s_tot[4], yy = s_tot[5], zz = s_tot[6],
               xy = s_tot[7], xz = s_tot[8], yz = s_tot[9];
  const int r = threadIdx.x / 6, c = threadIdx.x % 6;
  double o = 0.0;
  if (r < 3 && c < 3) {
    if (r == c) o = r == 0 ? yy + zz : (r == 1 ? xx + zz : xx + yy);
    else {
      const int lo = r < c ? r : c, hi = r < c ? c : r;
      o = -(lo == 0 ? (hi == 1 ? xy : xz) : yz);
    }
  } else if (r >= 3 && c >= 3) {
    o = r == c ? n : 0.0;
  } else {
    // rows alpha, beta, gamma against tx, ty, tz: [[0, -z, y], [z, 0, -x], [-y, x, 0]]; the block below is its transpose
    const int rr = r < 3 ? r : c, cc = (r < 3 ? c : r) - 3;
    if (rr == 0) o = cc == 1 ? -z : (cc == 2 ? y : 0.0);
    else if (rr == 1) o = cc == 0 ? z : (cc == 2 ? -x : 0.0);
    else o = cc == 0 ? -y : (cc == 1 ? x : 0.0);
  }
  info[(size_t)prob * 36 + threadIdx.x] = o;
}

struct InfoScratch {
  void* grid;
  float4* rows;
  double* partial;
};

static int info_total_blocks(int64_t n_src_total, int nb) { return (int)(cdiv64(n_src_total, kInfoBlock) + nb); }

static InfoScratch info_walk(AprArena& a, int64_t n, int64_t m, int nb) {
  InfoScratch s;
  s.grid = a.take<char>(apr_internal_grid_bytes(m));      // points.hip's search grid: its own carve
  s.rows = a.take<float4>(m > 0 ? m : 1);
  s.partial = a.take<double>((size_t)info_total_blocks(n > 0 ? n : 1, nb) * kInfoSums);
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// pose graph

constexpr int kPgMaxNodes = APR_POSEGRAPH_MAX_NODES;
constexpr int kPgMaxEdges = kPgMaxNodes * (kPgMaxNodes - 1) / 2;
constexpr int kPgDim = 6 * kPgMaxNodes;
constexpr int kPgBlock = 256;
constexpr int kPgMaxIteration = 100, kPgMaxIterationLm = 20;
constexpr double kPgMin = 1e-6;        // every min_* of GlobalOptimizationConvergenceCriteria

struct PgShared {
  double P[kPgMaxNodes][16], Pn[kPgMaxNodes][16];   // current and trial poses
  double Ti[kPgMaxEdges][16];                       // T_e^-1
  double X[kPgMaxEdges][16];                        // T_e^-1 P_t^-1
  double err[kPgMaxEdges][6], Le[kPgMaxEdges][6], r[kPgMaxEdges];
  double A[kPgMaxEdges][36], g[kPgMaxEdges][6];     // the Jacobians themselves live in L between two solves
  double conf[kPgMaxEdges];
  double H[kPgDim][kPgDim], L[kPgDim][kPgDim + 1], b[kPgDim], d[kPgDim], x[kPgDim];
  int es[kPgMaxEdges], et[kPgMaxEdges], unc[kPgMaxEdges], act[kPgMaxEdges];
  double lambda, ni, cur, rho, mu;
  int stop, iter, lm, status;
};

__device__ __forceinline__ void pg_mul(const double* a, const double* b, double* c) {   // affine 4x4: last row (0,0,0,1)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c[4 * i + j] = (a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j] + (j == 3 ? a[4 * i + 3] : 0.0);
  }
  c[12] = c[13] = c[14] = 0.0;
  c[15] = 1.0;
}

// inverse of an affine 4x4 [A t; 0 1] by the adjugate of A (no assumption that A is a rotation)
__device__ __forceinline__ void pg_inv(const double* m, double* o) {
  const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], k = m[10];
  const double c00 = e * k - f * h, c01 = f * g - d * k, c02 = d * h - e * g;
  const double id = 1.0 / (a * c00 + b * c01 + c * c02);
  o[0] = c00 * id; o[1] = (c * h - b * k) * id; o[2] = (b * f - c * e) * id;
  o[4] = c01 * id; o[5] = (a * k - c * g) * id; o[6] = (c * d - a * f) * id;
  o[8] = c02 * id; o[9] = (b * g - a * h) * id; o[10] = (a * e - b * d) * id;
#pragma unroll
  for (int i = 0; i < 3; ++i) o[4 * i + 3] = -((o[4 * i] * m[3] + o[4 * i + 1] * m[7]) + o[4 * i + 2] * m[11]);
  o[12] = o[13] = o[14] = 0.0;
  o[15] = 1.0;
}

__device__ __forceinline__ void pg_vec(const double* M, double* v) {
  const double sy = hypot(M[0], M[4]);
  if (sy >= 1e-6) {
    v[0] = atan2(M[9], M[10]);
    v[1] = atan2(-M[8], sy);
    v[2] = atan2(M[4], M[0]);
  } else {
    v[0] = atan2(-M[6], M[5]);
    v[1] = atan2(-M[8], sy);
    v[2] = 0.0;
  }
  v[3] = M[3]; v[4] = M[7]; v[5] = M[11];
}

__device__ __forceinline__ void pg_mat(const double* v, double* M) {     // Rz(gamma) Ry(beta) Rx(alpha)
  const double ca = cos(v[0]), sa = sin(v[0]), cb = cos(v[1]), sb = sin(v[1]), cg = cos(v[2]), sg = sin(v[2]);
  M[0] = cg * cb; M[1] = cg * sb * sa - sg * ca; M[2] = cg * sb * ca + sg * sa; M[3] = v[3];
  M[4] = sg * cb; M[5] = sg * sb * sa + cg * ca; M[6] = sg * sb * ca - cg * sa; M[7] = v[4];
  M[8] = -sb;     M[9] = cb * sa;                M[10] = cb * ca;               M[11] = v[5];
  M[12] = M[13] = M[14] = 0.0;
  M[15] = 1.0;
}

// errors (and, with `jac`, Jacobians and the per-edge blocks A = Js^T Lambda Js, g = Js^T Lambda e) of the active edges at
// the poses P.  Ends on a barrier.
__device__ void pg_eval(PgShared& s, const double (*P)[16], int ne, const double* __restrict__ lam, bool jac) {
  const int tid = threadIdx.x;
  if (tid < ne && s.act[tid]) {
    double inv[16], X[16], Z[16], e[6];
    pg_inv(P[s.et[tid]], inv);
    pg_mul(s.Ti[tid], inv, X);
    pg_mul(X, P[s.es[tid]], Z);
    pg_vec(Z, e);
    const double* Lm = lam + (size_t)tid * 36;
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) a += Lm[6 * i + j] * e[j];
      s.Le[tid][i] = a;
      s.err[tid][i] = e[i];
      r += e[i] * a;
    }
    s.r[tid] = r;
#pragma unroll
    for (int i = 0; i < 16; ++i) s.X[tid][i] = X[i];
  }
  __syncthreads();
  if (!jac) return;
  static_assert(sizeof(s.L) >= sizeof(double) * kPgMaxEdges * 36, "the Jacobians borrow L");
  double (*Js)[36] = reinterpret_cast<double (*)[36]>(&s.L[0][0]);
  // Js[:, i] = lin(X O_i P_s): O_i P_s has at most two non-zero rows
  if (tid < ne * 6 && s.act[tid / 6]) {
    const int e = tid / 6, i = tid % 6;
    const double* Ps = P[s.es[e]];
    double W[16], M[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) W[k] = 0.0;
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { W[4 + k] = -Ps[8 + k]; W[8 + k] = Ps[4 + k]; }
    } else if (i == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { W[k] = Ps[8 + k]; W[8 + k] = -Ps[k]; }
    } else if (i == 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { W[k] = -Ps[4 + k]; W[4 + k] = Ps[k]; }
    } else {
      W[4 * (i - 3) + 3] = 1.0;                                // O_i P_s: row i - 3 = the last row of P_s = (0, 0, 0, 1)
    }
    const double* X = s.X[e];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) M[4 * a + c] = (X[4 * a] * W[c] + X[4 * a + 1] * W[4 + c]) + X[4 * a + 2] * W[8 + c];
    Js[e][0 * 6 + i] = (M[9] - M[6]) * 0.5;
    Js[e][1 * 6 + i] = (M[2] - M[8]) * 0.5;
    Js[e][2 * 6 + i] = (M[4] - M[1]) * 0.5;
    Js[e][3 * 6 + i] = M[3];
    Js[e][4 * 6 + i] = M[7];
    Js[e][5 * 6 + i] = M[11];
  }
  __syncthreads();
  for (int t = tid; t < ne * 42; t += kPgBlock) {
    const int e = t / 42, q = t % 42;
    if (!s.act[e]) continue;
    const double* J = Js[e];
    if (q < 36) {
      const int i = q / 6, j = q % 6;
      const double* Lm = lam + (size_t)e * 36;
      double acc = 0.0;
      for (int k = 0; k < 6; ++k) {
        double m = 0.0;
        for (int l = 0; l < 6; ++l) m += Lm[6 * k + l] * J[6 * l + j];
        acc += J[6 * k + i] * m;
      }
      s.A[e][q] = acc;
    } else {
      const int i = q - 36;
      double acc = 0.0;
      for (int k = 0; k < 6; ++k) acc += J[6 * k + i] * s.Le[e][k];
      s.g[e][i] = acc;
    }
  }
  __syncthreads();
}

// H and b: a thread owns an entry and walks the edges in ascending order.  Jt = -Js, so with A = Js^T Lambda Js and
// g = Js^T Lambda e: H_ss += l A, H_tt += l A, H_st -= l A, H_ts -= l A, b_s -= l g, b_t += l g.  Ends on a barrier.
__device__ void pg_assemble(PgShared& s, int n, int ne) {
  const int N = 6 * n;
  for (int t = threadIdx.x; t < N * N + N; t += kPgBlock) {
    if (t < N * N) {
      const int r = t / N, c = t % N, a = r / 6, bnode = c / 6, q = (r % 6) * 6 + c % 6;
      double h = 0.0;
      for (int e = 0; e < ne; ++e) {
        if (!s.act[e]) continue;
        const double l = s.unc[e] ? s.conf[e] : 1.0;
        const int es = s.es[e], et = s.et[e];
        if (a == bnode) {
          if (es == a || et == a) h += l * s.A[e][q];
        } else if ((es == a && et == bnode) || (es == bnode && et == a)) {
          h -= l * s.A[e][q];
        }
      }
      s.H[r][c] = h;
    } else {
      const int r = t - N * N, a = r / 6, i = r % 6;
      double v = 0.0;
      for (int e = 0; e < ne; ++e) {
        if (!s.act[e]) continue;
        const double l = s.unc[e] ? s.conf[e] : 1.0;
        if (s.es[e] == a) v -= l * s.g[e][i];
        else if (s.et[e] == a) v += l * s.g[e][i];
      }
      s.b[r] = v;
    }
  }
  __syncthreads();
}

// sum_e [ l e^T Lambda e + mu (sqrt(l) - 1)^2 if uncertain ] in ascending order (one thread)
__device__ inline double pg_residual(const PgShared& s, int ne) {
  double tot = 0.0;
  for (int e = 0; e < ne; ++e) {
    if (!s.act[e]) continue;
    if (s.unc[e]) {
      const double l = s.conf[e], q = sqrt(l) - 1.0;
      tot += l * s.r[e] + s.mu * q * q;
    } else {
      tot += s.r[e];
    }
  }
  return tot;
}

// (H + lambda I) d = b by Cholesky in LDS; the matrix is positive definite for lambda > 0.  -> s.d.  A pivot that is not
// positive and finite sets status 3 and stop.  Ends on a barrier.
__device__ void pg_solve(PgShared& s, int N) {
  const int tid = threadIdx.x;
  for (int t = tid; t < N * N; t += kPgBlock) {
    const int r = t / N, c = t % N;
    s.L[r][c] = s.H[r][c] + (r == c ? s.lambda : 0.0);
  }
  if (tid < N) s.d[tid] = s.b[tid];
  __syncthreads();
  for (int j = 0; j < N; ++j) {
    if (tid == 0) {
      const double p = s.L[j][j];
      if (!(p > 0.0) || !(p < 1e300)) {
        s.status = 3;
        s.stop = 1;
        s.L[j][j] = 1.0;
      } else {
        s.L[j][j] = sqrt(p);
      }
    }
    __syncthreads();
    const double piv = s.L[j][j];
    for (int i = j + 1 + tid; i < N; i += kPgBlock) s.L[i][j] /= piv;
    __syncthreads();
    const int w = N - j - 1;
    for (int t = tid; t < w * w; t += kPgBlock) {
      const int i = j + 1 + t / w, k = j + 1 + t % w;
      if (k <= i) s.L[i][k] -= s.L[i][j] * s.L[k][j];
    }
    __syncthreads();
  }
  for (int j = 0; j < N; ++j) {                                // L y = b
    if (tid == 0) s.d[j] /= s.L[j][j];
    __syncthreads();
    const double y = s.d[j];
    for (int i = j + 1 + tid; i < N; i += kPgBlock) s.d[i] -= s.L[i][j] * y;
    __syncthreads();
  }
  for (int j = N - 1; j >= 0; --j) {                           // L^T d = y
    if (tid == 0) s.d[j] /= s.L[j][j];
    __syncthreads();
    const double y = s.d[j];
    for (int i = tid; i < j; i += kPgBlock) s.d[i] -= s.L[j][i] * y;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kPgBlock) void k_posegraph(const int* __restrict__ node_off, const int* __restrict__ edge_off,
                                                        const int* __restrict__ edges, const double* __restrict__ Te,
                                                        int64_t t_stride, const double* __restrict__ lam_all,
                                                        const double* __restrict__ init, double mcd2, double preference,
                                                        double prune, double* __restrict__ poses, double* __restrict__ conf_out,
                                                        int* __restrict__ kept, int* __restrict__ iters, int* __restrict__ status) {
  __shared__ PgShared s;
  const int gph = blockIdx.x, tid = threadIdx.x;
  const int n0 = node_off[gph], n = node_off[gph + 1] - n0, e0 = edge_off[gph], ne = edge_off[gph + 1] - e0;
  if (tid == 0) {
    iters[2 * gph] = 0;
    iters[2 * gph + 1] = 0;
  }
  if (n < 1 || n > kPgMaxNodes || ne < 0 || ne > kPgMaxEdges || n0 < 0 || e0 < 0) {   // nothing of this graph is touched
    if (tid == 0) status[gph] = 4;
    return;
  }
  const double* lam = lam_all + (size_t)e0 * 36;
  if (tid == 0) {
    s.status = 0;
    s.stop = 0;
  }
  __syncthreads();
  if (tid < ne) {
    const int a = edges[3 * (e0 + tid)], b = edges[3 * (e0 + tid) + 1];
    s.es[tid] = a;
    s.et[tid] = b;
    s.unc[tid] = edges[3 * (e0 + tid) + 2] != 0;
    s.act[tid] = 1;
    s.conf[tid] = 1.0;
    if (!(a >= 0 && a < b && b < n)) s.status = 4;             // every writer stores the same value
    else {
      double T[16];
      const double* src = Te + (size_t)(e0 + tid) * t_stride;
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = src[k];
      pg_inv(T, s.Ti[tid]);
    }
  }
  __syncthreads();
  if (s.status == 0 && tid == 0) {
    if (init) {
      for (int i = 0; i < n; ++i)
        for (int k = 0; k < 16; ++k) s.P[i][k] = k < 12 ? init[(size_t)(n0 + i) * 16 + k] : (k == 15 ? 1.0 : 0.0);
    } else {
      // the odometry chain: P_0 = I, odo <- T_(j,j+1) odo, P_(j+1) = odo^-1.  odo^-1 is carried instead:
      // (T odo)^-1 = odo^-1 T^-1, one product per node and no inverse of a product
      for (int k = 0; k < 16; ++k) s.P[0][k] = (k % 5 == 0) ? 1.0 : 0.0;
      for (int j = 0; j + 1 < n && s.status == 0; ++j) {
        int found = -1;
        for (int e = 0; e < ne && found < 0; ++e)
          if (s.es[e] == j && s.et[e] == j + 1) found = e;
        if (found < 0) s.status = 4;
        else pg_mul(s.P[j], s.Ti[found], s.P[j + 1]);
      }
    }
  }
  __syncthreads();
  if (s.status != 0) {
    if (tid == 0) status[gph] = s.status;
    return;
  }
  const int N = 6 * n;
  if (tid < n) pg_vec(s.P[tid], &s.x[6 * tid]);
  __syncthreads();

  for (int pass = 0; pass < 2; ++pass) {
    if (tid == 0) {
      double sum = 0.0;
      int cnt = 0;
      for (int e = 0; e < ne; ++e)
        if (s.act[e]) {
          sum += lam[(size_t)e * 36 + 35];
          ++cnt;
        }
      s.mu = cnt > 0 ? preference * mcd2 * (sum / (double)cnt) : 0.0;
      if (!(s.mu > 0.0) || !(s.mu < 1e300)) s.status = pass == 0 ? 1 : 2;   // degenerate: the poses stay as they are
      s.iter = 0;
    }
    __syncthreads();
    if (s.status != 0) break;
    pg_eval(s, s.P, ne, lam, true);
    pg_assemble(s, n, ne);
    if (tid == 0) {
      s.cur = pg_residual(s, ne);
      double md = s.H[0][0], mb = s.b[0];
      for (int i = 1; i < N; ++i) {
        md = fmax(md, s.H[i][i]);
        mb = fmax(mb, s.b[i]);
      }
      s.lambda = 1e-5 * md;
      s.ni = 2.0;
      s.stop = mb < kPgMin;
    }
    __syncthreads();
    while (!s.stop && s.iter < kPgMaxIteration) {
      __syncthreads();                                         // everyone has read stop / iter before thread 0 moves on
      if (tid == 0) {
        s.lm = 0;
        s.rho = 0.0;
      }
      bool again = true;
      while (again) {
        pg_solve(s, N);
        if (tid == 0 && !s.stop) {
          double dn = 0.0, xn = 0.0;
          for (int i = 0; i < N; ++i) {
            dn += s.d[i] * s.d[i];
            xn += s.x[i] * s.x[i];
          }
          if (sqrt(dn) < kPgMin * (sqrt(xn) + kPgMin)) s.stop = 1;
        }
        __syncthreads();
        if (!s.stop) {
          if (tid < n) {
            double D[16];
            pg_mat(&s.d[6 * tid], D);
            pg_mul(D, s.P[tid], s.Pn[tid]);
          }
          __syncthreads();
          pg_eval(s, s.Pn, ne, lam, false);
          if (tid == 0) {
            const double nw = pg_residual(s, ne);
            double den = 0.0;
            for (int i = 0; i < N; ++i) den += s.d[i] * (s.lambda * s.d[i] + s.b[i]);
            const double rho = (s.cur - nw) / (den + 1e-3);
            s.rho = rho;
            if (rho > 0.0) {
              if (s.cur - nw < kPgMin * s.cur || nw < kPgMin) s.stop = 1;
              const double c = 2.0 * rho - 1.0;
              s.lambda *= fmax(1.0 / 3.0, fmin(1.0 - c * c * c, 2.0 / 3.0));
              s.ni = 2.0;
              s.cur = nw;
            } else {
              s.lambda *= s.ni;
              s.ni *= 2.0;
            }
          }
          __syncthreads();
          if (s.rho > 0.0) {                                   // accept: poses, confidences, H and b at the new poses
            if (tid < n * 16) s.P[tid / 16][tid % 16] = s.Pn[tid / 16][tid % 16];
            if (tid < ne && s.act[tid] && s.unc[tid]) {
              const double q = s.mu / (s.mu + s.r[tid]);
              s.conf[tid] = q * q;
            }
            __syncthreads();
            if (tid < n) pg_vec(s.P[tid], &s.x[6 * tid]);
            pg_eval(s, s.P, ne, lam, true);
            pg_assemble(s, n, ne);
            if (tid == 0) {
              double mb = s.b[0];
              for (int i = 1; i < N; ++i) mb = fmax(mb, s.b[i]);
              if (mb < kPgMin) s.stop = 1;
            }
          }
        }
        __syncthreads();
        if (tid == 0) {
          s.lm += 1;
          if (s.lm > kPgMaxIterationLm) s.stop = 1;
        }
        __syncthreads();
        again = !(s.rho > 0.0 || s.stop);
        __syncthreads();
      }
      if (tid == 0) s.iter += 1;
      __syncthreads();
    }
    __syncthreads();
    if (tid == 0) iters[2 * gph + pass] = s.iter;
    if (pass == 0) {
      if (tid < ne) {
        const double c = s.unc[tid] ? s.conf[tid] : 1.0;
        const int keep = !(s.unc[tid] && c < prune);
        conf_out[e0 + tid] = c;
        kept[e0 + tid] = keep;
        s.act[tid] = keep;
      }
      if (tid == 0 && s.status == 0) s.stop = 0;
    }
    __syncthreads();
    if (s.status != 0) break;
  }
  if (s.status == 1 && tid < ne) {                             // no pass ran: every edge as it came in
    conf_out[e0 + tid] = 1.0;
    kept[e0 + tid] = 1;
  }
  if (tid < n * 16) poses[(size_t)n0 * 16 + tid] = s.P[tid / 16][tid % 16];
  if (tid == 0) status[gph] = s.status;
}

}  // namespace

APR_API size_t apr_information_scratch_bytes(int64_t n_src_total, int64_t n_tgt_total, int32_t nb) {
  AprArena a(nullptr);
  info_walk(a, n_src_total, n_tgt_total, nb > 0 ? nb : 1);
  return a.bytes();
}

APR_API int apr_information_batch(const float* src, const int64_t* src_offsets_host, const float* tgt,
                                  const int64_t* tgt_offsets_host, int32_t n_tgt, const int32_t* tgt_of_problem_host, int32_t nb,
                                  const double* T, int64_t t_stride, double max_dist, double* info, double* sums, int32_t* corr,
                                  void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(nb >= 1 && nb <= kInfoMaxProblems, "apr_information_batch: 1 .. %d problems, got %d", kInfoMaxProblems, (int)nb);
  APR_CHECK_ARG(n_tgt >= 1 && n_tgt <= kInfoMaxProblems, "apr_information_batch: 1 .. %d target segments", kInfoMaxProblems);
  APR_CHECK_ARG(src && tgt && src_offsets_host && tgt_offsets_host && T && info, "apr_information_batch: NULL argument");
  APR_CHECK_ARG(t_stride >= 12, "apr_information_batch: a transform needs a stride of at least 12 doubles");
  APR_CHECK_ARG(max_dist > 0.0 && max_dist < 1e18, "apr_information_batch: max_dist must be positive and finite");
  APR_CHECK_ARG(tgt_of_problem_host || n_tgt == nb,
                "apr_information_batch: without tgt_of_problem, one target segment per problem");
  APR_CHECK_ARG(src_offsets_host[0] == 0 && tgt_offsets_host[0] == 0, "apr_information_batch: offsets start at 0");
  for (int i = 0; i < nb; ++i)
    APR_CHECK_ARG(src_offsets_host[i + 1] > src_offsets_host[i], "apr_information_batch: empty source of problem %d", i);
  for (int i = 0; i < n_tgt; ++i)
    APR_CHECK_ARG(tgt_offsets_host[i + 1] > tgt_offsets_host[i], "apr_information_batch: empty target segment %d", i);
  const int64_t n = src_offsets_host[nb], m = tgt_offsets_host[n_tgt];
  APR_CHECK_ARG(n < (1ll << 31) - kInfoBlock * (kInfoMaxProblems + 1) && m < (1ll << 31) - 1,
                "apr_information_batch: oversized clouds");
  AprArena arena(scratch);
  const InfoScratch w = info_walk(arena, n, m, nb);
  APR_CHECK_ARG(scratch && arena.fits(scratch_bytes), "apr_information_batch: scratch too small");
  InfoBatch sg;
  sg.nb = nb;
  sg.blk0[0] = 0;
  int32_t tlen[kInfoMaxProblems];
  for (int i = 0; i < nb; ++i) {
    const int seg = tgt_of_problem_host ? tgt_of_problem_host[i] : i;
    APR_CHECK_ARG(seg >= 0 && seg < n_tgt, "apr_information_batch: problem %d names target segment %d of %d", i, seg, (int)n_tgt);
    sg.tseg[i] = seg;
    sg.a0[i] = (int)src_offsets_host[i];
    sg.blk0[i + 1] = sg.blk0[i] + (int)cdiv64(src_offsets_host[i + 1] - src_offsets_host[i], kInfoBlock);
  }
  sg.a0[nb] = (int)n;
  for (int i = 0; i <= n_tgt; ++i) {
    sg.b0[i] = (int)tgt_offsets_host[i];
    if (i) tlen[i - 1] = (int32_t)(tgt_offsets_host[i] - tgt_offsets_host[i - 1]);
  }
  const float rf = (float)max_dist;
  const float r2 = rf * rf;                      // the strict bound, in the precision of d^2
  AprSearchGrid g;
  int rc = apr_internal_search_grid_batch(tgt, m, tlen, n_tgt, rf * 1.01f, w.grid, &g, st);
  if (rc != APR_OK) return rc;
  rc = apr_internal_icp_pack(tgt, m, g, w.rows, st);
  if (rc != APR_OK) return rc;
  hipLaunchKernelGGL(k_info_assoc, dim3((unsigned)sg.blk0[nb]), dim3(kInfoBlock), 0, st, src, (const float4*)w.rows, g, sg, r2,
                     T, t_stride, w.partial, corr);
  hipLaunchKernelGGL(k_info_reduce, dim3((unsigned)nb), dim3(kInfoBlock), 0, st, sg, (const double*)w.partial, g.status, info,
                     sums);
  APR_LAUNCH_CHECK();
  static thread_local int* status_host = nullptr;            // pinned
  if (!status_host) APR_HIP(hipHostMalloc((void**)&status_host, sizeof(int), hipHostMallocDefault));
  APR_HIP(hipMemcpyAsync(status_host, g.status, sizeof(int), hipMemcpyDeviceToHost, st));
  APR_HIP(hipStreamSynchronize(st));
  if (*status_host != 0) {
    apr_set_error("apr_information_batch: search grid refused, status %d (1: cell index outside the packed key, 2: cell table "
                  "full, 3: a target segment spans more than %d cells of 1.01 * max_dist); info, sums and corr were not written",
                  *status_host, APR_GRID_MARGIN_CELLS);
    return APR_ERANGE;
  }
  return APR_OK;
}

APR_API int apr_posegraph_optimize(const int32_t* node_offsets, const int32_t* edge_offsets, int32_t ng, const int32_t* edges,
                                   const double* T, int64_t t_stride, const double* info, const double* init_poses,
                                   double max_correspondence_distance, double edge_prune_threshold,
                                   double preference_loop_closure, double* poses, double* confidence, int32_t* kept,
                                   int32_t* iterations, int32_t* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(ng >= 1 && ng <= (1 << 20), "apr_posegraph_optimize: 1 .. 2^20 graphs, got %d", (int)ng);
  APR_CHECK_ARG(node_offsets && edge_offsets && edges && T && info && poses && confidence && kept && iterations && status,
                "apr_posegraph_optimize: NULL argument");
  APR_CHECK_ARG(t_stride >= 12, "apr_posegraph_optimize: a transform needs a stride of at least 12 doubles");
  APR_CHECK_ARG(max_correspondence_distance > 0.0 && max_correspondence_distance < 1e18,
                "apr_posegraph_optimize: max_correspondence_distance must be positive and finite");
  APR_CHECK_ARG(edge_prune_threshold >= 0.0 && edge_prune_threshold <= 1.0, "apr_posegraph_optimize: prune threshold in [0, 1]");
  APR_CHECK_ARG(preference_loop_closure > 0.0 && preference_loop_closure < 1e18,
                "apr_posegraph_optimize: preference_loop_closure must be positive and finite");
  hipLaunchKernelGGL(k_posegraph, dim3((unsigned)ng), dim3(kPgBlock), 0, st, node_offsets, edge_offsets, edges, T, t_stride, info,
                     init_poses, max_correspondence_distance * max_correspondence_distance, preference_loop_closure,
                     edge_prune_threshold, poses, confidence, kept, iterations, status);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

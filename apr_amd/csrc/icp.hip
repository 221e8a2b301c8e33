// Point-to-point ICP (open3d >= 0.12 RegistrationICP + TransformationEstimationPointToPoint) for a BATCH of independent
// problems, the pose refinement APR runs on every pose that feeds the aggregated point cloud:
//   FCGF_APR/lib/complement_data_loader.py:369-405 (_get_icp, _get_neighbourhood_icp), FCGF_APR/lib/data_loaders.py:460-463,
//   Predator_APR/datasets/kitti.py:201-204, 424-428, 558-560.
//
// One call = one grid build over the target segments (cell = max_dist, widened by 1 %: the cell coordinate is a rounded
// fp32 quotient, and a target at d < max_dist must never fall outside the 27 cells probed -- proven for cell indices below
// APR_GRID_MARGIN_CELLS, common.h; a segment that extends further is refused with APR_ERANGE), then per ROUND two launches
// that cover every problem of the batch:
//   k_icp_assoc : thread per source row.  p = fl32(T * s) (fp64 product of the ORIGINAL row with the cumulative fp64 T,
//                 rounded once), 27-cell probe, d^2 = (dx^2 + dy^2) + dz^2 in fp32 with every operation rounded, d^2 < r^2
//                 strictly, ties to the smallest target row.  The moved cloud never reaches memory: each workgroup leaves 17
//                 fp64 partial sums (count, sum p, sum q, sum p q^T, sum d^2) combined in a fixed order.
//   k_icp_update: workgroup per problem.  Adds the partials in a fixed order, derives fitness / rmse of the current T, applies
//                 open3d's stopping rule, else Horn's closed form on the 3x3 cross-covariance (fp64 Jacobi) and T = U * T.
// No float atomics anywhere: the same bits run to run, and for a problem alone or inside a batch (the partials of a
// problem are laid out from its own first row).  A finished problem sets its `done` flag; both kernels leave at once on
// it.  The host enqueues rounds in chunks and looks at the flags once per chunk, one chunk behind what it has enqueued, so
// the device never waits for the host.
#include "common.h"

namespace {

constexpr int kIcpMaxProblems = 64;   // = the segment limit of the batched search grid
constexpr int kIcpBlock = 256;
constexpr int kIcpSums = 17;          // count, p[3], q[3], p q^T [9], d^2
constexpr int kIcpChunk = 8;          // rounds enqueued between two looks at the flags


struct IcpBatch {
  int nb;
  int blk0[kIcpMaxProblems + 1];   // first workgroup (= first row of partials) of every problem
  int a0[kIcpMaxProblems + 1];     // source rows
  int tseg[kIcpMaxProblems];       // target segment of every problem
  int b0[kIcpMaxProblems + 1];     // target rows of every SEGMENT
};

__device__ inline float icp_d2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__global__ void k_icp_init(const double* __restrict__ init, int nb, double* __restrict__ rec, int* __restrict__ done) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nb * APR_ICP_RECORD_DOUBLES) return;
  const int b = t / APR_ICP_RECORD_DOUBLES, k = t % APR_ICP_RECORD_DOUBLES;
  rec[t] = k < 16 ? init[b * 16 + k] : 0.0;
  if (k == 0) done[b] = 0;
}

// target rows in bucket order, one 16-B record each: (x, y, z, bits(global row)).  A grid whose status word is set is not
// read at all, here or in the rounds: a row outside the key range is in no bucket, so the buckets end at
// start[n_cells] < m and the tail of `sorted` behind them was never written -- an index from there is anything.  The
// bound on e keeps that true whatever the status says.
__global__ void k_icp_pack(const float* __restrict__ b, int64_t m, AprSearchGrid g, float4* __restrict__ rows) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (*g.status != 0 || e >= m || e >= g.start[*g.n_cells]) return;
  const int j = g.sorted[e];
  rows[e] = make_float4(b[3 * (int64_t)j], b[3 * (int64_t)j + 1], b[3 * (int64_t)j + 2], __int_as_float(j));
}

// sum over the 256 threads in a fixed order: xor butterfly inside each wave, then (w0 + w1) + (w2 + w3)
__device__ inline void block_sums(double* v, double (*s_w)[kIcpSums]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) {
    double x = v[k];
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if (lane == 0) s_w[wave][k] = x;
  }
  __syncthreads();
  if (threadIdx.x < kIcpSums) {
    const int k = threadIdx.x;
    v[0] = (s_w[0][k] + s_w[1][k]) + (s_w[2][k] + s_w[3][k]);
  }
}

__global__ __launch_bounds__(kIcpBlock) void k_icp_assoc(const float* __restrict__ a, const float4* __restrict__ rows,
                                                         AprSearchGrid g, IcpBatch sg, float r2, const double* __restrict__ rec,
                                                         const int* __restrict__ done, double* __restrict__ partial,
                                                         int* __restrict__ corr) {
  __shared__ double s_w[4][kIcpSums];
  int prob = 0;
  while (prob + 1 < sg.nb && (int)blockIdx.x >= sg.blk0[prob + 1]) ++prob;
  if (done[prob] || *g.status != 0) return;                  // a flagged grid is never searched (k_icp_pack)
  const int seg = sg.tseg[prob];
  const int64_t i = (int64_t)sg.a0[prob] + (int64_t)((int)blockIdx.x - sg.blk0[prob]) * kIcpBlock + threadIdx.x;
  double v[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
  if (i < sg.a0[prob + 1]) {
    const double* T = rec + (size_t)prob * APR_ICP_RECORD_DOUBLES;
    const double sx = a[3 * i], sy = a[3 * i + 1], sz = a[3 * i + 2];
    float p[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      p[d] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[4 * d], sx), __dmul_rn(T[4 * d + 1], sy)),
                                        __dmul_rn(T[4 * d + 2], sz)), T[4 * d + 3]);
    int c[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) c[d] = (int)floorf(__fdiv_rn(__fsub_rn(p[d], g.mins[3 * seg + d]), g.cell));
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
        const float d2 = icp_d2(p[0], p[1], p[2], q.x, q.y, q.z);
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
      const double px = p[0], py = p[1], pz = p[2], qx = bq.x, qy = bq.y, qz = bq.z;
      v[0] = 1.0;
      v[1] = px; v[2] = py; v[3] = pz;
      v[4] = qx; v[5] = qy; v[6] = qz;
      v[7] = px * qx; v[8] = px * qy; v[9] = px * qz;
      v[10] = py * qx; v[11] = py * qy; v[12] = py * qz;
      v[13] = pz * qx; v[14] = pz * qy; v[15] = pz * qz;
      v[16] = (double)bd;
    }
  }
  block_sums(v, s_w);
  if (threadIdx.x < kIcpSums) partial[(size_t)blockIdx.x * kIcpSums + threadIdx.x] = v[0];
}

// Horn's closed form: the rotation maximising trace(R^T-aligned S), S = sum (p - mp)(q - mq)^T; equals Eigen::umeyama without
// scaling wherever the optimum is unique, and is a proper, finite rotation for every finite S (S = 0 -> identity)
__device__ inline void icp_horn(const double S[3][3], double R[3][3]) {
  double A[4][4];
  A[0][0] = S[0][0] + S[1][1] + S[2][2];
  A[0][1] = S[1][2] - S[2][1];
  A[0][2] = S[2][0] - S[0][2];
  A[0][3] = S[0][1] - S[1][0];
  A[1][1] = S[0][0] - S[1][1] - S[2][2];
  A[1][2] = S[0][1] + S[1][0];
  A[1][3] = S[2][0] + S[0][2];
  A[2][2] = -S[0][0] + S[1][1] - S[2][2];
  A[2][3] = S[1][2] + S[2][1];
  A[3][3] = -S[0][0] - S[1][1] + S[2][2];
  A[1][0] = A[0][1]; A[2][0] = A[0][2]; A[3][0] = A[0][3];
  A[2][1] = A[1][2]; A[3][1] = A[1][3]; A[3][2] = A[2][3];
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 4; ++p) {
      diag += A[p][p] * A[p][p];
      for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    }
    if (off <= 1e-32 * diag || off == 0.0) break;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
        for (int k = 0; k < 4; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - sn * akq;
          A[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - sn * aqk;
          A[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - sn * vkq;
          V[k][q] = sn * vkp + c * vkq;
        }
      }
  }
  int best = 0;
  for (int j = 1; j < 4; ++j)
    if (A[j][j] > A[best][best]) best = j;
  double qw = V[0][best], qx = V[1][best], qy = V[2][best], qz = V[3][best];
  const double n2 = qw * qw + qx * qx + qy * qy + qz * qz;
  if (!(n2 > 0.0) || !(n2 < 1e300)) {          // cannot happen for finite S (V stays orthonormal); never hand out NaN
    qw = 1.0; qx = qy = qz = 0.0;
  } else {
    const double s = 1.0 / sqrt(n2);
    qw *= s; qx *= s; qy *= s; qz *= s;
  }
  R[0][0] = 1 - 2 * (qy * qy + qz * qz); R[0][1] = 2 * (qx * qy - qw * qz); R[0][2] = 2 * (qx * qz + qw * qy);
  R[1][0] = 2 * (qx * qy + qw * qz); R[1][1] = 1 - 2 * (qx * qx + qz * qz); R[1][2] = 2 * (qy * qz - qw * qx);
  R[2][0] = 2 * (qx * qz - qw * qy); R[2][1] = 2 * (qy * qz + qw * qx); R[2][2] = 1 - 2 * (qx * qx + qy * qy);
}

__global__ __launch_bounds__(kIcpBlock) void k_icp_update(IcpBatch sg, const double* __restrict__ partial, int max_iteration,
                                                          double rel_fitness, double rel_rmse, const int* __restrict__ grid_status,
                                                          double* __restrict__ rec, int* __restrict__ done) {
  __shared__ double s_w[4][kIcpSums];
  __shared__ double s_tot[kIcpSums];
  const int prob = blockIdx.x;
  if (done[prob]) return;
  if (*grid_status != 0) {                                     // no association ran: the record stays at init, the host
    if (threadIdx.x == 0) done[prob] = 1;                      // stops enqueueing and returns APR_ERANGE
    return;
  }
  double v[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
  for (int blk = sg.blk0[prob] + (int)threadIdx.x; blk < sg.blk0[prob + 1]; blk += kIcpBlock)
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) v[k] += partial[(size_t)blk * kIcpSums + k];
  block_sums(v, s_w);
  if (threadIdx.x < kIcpSums) s_tot[threadIdx.x] = v[0];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* r = rec + (size_t)prob * APR_ICP_RECORD_DOUBLES;
  const double n = s_tot[0];
  const double fitness = n / (double)(sg.a0[prob + 1] - sg.a0[prob]);
  const double rmse = n > 0.0 ? sqrt(s_tot[16] / n) : 0.0;
  const int round = (int)r[19];
  const bool converged = round >= 1 && fabs(r[16] - fitness) < rel_fitness && fabs(r[17] - rmse) < rel_rmse;
  r[16] = fitness;
  r[17] = rmse;
  r[18] = n;
  if (converged || round >= max_iteration) {
    done[prob] = 1;
    return;
  }
  r[19] = (double)(round + 1);
  if (!(n > 0.0)) return;                                     // no correspondences: the update is the identity
  double mp[3], mq[3], S[3][3], R[3][3];
  for (int d = 0; d < 3; ++d) {
    mp[d] = s_tot[1 + d] / n;
    mq[d] = s_tot[4 + d] / n;
  }
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 3; ++y) S[x][y] = s_tot[7 + 3 * x + y] - n * mp[x] * mq[y];
  icp_horn(S, R);
  double U[12], Tn[12];
  for (int x = 0; x < 3; ++x) {
    U[4 * x] = R[x][0]; U[4 * x + 1] = R[x][1]; U[4 * x + 2] = R[x][2];
    U[4 * x + 3] = mq[x] - (R[x][0] * mp[0] + R[x][1] * mp[1] + R[x][2] * mp[2]);
  }
  for (int x = 0; x < 3; ++x)
    for (int y = 0; y < 4; ++y)
      Tn[4 * x + y] = U[4 * x] * r[y] + U[4 * x + 1] * r[4 + y] + U[4 * x + 2] * r[8 + y] + (y == 3 ? U[4 * x + 3] : 0.0);
  for (int k = 0; k < 12; ++k) r[k] = Tn[k];
}

static int icp_total_blocks(int64_t n_src_total, int nb) { return (int)(cdiv64(n_src_total, kIcpBlock) + nb); }

struct IcpScratch {
  void* grid;
  float4* rows;
  double* partial;
  int* done;
};

static IcpScratch icp_walk(AprArena& a, int64_t n, int64_t m, int nb) {
  IcpScratch s;
  s.grid = a.take<char>(apr_internal_grid_bytes(m));      // points.hip's search grid: its own carve
  s.rows = a.take<float4>(m > 0 ? m : 1);
  s.partial = a.take<double>((size_t)icp_total_blocks(n > 0 ? n : 1, nb) * kIcpSums);
  s.done = a.take<int>(kIcpMaxProblems);
  return s;
}

}  // namespace

int apr_internal_icp_pack(const float* tgt, int64_t m, AprSearchGrid g, float4* rows, hipStream_t st) {
  hipLaunchKernelGGL(k_icp_pack, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, st, tgt, m, g, rows);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API size_t apr_icp_scratch_bytes(int64_t n_src_total, int64_t n_tgt_total, int32_t nb) {
  AprArena a(nullptr);
  icp_walk(a, n_src_total, n_tgt_total, nb > 0 ? nb : 1);
  return a.bytes();
}

APR_API int apr_icp_batch(const float* src, const int64_t* src_offsets_host, const float* tgt, const int64_t* tgt_offsets_host,
                          int32_t n_tgt, const int32_t* tgt_of_problem_host, int32_t nb, const double* init,
                          double max_dist, int32_t max_iteration, double relative_fitness, double relative_rmse,
                          double* result, int32_t* corr, void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(nb >= 1 && nb <= kIcpMaxProblems, "apr_icp_batch: 1 .. %d problems, got %d", kIcpMaxProblems, (int)nb);
  APR_CHECK_ARG(n_tgt >= 1 && n_tgt <= kIcpMaxProblems, "apr_icp_batch: 1 .. %d target segments", kIcpMaxProblems);
  APR_CHECK_ARG(src && tgt && src_offsets_host && tgt_offsets_host && init && result, "apr_icp_batch: NULL argument");
  APR_CHECK_ARG(max_dist > 0.0 && max_dist < 1e18, "apr_icp_batch: max_dist must be positive and finite");
  APR_CHECK_ARG(max_iteration >= 0, "apr_icp_batch: max_iteration < 0");
  APR_CHECK_ARG(relative_fitness >= 0.0 && relative_rmse >= 0.0, "apr_icp_batch: negative convergence threshold");
  APR_CHECK_ARG(tgt_of_problem_host || n_tgt == nb, "apr_icp_batch: without tgt_of_problem, one target segment per problem");
  APR_CHECK_ARG(src_offsets_host[0] == 0 && tgt_offsets_host[0] == 0, "apr_icp_batch: offsets start at 0");
  for (int i = 0; i < nb; ++i)
    APR_CHECK_ARG(src_offsets_host[i + 1] > src_offsets_host[i], "apr_icp_batch: empty source of problem %d", i);
  for (int i = 0; i < n_tgt; ++i)
    APR_CHECK_ARG(tgt_offsets_host[i + 1] > tgt_offsets_host[i], "apr_icp_batch: empty target segment %d", i);
  const int64_t n = src_offsets_host[nb], m = tgt_offsets_host[n_tgt];
  APR_CHECK_ARG(n < (1ll << 31) - kIcpBlock * (kIcpMaxProblems + 1) && m < (1ll << 31) - 1, "apr_icp_batch: oversized clouds");
  AprArena arena(scratch);
  const IcpScratch w = icp_walk(arena, n, m, nb);
  APR_CHECK_ARG(scratch && arena.fits(scratch_bytes), "apr_icp_batch: scratch too small");
  IcpBatch sg;
  sg.nb = nb;
  sg.blk0[0] = 0;
  int32_t tlen[kIcpMaxProblems];
  for (int i = 0; i < nb; ++i) {
    const int seg = tgt_of_problem_host ? tgt_of_problem_host[i] : i;
    APR_CHECK_ARG(seg >= 0 && seg < n_tgt, "apr_icp_batch: problem %d names target segment %d of %d", i, seg, (int)n_tgt);
    sg.tseg[i] = seg;
    sg.a0[i] = (int)src_offsets_host[i];
    sg.blk0[i + 1] = sg.blk0[i] + (int)cdiv64(src_offsets_host[i + 1] - src_offsets_host[i], kIcpBlock);
  }
  sg.a0[nb] = (int)n;
  for (int i = 0; i <= n_tgt; ++i) {
    sg.b0[i] = (int)tgt_offsets_host[i];
    if (i) tlen[i - 1] = (int32_t)(tgt_offsets_host[i] - tgt_offsets_host[i - 1]);
  }
  const int nblk = sg.blk0[nb];

  const float rf = (float)max_dist;
  const float r2 = rf * rf;                      // the strict bound, in the precision of d^2
  AprSearchGrid g;
  int rc = apr_internal_search_grid_batch(tgt, m, tlen, n_tgt, rf * 1.01f, w.grid, &g, st);
  if (rc != APR_OK) return rc;
  hipLaunchKernelGGL(k_icp_pack, dim3((unsigned)cdiv64(m, 256)), dim3(256), 0, st, tgt, m, g, w.rows);
  hipLaunchKernelGGL(k_icp_init, dim3((unsigned)cdiv64(nb * APR_ICP_RECORD_DOUBLES, 256)), dim3(256), 0, st, init, (int)nb,
                     result, w.done);
  APR_LAUNCH_CHECK();

  // rounds 0 .. max_iteration; a look at the flags after every chunk, taken one chunk late so that the queue never drains
  static thread_local int* flags_host = nullptr;             // pinned, [2][kIcpMaxProblems], then the grid's status word
  if (!flags_host)
    APR_HIP(hipHostMalloc((void**)&flags_host, (2 * kIcpMaxProblems + 1) * sizeof(int), hipHostMallocDefault));
  int* grid_status = flags_host + 2 * kIcpMaxProblems;
  hipEvent_t ev[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k)
    if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) {
      if (k) (void)hipEventDestroy(ev[0]);
      apr_set_error("apr_icp_batch: hipEventCreate failed");
      return APR_EHIP;
    }
  const int rounds = max_iteration + 1;
  const int nchunk = (rounds + kIcpChunk - 1) / kIcpChunk;
  auto enqueue = [&](int c) -> int {
    const int r1 = (c + 1) * kIcpChunk < rounds ? (c + 1) * kIcpChunk : rounds;
    for (int r = c * kIcpChunk; r < r1; ++r) {
      hipLaunchKernelGGL(k_icp_assoc, dim3((unsigned)nblk), dim3(kIcpBlock), 0, st, src, (const float4*)w.rows, g, sg, r2,
                         (const double*)result, (const int*)w.done, w.partial, corr);
      hipLaunchKernelGGL(k_icp_update, dim3((unsigned)nb), dim3(kIcpBlock), 0, st, sg, (const double*)w.partial,
                         (int)max_iteration, relative_fitness, relative_rmse, g.status, result, w.done);
    }
    APR_LAUNCH_CHECK();
    APR_HIP(hipMemcpyAsync(flags_host + (c & 1) * kIcpMaxProblems, w.done, nb * sizeof(int), hipMemcpyDeviceToHost, st));
    if (c == 0) APR_HIP(hipMemcpyAsync(grid_status, g.status, sizeof(int), hipMemcpyDeviceToHost, st));
    APR_HIP(hipEventRecord(ev[c & 1], st));
    return APR_OK;
  };
  rc = enqueue(0);
  for (int c = 0; rc == APR_OK && c < nchunk; ++c) {
    if (c + 1 < nchunk) rc = enqueue(c + 1);
    if (rc != APR_OK) break;
    if (c + 1 == nchunk) break;                  // the last round finishes every problem: nothing left to decide
    rc = apr_event_wait(ev[c & 1], 20);
    if (rc != APR_OK) break;
    bool all = true;
    for (int i = 0; i < nb; ++i) all = all && flags_host[(c & 1) * kIcpMaxProblems + i] != 0;
    if (all) break;
  }
  // the pinned words are reused by the next call of this thread: what is still in flight must have landed before that
  if (rc == APR_OK && hipStreamSynchronize(st) != hipSuccess) {
    apr_set_error("apr_icp_batch: hipStreamSynchronize failed");
    rc = APR_EHIP;
  }
  // a flagged grid: every kernel after the build left at once (k_icp_pack), result holds init and corr was not written
  if (rc == APR_OK && *grid_status != 0) {
    if (*grid_status == 3)
      apr_set_error("apr_icp_batch: a target segment spans more than the cell range of the search grid, %d cells of 1.01 * "
                    "max_dist per axis (beyond it the 1 %% no longer covers the float32 rounding of the cell coordinate; "
                    "the packed key itself ends at %d)", APR_GRID_MARGIN_CELLS, APR_AXIS_BIAS);
    else
      apr_set_error("apr_icp_batch: search grid build failed, status %d (1: cell index outside the cell range of the "
                    "packed key, 2: cell table full)", *grid_status);
    rc = APR_ERANGE;
  }
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  return rc;
}

// The body of the loaders' __getitem__ on the device: open3d's voxel_down_sample (Predator_APR/datasets/kitti.py:464-475,
// 588-589 and the same lines of nuscenes.py), the loader's float64 augmentation (kitti.py:491-517) and the cloud mean of
// sample_random_trans (FCGF_APR/lib/complement_data_loader.py:33-38).
//
// open3d is not available to compare against, so the arithmetic below IS the restatement, float64
// throughout and every operation rounded on its own:
//   origin = (double)min - voxel * 0.5                     per cloud and axis (the fp32 minimum is exact)
//   index  = floor(((double)p - origin) / voxel)           a true division
//   sum    = 0.0; sum += (double)p                         over the voxel's rows in ASCENDING ROW ORDER (open3d's loop)
//   centroid = sum / (double)count
// Output rows: clouds in batch order, inside a cloud the voxels in ascending order of their first row -- the order in
// which apr_map_build numbers its cells, so a voxel's output row is its cell id and nothing is permuted afterwards.
//
// The buckets come from points.hip (apr_internal_buckets_*: cells -> apr_map_build -> count / scan / fill); k_fill leaves
// the rows of a cell in no particular order, so every cell is sorted by row before it is summed:
//   k_vox_sum     one WAVE per voxel of up to kVoxWaveCap rows: rank sort in LDS, the points staged kVoxStage rows at a
//                 time as fp32 (widening is exact: staging doubles would halve what fits and change no bit), lanes 0..2
//                 add the x, y, z chains;
//   k_vox_sum_big one 1024-thread workgroup per crowded voxel (the cells next to the sensor hold thousands of rows of a
//                 raw scan, tens of thousands of an aggregated cloud): bitonic sort in LDS up to kVoxBigLds rows and in
//                 place in global memory beyond, points staged kVoxBigStage rows at a time.
// No float atomics anywhere: a cloud gives the same bits alone and inside a batch, and from run to run.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBatch = 64;
constexpr int kVoxWaveCap = 1024;              // rows a wave sorts; more go to k_vox_sum_big
constexpr int kVoxStage = kVoxWaveCap / 3;     // 341 rows of 3 floats fit the wave's (dead) sort buffer
constexpr int kVoxBigLds = 8192;               // rows the big kernel sorts in LDS; more are sorted in global memory
constexpr int kVoxBigStage = 1024;             // rows it stages per round
constexpr double kVoxMaxIndex = 131071.0;      // APR_AXIS_RANGE - APR_AXIS_BIAS - 1: indices are >= 0 by construction


// The statements that carry the contract switch contraction off for their body (DESIGN sections 16, 18: the __d*_rn
// intrinsics are plain operators in this toolchain and fuse like any other expression).
__device__ inline double vox_origin(float lo, double voxel) {
#pragma clang fp contract(off)
  const double half = voxel * 0.5;
  return (double)lo - half;
}
__device__ inline double vox_index(float p, double origin, double voxel) {
#pragma clang fp contract(off)
  const double e = (double)p - origin;
  const double q = e / voxel;
  return floor(q);
}
__device__ inline double vox_add(double s, float p) {
#pragma clang fp contract(off)
  return s + (double)p;
}
__device__ inline double vox_centroid(double s, int count) {
#pragma clang fp contract(off)
  return s / (double)count;
}

__device__ inline int cloud_of(const int* __restrict__ starts, int nb, int i) {
  int b = 0;
  while (b + 1 < nb && i >= starts[b + 1]) ++b;
  return b;
}

// (cloud, ix, iy, iz) of every row.  A row with a non-finite coordinate, or whose index leaves [0, kVoxMaxIndex] (tested
// on the double, before any conversion to int), gets a coordinate outside the packed-key range: the cell map then files
// it nowhere and sets the status word.
__global__ void k_vox_coords(const float* __restrict__ pts, int64_t n, const int* __restrict__ starts, int nb,
                             const float* __restrict__ mins, double voxel, int4* __restrict__ coords) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b = cloud_of(starts, nb, (int)i);
  int c[3];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float p = pts[3 * i + d];
    const float lo = mins[3 * b + d];
    c[d] = 0;
    if (!isfinite(p) || !isfinite(lo)) {
      ok = false;
      continue;
    }
    const double q = vox_index(p, vox_origin(lo, voxel), voxel);
    if (q >= 0.0 && q <= kVoxMaxIndex) c[d] = (int)q;
    else ok = false;
  }
  coords[i] = ok ? make_int4(b, c[0], c[1], c[2]) : make_int4(b, APR_AXIS_RANGE, 0, 0);
}

__device__ inline void vox_store(int c, int lane, double s, int m, double* __restrict__ centroid,
                                 float* __restrict__ centroid32) {
  const double v = vox_centroid(s, m);
  if (centroid) centroid[3 * (int64_t)c + lane] = v;
  if (centroid32) centroid32[3 * (int64_t)c + lane] = (float)v;   // one rounding to nearest
}

__global__ __launch_bounds__(256) void k_vox_sum(const float* __restrict__ pts, const int* __restrict__ n_cells_dev,
                                                 const int* __restrict__ start, const int* __restrict__ sorted,
                                                 double* __restrict__ centroid, float* __restrict__ centroid32,
                                                 int* __restrict__ big_count, int* __restrict__ big_list) {
  __shared__ int s_raw[4][kVoxWaveCap];
  __shared__ int s_ord[4][kVoxWaveCap];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncell = *n_cells_dev;
  // grid-stride over the voxels (the host only knows an upper bound): wave-uniform loop, no workgroup barrier inside
  for (int c = blockIdx.x * 4 + wave; c < ncell; c += gridDim.x * 4) {
    const int lo = start[c], m = start[c + 1] - lo;
    if (m > kVoxWaveCap) {
      if (lane == 0) big_list[atomicAdd(big_count, 1)] = c;
      continue;
    }
    if (m == 1) {      // most voxels of the far field
      if (lane < 3) vox_store(c, lane, vox_add(0.0, pts[3 * (int64_t)sorted[lo] + lane]), 1, centroid, centroid32);
      continue;
    }
    // rank sort (k_barycentre's: a lane keeps up to 16 rows in registers, every LDS read is compared against all of them)
    int v[kVoxWaveCap / 64], rank[kVoxWaveCap / 64];
    __builtin_amdgcn_wave_barrier();       // the previous voxel's staged points are dead
#pragma unroll
    for (int u = 0; u < kVoxWaveCap / 64; ++u) {
      const int e = lane + 64 * u;
      v[u] = e < m ? sorted[lo + e] : 0x7fffffff;
      rank[u] = 0;
      if (e < m) s_raw[wave][e] = v[u];
    }
    __builtin_amdgcn_wave_barrier();
    const int nu = (m + 63) >> 6;          // wave-uniform
    for (int o = 0; o < m; ++o) {
      const int x = s_raw[wave][o];
#pragma unroll
      for (int u = 0; u < kVoxWaveCap / 64; ++u)
        if (u < nu) rank[u] += x < v[u] ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < kVoxWaveCap / 64; ++u)
      if (lane + 64 * u < m) s_ord[wave][rank[u]] = v[u];
    __builtin_amdgcn_wave_barrier();
    // the sort buffer is free again: all lanes fetch kVoxStage points into it, lanes 0..2 then add the three chains from LDS
    float* s_val = reinterpret_cast<float*>(s_raw[wave]);
    double acc = 0.0;
    for (int e0 = 0; e0 < m; e0 += kVoxStage) {
      const int cnt = m - e0 < kVoxStage ? m - e0 : kVoxStage;
      for (int e = lane; e < cnt; e += 64) {
        const int64_t i = s_ord[wave][e0 + e];
        s_val[3 * e] = pts[3 * i];
        s_val[3 * e + 1] = pts[3 * i + 1];
        s_val[3 * e + 2] = pts[3 * i + 2];
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < 3)
        for (int a = 0; a < cnt; ++a) acc = vox_add(acc, s_val[3 * a + lane]);
      __builtin_amdgcn_wave_barrier();
    }
    if (lane < 3) vox_store(c, lane, acc, m, centroid, centroid32);
  }
}

// k_barycentre_big's scheme: a bitonic network whose comparators all point the same way, so the padding up to a power
// of two is virtual (a missing upper element never moves down).
__global__ __launch_bounds__(1024) void k_vox_sum_big(const float* __restrict__ pts, const int* __restrict__ big_count,
                                                      const int* __restrict__ big_list, const int* __restrict__ start,
                                                      int* __restrict__ sorted, double* __restrict__ centroid,
                                                      float* __restrict__ centroid32) {
  __shared__ int s_keys[kVoxBigLds];
  __shared__ float s_val[3 * kVoxBigStage];
  const int nbig = *big_count;
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < nbig; b += gridDim.x) {   // workgroup-uniform
    const int c = big_list[b];
    const int lo = start[c], m = start[c + 1] - lo;
    int* glob = sorted + lo;
    const bool in_lds = m <= kVoxBigLds;
    if (in_lds)
      for (int e = t; e < m; e += 1024) s_keys[e] = glob[e];
    __syncthreads();
    int* arr = in_lds ? s_keys : glob;
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int k = 2; k <= np2; k <<= 1) {
      for (int i = t; i < (np2 >> 1); i += 1024) {       // the mirrored comparators of the merge
        const int blk = i / (k >> 1), off = i - blk * (k >> 1);
        const int a = blk * k + off, bb = blk * k + k - 1 - off;
        if (bb < m) {
          const int va = arr[a], vb = arr[bb];
          if (va > vb) {
            arr[a] = vb;
            arr[bb] = va;
          }
        }
      }
      __syncthreads();
      for (int j = k >> 2; j >= 1; j >>= 1) {            // the half-cleaners
        for (int i = t; i < (np2 >> 1); i += 1024) {
          const int a = (i / j) * 2 * j + (i % j), bb = a + j;
          if (bb < m) {
            const int va = arr[a], vb = arr[bb];
            if (va > vb) {
              arr[a] = vb;
              arr[bb] = va;
            }
          }
        }
        __syncthreads();
      }
    }
    double acc = 0.0;     // threads 0, 1, 2: the x, y, z chains
    for (int e0 = 0; e0 < m; e0 += kVoxBigStage) {
      const int cnt = m - e0 < kVoxBigStage ? m - e0 : kVoxBigStage;
      if (t < cnt) {
        const int64_t i = arr[e0 + t];
        s_val[3 * t] = pts[3 * i];
        s_val[3 * t + 1] = pts[3 * i + 1];
        s_val[3 * t + 2] = pts[3 * i + 2];
      }
      __syncthreads();
      if (t < 3)
        for (int a = 0; a < cnt; ++a) acc = vox_add(acc, s_val[3 * a + t]);
      __syncthreads();
    }
    if (t < 3) vox_store(c, t, acc, m, centroid, centroid32);
    __syncthreads();
  }
}

// count / first / index of every voxel, and the voxels per cloud: `first` ascends, so cloud b owns the voxels whose
// first row lies in [starts[b], starts[b + 1]) -- two binary searches, no atomics.
__global__ void k_vox_meta(const int* __restrict__ n_cells_dev, const int* __restrict__ start,
                           const long long* __restrict__ first64, const int4* __restrict__ cell_coords,
                           const int* __restrict__ starts, int nb, int* __restrict__ count, int* __restrict__ first,
                           int* __restrict__ index, int* __restrict__ lengths) {
  const int ncell = *n_cells_dev;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
    if (count) count[c] = start[c + 1] - start[c];
    if (first) first[c] = (int)first64[c];
    if (index) {
      const int4 k = cell_coords[c];
      index[3 * (int64_t)c] = k.y;
      index[3 * (int64_t)c + 1] = k.z;
      index[3 * (int64_t)c + 2] = k.w;
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < nb) {
    auto lower = [&](int v) {
      int lo = 0, hi = ncell;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (first64[mid] < v) lo = mid + 1;
        else hi = mid;
      }
      return lo;
    };
    lengths[threadIdx.x] = lower(starts[threadIdx.x + 1]) - lower(starts[threadIdx.x]);
  }
}

// ---- the loader's augmentation (kitti.py:491-517), one thread per coordinate triple --------------------------------
struct AugmentArgs {
  double noise, scale;
  double R[9];
  double shift[3];
  int rotate;
};

__global__ void k_sample_augment(const double* __restrict__ pts, const double* __restrict__ u, int64_t n, AugmentArgs a,
                                 float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double q[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double j = u[3 * i + d] - 0.5;
    const double jn = j * a.noise;
    q[d] = pts[3 * i + d] + jn;
  }
  if (a.rotate) {
    double r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double t0 = a.R[3 * j] * q[0];
      const double t1 = a.R[3 * j + 1] * q[1];
      const double t2 = a.R[3 * j + 2] * q[2];
      const double s01 = t0 + t1;
      r[j] = s01 + t2;
    }
    q[0] = r[0];
    q[1] = r[1];
    q[2] = r[2];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double s = q[d] * a.scale;
    const double v = s + a.shift[d];
    out[3 * i + d] = (float)v;
  }
}

// ---- float64 mean of a cloud: one workgroup, every thread sums its rows (stride 1024) in row order, then a fixed tree
constexpr int kMeanThreads = 1024;
__global__ __launch_bounds__(kMeanThreads) void k_cloud_mean(const float* __restrict__ pts, int64_t n,
                                                             double* __restrict__ mean) {
  __shared__ double s[3][kMeanThreads];
  const int t = threadIdx.x;
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t i = t; i < n; i += kMeanThreads)
#pragma unroll
    for (int d = 0; d < 3; ++d) a[d] += (double)pts[3 * i + d];
#pragma unroll
  for (int d = 0; d < 3; ++d) s[d][t] = a[d];
  __syncthreads();
  for (int w = kMeanThreads / 2; w >= 1; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int d = 0; d < 3; ++d) s[d][t] += s[d][t + w];
    }
    __syncthreads();
  }
  if (t < 3) mean[t] = s[t][0] / (double)n;
}

}  // namespace

namespace {
struct VoxelScratch {
  void* grid;           // points.hip's bucket build: its own carve
  long long* first64;   // [n] first row of every cell
};
VoxelScratch walk_voxel(AprArena& a, int64_t n) {
  VoxelScratch v;
  v.grid = a.take<char>(apr_internal_grid_bytes(n));
  v.first64 = a.take<long long>(n);
  return v;
}
}  // namespace

APR_API size_t apr_voxel_down_sample_scratch_bytes(int64_t n) {
  AprArena a(nullptr);
  walk_voxel(a, n < 1 ? 1 : n);
  return a.bytes();
}

APR_API int apr_voxel_down_sample(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, double voxel_size,
                                  double* centroid, float* centroid32, int32_t* count, int32_t* first, int32_t* index,
                                  int32_t* out_lengths_host, void* scratch, size_t scratch_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  APR_CHECK_ARG(pts && lengths_host && scratch && n > 0 && n < (1ll << 31) && nb > 0 && nb <= kMaxBatch &&
                    voxel_size > 0.0 && voxel_size < __builtin_inf(),
                "apr_voxel_down_sample: bad arguments");
  AprArena arena(scratch);
  const VoxelScratch v = walk_voxel(arena, n);
  APR_CHECK_ARG(arena.fits(scratch_bytes), "apr_voxel_down_sample: scratch too small");
  for (int b = 0; b < nb; ++b) APR_CHECK_ARG(lengths_host[b] > 0, "apr_voxel_down_sample: empty cloud in batch");
  AprCellBuckets g;
  int rc = apr_internal_buckets_begin(pts, n, lengths_host, nb, v.grid, &g, st);
  if (rc != APR_OK) return rc;
  long long* const first64 = v.first64;
  const unsigned nblk = (unsigned)cdiv64(n, kBlock);
  hipLaunchKernelGGL(k_vox_coords, dim3(nblk), dim3(kBlock), 0, st, pts, n, g.starts, nb, g.mins, voxel_size, g.coords);
  rc = apr_internal_buckets_finish(n, v.grid, (int64_t*)first64, st);
  if (rc != APR_OK) return rc;
  if (centroid || centroid32) {
    const unsigned grid = (unsigned)(cdiv64(n, 4) < 4096 ? cdiv64(n, 4) : 4096);
    hipLaunchKernelGGL(k_vox_sum, dim3(grid), dim3(256), 0, st, pts, g.n_cells, g.start, g.sorted, centroid, centroid32,
                       g.big_count, g.big_list);
    hipLaunchKernelGGL(k_vox_sum_big, dim3(64), dim3(1024), 0, st, pts, g.big_count, g.big_list, g.start, g.sorted,
                       centroid, centroid32);
  }
  const unsigned mgrid = (unsigned)(nblk < 1024 ? nblk : 1024);
  hipLaunchKernelGGL(k_vox_meta, dim3(mgrid), dim3(kBlock), 0, st, g.n_cells, g.start, first64, g.cell_coords, g.starts, nb,
                     count, first, index, g.spare);
  APR_LAUNCH_CHECK();
  int32_t host[kMaxBatch + 1];
  APR_HIP(hipMemcpyAsync(host, g.spare, nb * 4, hipMemcpyDeviceToHost, st));
  APR_HIP(hipMemcpyAsync(host + nb, g.status, 4, hipMemcpyDeviceToHost, st));
  APR_HIP(hipStreamSynchronize(st));
  if (host[nb] != 0) {
    apr_set_error("apr_voxel_down_sample: a row is not finite or its voxel index exceeds %d", (int)kVoxMaxIndex);
    return APR_ERANGE;
  }
  if (out_lengths_host) memcpy(out_lengths_host, host, nb * 4);
  return APR_OK;
}

APR_API int apr_sample_augment(const double* pts, const double* u, int64_t n, double noise, const double* rot_host,
                               double scale, const double* shift_host, float* out, void* stream) {
  APR_CHECK_ARG(n >= 0 && shift_host && (n == 0 || (pts && u && out)), "apr_sample_augment: bad arguments");
  if (n == 0) return APR_OK;
  AugmentArgs a;
  a.noise = noise;
  a.scale = scale;
  a.rotate = rot_host != nullptr;
  for (int k = 0; k < 9; ++k) a.R[k] = rot_host ? rot_host[k] : 0.0;
  for (int k = 0; k < 3; ++k) a.shift[k] = shift_host[k];
  hipLaunchKernelGGL(k_sample_augment, dim3((unsigned)cdiv64(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, pts, u, n,
                     a, out);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

APR_API int apr_cloud_mean(const float* pts, int64_t n, double* mean, void* stream) {
  APR_CHECK_ARG(pts && mean && n > 0, "apr_cloud_mean: bad arguments");
  hipLaunchKernelGGL(k_cloud_mean, dim3(1), dim3(kMeanThreads), 0, (hipStream_t)stream, pts, n, mean);
  APR_LAUNCH_CHECK();
  return APR_OK;
}

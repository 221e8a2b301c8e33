// Shared host/device helpers for libapr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/apr_hip.h"

// tuning / A-B switches read once from the environment
static inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

#define APR_API extern "C" __attribute__((visibility("default")))

void apr_set_error(const char* fmt, ...);

#define APR_CHECK_ARG(cond, ...)      \
  do {                                \
    if (!(cond)) {                    \
      apr_set_error(__VA_ARGS__);     \
      return APR_EINVAL;              \
    }                                 \
  } while (0)

#define APR_HIP(call)                                                            \
  do {                                                                           \
    hipError_t e_ = (call);                                                      \
    if (e_ != hipSuccess) {                                                      \
      apr_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return APR_EHIP;                                                           \
    }                                                                            \
  } while (0)

#define APR_LAUNCH_CHECK() APR_HIP(hipGetLastError())

static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- caller-owned scratch: every layout is ONE walk of an arena (DESIGN, "Scratch layouts") ----
__host__ __device__ static inline size_t apr_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The walk that sizes a scratch is the walk that carves it: on nullptr take() hands out nullptr and only counts.  Every
// region starts on a 256-byte boundary; bytes() allows for rounding an unaligned base up.  A region that another
// translation unit carves for itself is a take<char>() of that unit's own *_bytes().
struct AprArena {
  char* base;      // rounded up to 256; nullptr: sizing walk
  size_t off = 0;
  explicit AprArena(void* scratch) : base((char*)apr_align256((size_t)scratch)) {}
  template <typename T>
  T* take(size_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += apr_align256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off + 256; }
  bool fits(size_t scratch_bytes) const { return scratch_bytes >= bytes(); }
};

// match.hip: brute-force NN into an initialised `best`, run only if *run_if != 0 (NULL: always)
int apr_internal_nn_brute(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, uint64_t* best,
                          const unsigned* run_if, void* stream);

// hash.hip: memset as a kernel of the library's own (APR_FILL_KERNEL=0: hipMemsetAsync)
int apr_internal_fill(void* ptr, int32_t byte_value, size_t bytes, hipStream_t st);

// dense.hip: [M, cin] x [cin, cout] with the sparse conv's epilogue (identity kernel map); _ok = shape is supported
bool apr_internal_dense_ok(int64_t M, int32_t cin, int32_t cout);
int apr_internal_dense_g(int64_t M, int32_t cout);      // 1 / 2: k_dense_gemm<G>, 64 G rows per tile
bool apr_internal_dense_rows_route(int64_t M, int32_t cin, int32_t cout);      // dense_rows.hip
bool apr_internal_ws_bf3_only(const void* w_bf3, int32_t cin);                 // spconv_ws.hip
int apr_internal_dense_gemm(const float* in, int64_t ldi, int64_t M, int32_t cin, int32_t cout, const float* wp,
                            const float* scale, const float* shift, const float* residual, int64_t ldr, int32_t relu,
                            float* out, int64_t ldo, hipStream_t st);

// attention.hip: the training attention's kernels on the caller's operands -- P [heads, n, m] = softmax_j(<q_i, k_j> / sqrt(dim));
// out[i, ch] = scale * sum_j A[h, i, j] X[j, ch] (rowmat) and out[j, ch] = scale * sum_i A[h, i, j] X[i, ch] (colmat), h = ch % heads
int apr_internal_mha_probs(const float* q, const float* k, int32_t n, int32_t m, int32_t dim, int32_t heads, float* P, hipStream_t st);
int apr_internal_mha_rowmat(const float* A, const float* X, int32_t n, int32_t m, int32_t dim, int32_t heads, float scale, float* out,
                            hipStream_t st);
int apr_internal_mha_colmat(const float* A, const float* X, int32_t n, int32_t m, int32_t dim, int32_t heads, float scale, float* out,
                            hipStream_t st);

// spconv_bigk.hip: the tile family's kernel for 32 < K <= 125 (apr_spconv_bigk_supported shapes); _aligned = the 16-byte
// rows and vectors it loads and stores by
bool apr_internal_spconv_bigk_aligned(const apr_spconv_desc& d);
int apr_internal_spconv_bigk(const apr_spconv_desc& d, hipStream_t st);

// norm.hip: y = act((x - mean) * rstd (+ residual)) per row segment, mean / rstd rebuilt from per-block column sums
// partial[blk][2][c] (fp64; segment s owns blocks blk0[s] .. blk0[s + 1]) that another kernel left behind
int apr_internal_norm_apply_partials(const float* x, int64_t ldx, int32_t c, const int64_t* seg_row0, const int* seg_blk0,
                                     int32_t nseg, const double* partial, float eps, const float* residual, int64_t ldr,
                                     int32_t act_mode, float negative_slope, float* y, int64_t ldy, hipStream_t st);

#ifdef __HIPCC__
// Inclusive prefix sum over the 64 lanes with DPP adds only (no ds_bpermute round trips, ~6 VALU instead of 6
// LDS-crossbar shuffles): 4 shifts inside each row of 16 lanes, then the row totals are broadcast into the
// following rows (gfx9 row_bcast:15 / row_bcast:31).
__device__ inline int apr_wave_incl_scan(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, true);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, true);   // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, true);   // row_bcast:15 -> rows 1, 3
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, true);   // row_bcast:31 -> rows 2, 3
  return x;
}
#endif

// ---- packed voxel key: (b:10 | x:18 | y:18 | z:18), x/y/z biased by 2^17 ----
#define APR_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull
#define APR_AXIS_BIAS (1 << 17)
#define APR_AXIS_RANGE (1 << 18)

// batch index 1023 is reserved: (1023, max, max, max) would pack to APR_KEY_EMPTY
__host__ __device__ static inline bool apr_key_in_range(int b, int x, int y, int z) {
  return (unsigned)b < 1023u && (unsigned)(x + APR_AXIS_BIAS) < (unsigned)APR_AXIS_RANGE &&
         (unsigned)(y + APR_AXIS_BIAS) < (unsigned)APR_AXIS_RANGE &&
         (unsigned)(z + APR_AXIS_BIAS) < (unsigned)APR_AXIS_RANGE;
}

__host__ __device__ static inline uint64_t apr_pack_key(int b, int x, int y, int z) {
  return ((((uint64_t)(unsigned)b << 18 | (uint64_t)(unsigned)(x + APR_AXIS_BIAS)) << 18 |
           (uint64_t)(unsigned)(y + APR_AXIS_BIAS))
          << 18) |
         (uint64_t)(unsigned)(z + APR_AXIS_BIAS);
}

__host__ __device__ static inline uint32_t apr_hash_u64(uint64_t k) {
  // murmur3 finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

// floor division / floor-to-multiple for possibly negative ints, m > 0
__host__ __device__ static inline int apr_floor_to(int v, int m) {
  int q = v / m;
  if ((v % m) != 0 && v < 0) --q;
  return q * m;
}

// ---- internal helpers shared between translation units (not exported) ----
struct AprSearchGrid {
  const unsigned long long* keys;
  const int* vals;
  uint32_t mask;
  const int* start;   // [ncell + 1]
  const int* sorted;  // point indices bucketed by cell
  const float* mins;  // [3] cloud minimum = grid origin
  float cell;
  const int4* cell_coords;   // [n_cells] (cloud, cx, cy, cz) of every occupied cell, by cell id
  const int* n_cells;        // device-side count of occupied cells
  const int* status;         // device word, valid once the build has run: 0, or why the grid must not be searched --
                             // 1 / 2 from the cell map (key range, table full), 3 = a cell index >= APR_GRID_MARGIN_CELLS
};
// The search grids divide in fp32: a point's cell is floor(fl(fl(p - min) / cell)).  A caller that probes the 3^3 cells
// around a query for targets within r = cell / 1.01 (icp.hip) relies on the 1 % to cover that rounding.  Both roundings are
// relative (half an ulp of the extent, half an ulp of the quotient), so the quotient u is off by at most u * 2^-23 and the
// quotients of a query and of a target within reach differ by at most r / cell + (u_p + u_q) * 2^-23, where
// r / cell <= 0.9900992 (fl(1.01f), the rounded product, and the fp32 test d^2 < fl(r)^2 taken together).  The floors differ
// by at most 1 while that is <= 1, i.e. while u_p + u_q <= 0.0099008 * 2^23 = 83053: every cell index below 41526.
// Rounded down to 5 * 2^13; below the packed key's 2^17, so this is the limit that binds.
#define APR_GRID_MARGIN_CELLS 40960
size_t apr_internal_grid_bytes(int64_t n);
int apr_internal_search_grid(const float* pts, int64_t n, float cell, void* scratch, AprSearchGrid* out,
                             hipStream_t st);
int apr_internal_search_grid_batch(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, float cell, void* scratch,
                                   AprSearchGrid* out, hipStream_t st);
// points.hip: the same bucket build over cell coordinates of the caller's own making (voxel.hip).  Between _begin and
// _finish the caller's kernel writes coords[i] = (cloud, ix, iy, iz) for every row; a row whose coordinates leave the
// packed-key range belongs to no cell and sets the status word to 1.
struct AprCellBuckets {
  int4* coords;              // [n]   to be written by the caller
  const int* starts;         // [nb + 1] first row of every cloud
  const float* mins;         // [nb, 3] per-cloud minimum
  const int4* cell_coords;   // [n_cells] cells in ascending order of their first row
  const int* n_cells;
  const int* status;
  const int* start;          // [n_cells + 1]
  int* sorted;               // rows bucketed by cell, in no particular order inside a cell
  int* big_count;            // one zeroed word and n ints for a list of the caller's (crowded cells)
  int* big_list;
  int* spare;                // 64 ints, free after _finish
};
int apr_internal_buckets_begin(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, void* scratch,
                               AprCellBuckets* out, hipStream_t st);
int apr_internal_buckets_finish(int64_t n, void* scratch, int64_t* first, hipStream_t st);
// icp.hip: k_icp_pack on `st` -- rows[e] = (x, y, z, bits(global row)) of the target rows in bucket order, the layout
// k_icp_assoc probes; a grid whose status word is set is left alone.  Shared with posegraph.hip.
int apr_internal_icp_pack(const float* tgt, int64_t m, AprSearchGrid g, float4* rows, hipStream_t st);

__device__ static inline int apr_table_lookup(const unsigned long long* __restrict__ keys,
                                              const int* __restrict__ vals, uint32_t mask,
                                              unsigned long long key) {
  uint32_t slot = apr_hash_u64(key) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    unsigned long long k = keys[slot];
    if (k == key) return vals[slot];
    if (k == APR_KEY_EMPTY) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

/*
 * apr_hip.h -- C ABI of libapr_hip.so, the MI355X (gfx950) implementation of the
 * APR per-point feature-extraction hot path.
 *
 * Every entry point replaces one operator the reference reaches through a
 * Python binding of third-party or in-tree native code; the citation next to
 * each declaration is the reference interface it stands in for (paths relative
 * to /root/reference).  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     nothing synchronises unless the doc says so.
 *   - return value: 0 on success, negative APR_E* on error; apr_last_error()
 *     returns a message for the calling thread.
 *   - row-major tensors with an explicit leading dimension (`ld*`, in elements)
 *     so a conv can read from / write into a column slice of a wider buffer
 *     (fused ME.cat).
 */
#ifndef APR_HIP_H
#define APR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APR_OK 0
#define APR_EINVAL (-1)   /* bad argument / shape */
#define APR_EHIP (-2)     /* HIP runtime error */
#define APR_ETIMEOUT (-3) /* apr_event_wait_timeout: the event was not reached before the deadline */
#define APR_ERANGE (-3)   /* coordinate outside the packed-key range (apr_icp_batch: outside the search grid's cell range) */

const char* apr_last_error(void);
int apr_version(void);
/* Number of HIP devices visible; does not initialise a context. */
int apr_device_count(void);
/* sizeof of the structs of this header, in declaration order (apr_pair_desc, apr_spconv_desc, apr_resunet_layer,
 * apr_resunet_plan, apr_level_map, apr_pyramid, apr_kp_resnet_desc, apr_gcn_layer, apr_gcn_desc) -> out[0 .. n); returns how
 * many there are.  A binding compares them with its own layout at load time. */
int32_t apr_struct_sizes(int32_t* out, int32_t n);
/* Host wait for a HIP event (hipEvent_t) by hipEventQuery + nanosleep(poll_us): no spinning CPU (hipEventSynchronize spins on
 * this stack even for hipEventBlockingSync events) and, called through ctypes, no interpreter lock held while waiting.  The
 * reference's loop blocks in `.cpu()` / `.item()` at the same places (FCGF_APR/scripts/test_apr.py:137-146).
 * While it sleeps the calling thread's timer slack is 1 us (PR_SET_TIMERSLACK; the default 50 us would triple a 25 us poll);
 * the thread's previous value is restored before the call returns.
 * apr_event_wait_timeout: the same with a deadline (microseconds): APR_ETIMEOUT when the event has not been reached by then
 * (a wedged queue), so that a caller can report a hang instead of blocking for ever with the GIL released. */
int apr_event_wait(void* event, int32_t poll_us);
int apr_event_wait_timeout(void* event, int32_t poll_us, int64_t timeout_us);

/* ------------------------------------------------------------------------
 * Voxel hashing / coordinate maps
 *   replaces MinkowskiEngine's coordinate manager as used at
 *   FCGF_APR/scripts/test_apr.py:132-137 (ME.SparseTensor(F, coordinates=C)),
 *   FCGF_APR/lib/complement_data_loader.py:671-674,788-789
 *   (ME.utils.sparse_quantize(xyz / voxel_size, return_index=True)) and the
 *   implicit stride-2 maps of FCGF_APR/model/resunet.py:44,57,70.
 *
 * Key = (batch:10 | x:18 | y:18 | z:18) biased; open-addressing table of
 * `cap` (power of two, >= 2n) uint64 keys + int32 values.
 * ---------------------------------------------------------------------- */

/* Capacity (entries) the table needs for n coordinates. */
int64_t apr_hash_capacity(int64_t n);

/* Scratch bytes apr_map_build needs for n input rows. */
size_t apr_map_scratch_bytes(int64_t n);

/* xyz f32[n,3] -> coords i32[n,4] = (batch, floor(x/vs), floor(y/vs), floor(z/vs)),
 * fp32 division exactly as `xyz / voxel_size` on a float32 array: correctly rounded, denormal quotients kept
 * (a tiny negative x gives -1, -0.0 gives 0).  Every finite value whose quotient fits an int32 has a defined result,
 * in or out of the key range (apr_map_build reports the latter); inf and NaN have none. */
int apr_voxelize(const float* xyz, int64_t n, float voxel_size, int32_t batch,
                 int32_t* coords, void* stream);

/* Build one coordinate map.
 *   n_dev      nullable device row count: only min(n, *n_dev) rows are read, so a
 *              pyramid of maps can be chained without a host sync per level.
 *   coords_in  i32[n,4]; if `floor_to` > 0 the x,y,z columns are first floored to
 *              a multiple of `floor_to` (stride-2 map of a map at stride floor_to/2).
 *   keys/vals  hash table storage (cap entries each); on return the table maps
 *              key -> OUTPUT row index.
 *   out_coords i32[<=n,4]  unique coordinates in first-occurrence order.
 *   out_first  i64[<=n]    input row of each output row (nullable)
 *                          (== `index` of sparse_quantize(return_index=True)).
 *   n_out      i32[1]      device counter; read it back after a stream sync.
 *   status     i32[1]      device flag, set non-zero on key overflow (APR_ERANGE).
 * A live row outside the key range (batch < 0 or >= 1023, a floored x / y / z outside [-2^17, 2^17)) sets status and
 * belongs to no voxel; the rows in range still form the map they would form without it.  Rows at or past *n_dev are
 * never read: they may hold anything.  Rows of out_coords / out_first at or past *n_out are unspecified.
 */
int apr_map_build(const int32_t* coords_in, int64_t n, const int32_t* n_dev, int32_t floor_to,
                  uint64_t* keys, int32_t* vals, int64_t cap,
                  int32_t* out_coords, int64_t* out_first, int32_t* n_out,
                  int32_t* status, void* scratch, size_t scratch_bytes, void* stream);

/* Transpose of a kernel map: nbr i32[n_out, K] (rows of an n_in-row map, -1 = empty) -> nbr_t i32[n_in, K] with
 * nbr_t[i][k] = j  <=>  nbr[j][k] = i.  The table of a transposed (coarse -> fine) convolution is exactly the transpose
 * of the strided (fine -> coarse) table the encoder already built: a memset + one scatter instead of n_in * K hash
 * probes.  Requires that no (i, k) occurs twice in nbr (true for kernel maps). */
int apr_kernel_map_transpose(const int32_t* nbr, int64_t n_out, int32_t K, int64_t n_in, int32_t* nbr_t, void* stream);

/* apr_voxelize for the concatenated frames of a batch: point i gets batch index b with offsets[b] <= i < offsets[b+1]
 * (offsets i64[nseg+1] on the device, nseg <= 1023: batch index 1023 is reserved, its largest key is the empty-slot sentinel). */
int apr_voxelize_segments(const float* xyz, int64_t n, float voxel_size, const int64_t* offsets, int32_t nseg,
                          int32_t* coords, void* stream);

/* The same WITHOUT the concatenated copy (the reference voxelises frame by frame, FCGF_APR/lib/complement_data_loader.py:
 * 788-812; a batched step used to torch.cat its 2B frames first: 17 MB per 12-frame step): frames_host[b] = DEVICE pointer
 * of frame b (f32 [n_b, 3], contiguous), offsets_host[b] = points before frame b, offsets_host[nseg] = total; both arrays
 * live on the HOST and travel in the kernel arguments (nseg <= APR_MAX_FRAMES).  coords i32[total, 4] as
 * apr_voxelize_segments writes them; offsets_dev (nullable, i64[nseg + 1]) receives the offsets for apr_segment_counts.
 * apr_gather_frame_points: pts f32[*n_dev, 3] <- the input point behind every row of a map built with out_first over the
 * same frames (the representative point of each voxel, `xyz[sel]` of sparse_quantize(return_index=True)); n_max = rows
 * allocated for pts (>= *n_dev). */
#define APR_MAX_FRAMES 64
int apr_voxelize_frames(const float* const* frames_host, const int64_t* offsets_host, int32_t nseg, float voxel_size,
                        int32_t* coords, int64_t* offsets_dev, void* stream);
int apr_gather_frame_points(const float* const* frames_host, const int64_t* offsets_host, int32_t nseg,
                            const int64_t* out_first, const int32_t* n_dev, int64_t n_max, float* pts, void* stream);

/* Host-side glue of a step done by one launch instead of a chain of tensor ops: dst <- the concatenation of nsrc small
 * DEVICE int32 arrays (srcs_host[s][0 .. counts_host[s]); pointer and count arrays on the host, nsrc <= APR_MAX_PACK) --
 * the map sizes, status flags, per-frame row counts and bounding box that one device->host copy then brings over -- and
 * zero_words int32 words at zero_ptr cleared (nullable: the pair-list counters of the encode that follows).
 * apr_fill_bytes: hipMemsetAsync behind the C ABI (one fill for the three transposed tables of an encode, which
 * apr_kernel_map_transpose_prefilled then scatters into without a fill of its own). */
#define APR_MAX_PACK 96
int apr_pack_i32(const int32_t* const* srcs_host, const int32_t* counts_host, int32_t nsrc, int32_t* dst,
                 int32_t* zero_ptr, int64_t zero_words, void* stream);
int apr_fill_bytes(void* ptr, int32_t byte_value, size_t bytes, void* stream);
int apr_kernel_map_transpose_prefilled(const int32_t* nbr, int64_t n_out, int32_t K, int64_t n_in, int32_t* nbr_t,
                                       void* stream);

/* Rows per input segment of a map built over CONCATENATED point sets (a batch of frames voxelised in one build):
 * counts[b] = #{rows r < *n_dev : offsets[b] <= out_first[r] < offsets[b+1]}; out_first is ascending, the count
 * stays on the device so that it can be fetched together with the map sizes in the caller's single sync. */
int apr_segment_counts(const int64_t* out_first, const int32_t* n_dev, const int64_t* offsets, int32_t nseg,
                       int32_t* counts, void* stream);

/* Kernel map (neighbour table) of one sparse convolution:
 *   nbr[j, o] = row i of the input map with c_in[i] == c_out[j] + offset(o) * scale,
 *   or -1.  offset(o) enumerates {-h..h}^3 x fastest.  scale = +ts_in for a
 *   regular / strided conv; for a transposed conv pass the FINE map as
 *   out_coords, the COARSE table as the input table and scale = -ts_fine.
 *   A probed coordinate outside the key range ([-2^17, 2^17) per axis) is no row: -1, whatever its packed key
 *   would alias (the row across the range edge, the next batch index, the empty-slot sentinel).
 *   n_out_dev (nullable): device row count, rows >= *n_out_dev are skipped (their nbr entries are left untouched).
 *   replaces ME's kernel-map generation behind MinkowskiConvolution /
 *   MinkowskiConvolutionTranspose (FCGF_APR/model/resunet.py:31-140).
 */
/* The same table for a SAME-LEVEL map (input map == output map, scale = its tensor stride; the maps of every
 * stride-1 convolution of the network): nbr[j][o] = i <=> nbr[i][K-1-o] = j and the centre is the voxel itself, so
 * only the offsets below the centre are probed and each hit also stores its mirror entry — half the hash probes. */
int apr_kernel_map_same(const int32_t* coords, int64_t n, const uint64_t* keys, const int32_t* vals, int64_t cap,
                        int32_t kernel_size, int32_t scale, int32_t* nbr, void* stream);
int apr_kernel_map(const int32_t* out_coords, int64_t n_out, const int32_t* n_out_dev,
                   const uint64_t* in_keys, const int32_t* in_vals, int64_t cap,
                   int32_t kernel_size, int32_t scale, int32_t* nbr, void* stream);

/* ---- first convolution on constant-1 features (occ.hip) --------------------------------------------------------
 * FCGF feeds the encoder `feats = ones((n, 1))` (FCGF_APR/lib/complement_data_loader.py:805-812) into conv1 with
 * in_channels = 1 and a 5^3 / 7^3 kernel (FCGF_APR/model/resunet.py:57-63): every gathered value is 1, so the layer is
 *   out[j, :] = act((sum over the offsets k whose cell around voxel j is occupied of w[k, :]) * scale + shift)
 * and needs occupancy, not a neighbour table.  apr_coords_bbox: bbox_dev int32[8] <- {min x, y, z, max x, y, z, max
 * batch index, 0} of coords int32[n,4] (batch, x, y, z).  apr_occ_conv: the voxels are scattered into a bitmap over
 * that box (scratch: apr_occ_conv_scratch_bytes(bbox, ks), 0 = box empty / too large -> use apr_kernel_map +
 * apr_spconv; apr_occ_conv_pays(bbox, ks, n): 1 if the bitmap is also small against the n voxels it serves, at most
 * 1 KB per voxel + 4 MB -- an outlier voxel can stretch the box to gigabytes, and then the kernel map is the cheaper
 * structure) and every voxel reads the ks x-neighbours of a (dy, dz) row with one 8-byte load.  coords: unique rows;
 * bbox_host is in VOXEL units (the coords' own units) and must contain every row -- a row outside it is skipped as a
 * neighbour and gets a NaN output row, no access ever leaves the bitmap; offsets x-fastest as apr_kernel_map;
 * w f32[ks^3, cout], cout % 8 == 0, ks in {3, 5, 7}; same bits as apr_spconv over the apr_kernel_map table on all-ones
 * features. */
int apr_coords_bbox(const int32_t* coords, int64_t n, int32_t* bbox_dev, void* stream);
size_t apr_occ_conv_scratch_bytes(const int32_t* bbox_host, int32_t kernel_size);
int apr_occ_conv_pays(const int32_t* bbox_host, int32_t kernel_size, int64_t n);
int apr_occ_conv(const int32_t* coords, int64_t n, const int32_t* bbox_host, int32_t kernel_size, const float* w,
                 int32_t cout, const float* scale, const float* shift, const float* residual, int64_t ldr,
                 int32_t relu, float* out, int64_t ldo, void* scratch, size_t scratch_bytes, void* stream);
/* apr_kernel_map with the bitmap apr_occ_conv left in `occ_scratch` as a pre-filter of the probes (72 % of a LiDAR
 * map's probes hit an empty cell, the table's most expensive case): same table out, bit for bit.  bbox_host and
 * bitmap_kernel_size: those of the apr_occ_conv call that wrote occ_scratch (same stream, or ordered behind it);
 * in_keys / in_vals: the map the bitmap was built from; out_coords: that map's rows or a coarser map's.  Cells outside
 * the bitmap's box fall back to the table.  Replaces the same MinkowskiEngine kernel-map build as apr_kernel_map. */
int apr_kernel_map_occ(const int32_t* out_coords, int64_t n_out, const int32_t* n_out_dev, const uint64_t* in_keys,
                       const int32_t* in_vals, int64_t cap, int32_t kernel_size, int32_t scale,
                       const int32_t* bbox_host, int32_t bitmap_kernel_size, const void* occ_scratch, int32_t* nbr,
                       void* stream);

/* ------------------------------------------------------------------------
 * Sparse convolution forward (gather -> MFMA -> fused epilogue), fp32.
 *   out[j, :] = act( (sum_o in[nbr[j,o], :] @ W[o]) * scale + shift + residual[j, :] )
 *   replaces MinkowskiConvolution / MinkowskiConvolutionTranspose forward
 *   (+ the MinkowskiBatchNorm eval affine, residual add, MEF.relu and ME.cat
 *   around it: FCGF_APR/model/resunet.py:142-185, residual_block.py:37-53).
 *   nbr == NULL means K == 1 with the identity map (kernel_size 1: `F @ W`).
 * ---------------------------------------------------------------------- */

/* Floats needed for the packed copy of a [K,cin,cout] weight. */
int64_t apr_spconv_packed_size(int32_t K, int32_t cin, int32_t cout);
/* w f32[K,cin,cout] -> kernel-native layout (cin padded to a multiple of 4,
 * cout to a multiple of 16). */
int apr_spconv_pack_weights(const float* w, int32_t K, int32_t cin, int32_t cout,
                            float* w_packed, void* stream);

/* wt f32[K, cout, cin] = w[K, cin, cout] transposed per offset, offsets mirrored (k -> K-1-k) when flip != 0: the kernel
 * with which apr_spconv_fwd over the reverse map computes a convolution's INPUT gradient (same-level map: the same table
 * under the mirrored offset; strided <-> transposed maps: each other's table, no flip).  Backward of
 * ME.MinkowskiConvolution / ConvolutionTranspose under FCGF_APR/lib/complement_trainer.py:484. */
int apr_weights_flip_transpose(const float* w, int32_t K, int32_t cin, int32_t cout, int32_t flip, float* wt, void* stream);

int apr_spconv_fwd(const float* in, int64_t ldi, const int32_t* nbr, int64_t n_out,
                   int32_t K, int32_t cin, int32_t cout, const float* w_packed,
                   const float* scale, const float* shift,
                   const float* residual, int64_t ldr, int32_t relu,
                   float* out, int64_t ldo, void* stream);

/* Weight-stationary variant for maps with few pairs per output tile (strided / transposed convs, deep levels):
 * the kernel map is first turned into per-offset pair lists (apr_pairlist_build, once per map), then every
 * (offset, 64 pairs, 64 channels) work unit stages its weight piece once, writes per-pair products to
 * prod_scratch, and a second kernel sums them per output row in fixed offset order
 * with the same fused epilogue as apr_spconv_fwd.  Needs cin % 64 == 0, cin <= 512, cout % 64 == 0, K <= 27.
 * counters: int32[apr_pairlist_counter_ints()] = 32 counters APR_PAIR_COUNTER_STRIDE ints apart (the pair count of
 * offset k at counters[k * APR_PAIR_COUNTER_STRIDE]: one counter per 256 B, so the build's range reservations spread
 * over the L2 channels), ZERO before apr_pairlist_build (the caller clears them: one fill can clear the counters of
 * all maps of a forward pass); plist: apr_pairlist_bytes(n_out, K) bytes.
 * prod_scratch holds n_out*K rows of cout floats (offset k owns rows [k*n_out, (k+1)*n_out), sparsely used). */
#define APR_PAIR_COUNTER_STRIDE 64
int32_t apr_pairlist_counter_ints(void);
size_t apr_pairlist_bytes(int64_t n_out, int32_t K);
int apr_pairlist_build(const int32_t* nbr, int64_t n_out, int32_t K, int32_t* counters, void* plist,
                       size_t plist_bytes, void* stream);
int apr_spconv_ws_fwd(const float* in, int64_t ldi, const int32_t* counters, const void* plist, int64_t n_out,
                      int32_t K, int32_t cin,
                      int32_t cout, const float* w_packed, const float* scale, const float* shift,
                      const float* residual, int64_t ldr, int32_t relu, float* out, int64_t ldo,
                      float* prod_scratch, void* stream);
/* The same with the per-pair contraction on the bf16 MFMA in a 3-way split (hi/mid/lo bf16 pieces of every fp32
 * operand, 6 of the 9 cross terms: fp32-equivalent accuracy, ~2e-24 relative per product) - 2.7x fewer MFMA cycles
 * than the exact-fp32 form, which runs at 1/16 of the bf16 rate on gfx950.  w_bf3: apr_spconv_pack_weights_bf3 of the
 * layer's [K, cin, cout] kernel (apr_spconv_packed_bf3_bytes bytes; cin in {64, 128, 256}); NULL or another cin falls
 * back to w_packed / the fp32 form.  Packing takes cin % 64 == 0 and cout % 64 == 0; K = 1 (the dense layers'
 * images) also cin % 32 == 0 and cout % 16 == 0. */
int64_t apr_spconv_packed_bf3_bytes(int32_t K, int32_t cin, int32_t cout);
int apr_spconv_pack_weights_bf3(const float* w, int32_t K, int32_t cin, int32_t cout, void* w_bf3, void* stream);
/* The same image for the kernel of the INPUT GRADIENT, straight from the parameter: transposed != 0 reads w as f32
 * [K, cout, cin] (the image is that of its transpose), flip != 0 mirrors the offsets (k' = K - 1 - k: a same-level map's
 * reverse map) -- apr_weights_flip_transpose + apr_spconv_pack_weights_bf3 in one pass (the training step re-packs every
 * kernel after every optimizer step, FCGF_APR/lib/trainer.py:454-527).  w_bf3 16-byte aligned. */
int apr_spconv_pack_weights_bf3_ex(const float* w, int32_t K, int32_t cin, int32_t cout, int32_t flip, int32_t transposed,
                                   void* w_bf3, void* stream);
int apr_spconv_ws_fwd_bf3(const float* in, int64_t ldi, const int32_t* counters, const void* plist, int64_t n_out,
                          int32_t K, int32_t cin, int32_t cout, const float* w_packed, const void* w_bf3,
                          const float* scale, const float* shift, const float* residual, int64_t ldr, int32_t relu,
                          float* out, int64_t ldo, float* prod_scratch, void* stream);

/* Output-stationary form for the 64-channel levels (cin 64 or 128, cout % 64 == 0; same operator as apr_spconv_fwd,
 * FCGF_APR/model/resunet.py:31-140, model/residual_block.py:23-33): the kernel map is cut into tiles of R consecutive
 * output rows (R = apr_spconv_os_tile_rows, so that the tiles fill the chip in whole rounds), apr_spconv_os_pairs_build
 * turns each tile's [R, K] slab into K compact pair lists (deterministic positions, no atomics; input rows < 2^23), and
 * apr_spconv_os_fwd keeps a tile's fp32 accumulators in LDS while it walks the K offsets with the bf16-split weight
 * slice of the offset staged by LDS-DMA: no product row ever goes through HBM (apr_spconv_ws_fwd writes and re-reads
 * one per pair).  bf16 MFMA in the exact 3-way split (fp32-equivalent), sums in ascending offset order: bitwise
 * reproducible.  w_bf3 = apr_spconv_pack_weights_bf3(w, K, cin, cout). */
int32_t apr_spconv_os_tile_rows(int64_t n_out, int32_t cin, int32_t cout);
size_t apr_spconv_os_pairs_bytes(int64_t n_out, int32_t K, int32_t R);
int apr_spconv_os_pairs_build(const int32_t* nbr, int64_t n_out, int64_t n_in, int32_t K, int32_t R, void* os_pairs,
                              size_t os_pairs_bytes, void* stream);
/* Diagnostics for apr_spconv_os_fwd (APR_OS_TRACE=1 in the environment): per-wave s_memtime stamps of one workgroup of
 * the last launch, host_out[8 * 512] (tag << 56 | cycles; entry 511 of each wave = count). */
int apr_spconv_os_trace(uint64_t* host_out, int32_t n);
/* Run-time guard of k_os_conv's hand-counted load pipeline: 0 = production kernel, 1 = the diagnostics instantiation with
 * no ablation, 2 = the same with a full drain (s_waitcnt vmcnt(0)) in front of every counted wait.  The three must give
 * identical bits (tests/test_spconv_gpu.py::test_os_conv_debug_pipeline_matches_production); process-wide switch. */
int apr_spconv_os_set_debug(int32_t mode);
int apr_spconv_os_fwd(const float* in, int64_t ldi, const void* os_pairs, int64_t n_out, int32_t K, int32_t R,
                      int32_t cin, int32_t cout, const void* w_bf3, const float* scale, const float* shift,
                      const float* residual, int64_t ldr, int32_t relu, float* out, int64_t ldo, void* stream);

/* Weight gradient of apr_spconv_fwd (training; replaces what autograd does inside
 * MinkowskiConvolution / MinkowskiConvolutionTranspose, FCGF_APR/lib/trainer.py:454-527):
 *   dw f32[K, cin, cout] (plain layout, not packed) = sum_j [nbr[j,k] >= 0] in[nbr[j,k], :]^T dout[j, :].
 * nbr NULL = identity map (K = 1).  Deterministic (per-chunk partial sums reduced in fixed order).
 * The input gradient is apr_spconv_fwd itself: dout over the reverse map with transposed weights. */
size_t apr_spconv_wgrad_scratch_bytes(int64_t n_out, int32_t K, int32_t cin, int32_t cout);
int apr_spconv_wgrad(const float* in, int64_t ldi, const float* dout, int64_t ldo, const int32_t* nbr, int64_t n_out,
                     int32_t K, int32_t cin, int32_t cout, float* dw, void* scratch, size_t scratch_bytes,
                     void* stream);
/* The same when nbr is a SAME-LEVEL map (stride 1, odd kernel: the centre column holds every row, the others about a
 * quarter): the centre offset's rows are spread over four times as many workgroups.  Identical sums, another grouping of
 * the partials (results differ from apr_spconv_wgrad in the last bits; each entry point is bit-reproducible). */
int apr_spconv_wgrad_same_level(const float* in, int64_t ldi, const float* dout, int64_t ldo, const int32_t* nbr,
                                int64_t n_out, int32_t K, int32_t cin, int32_t cout, float* dw, void* scratch,
                                size_t scratch_bytes, void* stream);
/* What the two entry points launch for these operands (host only, no HIP call; the launcher follows it):
 * plan[6] = {kernel, CI, CO, S_all, S_c, k_c}.  APR_WGRAD_BF3: k_wgrad_bf3<CI, CO> on the bf16 split, S_all splits of the
 * 512-row blocks per offset, S_c for the centre offset k_c of a same-level map (k_c = -1: no such offset).
 * APR_WGRAD_PARTIAL: the fp32 k_wgrad_partial (rows of in / dout not 16-byte aligned, or a width off the 32-channel
 * granule): CI = CO = 64, S_all = S_c = the number of 512-row chunks, k_c = -1.  in / dout are looked at for alignment only. */
enum { APR_WGRAD_BF3 = 1, APR_WGRAD_PARTIAL = 2 };
int apr_spconv_wgrad_plan(const float* in, int64_t ldi, const float* dout, int64_t ldo, int64_t n_out, int32_t K,
                          int32_t cin, int32_t cout, int32_t same_level, int32_t* plan);

/* Triple pair lists for 27-offset maps (spconv_ws.hip): offsets are x fastest, so k = 3t + j are the three x-neighbours of
 * one (dy, dz); an ENTRY of triple t is an output row with its up to three input rows, and the gemm writes ONE product
 * row per entry (about half as many as pairs on LiDAR surfaces), accumulating the three offsets in registers -- the
 * product round trip that bounds the weight-stationary pair halves.  Same operator and epilogue as apr_spconv_ws_fwd_bf3
 * (FCGF_APR/model/resunet.py:31-140); counters: a zeroed apr_pairlist_counter_ints() block; prod_scratch f32
 * [9 * n_out, cout]; cin 64 / 128, cout % 64 == 0 (apr_spconv_ws3_supported). */
size_t apr_pairlist3_bytes(int64_t n_out);
int apr_pairlist3_build(const int32_t* nbr, int64_t n_out, int32_t K, int32_t* counters, void* plist3, size_t plist3_bytes,
                        void* stream);
int apr_spconv_ws3_supported(int32_t K, int32_t cin, int32_t cout);
int apr_spconv_ws3_fwd_bf3(const float* in, int64_t ldi, const int32_t* counters, const void* plist3, int64_t n_out,
                           int32_t cin, int32_t cout, const void* w_bf3, const float* scale, const float* shift,
                           const float* residual, int64_t ldr, int32_t relu, float* out, int64_t ldo, float* prod_scratch,
                           void* stream);

/* One launch description of apr_spconv_fwd; apr_spconv_fwd_batch enqueues n of them back to back
 * from a single call (the 23 fused conv launches of one ResUNet encode), so a host binding pays
 * one FFI transition instead of 23 and can overlap several encodes from different host threads. */
typedef struct apr_spconv_desc {
  const float* in; int64_t ldi; const int32_t* nbr; int64_t n_out;
  int32_t K, cin, cout, relu;
  const float* w_packed; const float* scale; const float* shift;
  const float* residual; int64_t ldr;
  float* out; int64_t ldo;
  /* What the caller has for this layer; which of it a launch uses is apr_spconv_route's decision (below). */
  int32_t* counters;      /* pair-list counters and ... */
  void* plist;            /* ... body (apr_pairlist_build; with ws3: apr_pairlist3_build), with ... */
  float* prod_scratch;    /* ... the product buffer of the weight-stationary families (n_out*K rows; ws3: 9 * n_out) */
  int64_t plist_bytes;    /* > 0: the routed family builds plist from nbr first (first use of the map in the batch) */
  const void* w_bf3;      /* the bf16-split weights (apr_spconv_pack_weights_bf3) */
  void* os_pairs;         /* the output-stationary tile lists of nbr, */
  int64_t os_rows;        /* ... of os_rows rows per tile; */
  int64_t os_build_bytes; /* > 0: apr_spconv_os_pairs_build(nbr -> os_pairs, n_in = os_n_in) first */
  int64_t os_n_in;
  int32_t l2norm;         /* != 0: out[j, :] /= |out[j, :]|_2 behind the epilogue (the encoder's normalize_feature,
                           * FCGF_APR/model/resunet.py:139-142): in the tile / dense-rows kernel's epilogue where that
                           * kernel holds the whole row (same bits as apr_l2_normalize), else as a second launch */
  int32_t ws3;            /* != 0: plist is a TRIPLE pair list */
} apr_spconv_desc;
/* The kernel family a descriptor's launch runs through -- the ONLY place that decides it ("How a conv layer is
 * routed"; apr_spconv_fwd_batch switches on it).  Host only: no HIP call, no device needed; reads the shape fields, the
 * leading dimensions, pointer alignment and which pointers are non-NULL, never w_packed -- a caller asks first and builds
 * the tile pack only for APR_ROUTE_TILE / APR_ROUTE_WS.  >= 0: a route id; < 0: APR_EINVAL, apr_last_error() says why (ws3
 * set on a weight-stationary shape that the triple lists do not cover, or without w_bf3). */
enum {
  APR_ROUTE_TILE = 0,   /* apr_spconv_fwd (with its own choice among the pairs / mfma / small-cin / generic / dense kernels) */
  APR_ROUTE_WS,         /* apr_spconv_ws_fwd: fp32 weight-stationary, reads w_packed */
  APR_ROUTE_WS_BF3,     /* apr_spconv_ws_fwd_bf3 on the split weights alone */
  APR_ROUTE_WS3,        /* apr_spconv_ws3_fwd_bf3 */
  APR_ROUTE_OS,         /* apr_spconv_os_fwd */
  APR_ROUTE_DENSE_ROWS, /* apr_dense_rows_bf3 */
  APR_ROUTE_DENSE_GEMM  /* apr_dense_gemm_bf3 */
};
int32_t apr_spconv_route(const apr_spconv_desc* d);
/* 1 if the weight-stationary families take the shape: K <= 27, cin % 64 == 0, cin <= 512, cout % 64 == 0. */
int32_t apr_spconv_ws_supported(int32_t K, int32_t cin, int32_t cout);
/* 1 if, inside APR_ROUTE_TILE, apr_spconv_fwd runs the shape on the big-kernel MFMA kernel (spconv_bigk.hip) instead of the
 * generic one: 32 < K <= 125, cin % 32 == 0, cout % 32 == 0 (a 5^3 kernel over real channels: the symmetric recipe's
 * generator conv1, FCGF_APR/lib/complement_trainer.py:52-60, and its input gradient).  Reads the plain [K, cin, cout]
 * buffer that apr_spconv_pack_weights leaves for K > 32. */
int32_t apr_spconv_bigk_supported(int32_t K, int32_t cin, int32_t cout);
/* Inside APR_ROUTE_TILE: the kernel and template instance that apr_spconv_fwd launches for a descriptor (d->l2norm says
 * whether the rows are to be normalised).  Host only, no HIP call; the launcher switches on this id and on nothing else.
 * id = APR_TILE_ID(kernel, TM, CN, CK) [| APR_TILE_FLAG] [| APR_TILE_NW8]:
 *   APR_TILE_PAIRS     k_spconv_pairs<TM, CN, CK, 4>; FLAG: the row normalisation rides in its epilogue; NW8: the 8-wave form
 *   APR_TILE_MFMA      k_spconv_mfma<TM, CN, .., CK> (out / residual rows not 16-byte aligned, or K 28..32)
 *   APR_TILE_DENSE     k_dense_gemm<TM / 64> (identity map, K = 1, enough workgroups); CN = CK = 64
 *   APR_TILE_BIGK      spconv_bigk.hip (32 < K <= 125 over real channels)
 *   APR_TILE_SMALLCIN  k_spconv_smallcin<CK> (cin 1 / 3): TM = 64 rows per workgroup, CN = 0
 *   APR_TILE_GENERIC   k_spconv_generic
 * APR_TILE_NONE (0): no rows, nothing is launched.  < 0: APR_EINVAL (a bad shape; an MFMA-shaped layer whose INPUT rows are
 * not 16-byte aligned), apr_last_error() says why.  apr_dense_gemm_bf3_variant: the same for apr_dense_gemm_bf3, kernel
 * APR_TILE_DENSE_BF3, TM 64 / 128, FLAG: the rows are staged through LDS (cin >= 128). */
enum { APR_TILE_NONE = 0, APR_TILE_PAIRS, APR_TILE_MFMA, APR_TILE_DENSE, APR_TILE_BIGK, APR_TILE_SMALLCIN, APR_TILE_GENERIC,
       APR_TILE_DENSE_BF3 };
#define APR_TILE_ID(kernel, tm, cn, ck) (((kernel) << 24) | ((tm) << 14) | ((cn) << 7) | (ck))
#define APR_TILE_FLAG (1 << 22)
#define APR_TILE_NW8 (1 << 23)
#define APR_TILE_KERNEL(id) ((id) >> 24)
#define APR_TILE_TM(id) (((id) >> 14) & 255)
#define APR_TILE_CN(id) (((id) >> 7) & 127)
#define APR_TILE_CK(id) ((id) & 127)
int32_t apr_spconv_tile_variant(const apr_spconv_desc* d);
int32_t apr_dense_gemm_bf3_variant(int64_t M, int32_t cin, int32_t cout);
int apr_spconv_fwd_batch(const apr_spconv_desc* descs_host, int32_t n, void* stream);
/* Same, with one HIP event pair per launch recorded on `stream` (around the conv kernels only, not a pair-list
 * build); synchronises and returns each layer's elapsed milliseconds in layer_ms[n].  Measurement aid
 * (bench.py's roofline leg): back-to-back launches from C, no host gaps inside a layer. */
int apr_spconv_fwd_batch_timed(const apr_spconv_desc* descs, int32_t n, float* layer_ms, void* stream);

/* ------------------------------------------------------------------------
 * One ResUNet encode as ONE call (round 4): ResUNet2.forward in eval mode, FCGF_APR/model/resunet.py:142-191, over the
 * four coordinate maps of a batch -- conv1 on the occupancy bitmap, the 7 + 3 kernel maps, the pair lists of every routed
 * layer and the 23 conv launches are enqueued from C over one scratch arena.  The kernels, their arguments and their order
 * are those of the module-by-module plan (apr_amd/fcgf/model/resunet.py forward_fused): same bits.  Python needed ~0.8 ms
 * per encode to issue the same ~60 launches; with one pair per call (the reference loop's shape, test_apr.py:111-163) the
 * host, not the GPU, set the pace.
 *   layer[3 s + 0 / 1 / 2]: stage s = "1", "2", "3", "4", "4_tr", "3_tr", "2_tr": its (strided / transposed) conv with
 *   the folded BN, then the two convs of its residual block; layer[21] = conv1_tr, layer[22] = final.
 *   ws_conv / ws_block / os_block: bit s = stage s takes the weight-stationary / output-stationary kernels where the
 *   shape allows (else the tile kernel).  lv[l]: the map of tensor stride 2^l (coords int32[n, 4], the hash table, n).
 *   counters: apr_pairlist_counter_ints() x n_counter_slots int32, ZERO on entry (one block per pair list; NULL: a
 *   block of the arena is cleared with one fill).  bbox_host: apr_coords_bbox of lv[0] (or a superset).
 *   apr_resunet_encode_supported: 1 if the occupancy form of conv1 applies (apr_occ_conv_pays) and every map is
 *   non-empty; otherwise the caller runs the module-by-module plan. */
typedef struct apr_resunet_layer {
  int32_t K, cin, cout, relu;
  const float* w_packed;          /* apr_spconv_pack_weights image */
  const void* w_bf3;              /* apr_spconv_pack_weights_bf3 image, or NULL */
  const float* scale; const float* shift;     /* folded BatchNorm / bias, nullable */
} apr_resunet_layer;
typedef struct apr_resunet_plan {
  apr_resunet_layer layer[23];
  const float* conv1_w;           /* conv1's raw kernel f32 [ks^3, cout] (occupancy form) */
  int32_t conv1_ks, normalize;
  uint32_t ws_conv, ws_block, os_block;
  int32_t ws3, ws3_cin128, os_min_rows, occ_kernel_map;
  int64_t ws3_max_rows_128;
} apr_resunet_plan;
typedef struct apr_level_map {
  const int32_t* coords; const uint64_t* keys; const int32_t* vals; int64_t cap; int64_t n;
} apr_level_map;
int apr_resunet_encode_supported(const apr_resunet_plan* plan, const apr_level_map* lv, const int32_t* bbox_host);
size_t apr_resunet_encode_scratch_bytes(const apr_resunet_plan* plan, const apr_level_map* lv, const int32_t* bbox_host);
int apr_resunet_encode(const apr_resunet_plan* plan, const apr_level_map* lv, const int32_t* bbox_host, int32_t* counters,
                       int32_t n_counter_slots, void* scratch, size_t scratch_bytes, float* out, int64_t ldo, void* stream);

/* The front end of a step as ONE call: frames -> voxel coordinates -> the de-duplicated stride-1 map (its rows in first-
 * occurrence order = frame order, the representative input point of every row, rows per frame, bounding box) -> that map
 * re-inserted into a table of its own size -> the three coarser maps, chained on device-side row counts -> ONE int32
 * header with everything the host needs, ready for a single device -> host copy.  Replaces ME.utils.sparse_quantize +
 * batched_coordinates + the coordinate manager's strided maps (FCGF_APR/lib/complement_data_loader.py:776-812,
 * FCGF_APR/scripts/test_apr.py:120-131) for a batch of frames; the kernels and their order are those of the tensor-by-
 * tensor front end (apr_voxelize_frames, apr_map_build x 5, apr_segment_counts, apr_coords_bbox, apr_gather_frame_points,
 * apr_pack_i32): same bits.  Python needed ~45 allocations and a dozen calls for it, and with one pair per call the GPU
 * idled between its kernels.
 *   arena: apr_voxel_pyramid_scratch_bytes(total points, nseg) bytes; every pointer of *out points into it.
 *   out->lv[l]: level l's map; lv[l].n = rows ALLOCATED (the true count is in the header).  out->header (device):
 *   int32 {n, status} x 5 maps (levels 0..3, then the de-duplicating table when compact != 0, else zeros), rows per frame
 *   [nseg], bounding box [8]; header_ints of them.  status != 0: a coordinate outside the packed key range.
 *   compact != 0: level 0 is the compact table over the first compact_rows rows of the de-duplicated map; if the header
 *   says the de-duplicated map has MORE rows than that (more than a quarter of the points are distinct voxels: never on
 *   LiDAR input) the caller must rebuild through the tensor-by-tensor path.
 *   out->counters: apr_pairlist_counter_ints() x 16 int32, zeroed (for apr_resunet_encode). */
typedef struct apr_pyramid {
  apr_level_map lv[4];
  const int64_t* first;           /* [rows allocated] index of the first input point of every level-0 row */
  const float* pts;               /* [rows allocated, 3] that point */
  int32_t* header; int32_t header_ints;
  int32_t compact; int64_t compact_rows;
  int32_t* counters; int32_t n_counter_slots;
} apr_pyramid;
size_t apr_voxel_pyramid_scratch_bytes(int64_t n_points, int32_t nseg);
int apr_voxel_pyramid(const float* const* frames_host, const int64_t* offsets_host, int32_t nseg, float voxel_size,
                      void* arena, size_t arena_bytes, apr_pyramid* out, void* stream);

/* ------------------------------------------------------------------------
 * Normalisation / elementwise on feature rows [n, c]
 * ---------------------------------------------------------------------- */

/* Per-channel batch statistics over rows (training-mode MinkowskiBatchNorm,
 * FCGF_APR/model/common.py:6): mean[c], biased var[c].  fp64 accumulation. */
int apr_bn_stats(const float* x, int64_t ld, int64_t n, int32_t c,
                 float* mean, float* var, void* scratch, size_t scratch_bytes, void* stream);
size_t apr_bn_stats_scratch_bytes(int64_t n, int32_t c);

/* Backward of y = (x - mean) * rstd * gamma + beta over all n rows (training-mode MinkowskiBatchNorm,
 * FCGF_APR/model/common.py:6 under FCGF_APR/lib/trainer.py:454-527; gamma = NULL: the affine-free InstanceNorm1d of
 * KPFCNN's blocks, Predator_APR/models/blocks.py:459-468 under Predator_APR/lib/trainer.py:142-280): dx, and (non-NULL)
 * dgamma[c], dbeta[c].  mean / rstd: the forward's batch statistics (rstd = 1 / sqrt(var + eps)).  fp64 partial sums
 * combined in fixed order: deterministic. */
size_t apr_norm_backward_scratch_bytes(int64_t n, int32_t c);
int apr_norm_backward(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t n, int32_t c,
                      const float* mean, const float* rstd, const float* gamma, float* dx, int64_t lddx,
                      float* dgamma, float* dbeta, void* scratch, size_t scratch_bytes, void* stream);

/* Training-mode BatchNorm fused with the residual add and the ReLU -- the unit a training encode repeats per convolution
 * (MinkowskiBatchNorm in train(), FCGF_APR/model/common.py:6, model/residual_block.py:37-53, under
 * lib/complement_trainer.py:350-512 / lib/trainer.py:454-527):
 *   y = act((z - mean) * rstd * gamma + beta (+ residual)),  mean / biased var over the n rows (fp64 partial sums);
 *   running_mean / running_var (nullable pair) updated in place as torch.nn.BatchNorm1d does (momentum, unbiased var);
 *   save_mean / save_rstd [c] kept for the backward; *num_batches_tracked (nullable device int64) += 1.  relu: 0 / 1.
 *   Two launches.  scratch: apr_bn_stats_scratch_bytes.
 * apr_bn_train_bwd: g = dy masked by y > 0 (relu = 1); dres (nullable) = g, the residual branch's gradient;
 *   dgamma = sum g * xhat, dbeta = sum g (nullable); dx = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)).
 *   Partial sums in fp64 combined in a fixed order: the same bits every run.  Two launches.
 * seg_offsets_host (int64 [nseg + 1], 0 .. n; NULL / nseg <= 1: one segment): the rows of several forward calls of the
 *   reference stacked into one launch -- the two frames of a pair, FCGF_APR/lib/complement_trainer.py:386-394 -- each
 *   normalised with its own statistics (save_mean / save_rstd [nseg, c]); the running statistics take the segments'
 *   updates in order and *num_batches_tracked += nseg, exactly as consecutive calls would; dgamma / dbeta sum over all
 *   segments.  scratch: apr_bn_stats_scratch_bytes(n + 256 * nseg, c). */
int apr_bn_train_fwd(const float* z, int64_t ldz, int64_t n, int32_t c, const float* gamma, const float* beta,
                     float eps, float momentum, float* running_mean, float* running_var, const float* residual,
                     int64_t ldr, int32_t relu, float* y, int64_t ldy, float* save_mean, float* save_rstd,
                     int64_t* num_batches_tracked, const int64_t* seg_offsets_host, int32_t nseg, void* scratch,
                     size_t scratch_bytes, void* stream);
int apr_bn_train_bwd(const float* z, int64_t ldz, const float* y, int64_t ldy, const float* dy, int64_t lddy,
                     int64_t n, int32_t c, const float* mean, const float* rstd, const float* gamma, int32_t relu,
                     float* dx, int64_t lddx, float* dres, int64_t lddres, float* dgamma, float* dbeta,
                     const int64_t* seg_offsets_host, int32_t nseg, void* scratch, size_t scratch_bytes, void* stream);

/* sums[c] = sum over the n rows of x[:, c] (same scratch as apr_bn_stats; fp64 partial sums in fixed order): the bias
 * gradient of the 1x1 convolutions with bias in KPFCNN's training path (Predator_APR/models/architectures.py:92-101 under
 * lib/trainer.py:142-280). */
int apr_col_sums(const float* x, int64_t ld, int64_t n, int32_t c, float* sums, void* scratch, size_t scratch_bytes,
                 void* stream);

/* Per-channel normalisation parameters over all rows, no affine: scale = 1/sqrt(var + eps),
 * shift = -mean*scale (InstanceNorm1d over the stacked points, Predator_APR/models/blocks.py:451-466;
 * InstanceNorm2d of the edge convolutions, models/gcn.py:41-48).  Same scratch as apr_bn_stats. */
int apr_norm_params(const float* x, int64_t ld, int64_t n, int32_t c, float eps, float* scale, float* shift,
                    void* scratch, size_t scratch_bytes, void* stream);

/* apr_norm_params + apr_affine_act in one call and two launches (statistics, then rebuild-and-apply): y = act((x -
 * mean) / sqrt(var + eps) (+ residual)) per channel over all rows: the InstanceNorm1d + LeakyReLU / residual that
 * follows every Linear and KPConv of KPFCNN (Predator_APR/models/blocks.py:451-468,499-504,653-681).  51 of them per
 * forward: the pair path is bound by the host cost of its ~600 launches.  Same scratch as apr_bn_stats. */
int apr_instance_norm_act(const float* x, int64_t ldx, int64_t n, int32_t c, float eps, const float* residual,
                          int64_t ldr, int32_t relu, float negative_slope, float* y, int64_t ldy, void* scratch,
                          size_t scratch_bytes, void* stream);
/* The same per row segment [seg_offsets_host[s], seg_offsets_host[s+1]) (int64, 0 .. n): several scan pairs stacked into
 * one KPFCNN forward keep the reference's statistics (over the stacked points of ONE pair).  scratch:
 * apr_bn_stats_scratch_bytes(n + 256 * nseg, c). */
int apr_instance_norm_act_seg(const float* x, int64_t ldx, int64_t n, int32_t c, float eps, const float* residual,
                              int64_t ldr, int32_t relu, float negative_slope, float* y, int64_t ldy,
                              const int64_t* seg_offsets_host, int32_t nseg, void* scratch, size_t scratch_bytes,
                              void* stream);

/* y = act(x * scale[c] + shift[c] (+ residual)); scale/shift/residual nullable.
 * relu: 0 none, 1 ReLU, 2 LeakyReLU(negative_slope) (Predator_APR/models/blocks.py:489,574). */
int apr_affine_act(const float* x, int64_t ldx, int64_t n, int32_t c,
                   const float* scale, const float* shift,
                   const float* residual, int64_t ldr, int32_t relu, float negative_slope,
                   float* y, int64_t ldy, void* stream);
/* Backward of that activation from its OUTPUT y: dz = dy where y > 0, dy * negative_slope (mode 2) or 0 (mode 1) elsewhere;
 * mode 0 copies (training path: Predator_APR/models/blocks.py:459-468 under lib/trainer.py:142-280). */
int apr_act_backward(const float* dy, int64_t lddy, const float* y, int64_t ldy, int64_t n, int32_t c, int32_t mode,
                     float negative_slope, float* dz, int64_t lddz, void* stream);

/* Row L2 normalisation F / ||F||_2 (FCGF_APR/model/resunet.py:187-191). */
int apr_l2_normalize(const float* x, int64_t ldx, int64_t n, int32_t c,
                     float* y, int64_t ldy, void* stream);
/* Its backward, dx = (dy - y (y . dy)) / |x| per row (the normalisation at the end of ResUNet2.forward under
 * FCGF_APR/lib/complement_trainer.py:484). */
int apr_l2_normalize_backward(const float* x, int64_t ldx, const float* dy, int64_t lddy, int64_t n, int32_t c,
                              float* dx, int64_t lddx, void* stream);

/* ------------------------------------------------------------------------
 * Feature nearest neighbour (squared L2), replaces find_nn_gpu / pdist
 *   (FCGF_APR/lib/eval.py:18-48, lib/metrics.py:22-29) and the feature KD-tree
 *   search inside open3d's registration_ransac_based_on_feature_matching
 *   (FCGF_APR/scripts/test_apr.py:148-156).
 *   best[i] = (bits(d2) << 32) | j  minimising d2 = ||F0[i]-F1[j]||^2, ties ->
 *   smallest j.  d2 is accumulated in a fixed fp32 order (4 interleaved fma
 *   chains) so the C oracle reproduces it bit for bit.
 *   `best` must be u64[n0]; it is initialised by the call.
 * ---------------------------------------------------------------------- */
int apr_feature_nn(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c,
                   uint64_t* best, void* stream);
/* Unpack: idx i64[n], d2 f32[n] (either nullable). */
/* Same result, bit for bit, by filter + exact refine: a split-bf16 (hi + lo) MFMA pass bounds every distance
 * rigorously (|approx - d| <= 1e-4 |a||b| + 5e-5 (|a|^2 + |b|^2)), a second pass evaluates the exact fp32 direct form only
 * for the pairs that can still be the arg-min.  c in {32, 64, 128}; scratch from apr_feature_nn_fast_scratch_bytes. */
size_t apr_feature_nn_fast_scratch_bytes(int64_t n0, int64_t n1, int32_t c);
int apr_feature_nn_fast(const float* f0, int64_t n0, const float* f1, int64_t n1, int32_t c, uint64_t* best,
                        void* scratch, size_t scratch_bytes, void* stream);
int apr_nn_unpack(const uint64_t* best, int64_t n, int64_t* idx, float* d2, void* stream);

/* ------------------------------------------------------------------------
 * RANSAC + Kabsch (SVD) pose from feature correspondences, replaces
 *   open3d registration_ransac_based_on_feature_matching as called at
 *   FCGF_APR/scripts/test_apr.py:148-156 and
 *   Predator_APR/lib/benchmark_utils.py:213-225.
 *   corr i64[n0]: target index of every source point (from apr_feature_nn).
 *   Hypothesis `it` samples ransac_n=4 source indices from a counter-based RNG
 *   (seed, it, slot); edge-length checker (ratio), Kabsch without scale in fp64,
 *   distance checker; every surviving hypothesis is scored by the number of
 *   correspondences within `max_dist` (then lower RMSE, then lower `it`).
 *   result_host f64[20]: T (row-major 4x4), inliers, rmse, best_it, n_valid.
 *   Synchronises the stream before returning.
 * ---------------------------------------------------------------------- */
size_t apr_ransac_scratch_bytes(int64_t n0, int64_t max_iter);
int apr_ransac_pose(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1,
                    const int64_t* corr, double max_dist, double edge_ratio,
                    int64_t max_iter, uint64_t seed,
                    void* scratch, size_t scratch_bytes, double* result_host, void* stream);

/* Same sampler / checkers / Kabsch, but open3d <= 0.11 semantics as used by
 *   Predator_APR/lib/benchmark_utils.py:213-225 (`o3d.registration`, RANSACConvergenceCriteria(50000, 1000)):
 *   only the first `max_validation` surviving hypotheses (in iteration order) are validated, and a
 *   hypothesis is scored GEOMETRICALLY: a transformed source point is an inlier when its nearest
 *   target point lies within max_dist (uniform-grid NN search); fitness = inliers / n0, then RMSE.
 *   max_iter <= 2^20.  result_host as apr_ransac_pose.  Synchronises the stream. */
size_t apr_ransac_geometric_scratch_bytes(int64_t n0, int64_t n1, int64_t max_iter);
int apr_ransac_pose_geometric(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1,
                              const int64_t* corr, double max_dist, double edge_ratio,
                              int64_t max_iter, int64_t max_validation, uint64_t seed,
                              void* scratch, size_t scratch_bytes, double* result_host, void* stream);
/* The same without the host synchronisation: the raw result (apr_ransac_raw_bytes() bytes) is copied to `raw_dev`
 * (device memory of the caller's); fetch the raw results of a whole batch with one copy and decode each on the host
 * with apr_ransac_decode (result_host as apr_ransac_pose). */
size_t apr_ransac_raw_bytes(void);
int apr_ransac_pose_geometric_async(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1,
                                    const int64_t* corr, double max_dist, double edge_ratio, int64_t max_iter,
                                    int64_t max_validation, uint64_t seed, void* scratch, size_t scratch_bytes,
                                    void* raw_dev, void* stream);
int apr_ransac_decode(const void* raw_host, double* result_host);
/* apr_ransac_pose without the host synchronisation: ALL max_iter iterations in a single round (the per-pair body of
 * apr_match_pose_batch), the raw result copied to `raw_dev`.  Scratch: apr_ransac_scratch_bytes(n0, max_iter).  The
 * decoded result equals apr_ransac_pose's whenever total_valid <= 2^20 or max_iter <= 2^20; otherwise the hypothesis
 * list of the single round overflowed, the pose is NOT final and the pair has to be redone through apr_ransac_pose
 * (apr_fcgf_test_pair's column [28] says so on the device).  Call site: FCGFTestEpoch (apr_amd/fcgf/lib/tester.py). */
int apr_ransac_pose_async(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int64_t* corr,
                          double max_dist, double edge_ratio, int64_t max_iter, uint64_t seed, void* scratch,
                          size_t scratch_bytes, void* raw_dev, void* stream);

/* B independent pairs, matching + pose, in ONE call and ONE host synchronisation: per pair apr_feature_nn_fast
 * (apr_feature_nn for channel counts other than 32/64/128) -> apr_nn_unpack -> single-round RANSAC, enqueued back to
 * back on `stream`; results_host f64[B][20] in the layout of apr_ransac_pose.  Identical results to the per-pair
 * entry points (a pair whose hypothesis list overflows is redone through apr_ransac_pose).  This is the body of the
 * reference's per-pair loop after the encoder (FCGF_APR/scripts/test_apr.py:139-156), batched. */
typedef struct {
  const float* f0; int64_t n0;     /* features of frame 0 (queries), row-major [n0, c], 16-byte aligned */
  const float* f1; int64_t n1;     /* features of frame 1 (targets) [n1, c] */
  const float* xyz0;               /* representative points of frame 0, f32 [n0, 3] */
  const float* xyz1;               /* ... of frame 1, f32 [n1, 3] */
  uint64_t seed;                   /* RANSAC hypothesis stream of this pair */
} apr_pair_desc;
size_t apr_match_pose_batch_scratch_bytes(int32_t B, int64_t n0_max, int64_t n1_max, int32_t c, int64_t max_iter);
int apr_match_pose_batch(const apr_pair_desc* pairs, int32_t B, int32_t c, double max_dist, double edge_ratio,
                         int64_t max_iter, void* scratch, size_t scratch_bytes, double* results_host, void* stream);
/* The same in two halves, for a host that keeps several batches in flight from ONE thread (bench.py): _enqueue
 * launches everything and ends with an asynchronous copy of the B result slots into slots_host
 * (apr_match_pose_batch_slot_bytes(B) bytes; pinned host memory makes the copy asynchronous) - no host
 * synchronisation; _finish decodes the slots into results_host f64[B][20] once the caller has waited for that copy (an
 * event recorded on `stream` behind the enqueue call).  Same pairs / parameters / scratch for both halves. */
size_t apr_match_pose_batch_slot_bytes(int32_t B);
int apr_match_pose_batch_enqueue(const apr_pair_desc* pairs, int32_t B, int32_t c, double max_dist, double edge_ratio,
                                 int64_t max_iter, void* scratch, size_t scratch_bytes, void* slots_host, void* stream);
int apr_match_pose_batch_finish(const apr_pair_desc* pairs, int32_t B, int32_t c, double max_dist, double edge_ratio,
                                int64_t max_iter, void* scratch, size_t scratch_bytes, const void* slots_host,
                                double* results_host, void* stream);

/* Which RANSAC sampling kernel the calls that follow use: 1 = first edge screened out of LDS (k_sample_screen: lowest
 * latency for a caller with ONE step in flight), 0 = the plain staged checker (k_sample_check: leaves the CUs' LDS to the
 * kernels of a pipelined caller's other streams), -1 = APR_RANSAC_SCREEN from the environment (default 1).  Same
 * candidate set either way (FCGF_APR/scripts/test_apr.py:148-156). */
int apr_ransac_set_screen(int32_t mode);
/* Launch counts of the two sampling kernels since the library was loaded: out2[0] = k_sample_check, out2[1] =
 * k_sample_screen.  The library silently takes the former when the correspondence table does not fit the LDS, a call has
 * fewer than 2^17 iterations or the 160 KB LDS opt-in failed: a measurement reports the difference of two readings, not
 * the switch it asked for (bench.py `config.ransac_sampling_kernel`). */
int apr_ransac_set_option(int32_t option, int32_t value);
/* ^ A/B and test switches of the matcher without touching the environment (the library reads APR_RANSAC_* once per process;
 * a getenv per call from GIL-free threads would race with the host application's setenv): option 0 screen, 1 count (0 = every
 * survivor scored in fp64), 2 prune (0 = counts over all correspondences), 3 force_rounds (1 = no single-round fast path);
 * value -1 restores the environment's default.  Results do not depend on any of them. */
int apr_ransac_sampling_launches(int64_t* out2);

/* Deal the pairs of a batch over `lanes` streams (1 .. 4): lane 0 is the caller's stream, the others are library-owned
 * streams forked from it by an event and joined back before the result copy, each with its own matching / RANSAC
 * scratch - ordering as seen by the caller is unchanged, results are identical.  Default 1 (or APR_MATCH_LANES): a
 * remedy for a caller with ONE step in flight; with several steps in flight on the caller's own streams the card is
 * already full and more lanes cost throughput.  Set it before apr_match_pose_batch_scratch_bytes (whose answer
 * depends on it) and not while batches are between _enqueue and _finish. */
int apr_match_pose_set_lanes(int32_t lanes);

/* Robust linearised 6-DoF pose (20 IRLS iterations), replaces
 * est_quad_linear_robust (FCGF_APR/util/transform_estimation.py:89-116).
 * pts0/pts1 f32[n,3] paired, weight f32[n] nullable; T_host f32[16]; syncs. */
int apr_irls_pose(const float* pts0, const float* pts1, const float* weight, int64_t n,
                  float* T_host, void* scratch, size_t scratch_bytes, void* stream);
size_t apr_irls_scratch_bytes(int64_t n);

/* Matching metrics of one validation pair, replaces the host-chained statements of
 *   GenerativePairTrainer._valid_epoch (FCGF_APR/lib/complement_trainer.py:555-572): find_corr's gathers,
 *   est_quad_linear_robust, corr_dist, rte, rre, evaluate_hit_ratio (lib/trainer.py:392-395).
 * One launch of one persistent workgroup, nothing synchronises, every result stays on the device:
 *   xyz0 f32[n0,3], xyz1 f32[n1,3]: the clouds (the collate's pcd0[0], pcd1[0]);
 *   sel0 i64[m0], sel1 i64[m1]: find_corr's subsample rows, NULL = every row (then m0 == n0 / m1 == n1);
 *   nn i64[m0]: feature nearest neighbour of subsampled source row i among the m1 subsampled target rows;
 *   T_gt f32[16] row-major ground truth; hit_thresh: config.hit_ratio_thresh.
 * Writes record `slot` of records f32[n_slots, APR_VALID_RECORD_FLOATS]:
 *   [0] corr_dist = mean over ALL n0 rows of min(|T_est x - T_gt x|, 1)      [1] rte = |t_est - t_gt|
 *   [2] rre = arccos((trace(R_est^T R_gt) - 1) / 2) in radians, NaN when the argument leaves [-1, 1] (as NumPy)
 *   [3] hit_ratio = share of the m0 correspondences with sqrt(|T_gt x0 - x1|^2 + 1e-6) < hit_thresh
 *   [4] n_corr = m0, or MINUS the number of sel0 / sel1 / nn entries out of range (those read row 0)
 *   [5..20] T_est row-major, the bits apr_irls_pose gives on the same correspondences
 *   [21], [22] left untouched for the caller (the NPR validation terms)       [23] hit count.
 * Sums run in a fixed order (no float atomics): the same bits on every run. */
#define APR_VALID_RECORD_FLOATS 24
int apr_valid_pair(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int64_t* sel0,
                   const int64_t* sel1, int64_t m0, int64_t m1, const int64_t* nn, const float* T_gt,
                   float hit_thresh, float* records, int64_t n_slots, int64_t slot, void* scratch,
                   size_t scratch_bytes, void* stream);
size_t apr_valid_pair_scratch_bytes(int64_t m0);

/* The record of one validated Predator pair, replaces the stat picking, the two additions and the five float()
 *   synchronisations at the end of Trainer.inference_one_batch(inputs, 'val') (Predator_APR/lib/trainer.py:253-278).
 * One small launch, nothing synchronises.  Device pointers: overlap8 / saliency8 f32[8]: the apr_weighted_bce_forward
 *   results of the overlap and the saliency scores (loss, w_negative, precision, recall, ...); circle4 f32[4]: the
 *   apr_circle_forward result (circle_loss, recall, anchors used, ...); count i32[1]: the filtered correspondences
 *   (apr_circle_select); chamfer0/1, reg0/1 f32[1]: the two frames' Chamfer and regulariser values.  n_src, n_tgt: rows
 *   of the two clouds (host values, < 2^24).
 * Writes record `slot` of records f32[n_slots, APR_PREDATOR_VALID_RECORD_FLOATS]:
 *   [0..7] circle_loss, recall, overlap_loss, overlap_recall, overlap_precision, saliency_loss, saliency_recall,
 *          saliency_precision (lib/loss.py:99-178)
 *   [8] chamfer_loss = chamfer0 + chamfer1        [9] regularization_loss = reg0 + reg1 (float32 adds, :253-264)
 *   [10] filtered count   [11] anchors used   [12] n_src   [13] n_tgt   [14] how many of chamfer0/1 are NaN   [15] 0 */
#define APR_PREDATOR_VALID_RECORD_FLOATS 16
int apr_predator_valid_record(const float* overlap8, const float* saliency8, const float* circle4,
                              const int32_t* count, const float* chamfer0, const float* chamfer1, const float* reg0,
                              const float* reg1, int64_t n_src, int64_t n_tgt, float* records, int64_t n_slots,
                              int64_t slot, void* stream);

/* The record of one tested Predator pair: what KITTITester.test / NUSCENESTester.test compute on the host after their
 *   per-pair loop (Predator_APR/lib/tester.py:104-124, the same statements at the end of NUSCENESTester.test, :158-268;
 *   get_angle_deviation lib/benchmark_utils.py:170-185), taken
 *   from the RAW RANSAC result on the device (raw_dev: what apr_ransac_pose_geometric_async left, apr_ransac_raw_bytes()
 *   bytes, 8-byte aligned).  One launch of one 1024-thread workgroup, nothing synchronises, sums in a fixed order.
 *   s_p f32[ns,3], t_p f32[nt,3]: the sampled clouds; corr i64[ns]: feature nearest neighbour of source row i;
 *   rot_gt f32[9], trans_gt f32[3]: the pair's ground truth; distance_threshold: the RANSAC distance; 0 < ns < 2^24.
 * Writes record `slot` of records f64[n_slots, APR_PREDATOR_TEST_RECORD_FLOATS]:
 *   [0] RRE in degrees = arccos(clip((trace(R_est R_gt^T) - 1) / 2, -1, 1)) / pi * 180 in double
 *   [1] RTE = |t_est - t_gt|    [2] 1.0 if RRE < rot_threshold && RTE < trans_threshold (both strict), else 0.0
 *   [3] |t_gt|
 *   [4] share of rows with |rot_gt s_p[i] + trans_gt - t_p[corr[i]]| < inlier_distance_threshold, in the float32
 *       arithmetic of apr_inlier_ratio's 'wo' leg       [5] the same under the estimate at distance_threshold
 *   [6] ns   [7] nt   [8..23] the estimate, row-major 4x4, as apr_ransac_decode gives it
 *   [24] inliers   [25] rmse   [26] n_valid (total_valid)   [27] best iteration
 *   [28] corr entries outside [0, nt): such a row reads target row 0 and is counted      [29..31] 0 */
#define APR_PREDATOR_TEST_RECORD_FLOATS 32
int apr_predator_test_pair(const float* s_p, int64_t ns, const float* t_p, int64_t nt, const int64_t* corr,
                           const float* rot_gt, const float* trans_gt, const void* raw_dev, double distance_threshold,
                           double inlier_distance_threshold, double rot_threshold, double trans_threshold,
                           double* records, int64_t n_slots, int64_t slot, void* stream);

/* The record of one tested FCGF pair: what FCGF_APR/scripts/test_apr.py:120-186 and scripts/test_fcgf.py:121-195 compute
 *   on the host per pair around their RANSAC call (evaluate_nn_dist on find_corr's correspondences, RTE, RRE, the success
 *   flag, |t_gt|), taken from the RAW RANSAC result on the device (raw_dev: what apr_ransac_pose_async left,
 *   apr_ransac_raw_bytes() bytes, 8-byte aligned).  One launch of one 1024-thread workgroup, nothing synchronises, integer
 *   sums in a fixed order.  Call site: FCGFTestEpoch (apr_amd/fcgf/lib/tester.py).  Device pointers:
 *   xyz0 f32[n0,3], xyz1 f32[n1,3]: the clouds (the collate's pcd0[0], pcd1[0]);
 *   sel0 i64[m0], sel1 i64[m1]: find_corr's subsample rows, NULL = every row (then m0 == n0 / m1 == n1);
 *   nn i64[m0]: feature nearest neighbour of subsampled source row i among the m1 subsampled target rows;
 *   r0 f32[k0,3], r1 f32[k1,3], corr i64[k0]: the point sets RANSAC ran on and their correspondences (test_apr: the clouds
 *   themselves; test_fcgf: random_sample's rows);  T_gt f32[16] row-major;  dists f32[m0] or NULL.
 *   Host values: distance_threshold (the RANSAC distance), rte_thresh (metres), rre_thresh_deg, max_iter (of the RANSAC
 *   call that wrote raw_dev); 0 < m0, k0 < 2^24.
 * Writes record `slot` of records f64[n_slots, APR_FCGF_TEST_RECORD_FLOATS].  T_ransac is the raw pose rounded to float32
 *   (`.astype(np.float32)`, test_apr.py:156); [0], [1], [3] are double arithmetic on it and the float32 ground truth:
 *   [0] RTE = sqrt(sum_a (t_est[a] - t_gt[a])^2), the squares added in the order a = 0, 1, 2
 *   [1] RRE in radians = arccos((tr - 1) / 2), tr = sum_a (sum_b R_est[a][b] * R_gt[a][b]), each row sum started at 0 and
 *       added left to right, the rows added in order; unclipped: NaN when the argument leaves [-1, 1] (as apr_valid_pair)
 *   [2] 1.0 if RTE < rte_thresh && RRE == RRE && RRE < pi / 180 * rre_thresh_deg (both strict, test_apr.py:177), else 0.0
 *   [3] |t_gt|   [4] m0   [5] k0   [6] k1
 *   [7] sel0 / sel1 / nn / corr entries out of range: such an entry reads row 0 and is counted
 *   [8..23] T_ransac, row-major 4x4, widened      [24] inliers   [25] rmse   [26] total_valid   [27] best iteration
 *   [28] 1.0 if total_valid > 2^20 && max_iter > 2^20 (the single round overflowed: the pose is not final), else 0.0
 *   [29] share of the k0 correspondences with |R_est r0[i] + t_est - r1[corr[i]]| < distance_threshold, in the float32
 *        arithmetic of apr_inlier_ratio's 'wo' leg      [30] the same under the ground truth      [31] 0
 *   [32..41] how many of the m0 find_corr correspondences have (double)d_i < k * 0.1, k = 1 .. 10, where
 *        d_i = sqrt(|R_gt x0 + t_gt - x1|^2 + 1e-6) in float32 (evaluate_nn_dist, test_apr.py:64-67) and k * 0.1 is the
 *        double product (0.30000000000000004 for k = 3), as the tables at test_apr.py:200-213 form it      [42..47] 0
 *   dists, when not NULL, receives the d_i: the pair's row of dists_nn. */
#define APR_FCGF_TEST_RECORD_FLOATS 48
int apr_fcgf_test_pair(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int64_t* sel0,
                       const int64_t* sel1, int64_t m0, int64_t m1, const int64_t* nn, const float* r0, int64_t k0,
                       const float* r1, int64_t k1, const int64_t* corr, const float* T_gt, const void* raw_dev,
                       double distance_threshold, double rte_thresh, double rre_thresh_deg, int64_t max_iter,
                       float* dists, double* records, int64_t n_slots, int64_t slot, void* stream);

/* Hardest-contrastive mining (forward), replaces the mining + masking + loss arithmetic of
 *   contrastive_hardest_negative_loss (FCGF_APR/lib/trainer.py:400-452, `_hash` util/misc.py:6-18).
 *   pos_f0/pos_f1 f32[p,c]: features of the sampled positive pairs; nn01/nn10 u64[p]: packed
 *   apr_feature_nn results of pos_f0 in F1[sel1] / pos_f1 in F0[sel0]; sorted_pos_keys: ascending
 *   int64 keys i + j*hash_seed of ALL positive pairs.  out6 f64[6] (device) =
 *   {sum pos_loss, p, sum neg_loss0, count0, sum neg_loss1, count1}. */
int apr_contrastive_reduce(const float* pos_f0, const float* pos_f1, int32_t p, int32_t c,
                           const uint64_t* nn01, const uint64_t* nn10, const int64_t* sel0, const int64_t* sel1,
                           const int64_t* pos_ind0, const int64_t* pos_ind1, const int64_t* sorted_pos_keys,
                           int32_t n_keys, int64_t hash_seed, float pos_thresh, float neg_thresh,
                           double* out6, void* stream);

/* Pair-list losses: the arithmetic of the random-negative contrastive, triplet and hardest-triplet trainers, forward
 *   and backward, with nothing read back by the host.  A loss is a list of n cross-cloud row pairs (r0[t], r1[t]) (i32;
 *   a row outside its cloud gives a NaN distance and no gradient) over F0 f32[N0,c], F1 f32[N1,c] (c % 4 == 0, c <= 256,
 *   16-byte aligned) and a table of terms over the pairs' distances. */
#define APR_PAIR_MAX_GROUPS 4
#define APR_PAIR_TERM_STAT 0      /* value d[pa], no gradient (a logged mean) */
#define APR_PAIR_TERM_SQ 1        /* value d[pa] of a plain-square pair: the positive term of trainer.py:260 */
#define APR_PAIR_TERM_NEG 2       /* value relu(margin - d[pb])^2: the negative term of trainer.py:263-264 */
#define APR_PAIR_TERM_TRIPLET 3   /* value relu(d[pa] + margin - d[pb]): trainer.py:577, :724-729 */
/* rows[i] = sel[best[i] & 0xffffffff] (-1 where that index is >= m): the D01ind = sel1[D01ind] step of
 *   FCGF_APR/lib/trainer.py:698-699 on the packed apr_feature_nn result, without the copy to the host. */
int apr_pair_rows_from_nn(const uint64_t* best, int64_t p, const int64_t* sel, int64_t m, int32_t* rows, void* stream);
/* d[t] = |F0[r0[t]] - F1[r1[t]]|^2 for t < n_plain, sqrt(that + eps) for the rest, in the difference-square form of
 *   FCGF_APR/lib/metrics.py:22-29 (as trainer.py:260, :264, :560, :574-575, :707, :721-722); coef[t] = 0, grp[t] = 0. */
int apr_pair_dist(const float* F0, int64_t N0, const float* F1, int64_t N1, int32_t c, const int32_t* r0, const int32_t* r1,
                  int64_t n, int64_t n_plain, float eps, float* d, float* coef, int32_t* grp, void* stream);
/* The filter, hinge and means of FCGF_APR/lib/trainer.py:259-267, :568-579, :700-731.  terms i32[n_terms,4] =
 *   (pa, pb, kp, kind | group << 8): pair indices (-1: none), kp = the pair whose key r0 + r1 * hash_seed drops the term
 *   when it is among sorted_pos_keys (ascending i64; kp = -1: no filter).  Out: red f64[2 * n_groups] = {sum, count} of
 *   the kept terms per group, summed in a fixed order (thread order inside a block, blocks ascending); mean f32[n_groups]
 *   = sum / count, NaN for an empty group; coef[t] / grp[t] for every pair of a kept, active term of kind SQ / NEG /
 *   TRIPLET: the factor of (F0[r0] - F1[r1]) in dF0 before the 1 / count, and the term's group -- a pair may stand in at
 *   most one such term; kept u8[n_terms] (nullable). */
size_t apr_pair_terms_scratch_bytes(int64_t n_terms);
int apr_pair_terms_reduce(const float* d, const int32_t* r0, const int32_t* r1, int64_t n, const int32_t* terms,
                          int64_t n_terms, const int64_t* sorted_pos_keys, int64_t n_keys, int64_t hash_seed, float margin,
                          int32_t n_groups, double* red, float* mean, float* coef, int32_t* grp, uint8_t* kept,
                          void* scratch, size_t scratch_bytes, void* stream);
/* The backward of the index_select / boolean-index gathers under FCGF_APR/lib/trainer.py:271, :499, :626 without atomics:
 *   dF0[r,:] = sum over t with r0[t] = r, in ascending t, of coef[t] * gout[grp[t]] / count[grp[t]] * (F0[r] - F1[r1[t]]),
 *   dF1 mirrored; a row in no pair, or only in pairs with coef 0, gets exact zeros.  gout f32[n_gout]: the upstream
 *   gradient of the first n_gout group means; red: as apr_pair_terms_reduce left it. */
size_t apr_pair_grad_scratch_bytes(int64_t n, int64_t N0, int64_t N1);
int apr_pair_grad(const float* F0, int64_t N0, const float* F1, int64_t N1, int32_t c, const int32_t* r0, const int32_t* r1,
                  int64_t n, const float* coef, const int32_t* grp, const double* red, const float* gout, int32_t n_gout,
                  float* dF0, float* dF1, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Point-set index builds of the KPConv encoder (Predator_APR)
 * ---------------------------------------------------------------------- */

/* Barycentre grid subsampling of a batch of clouds; replaces
 *   cpp_wrappers.cpp_subsampling.grid_subsampling.subsample_batch(points, batches, sampleDl=)
 *   (Predator_APR/cpp_wrappers/cpp_subsampling/wrapper.cpp:75-82 ->
 *    grid_subsampling/grid_subsampling.cpp:5-107,109-211).
 *   pts f32[n,3] (clouds concatenated), lengths_host i32[nb] (HOST), dl = cell size.
 *   out_pts f32[<=n,3], out_feats (nullable) f32[<=n,fdim], out_lengths_host i32[nb] (HOST).
 *   Barycentres are bit-identical to the reference's; rows come in first-occurrence order of the
 *   cells instead of libstdc++ unordered_map order.  Synchronises the stream. */
size_t apr_grid_subsample_scratch_bytes(int64_t n);
int apr_grid_subsample(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, float dl,
                       const float* feats, int32_t fdim, float* out_pts, float* out_feats,
                       int32_t* out_lengths_host, void* scratch, size_t scratch_bytes, void* stream);
/* The same without the host synchronisation: lengths_status_dev = int32[nb + 1] on the device (nb subsampled lengths,
 * then 0 or the out-of-range flag); out_pts / out_feats hold n rows, the result is their first sum(lengths) rows. */
int apr_grid_subsample_async(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, float dl,
                             const float* feats, int32_t fdim, float* out_pts, float* out_feats,
                             int32_t* lengths_status_dev, void* scratch, size_t scratch_bytes, void* stream);

/* open3d's voxel centroids of a batch of clouds; replaces
 *   open3d.geometry.PointCloud.voxel_down_sample(voxel_size=) as the loaders call it
 *   (Predator_APR/datasets/kitti.py:464-475,588-589 and the same lines of datasets/nuscenes.py).
 *   pts f32[n,3] (clouds concatenated), lengths_host i32[nb] (HOST, 1 <= nb <= 64, every length > 0).
 *   Per cloud and axis, float64 with every operation rounded on its own:
 *     origin = (double)min - voxel_size * 0.5;  index = floor(((double)p - origin) / voxel_size);
 *     sum = 0.0, sum += (double)p over the voxel's rows in ascending row order;  centroid = sum / (double)count.
 *   Output rows: clouds in batch order, inside a cloud the voxels in ascending order of their first row.
 *   centroid f64[<=n,3], centroid32 f32[<=n,3] (the centroid rounded to nearest once), count i32[<=n],
 *   first i32[<=n] (the voxel's first row in pts), index i32[<=n,3]; out_lengths_host i32[nb] (HOST): voxels per
 *   cloud.  Any of the six may be NULL; the device arrays must hold n rows.  A cloud gives the same bits alone and
 *   inside a batch, and from run to run.  APR_ERANGE (outputs undefined): a row is not finite, or an index exceeds
 *   131071.  Synchronises the stream. */
size_t apr_voxel_down_sample_scratch_bytes(int64_t n);
int apr_voxel_down_sample(const float* pts, int64_t n, const int32_t* lengths_host, int32_t nb, double voxel_size,
                          double* centroid, float* centroid32, int32_t* count, int32_t* first, int32_t* index,
                          int32_t* out_lengths_host, void* scratch, size_t scratch_bytes, void* stream);

/* The augmentation of a Predator_APR sample on its float64 centroids; replaces
 *   Predator_APR/datasets/kitti.py:494-517 (noise, rotation of one side, scale, shift) and the `.float()` of
 *   datasets/dataloader.py:163.  pts f64[n,3], u f64[n,3] (the loader's np.random.rand draws) on the device;
 *   rot_host f64[9] row-major (HOST; NULL: this side does not rotate), shift_host f64[3] (HOST).
 *     q = p + (u - 0.5) * noise;  q_j = (R[j,0]*q_0 + R[j,1]*q_1) + R[j,2]*q_2;  out = (float)(q * scale + shift),
 *   every operation a separately rounded float64 operation, one rounding to fp32 at the end. */
int apr_sample_augment(const double* pts, const double* u, int64_t n, double noise, const double* rot_host,
                       double scale, const double* shift_host, float* out, void* stream);

/* Float64 mean of a cloud's rows, the same bits from run to run; stands in for the np.mean of
 *   sample_random_trans (FCGF_APR/lib/complement_data_loader.py:33-38).  pts f32[n,3], mean f64[3] (device). */
int apr_cloud_mean(const float* pts, int64_t n, double* mean, void* stream);

/* Batched radius neighbours, sorted by distance; replaces
 *   cpp_wrappers.cpp_neighbors.radius_neighbors.batch_query(queries, supports, q_batches, s_batches, radius=)
 *   (Predator_APR/cpp_wrappers/cpp_neighbors/wrapper.cpp:71-75 -> neighbors/neighbors.cpp:211-333)
 *   followed by the `[:, :limit]` truncation of datasets/dataloader.py:66-68.
 *   out i32[nq, out_ld]; columns [0,width) of every row are written: neighbour indices into the
 *   concatenated supports, ascending distance, padded with ns.  width = min(max_count, limit)
 *   (limit <= 0: no limit) is returned in *width_host.  out == NULL: size query only.
 *   Synchronises the stream. */
size_t apr_radius_scratch_bytes(int64_t nq, int64_t ns);
int apr_radius_neighbors(const float* queries, int64_t nq, const float* supports, int64_t ns,
                         const int32_t* q_lengths_host, const int32_t* s_lengths_host, int32_t nb, float radius,
                         int32_t limit, int32_t* out, int64_t out_ld, int32_t* width_host,
                         void* scratch, size_t scratch_bytes, void* stream);

/* The same table without a host synchronisation, for callers that know the column limit (KPConv's calibrated
 * neighbourhood limits, collate_fn_descriptor :121-180): out i32[nq, >= limit] gets the `limit` nearest neighbours per
 * query (sorted by distance, padded with ns); flags_dev i32[2] on the device: [0] = largest neighbour count of any
 * query (the reference's table width is min([0], limit); columns [that, limit) are all padding), [1] != 0 if a query
 * had more neighbours within the radius than the kernel's candidate buffer holds (error). */
int apr_radius_neighbors_async(const float* queries, int64_t nq, const float* supports, int64_t ns,
                               const int32_t* q_lengths_host, const int32_t* s_lengths_host, int32_t nb, float radius,
                               int32_t limit, int32_t* out, int64_t out_ld, int32_t* flags_dev,
                               void* scratch, size_t scratch_bytes, void* stream);
/* Same, searching the grid the PREVIOUS apr_radius_neighbors_async call left in `scratch` (same supports, lengths,
 * radius and stream): skips the grid build. */
int apr_radius_neighbors_regrid_async(const float* queries, int64_t nq, const float* supports, int64_t ns,
                               const int32_t* q_lengths_host, const int32_t* s_lengths_host, int32_t nb, float radius,
                               int32_t limit, int32_t* out, int64_t out_ld, int32_t* flags_dev,
                               void* scratch, size_t scratch_bytes, void* stream);

/* k nearest neighbours inside one cloud (brute force, k + skip_first <= 16); replaces the dense
 * square_distance + topk(k+1)[..., 1:] of Predator_APR/models/gcn.py:19-23.  out i32[n,k]. */
int apr_knn(const float* pts, int32_t n, int32_t k, int32_t skip_first, int32_t* out, void* stream);

/* ------------------------------------------------------------------------
 * KPConv encoder + overlap attention (Predator_APR/models/blocks.py, gcn.py, architectures.py)
 * ---------------------------------------------------------------------- */

/* out[i] = sum_c x[i,c]  (neighbour-count normaliser of KPConv, blocks.py:369-372). */
/* Dense out = act((in[M, cin] @ W) * scale + shift + residual) on the bf16 MFMA in the 3-way split (fp32-equivalent
 * accuracy, see apr_spconv_ws_fwd_bf3): the unary / bottleneck Linear layers and KPConv's second step
 * [N, 15 cin] x [15 cin, cout] of KPFCNN (Predator_APR/models/blocks.py:347-374, 499-504), and K = 1 convolutions.
 * w_bf3 = apr_spconv_pack_weights_bf3(w, 1, cin, cout).  cin % 64 == 0, cout % 64 == 0; rows of in / out / residual
 * and scale / shift 16-byte aligned. */
int apr_dense_gemm_bf3(const float* in, int64_t ldi, int64_t M, int32_t cin, int32_t cout, const void* w_bf3,
                       const float* scale, const float* shift, const float* residual, int64_t ldr, int32_t relu,
                       float* out, int64_t ldo, void* stream);
/* The same operator for FEW input channels over MANY rows -- the K = 1 layers at the end of the encoders
 * (FCGF_APR/model/resunet.py:126-142: conv1_tr 96 -> 64 / 160 -> 128 and `final` 64 -> 32 / 128 -> 128 on the finest level) --
 * as a row stream past weights that stay in LDS for the life of a workgroup: every row is read once, a wave owns whole rows,
 * so the row normalisation of `normalize_feature` (l2norm != 0: out[j] /= |out[j]|_2, same bits as apr_l2_normalize behind
 * the plain call) is part of the epilogue.  cin in {64, 96, 128, 160, 192}, cout in {32, 64, 128}
 * (apr_dense_rows_bf3_ok); w_bf3 = apr_spconv_pack_weights_bf3(w, 1, cin, cout), which for K = 1 takes cin % 32 == 0 and
 * cout % 16 == 0 (columns padded with zeros to a multiple of 64 inside the image).  Same bits as apr_dense_gemm_bf3 where
 * both take the shape.  apr_dense_rows_bf3_route: what apr_spconv_fwd_batch / apr_resunet_encode do with a K = 1 layer of M
 * rows -- 1: this kernel (an instantiated shape and M >= APR_DENSE_ROWS_MIN, default 32768 rows). */
int32_t apr_dense_rows_bf3_ok(int32_t cin, int32_t cout);
int32_t apr_dense_rows_bf3_route(int64_t M, int32_t cin, int32_t cout);
int apr_dense_rows_bf3(const float* in, int64_t ldi, int64_t M, int32_t cin, int32_t cout, const void* w_bf3,
                       const float* scale, const float* shift, const float* residual, int64_t ldr, int32_t relu,
                       int32_t l2norm, float* out, int64_t ldo, void* stream);
/* out = act(instance_norm(in @ W) (+ residual)) -- the Linear + InstanceNorm1d (+ shortcut) (+ LeakyReLU) every unary /
 * bottleneck layer of KPFCNN is (Predator_APR/models/blocks.py:451-468, 499-504, 653-681) -- in TWO launches: the GEMM leaves
 * the raw product in `out` and the per-tile column sums (fp64, rows in order) in scratch, the apply kernel rebuilds mean /
 * rstd from them and normalises in place.  act_mode 0 none, 1 ReLU, 2 LeakyReLU(negative_slope).  seg_offsets_host (int64
 * [nseg + 1], 0 .. M; NULL / nseg <= 1: one segment): the scan pairs stacked into one forward, each normalised on its own;
 * row tiles never straddle a segment.  Same operator as apr_dense_gemm_bf3 followed by apr_instance_norm_act[_seg]; the
 * statistics group their fp64 partial sums by GEMM tile instead of by 256 rows (results agree to the last bits, not bit for
 * bit).  `out` may not alias `in`; residual may alias neither. */
size_t apr_dense_gemm_bf3_norm_scratch_bytes(int64_t M, int32_t cout, int32_t nseg);
int apr_dense_gemm_bf3_norm_act(const float* in, int64_t ldi, int64_t M, int32_t cin, int32_t cout, const void* w_bf3,
                                float eps, const float* residual, int64_t ldr, int32_t act_mode, float negative_slope,
                                float* out, int64_t ldo, const int64_t* seg_offsets_host, int32_t nseg, void* scratch,
                                size_t scratch_bytes, void* stream);

/* One ResnetBottleneckBlock of the KPConv encoder (Predator_APR/models/blocks.py:596-681; eval mode, use_batch_norm, rigid
 * KPConv, widths multiples of 64) enqueued by ONE call: unary1 (Linear + InstanceNorm + LeakyReLU; absent when in_dim ==
 * mid), KPConv (apr_row_sums, apr_kpconv_weighted, [n_out, n_kp mid] x [n_kp mid, mid]) + InstanceNorm + LeakyReLU, the
 * shortcut (apr_gather_pool max over `nbr` when strided; Linear + InstanceNorm when in_dim != out_dim), unary2 (Linear) +
 * InstanceNorm + shortcut + LeakyReLU -> out.  The same kernels in the same order as the single calls (same bits).
 * Weights: apr_spconv_pack_weights_bf3(K = 1) images of the [cin, cout] matrices (w_kpconv: [n_kp * mid, mid]).  nbr:
 * [n_out, H] rows of the n_in-row input level (the level's `neighbors`, or `pools` of the coarser level when strided);
 * seg_in / seg_out: host row offsets (nseg + 1) of the scan pairs stacked at the input / output level (nseg <= 1: one
 * statistic over all rows).  scratch: apr_kp_resnet_scratch_bytes(desc) device bytes. */
typedef struct apr_kp_resnet_desc {
  const float* x; int64_t ldx; int64_t n_in;
  int32_t in_dim, mid, out_dim, strided;
  const float* q_pts; const float* s_pts; int64_t n_out;
  const int32_t* nbr; int32_t H; int32_t n_kp;
  const float* kernel_points; float extent; float eps; float slope; int32_t nseg;
  const void* w_unary1; const void* w_kpconv; const void* w_unary2; const void* w_shortcut;
  const int64_t* seg_in; const int64_t* seg_out;
  float* out; int64_t ldo;
  void* scratch; size_t scratch_bytes;
  int32_t kpconv_route;      /* 0: apr_kpconv_weighted (n_kp = 15; any other n_kp in 1..32: apr_kpconv_weighted_nk, linear / sum)
                              * + the dense GEMM; 1: apr_kpconv_fused + InstanceNorm (the wf region of the scratch stays
                              * unused; n_kp != 15 or a shape apr_kpconv_fused_ok rejects is an argument error) */
} apr_kp_resnet_desc;
size_t apr_kp_resnet_scratch_bytes(const apr_kp_resnet_desc* desc);
int apr_kp_resnet_block(const apr_kp_resnet_desc* desc, void* stream);

/* Host-only (no device needed): ONE round of NumPy's legacy `RandomState.choice(n, size, replace=False, p=p)` loop
 * (Predator_APR/lib/tester.py:83-92 draws its 5000 interest points per cloud with it).  The caller owns the RNG: per
 * round it passes k = size - n_uniq uniforms from `random_sample`.  p: float64 working copy (zeroed in place for found
 * indices; n_new_zeroed = how many of found[0..n_uniq) were added by the previous round); cdf: double[n] work; stamp:
 * int32[n] work, zero before round 1; round_id = 1, 2, ...  Returns the new n_uniq (loop until it reaches size), or a
 * negative error code. */
int64_t apr_weighted_choice_round(double* p, int64_t n, int64_t* found, int64_t n_uniq, int64_t n_new_zeroed,
                                  const double* x, int64_t k, double* cdf, int32_t* stamp, int32_t round_id);

int apr_row_sums(const float* x, int64_t ld, int64_t n, int32_t c, float* out, void* stream);

/* KPConv step 1 (blocks.py:269-289,326-329,347-372): kernel-point correlation
 *   wf[q, k*cin + c] = ( sum_h max(0, 1 - |s[nbr[q,h]] - q - kp[k]| / extent) * x[nbr[q,h], c] ) / num[q]
 *   num[q] = max(#{h : rowsum[nbr[q,h]] > 0}, 1); nbr entries >= ns (or < 0) are shadow neighbours.
 * Step 2 is apr_spconv_fwd(wf, nbr = NULL, K = 1, cin = 15*cin, cout) with the [15,cin,cout] weights. */
int apr_kpconv_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                        int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                        int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf, void* stream);
/* KPConv step 1 (blocks.py:269-372) for cin = 32 on the fp32 MFMA: what apr_kpconv_weighted computes, for the first layer of
 * the symmetric generator (KPFCNNDecoder reads the encoder's 32-d descriptors on the finest level), where
 * apr_kpconv_weighted runs its one-thread-per-(query, kernel point) kernel.  Linear influence, sum aggregation.  Takes
 * n_kp = 15, cin = 32, 1 <= H <= 128, ldx and ldwf even, x and wf 8-byte aligned; everything else is refused before any
 * launch (no other route inside) and a refused call writes nothing.  nq == 0 launches nothing; columns of wf behind 480
 * are never written; a shadow neighbour (nbr < 0 or >= ns) contributes nothing and is not counted. */
int apr_kpconv_weighted_c32(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                            int32_t H, const float* x, int64_t ldx, int32_t cin, const float* kernel_points,
                            int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf, void* stream);
/* Both steps of the rigid KPConv in ONE kernel (kpconv_fused.hip): out[q, :] = wf[q, :] @ W.reshape(15 cin, cout) with wf as
 * apr_kpconv_weighted defines it; the [queries, 15 cin] tile lives in LDS and registers only.  Correlation in fp32 on the
 * fp32 MFMA, contraction on the bf16 MFMA in the 3-way split (six cross terms, fp32 accumulate), no atomics: the same bits
 * on every run.  w_bf3: apr_spconv_pack_weights_bf3(W[15 cin, cout], K = 1) -- the image apr_dense_gemm_bf3 reads.  rowsum:
 * apr_row_sums of x.  apr_kpconv_fused_ok (host only): n_kp = 15, cin and cout multiples of 64 in 64 .. 512, 1 <= H <= 128.
 * apr_kpconv_fused also needs ldx % 4 == 0, ldo % 4 == 0 and x / out / w_bf3 16-byte aligned; everything else is refused
 * before any launch (no fallback inside).  nq == 0 launches nothing; columns of out behind cout are never written.
 * apr_kpconv_fused_route (host only): 1 for the shapes where the fused kernel measured faster than the two launches. */
int32_t apr_kpconv_fused_ok(int32_t cin, int32_t cout, int32_t H);
int32_t apr_kpconv_fused_route(int64_t nq, int32_t cin, int32_t cout, int32_t H);
int apr_kpconv_fused(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                     const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp, float extent,
                     const float* rowsum, const void* w_bf3, int32_t cout, float* out, int64_t ldo, void* stream);
/* Backward of apr_kpconv_weighted with respect to the neighbour features (training path, SURVEY 8(f) next-3;
 * Predator_APR/models/blocks.py:326-374 through lib/trainer.py:142-280): dx[nbr[q,h], c] += (1 / num_q) * sum_k
 * w[q,k,h] * dwf[q, k*cin + c] with float atomics (dx must be zero-initialised; f32 [ns, cin]).  The weight gradient of
 * the layer is apr_spconv_wgrad on (wf, dout) with the identity map; d wf is a dense apr_spconv_fwd with the transposed
 * weights.  rowsum: apr_row_sums of the forward's x. */
int apr_kpconv_dfeat(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                     const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                     float extent, const float* rowsum, float* dx, int64_t lddx, void* stream);

/* The same gradient without float atomics (deterministic): apr_kpconv_dfeat_contrib writes the contribution of every
 * (query, neighbour) entry to contrib f32 [nq * H, cin]; apr_reverse_table_build sorts the table's flat positions by the
 * support row they point at (stable: ties in ascending position; once per neighbour table) and apr_reverse_gather sums
 * every support row's contributions in that order: dx f32 [ns, cin] is WRITTEN, not accumulated. */
int apr_kpconv_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                             const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                             float extent, const float* rowsum, float* contrib, void* stream);
/* Deformable / modulated KPConv (Predator_APR/models/blocks.py:235-374 with deformable=True; kpconv_deform.hip).  dkp f32
 * [nq, 15, 3] = kernel_points + extent * offsets (blocks.py:258, 279) are the query's OWN kernel points; mod f32 [nq, 15] = 2
 * sigmoid(offset_features[:, 45:]) (blocks.py:247) or NULL (= 1).  With diff = s[nbr[q,h]] - q - dkp[q,k], d2 = |diff|^2:
 *   w[q,k,h]     = max(0, 1 - sqrt(d2) / extent) for a real neighbour (0 <= nbr < ns), 0 for padding   (blocks.py:326-329)
 *   min_d2[q,k]  = min over ALL H slots of d2, a padding slot entering as the point (1e6, 1e6, 1e6)     (blocks.py:295)
 *   num[q]       = max(1, #{h real : d2 < extent^2 for some k, and rowsum[nbr[q,h]] > 0})               (blocks.py:298-316,
 *                  369-371: the reference's topk re-gather drops the out-of-range neighbours from the count; a support
 *                  beyond every DEFORMED kernel point does not count, unlike apr_kpconv_weighted)
 *   wf[q, k*cin + c] = mod[q,k] / num[q] * sum_h w[q,k,h] * x[nbr[q,h], c]                             (blocks.py:354-358)
 * apr_kpconv_deform_weighted writes wf f32 [nq, ldwf >= 15 cin] and, when min_d2 != NULL, min_d2 f32 [nq, 15]; step 2 is the
 * dense GEMM with the [15 cin, cout] weights, as for the rigid layer.  One wave per query on the fp32 MFMA, no atomics: the
 * same bits on every run.
 * Backward (num and the in-range flags are constants, as in the graph torch builds), dwf = d_out @ W^T f32 [nq, lddwf]:
 *   apr_kpconv_deform_dfeat_contrib: contrib f32 [nq * H, cin], row (q, h) = sum_k mod w dwf[q, k*cin + :] / num for a real
 *     neighbour; rows of padding neighbours are left untouched.  apr_reverse_gather(_range) sums them per support row.
 *   apr_kpconv_deform_dgeom: with P[h,k] = <x[nbr[q,h], :], dwf[q, k*cin + :]> (fp32 MFMA, dwf[q] stationary),
 *     d_mod[q,k] = sum_h w P / num,   d_dkp[q,k,:] = mod / num * sum_{h real, 0 < d < extent} diff / (d * extent) * P;
 *     every element of d_dkp f32 [nq, 15, 3] and d_mod f32 [nq, 15] is written (mod == NULL: d_mod is still written).
 *     DEVIATION: a neighbour exactly on a deformed kernel point (d = 0) contributes 0; the reference's graph gives NaN.
 * All three: n_kp = 15, cin % 64 == 0, 64 <= cin <= 512, 1 <= H <= 128, 0 < ns < 2^30, extent > 0, x / wf / dwf rows 16-byte
 * aligned where they are read or written as vectors (weighted: x, wf; dgeom: x, dwf).  Everything else returns APR_EINVAL
 * before any launch and leaves the outputs untouched; nq == 0 launches nothing.  rowsum: apr_row_sums of x. */
int apr_kpconv_deform_weighted(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                               const float* x, int64_t ldx, int32_t cin, const float* dkp, const float* mod, int32_t n_kp,
                               float extent, const float* rowsum, float* wf, int64_t ldwf, float* min_d2, void* stream);
int apr_kpconv_deform_dfeat_contrib(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                    int32_t H, const float* dwf, int64_t lddwf, int32_t cin, const float* dkp, const float* mod,
                                    int32_t n_kp, float extent, const float* rowsum, float* contrib, void* stream);
int apr_kpconv_deform_dgeom(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                            const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf, const float* dkp,
                            const float* mod, int32_t n_kp, float extent, const float* rowsum, float* d_dkp, float* d_mod,
                            void* stream);
/* KPConv's other influence functions and aggregation (Predator_APR/models/blocks.py:61-68, 320-345): the five entry points
 * above with two more arguments, influence (0 constant, 1 linear, 2 gaussian) and closest (0 sum, 1 closest); with (1, 0)
 * each launches exactly what its namesake launches (the same bits).  With d2 = |s[nbr[q,h]] - q - KP[q,k]|^2:
 *   constant  w = 1 for every real (neighbour, kernel point)                                              (blocks.py:321-324)
 *   linear    w = max(0, 1 - sqrt(d2) / extent)                                                          (blocks.py:326-329)
 *   gaussian  w = exp(-d2 / (2 sigma^2 + 1e-9)), sigma = 0.3 extent, NOT clipped at the extent (expf)     (blocks.py:331-335)
 *   closest   w[q,k,h] is kept for k = argmin_k d2[q,h,k] alone, the lowest k winning an exact tie (torch.argmin); the
 *             one-hot mask is a constant of the graph (blocks.py:339-342).  Every kernel of a layer finds that kernel point
 *             with the same float32 statement (kpconv.h).
 * Rigid layers (apr_kpconv_weighted_mode: blocks.py:320-372; apr_kpconv_dfeat_contrib_mode: the same lines differentiated
 * with respect to x): every real neighbour takes part.  Deformable layers (apr_kpconv_deform_*_mode, blocks.py:292-358): only
 * the neighbours inside some deformed ball (d2 < extent^2 for some k, blocks.py:298-316) take part -- for the constant and
 * the gaussian influence a real neighbour outside every ball contributes nothing, one inside carries its influence to all
 * 15 kernel points (sum) or to its closest one; min_d2, num and mod are as above.  apr_kpconv_deform_dgeom_mode: d_mod =
 * sum_h w P / num with the mode's w; d_dkp linear as above (masked by the one-hot when closest), gaussian mod / num *
 * sum_{h in range} w 2 diff / (2 sigma^2 + 1e-9) P (no singularity at d = 0: no deviation), constant exactly 0.
 * Shapes, alignment and refusals as the namesakes; an influence outside 0..2 or closest outside 0..1 returns APR_EINVAL
 * before any launch.  No atomics, fixed summation orders: the same bits on every run. */
int apr_kpconv_weighted_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                             const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp, float extent,
                             const float* rowsum, float* wf, int64_t ldwf, int32_t influence, int32_t closest, void* stream);
int apr_kpconv_dfeat_contrib_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                  const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                                  float extent, const float* rowsum, float* contrib, int32_t influence, int32_t closest,
                                  void* stream);
int apr_kpconv_deform_weighted_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                    int32_t H, const float* x, int64_t ldx, int32_t cin, const float* dkp, const float* mod,
                                    int32_t n_kp, float extent, const float* rowsum, float* wf, int64_t ldwf, float* min_d2,
                                    int32_t influence, int32_t closest, void* stream);
int apr_kpconv_deform_dfeat_contrib_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                         int32_t H, const float* dwf, int64_t lddwf, int32_t cin, const float* dkp,
                                         const float* mod, int32_t n_kp, float extent, const float* rowsum, float* contrib,
                                         int32_t influence, int32_t closest, void* stream);
int apr_kpconv_deform_dgeom_mode(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                 const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf, const float* dkp,
                                 const float* mod, int32_t n_kp, float extent, const float* rowsum, float* d_dkp, float* d_mod,
                                 int32_t influence, int32_t closest, void* stream);
/* Rigid KPConv with any kernel-point count (the reference's num_kernel_points; csrc/kpconv_nk.hip): apr_kpconv_weighted_mode
 * and apr_kpconv_dfeat_contrib_mode -- their arguments, contract, influences and aggregations -- for 1 <= n_kp <= 32 with
 * kernel_points f32 [n_kp, 3], wf f32 [nq, ldwf >= n_kp * cin] (wf[q, k * cin + c], k < n_kp; nothing beyond column
 * n_kp * cin is written) and dwf f32 [nq, lddwf >= n_kp * cin].  The two entries above stay built for 15 kernel points and
 * refuse every other count; at n_kp = 15 these give their bits (neighbours accumulate in slot order, kernel points in
 * ascending order, the closest kernel point is the same float32 statement with five index bits).
 * apr_kpconv_weighted_nk: cin % 64 == 0, H <= 128 and 16-byte rows of x and wf run one wave per query on the fp32 MFMA -- one
 * 16-row tile of kernel points for n_kp <= 16, two for 17..32 --, any other cin, H or alignment one thread per (query, kernel
 * point).  apr_kpconv_dfeat_contrib_nk: H <= 128, cin <= 512; rows (q, h) of contrib f32 [nq * H, cin], the rows of padding
 * neighbours untouched; apr_reverse_gather sums them.  There is no atomic form.
 * APR_EINVAL, with a message that names the entry, before anything is read or launched: n_kp outside 1..32, an influence
 * outside 0..2 or closest outside 0..1, H, cin or a leading dimension out of range, a null contrib.  nq = 0 returns APR_OK. */
int apr_kpconv_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                           const float* x, int64_t ldx, int32_t cin, const float* kernel_points, int32_t n_kp, float extent,
                           const float* rowsum, float* wf, int64_t ldwf, int32_t influence, int32_t closest, void* stream);
int apr_kpconv_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                const float* dwf, int64_t lddwf, int32_t cin, const float* kernel_points, int32_t n_kp,
                                float extent, const float* rowsum, float* contrib, int32_t influence, int32_t closest,
                                void* stream);
/* Deformable / modulated KPConv with any kernel-point count (csrc/kpconv_deform_nk.hip): the three apr_kpconv_deform_*_mode
 * entries -- their arguments, contract, influences, aggregations and deviation at d = 0 -- for 1 <= n_kp <= 32 with dkp f32
 * [nq, n_kp, 3], mod f32 [nq, n_kp] or null, min_d2 f32 [nq, n_kp] or null, wf f32 [nq, ldwf >= n_kp * cin] (wf[q, k * cin +
 * c], k < n_kp), dwf f32 [nq, lddwf >= n_kp * cin], d_dkp f32 [nq, n_kp, 3], d_mod f32 [nq, n_kp].  The entries above stay
 * built for 15 kernel points and refuse every other count; at n_kp = 15 these agree with them inside the float32 error
 * bounds of both (not bit for bit: the squared distance is contracted differently).  One wave per query on the fp32 MFMA,
 * one 16-row tile of kernel points for n_kp <= 16, two for 17..32; the closest kernel point is closest_kp_nk's float32
 * statement (five index bits, the lowest index wins a tie) in all three.  The same shape limits: cin % 64 == 0,
 * 64 <= cin <= 512, 1 <= H <= 128, ns > 0, extent > 0, 16-byte aligned rows of x, wf and dwf.
 * APR_EINVAL, with a message that names the entry, before anything is read, written or launched: n_kp outside 1..32, an
 * influence outside 0..2 or closest outside 0..1, a shape or leading dimension out of range, a misaligned row, a null
 * buffer.  nq = 0 returns APR_OK.  No atomics, fixed summation orders: the same bits on every run. */
int apr_kpconv_deform_weighted_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                                  const float* x, int64_t ldx, int32_t cin, const float* dkp, const float* mod, int32_t n_kp,
                                  float extent, const float* rowsum, float* wf, int64_t ldwf, float* min_d2, int32_t influence,
                                  int32_t closest, void* stream);
int apr_kpconv_deform_dfeat_contrib_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr,
                                       int32_t H, const float* dwf, int64_t lddwf, int32_t cin, const float* dkp,
                                       const float* mod, int32_t n_kp, float extent, const float* rowsum, float* contrib,
                                       int32_t influence, int32_t closest, void* stream);
int apr_kpconv_deform_dgeom_nk(const float* q_pts, int64_t nq, const float* s_pts, int64_t ns, const int32_t* nbr, int32_t H,
                               const float* x, int64_t ldx, int32_t cin, const float* dwf, int64_t lddwf, const float* dkp,
                               const float* mod, int32_t n_kp, float extent, const float* rowsum, float* d_dkp, float* d_mod,
                               int32_t influence, int32_t closest, void* stream);
size_t apr_reverse_table_scratch_bytes(int64_t nq, int32_t H, int64_t ns);
int apr_reverse_table_build(const int32_t* nbr, int64_t nq, int32_t H, int64_t ns, int32_t* rev_t, int32_t* start,
                            void* scratch, size_t scratch_bytes, void* stream);
int apr_reverse_gather(const float* src, int32_t c, const int32_t* rev_t, const int32_t* start, int64_t ns, float* out,
                       int64_t ldo, void* stream);
/* The same over the flat positions [t_lo, t_hi) only (src f32 [t_hi - t_lo, c]: their rows), continuing the sums in `out`
 * when accumulate != 0: chunk after chunk in ascending t this is bit for bit one apr_reverse_gather over the whole table
 * with a contribution buffer the size of ONE chunk (the finest KPConv level of one pair needs 400 MB unchunked). */
int apr_reverse_gather_range(const float* src, int32_t c, const int32_t* rev_t, const int32_t* start, int64_t ns,
                             int64_t t_lo, int64_t t_hi, int32_t accumulate, float* out, int64_t ldo, void* stream);

/* mode 0: max_pool(x, inds) (blocks.py:86-102); mode 1: closest_pool(x, inds) (blocks.py:71-83).
 * Index ns addresses an implicit all-zero shadow row. */
int apr_gather_pool(const float* x, int64_t ldx, int64_t ns, int32_t c, const int32_t* inds, int32_t H,
                    int64_t nq, int32_t mode, float* out, int64_t ldo, void* stream);

/* Training path of the pooling gathers (Predator_APR/models/blocks.py:71-102 under lib/trainer.py:142-280): the forward of
 * max_pool that also records which neighbour gave each maximum (amax u8 [nq, c]: the first h at the maximum, H <= 255), and
 * the input gradient of max_pool (mode 0) / closest_pool (mode 1) as a gather over the reverse table of the same index
 * tensor (apr_reverse_table_build): dx[s, c] = sum of dout[q, c] over the entries (q, h) that point at s and were the
 * maximum (mode 0) / the first neighbour (mode 1), in table order -- deterministic, no float atomics. */
int apr_gather_pool_argmax(const float* x, int64_t ldx, int64_t ns, int32_t c, const int32_t* inds, int32_t H, int64_t nq,
                           float* out, int64_t ldo, uint8_t* amax, void* stream);
int apr_gather_pool_backward(const float* dout, int64_t lddo, int32_t c, const int32_t* rev_t, const int32_t* start,
                             int64_t ns, int32_t H, const uint8_t* amax, int32_t mode, float* dx, int64_t lddx, void* stream);

/* get_graph_feature (gcn.py:9-35) as rows: out[(i*k + j), :] = [f_i, f_knn(i,j) - f_i], f32 [n*k, 2c]. */
int apr_edge_features(const float* f, int64_t ldf, int32_t n, int32_t c, const int32_t* knn, int32_t k,
                      float* out, void* stream);

/* Training path (gcn.py:9-35 under Predator_APR/lib/trainer.py:142-280): the input gradient of apr_edge_features from
 * de f32 [n*k, 2c], first half -- d_center[i] = sum_j (de[(i,j), :c] - de[(i,j), c:]) and the neighbours' terms as
 * contribution rows contrib f32 [n*k, c] = de[:, c:]; apr_reverse_gather_range over the reverse table of knn (ns = n,
 * accumulate = 1) then adds every row's contributions in table order: deterministic, no float atomics. */
int apr_edge_features_backward(const float* de, int32_t n, int32_t c, int32_t k, float* d_center, int64_t ldd,
                               float* contrib, void* stream);

/* out[i,:] = max_j leaky(y[i*k+j,:] * scale + shift)  (InstanceNorm2d + LeakyReLU(0.2) + max, gcn.py:67-72). */
int apr_group_max(const float* y, int64_t ldy, int32_t n, int32_t k, int32_t c, const float* scale,
                  const float* shift, float slope, float* out, int64_t ldo, void* stream);

/* Multi-head softmax attention, channel c = d*heads + h (gcn.py:94-116). q f32[n,dim*heads], k/v f32[m,...]. */
int apr_mha(const float* q, const float* k, const float* v, int32_t n, int32_t m, int32_t dim, int32_t heads,
            float* out, void* stream);

/* The same attention for the TRAINING path (Predator_APR/lib/trainer.py:142-280): the forward keeps the probabilities
 * P f32 [heads, n, m]; the backward turns them and dout f32 [n, dim*heads] into dq, dk, dv (dS f32 [heads, n, m]: scratch).
 * Fixed summation orders, no float atomics: the same bits every run.  No limit on m. */
int apr_mha_train_forward(const float* q, const float* k, const float* v, int32_t n, int32_t m, int32_t dim, int32_t heads,
                          int32_t vdim, float* P, float* out, void* stream);
int apr_mha_train_backward(const float* q, const float* k, const float* v, const float* P, const float* dout, int32_t n,
                           int32_t m, int32_t dim, int32_t heads, int32_t vdim, float* dS, float* dq, float* dk, float* dv,
                           void* stream);
/* vdim: channels per head of v / out / dout (0: = dim).  vdim = 1 with heads = 1 is the cross-saliency
 * softmax(<a_i, b_j> / T) @ s of Predator_APR/models/architectures.py:176-181 (q = a * sqrt(dim) / T). */

/* apr_mha with q / k / v handed over HEAD-MAJOR (channel h*dim + d: the caller permutes the output channels of the
 * three projections, gcn.py:101-108) and out in apr_mha's interleaved layout; fp32 MFMA, dim = 64 only, q / k / v
 * 16-byte aligned, no limit on m. */
int apr_mha_headmajor(const float* q, const float* k, const float* v, int32_t n, int32_t m, int32_t dim,
                      int32_t heads, float* out, void* stream);

/* Geometric cross attention ('cross_cat': MultiHeadedAttentionCat, Predator_APR/models/gcn.py:131-156).  With P the
 * attention's probabilities (scale 1 / sqrt(dim)), c0 f32 [n, 3] the queries' coordinates and c1 f32 [m, 3] the keys':
 *   y[i, e*heads + h], e in [0, dim + 7):  e < dim: sum_j P_ij v[j, e, h];  dim .. dim+2: soft = sum_j P_ij c1[j];
 *   dim+3 .. dim+5: aug1 = soft - c0[i];  dim+6: aug2 = ||aug1||_2.
 * y has leading dimension ldy >= (dim + 7) * heads; columns from (dim + 7) * heads on are not written.
 * _headmajor: the inference kernel on the fp32 MFMA; q / k / v HEAD-MAJOR and 16-byte aligned as for apr_mha_headmajor,
 *   dim = 64 only, no limit on m.
 * _train_forward: q / k / v interleaved, dim <= 1024; keeps P f32 [heads, n, m].
 * _train_backward: dy f32 [n, ldy] (the gradient of y, same layout) -> dq, dk, dv; y as the forward wrote it; dS f32
 *   [heads, n, m] is scratch.  The coordinates take no gradient; the aug2 term is 0 where aug2 == 0.  Fixed summation
 *   orders, no float atomics: the same bits every run. */
int apr_mha_cat_headmajor(const float* q, const float* k, const float* v, const float* c0, const float* c1, int32_t n,
                          int32_t m, int32_t dim, int32_t heads, float* y, int64_t ldy, void* stream);
int apr_mha_cat_train_forward(const float* q, const float* k, const float* v, const float* c0, const float* c1, int32_t n,
                              int32_t m, int32_t dim, int32_t heads, float* P, float* y, int64_t ldy, void* stream);
int apr_mha_cat_train_backward(const float* q, const float* k, const float* v, const float* c0, const float* c1,
                               const float* P, const float* y, const float* dy, int64_t ldy, int32_t n, int32_t m,
                               int32_t dim, int32_t heads, float* dS, float* dq, float* dk, float* dv, void* stream);

/* The overlap-attention module of one scan pair (GCN.forward, Predator_APR/models/gcn.py:171-205: 'self' = SelfAttention
 * :38-77 on each cloud, 'cross' = AttentionalPropagation :119-128 in both directions with the residual add) as ONE call.
 * The module issued 62 library calls and 6 concatenations per pair on ~1.4 k points -- the largest share of the 110 calls
 * per pair that kept KPFCNN's scheduler thread, not the GPU, at its limit.  Same kernels, arguments and order as the
 * modules' own (apr_knn, apr_edge_features, apr_dense_gemm_bf3, apr_norm_params, apr_group_max, apr_instance_norm_act,
 * apr_mha_headmajor, apr_affine_act): same bits; the concatenations become column slices of one buffer.
 *   c % 64 == 0, c / heads == 64, k + 1 <= 16; weights: apr_spconv_pack_weights_bf3(K = 1) images ([cin, cout] as the
 *   layers' own Linear / Conv1d weights transposed; wq / wk / wv with their output channels head-major, as
 *   apr_mha_headmajor reads them); biases f32, 16-byte aligned, nullable.  x0 [n0, c] / x1 [n1, c] in, out0 / out1 out. */
#define APR_GCN_MAX_LAYERS 8
typedef struct apr_gcn_layer {
  int32_t kind;                   /* 0: self attention, 1: cross attention */
  int32_t k, heads;               /* self: neighbours of the kNN graph; cross: attention heads */
  float eps1, eps2, eps3;         /* self: InstanceNorm eps of in1 / in2 / in3; cross: eps1 = mlp[1].eps */
  const void *w1, *w2, *w3;       /* self: conv1 [2c, c], conv2 [2c, 2c], conv3 [4c, c]; cross: w1 = mlp[0] [2c, 2c], w2 = mlp[3] [2c, c] */
  const float *b1, *b2;           /* cross: biases of mlp[0], mlp[3] */
  const void *wq, *wk, *wv, *wm;  /* cross: the three projections (head-major) and merge, [c, c] */
  const float *bq, *bk, *bv, *bm;
} apr_gcn_layer;
typedef struct apr_gcn_desc {
  int32_t n_layers, c;
  apr_gcn_layer layer[APR_GCN_MAX_LAYERS];
} apr_gcn_desc;
size_t apr_gcn_scratch_bytes(const apr_gcn_desc* d, int32_t n0, int32_t n1);
int apr_gcn_forward(const apr_gcn_desc* d, const float* pts0, int32_t n0, const float* pts1, int32_t n1, const float* x0,
                    int64_t ldx0, const float* x1, int64_t ldx1, float* out0, int64_t ldo0, float* out1, int64_t ldo1,
                    void* scratch, size_t scratch_bytes, void* stream);

/* out[i] = sum_j softmax_j(<a_i, b_j> / temperature) * w[j]  (cross saliency, architectures.py:176-181). */
int apr_softmax_matvec(const float* a, const float* b, const float* w, int32_t n, int32_t m, int32_t c,
                       float temperature, float* out, void* stream);
/* The same with b handed over transposed (bt [c, m] row-major): coalesced reads, several queries per workgroup; the
 * result has the same bits. */
int apr_softmax_matvec_bt(const float* a, const float* bt, const float* w, int32_t n, int32_t m, int32_t c,
                          float temperature, float* out, void* stream);
/* The same on the fp32 MFMA: a and b row-major as in apr_softmax_matvec, 16-byte aligned, c in {32, 64, 128, 256}, any
 * m; equal to fp32 summation order. */
int apr_softmax_matvec_mfma(const float* a, const float* b, const float* w, int32_t n, int32_t m, int32_t c,
                            float temperature, float* out, void* stream);

/* y[i] = clamp(sigmoid(x[i*ldx]), 0, 1), NaN/Inf -> 0  (architectures.py:131-134,203-207). */
int apr_score_head(const float* x, int64_t ldx, int64_t n, float* y, void* stream);

/* ------------------------------------------------------------------------
 * Adjacent components: APG aggregation and Chamfer 1-NN sums
 * ---------------------------------------------------------------------- */

/* out = pts @ R^T + t in fp32, T16_dev = row-major 4x4 on the device
 * (apply_transform, FCGF_APR/lib/complement_data_loader.py:65-70). */
int apr_transform_points(const float* pts, int64_t n, const float* T16_dev, float* out, void* stream);

/* Keep the points with |p|^2 < max_i |key_i|^2, order preserved
 * (crop of the aggregated complement frames, complement_data_loader.py:620-628).
 * out f32[<=n,3]; *n_out_dev device counter. */
size_t apr_crop_scratch_bytes(int64_t n);
int apr_crop_to_radius(const float* key_pts, int64_t n_key, const float* pts, int64_t n, float* out,
                       int32_t* n_out_dev, void* scratch, size_t scratch_bytes, void* stream);

/* *out_dev (f64) = sum_i min_j |a_i - b_j|^2 -- one direction of chamferdist.ChamferDistance()(a, b) as used by
 * chamfer_distance (FCGF_APR/lib/complement_trainer.py:188-196).  scratch >= 4*n bytes. */
int apr_chamfer_sum(const float* a, int64_t n, const float* b, int64_t m, double* out_dev, void* scratch,
                    size_t scratch_bytes, void* stream);

/* Exact 1-NN of every row of a [n,3] among the rows of b [m,3] in fp32, (dx^2 + dy^2) + dz^2 with every operation rounded
 * (no contraction): out_packed[i] = (bits(d^2) << 32) | j, ties -> the smallest j.  sum_dev (may be NULL): f64 sum of
 * the n minima in a fixed order (bit-reproducible).  The arg-min is what the backward of the Chamfer term needs
 * (Predator_APR/lib/trainer.py:131-140, 179-183; FCGF_APR/lib/complement_trainer.py:188-196, 446-448): the gradient
 * of sum_i min_j |a_i - b_j|^2 reaches a_i and b_argmin(i) only.
 * cell > 0: a uniform grid over b answers the queries whose neighbour lies within ~6.5 cells (ring after ring), the rest
 * fall through to the full search -- the same bits as cell = 0 (brute force, scratch unused) for every input.
 * A good `cell` is several voxel sizes (the clouds here carry one point per 0.3 m voxel; the Python layer passes 1.2 m). */
size_t apr_nn3_scratch_bytes(int64_t n, int64_t m);
int apr_nn3(const float* a, int64_t n, const float* b, int64_t m, float cell, uint64_t* out_packed, double* sum_dev,
            void* scratch, size_t scratch_bytes, void* stream);
/* nb independent searches in ONE call (the clouds of a training batch: FCGF_APR/lib/complement_trainer.py:424-449 runs the
 * Chamfer term cloud by cloud): rows a_offsets_host[s] .. [s + 1] of a are searched among rows b_offsets_host[s] .. [s + 1] of
 * b only (the grid's cells carry the cloud index).  out_packed[i] = (bits(d^2) << 32) | j with j the GLOBAL row of b;
 * sums_dev[nb]: per-cloud sums of the minima (fixed order), multiplied by sum_scale_host[s] when that is given (1 / rows: the
 * mean the Chamfer term divides by, without a host->device copy).  Same bits per cloud as apr_nn3 on that cloud alone.
 * scratch: apr_nn3_scratch_bytes(total rows of a, total rows of b); cell > 0. */
int apr_nn3_batch(const float* a, const int64_t* a_offsets_host, const float* b, const int64_t* b_offsets_host, int32_t nb,
                  float cell, uint64_t* out_packed, double* sums_dev, const double* sum_scale_host, void* scratch,
                  size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Predator_APR's descriptor loss, MetricLoss (Predator_APR/lib/loss.py:16-178).  Deterministic: no float atomics,
 * fixed reduction order, the same bits run to run.  Nothing is sized by (#src rows) x (#tgt rows).
 * ---------------------------------------------------------------------- */

/* loss.py:114-123.  corr i64[n_corr,2].  gt f32[n_src + n_tgt] = the 0/1 overlap labels (src part, then tgt part);
 * src_idx i32[n_src] / tgt_idx i32[n_tgt] = the unique first / second columns of corr in ASCENDING order (the reference
 * takes them from a Python set, whose order is unspecified); counts3 i32[3] on the device = #src_idx, #tgt_idx, their sum. */
int apr_overlap_labels(const int64_t* corr, int64_t n_corr, int64_t n_src, int64_t n_tgt, float* gt, int32_t* src_idx,
                       int32_t* tgt_idx, int32_t* counts3, void* stream);

/* loss.py:79-97, get_weighted_bce_loss.  pred / gt f32[n]; n_dev (may be NULL): device count that replaces n when it is
 * smaller.  out8 f32[8] = loss, w_negative, precision, recall, tp, fp, fn, n.  Each log is clamped at -100 (nn.BCELoss),
 * round() is half-to-even (0.5 predicts 0), a zero denominator gives precision / recall 0 (sklearn). */
size_t apr_weighted_bce_scratch_bytes(void);
int apr_weighted_bce_forward(const float* pred, const float* gt, int64_t n, const int32_t* n_dev, float* out8, void* scratch,
                             size_t scratch_bytes, void* stream);
/* d loss / d pred = grad_out[0] * w_i / n * (p - g) / max((1 - p) p, 1e-12), written to dpred[i], or to
 * dpred[scatter_pos[i]] when scatter_pos is given (the gather of loss.py:142-144 undone; positions are unique). */
int apr_weighted_bce_backward(const float* pred, const float* gt, int64_t n, const int32_t* n_dev, const float* out8,
                              const float* grad_out, const int32_t* scatter_pos, float* dpred, void* stream);

/* loss.py:132-138: for scores = a[a_idx] @ b[b_idx].T (never formed) row_arg i32[na] = arg-max along each row and
 * col_arg i32[nb] = arg-max along each column, as positions in the index lists; ties go to the lowest position.
 * *na_dev / *nb_dev: device-side list lengths (<= na_max / nb_max, which size the grids); neither may be NULL.  Every
 * listed index must be a row of its matrix (the lists apr_overlap_labels writes are): the entry point does not know the
 * row counts and does not check.  d must be 32; exact fp32 (v_mfma_f32_16x16x4_f32). */
int apr_gathered_argmax(const float* a, const int32_t* a_idx, const int32_t* na_dev, int64_t na_max, const float* b,
                        const int32_t* b_idx, const int32_t* nb_dev, int64_t nb_max, int32_t d, int32_t* row_arg,
                        int32_t* col_arg, void* stream);

/* loss.py:136-144: dist[i] = |rot src + trans - tgt| between every listed point and its arg-max partner (src list, then
 * tgt list), labels = dist < radius, sel_scores = scores_saliency at the listed points, pos = their position in
 * scores_saliency [n_src + n_tgt]. */
int apr_saliency_labels(const float* src_pcd, const float* tgt_pcd, const float* rot9, const float* trans3,
                        const int32_t* src_idx, const int32_t* tgt_idx, const int32_t* counts3, const int32_t* row_arg,
                        const int32_t* col_arg, const float* scores_saliency, int64_t n_src, int64_t n_tgt, float radius,
                        float* labels, float* sel_scores, int32_t* pos, float* dist, void* stream);

/* loss.py:153-155: filt i32[<= n_corr] = the rows of corr with |rot src + trans - tgt| < thresh, in order; *count on
 * the device. */
int apr_circle_select(const int64_t* corr, int64_t n_corr, const float* src_pcd, int64_t n_src, const float* tgt_pcd,
                      int64_t n_tgt, const float* rot9, const float* trans3, float thresh, int32_t* filt, int32_t* count,
                      void* stream);

/* loss.py:156-162: anchor k = corr[filt[choice[k]]], k < p <= 512: rows (a_row / b_row, -1 where choice[k] is outside the
 * filtered list: an absent anchor), transformed src point / tgt point, the two feature rows (d == 32). */
int apr_circle_gather(const int64_t* corr, const int32_t* filt, const int32_t* count, const int64_t* choice, int32_t p,
                      const float* src_pcd, const float* tgt_pcd, const float* src_feats, const float* tgt_feats, int32_t d,
                      const float* rot9, const float* trans3, int32_t* a_row, int32_t* b_row, float* a_pts, float* b_pts,
                      float* a_feats, float* b_feats, void* stream);

/* loss.py:34-77 (get_circle_loss, get_recall) and :166-167.  Either the gathered anchors (coords_dist == NULL), from
 * which both distance matrices are formed on the fly, sqrt(clamp(., 1e-12)) as lib/utils.py:78-98, or the two dense
 * [na, nb] matrices themselves.  params_host f32[7] = pos_radius, safe_radius, pos_optimal, neg_optimal, pos_margin,
 * neg_margin, log_scale.  st_a f32[na,8] / st_b f32[nb,8]: per-row / per-column records the backward reads.  out4 =
 * circle_loss, recall, #row_sel, #col_sel; an empty selection gives NaN as mean() of nothing.  nn i32[na] (may be
 * NULL): arg-min of feats_dist along each row.  na, nb <= 512. */
int apr_circle_forward(const float* a_feats, const float* a_pts, const int32_t* a_row, int32_t na, const float* b_feats,
                       const float* b_pts, const int32_t* b_row, int32_t nb, const float* coords_dist,
                       const float* feats_dist, const float* params_host, float* st_a, float* st_b, float* out4, int32_t* nn,
                       void* stream);
/* d circle_loss / d a_feats, d b_feats (anchors; zero gradient where the 1e-12 clamp binds), or / d feats_dist (dense). */
int apr_circle_backward(const float* a_feats, const float* a_pts, const int32_t* a_row, int32_t na, const float* b_feats,
                        const float* b_pts, const int32_t* b_row, int32_t nb, const float* coords_dist,
                        const float* feats_dist, const float* params_host, const float* st_a, const float* st_b,
                        const float* out4, const float* grad_out, float* d_a, float* d_b, float* d_feats_dist, void* stream);
/* d_full[row[k]] = sum of d_anchor[k'] over the anchors k' that share the row, in ascending k' (loss.py:161-162 undone);
 * rows that no anchor names are left as they are (zero them first). */
int apr_circle_scatter(const float* d_anchor, const int32_t* row, int32_t p, int32_t d, float* d_full, int64_t n_rows,
                       void* stream);

/* ------------------------------------------------------------------------
 * Point-to-point ICP, the pose refinement in front of the aggregated point cloud:
 *   o3d.pipelines.registration.registration_icp(next, curr, 0.2, eye(4), TransformationEstimationPointToPoint(),
 *   ICPConvergenceCriteria(max_iteration=200)) at FCGF_APR/lib/complement_data_loader.py:369-405 (_get_icp,
 *   _get_neighbourhood_icp), FCGF_APR/lib/data_loaders.py:460-463, Predator_APR/datasets/kitti.py:201-204, 424-428, 558-560.
 *
 * nb independent problems in ONE call (the 2k complement frames of a key frame, or a batch of pairs).  Problem i moves the
 * source rows src_offsets_host[i] .. [i + 1] onto target SEGMENT tgt_of_problem_host[i] (rows tgt_offsets_host[s] .. [s + 1]
 * of tgt; NULL: segment i, n_tgt == nb), so several problems may share one target.  init f64[nb,16] (row-major 4x4).
 * nb, n_tgt <= 64.
 *
 * open3d >= 0.12 RegistrationICP: evaluate T = init; up to max_iteration times { U = Umeyama (rotation + translation, no
 * scale) of the corresponded pairs, T = U T, evaluate again, stop when |d fitness| < relative_fitness and |d rmse| <
 * relative_rmse }.  No correspondences: U is the identity.  max_iteration = 0: the evaluation of init.
 * Arithmetic: p = fl32(T s) from the ORIGINAL fp32 row and the cumulative fp64 T, ((T0 x + T1 y) + T2 z) + T3 in fp64,
 * rounded once; d^2 = (dx^2 + dy^2) + dz^2 in fp32, every operation rounded; a correspondence needs d^2 < fl32(max_dist)^2
 * (fp32 product) STRICTLY; ties go to the smallest target row.  Means, cross-covariance and sum d^2 in fp64, fixed order:
 * the same bits run to run and for a problem alone or inside a batch.
 *
 * result f64[nb, APR_ICP_RECORD_DOUBLES]: T[16], fitness = #corr / #source rows, inlier_rmse = sqrt(sum d^2 / #corr) (0
 * without correspondences), #corr, iterations run.  corr i32[total source rows] (may be NULL): the target row of every
 * source row, counted from the start of its target segment, or -1.
 * The iteration runs on the device: the host enqueues rounds in chunks and reads the per-problem `done` flags once per
 * chunk, one chunk behind the queue; kernels of a finished problem return at once.  Synchronises `stream` before it
 * returns.
 *
 * Range: the search grid's cell is fl32(max_dist) * 1.01f, its origin the minimum of each target segment.  A segment may span
 * at most 40960 cells per axis (extent < 41369 * max_dist: 8.2 km at max_dist = 0.2, 41 m at 1e-3).  Up to that index the
 * 1 % widening provably covers the float32 rounding of a cell coordinate, so that no target within max_dist is missed; the
 * packed cell key itself would end at 2^17.  A segment beyond it: APR_ERANGE; no kernel searches such a grid, result holds
 * init (iterations 0) and corr is not written.  The flag travels with the first copy of the `done` flags and is looked at
 * after the synchronisation above.  Source rows may lie anywhere: a row too far from its segment has no correspondence. */
#define APR_ICP_RECORD_DOUBLES 20
size_t apr_icp_scratch_bytes(int64_t n_src_total, int64_t n_tgt_total, int32_t nb);
int apr_icp_batch(const float* src, const int64_t* src_offsets_host, const float* tgt, const int64_t* tgt_offsets_host,
                  int32_t n_tgt, const int32_t* tgt_of_problem_host, int32_t nb, const double* init, double max_dist,
                  int32_t max_iteration, double relative_fitness, double relative_rmse, double* result, int32_t* corr,
                  void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Mutual nearest-neighbour matching, inlier ratios and the pair-list RANSAC of the Predator tester
 * (Predator_APR/lib/benchmark_utils.py:187-211, :227-268, :271-295).  No n_src x n_tgt array exists on this path.
 * ------------------------------------------------------------------------ */

/* benchmark_utils.py:271-295 (mutual_selection) + np.where (:201, :261) on the arg-max vectors apr_gathered_argmax writes:
 * pairs i32[min(n_src_max, n_tgt_max), 2] (row-major) = (i, row_arg[i]) for every i with col_arg[row_arg[i]] == i, in
 * ascending i; *count i32 on the device = their number.  Entries of `pairs` past *count are not written.  *n_src_dev /
 * *n_tgt_dev: device-side lengths of row_arg / col_arg (clamped to n_src_max / n_tgt_max; NULL: the max).  Ties were
 * settled by the arg-max (lowest index, as np.argmax); a row_arg outside [0, n_tgt) is no pair.  Positions come from
 * ballot + popcount + a block scan: the same bits run to run. */
int apr_mutual_select(const int32_t* row_arg, const int32_t* n_src_dev, int64_t n_src_max, const int32_t* col_arg,
                      const int32_t* n_tgt_dev, int64_t n_tgt_max, int32_t* pairs, int32_t* count, void* stream);

/* benchmark_utils.py:246-266 (get_inlier_ratio) in one launch.  src_pcd f32[n_src,3], tgt_pcd f32[n_tgt,3], rot9 f32[9]
 * (row-major 3x3), trans3 f32[3], row_arg i32[n_src] (the arg-max along each score row), pairs i32[pairs_cap,2] and *count
 * (device) as apr_mutual_select leaves them.  q = rot p + trans and |q - t| in float32, every operation rounded, sums left
 * to right.  dist_wo f32[n_src]: distance of every source point to tgt[row_arg]; dist_w f32[pairs_cap]: the same over the
 * first *count pairs (the rest is not written).  out8 f32[8] = ratio_wo = #(dist_wo < threshold) / n_src, ratio_w =
 * #(dist_w < threshold) / *count (NaN for an empty list: the mean of nothing), the two integer counts, n_src, *count, 0, 0.
 * The counts are integer sums; n_src < 2^24 so that they are exact as float32.  An index outside its cloud gives +inf. */
int apr_inlier_ratio(const float* src_pcd, int64_t n_src, const float* tgt_pcd, int64_t n_tgt, const float* rot9,
                     const float* trans3, const int32_t* row_arg, const int32_t* pairs, const int32_t* count,
                     int64_t pairs_cap, float threshold, float* dist_wo, float* dist_w, float* out8, void* stream);

/* np.argmax(scores, 1) / np.argmax(scores, 0) of a dense row-major f32[n,m] matrix the caller already holds (the
 * compatibility form of mutual_selection): row_arg i32[n], col_arg i32[m], ties to the lowest index.  NaN never wins. */
int apr_dense_argmax(const float* scores, int64_t n, int64_t m, int32_t* row_arg, int32_t* col_arg, void* stream);

/* benchmark_utils.py:205-210: open3d <= 0.11 RegistrationRANSACBasedOnCorrespondence(source, target, corres, max_dist,
 * TransformationEstimationPointToPoint(false), ransac_n = 4, RANSACConvergenceCriteria(max_iter, max_validation)).
 * PARITY UNPINNED (open3d is not part of this build): restated from the open3d 0.10 source --
 *   for it < min(max_iter, max_validation): draw 4 entries of the pair list (here the counter RNG (seed, it, slot) of the
 *   other RANSAC entries, index = high word of rng * n_pairs); T = Kabsch without scale (fp64); NO edge-length or distance
 *   checker; score T geometrically over the WHOLE source cloud: an inlier is a transformed source point whose nearest
 *   target point lies within max_dist (fp32 d^2 < fl32(max_dist^2), as apr_ransac_pose_geometric).
 * The best hypothesis: more inliers (fitness), then lower rmse, then lower it.  A hypothesis without inliers never
 * replaces the default result; n_pairs < 4 returns it at once: identity, fitness 0, best_iteration -1.
 * pairs i32[n_pairs,2] on the device, rows (source index, target index); n_pairs is a HOST value (one 4-byte fetch of
 * apr_mutual_select's count).  A pair outside its cloud is read as (0, 0).  result_host f64[20] as apr_ransac_pose
 * (T[16], inliers, rmse, best iteration, hypotheses scored).  Synchronises `stream`. */
size_t apr_ransac_pairs_geometric_scratch_bytes(int64_t n0, int64_t n1, int64_t n_pairs, int64_t max_iter,
                                                int64_t max_validation);
int apr_ransac_pose_pairs_geometric(const float* xyz0, int64_t n0, const float* xyz1, int64_t n1, const int32_t* pairs,
                                    int64_t n_pairs, double max_dist, int64_t max_iter, int64_t max_validation, uint64_t seed,
                                    void* scratch, size_t scratch_bytes, double* result_host, void* stream);

/* ------------------------------------------------------------------------
 * Multiway registration, the default route to the poses of the aggregated point cloud (use_old_pose and not
 * debug_use_old_complement): FCGF_APR/lib/complement_data_loader.py:408-516 (pairwise_registration, full_registration,
 * multiway_registration), Predator_APR/datasets/kitti.py:197-297.  PARITY UNPINNED (open3d is not part of this build): both
 * entries implement the restatement of DESIGN section 19.
 * ------------------------------------------------------------------------ */

/* o3d.pipelines.registration.get_information_matrix_from_point_clouds(source, target, max_dist, T)
 * (complement_data_loader.py:417-419, kitti.py:207-209) for nb problems in ONE call.  src / offsets / tgt / segments /
 * tgt_of_problem_host / nb as apr_icp_batch.  T f64 on the device, problem i at T + i * t_stride (row-major 4x4, the first 12
 * doubles are read; t_stride >= 12): apr_icp_batch's result records as they lie with t_stride = APR_ICP_RECORD_DOUBLES.
 * Association = apr_icp_batch's evaluation step with its arithmetic contract: p = fl32(T s) from the original fp32 row,
 * d^2 in fp32 with every operation rounded, d^2 < fl32(max_dist)^2 strictly, ties to the smallest target row; search-grid
 * cell 1.01 * max_dist, APR_ERANGE from the grid's status word (nothing is written then).
 * sums f64[nb, APR_INFORMATION_SUMS] (may be NULL) over the matched TARGET rows (x, y, z) -- the target's own coordinates,
 * products in fp64 from the fp32 values --: n, x, y, z, xx, yy, zz, xy, xz, yz.  Fixed order (xor butterfly per wave,
 * (w0 + w1) + (w2 + w3) per workgroup, the partial rows of a problem by one workgroup), no atomics: the same bits run to run
 * and for a problem alone or inside a batch.
 * info f64[nb,36] = Lambda row-major, components (alpha, beta, gamma, tx, ty, tz) = sum G^T G over g1 = (0, z, -y, 1, 0, 0),
 * g2 = (-z, 0, x, 0, 1, 0), g3 = (y, -x, 0, 0, 0, 1): rotation block [[yy + zz, -xy, -xz], [-xy, xx + zz, -yz],
 * [-xz, -yz, xx + yy]], translation block n I, rotation-translation block [[0, -z, y], [z, 0, -x], [-y, x, 0]] and its
 * transpose.  No correspondence: Lambda = 0.  corr i32[total source rows] (may be NULL) as apr_icp_batch.
 * Synchronises `stream` (the grid's status word). */
#define APR_INFORMATION_SUMS 10
size_t apr_information_scratch_bytes(int64_t n_src_total, int64_t n_tgt_total, int32_t nb);
int apr_information_batch(const float* src, const int64_t* src_offsets_host, const float* tgt, const int64_t* tgt_offsets_host,
                          int32_t n_tgt, const int32_t* tgt_of_problem_host, int32_t nb, const double* T, int64_t t_stride,
                          double max_dist, double* info, double* sums, int32_t* corr, void* scratch, size_t scratch_bytes,
                          void* stream);

/* o3d.pipelines.registration.global_optimization(pose_graph, GlobalOptimizationLevenbergMarquardt(),
 * GlobalOptimizationConvergenceCriteria(), GlobalOptimizationOption(max_correspondence_distance, edge_prune_threshold,
 * reference_node = 0)) (complement_data_loader.py:453-461, kitti.py:243-251) for ng graphs in ONE launch, one workgroup per
 * graph, fp64 throughout; every pointer is a device pointer.  Graph g owns nodes node_offsets[g] .. [g + 1] (1 .. 8) and
 * edges edge_offsets[g] .. [g + 1] (0 .. 28).  edges i32[n_edges, 3] = (source, target, uncertain) with LOCAL node numbers,
 * source < target.  Edge e: transform at T + e * t_stride (row-major 4x4, 12 doubles read; ICP records as they lie with
 * t_stride = APR_ICP_RECORD_DOUBLES), information matrix info[e * 36 ..].  init_poses f64[n_nodes, 16], or NULL: the
 * odometry chain P_0 = I, odo <- T_(j,j+1) odo, P_(j+1) = odo^-1 (:426-438), which needs an edge (j, j + 1) for every j.
 * The algorithm (error vector, Jacobian, line process, LM loop, default criteria, pruning and the second pass) is DESIGN
 * section 19.  H and b are assembled by one owner thread per entry over the edges in ascending order, no atomics: a graph
 * gives the same bits alone or in a batch, and run to run.  reference_node compensation is NOT applied; P_0^-1 P_i, the only
 * product the callers use (:508-509), does not depend on it.
 * poses f64[n_nodes,16]; confidence f64[n_edges] after the FIRST pass (1 for certain edges); kept i32[n_edges] (0 = pruned);
 * iterations i32[ng,2] (outer iterations of both passes); status i32[ng]: 0 ok, 1 line-process weight mu = 0 (every Lambda(5,5)
 * zero or no edge: the initial poses are returned, no division), 2 the same after pruning (first-pass poses), 3 a pivot of
 * the damped system was not positive and finite (poses of the last accepted step), 4 malformed graph (node / edge counts,
 * an edge outside source < target < n, a missing odometry edge without init_poses: nothing else of that graph is written).
 * Does not synchronise. */
#define APR_POSEGRAPH_MAX_NODES 8
int apr_posegraph_optimize(const int32_t* node_offsets, const int32_t* edge_offsets, int32_t ng, const int32_t* edges,
                           const double* T, int64_t t_stride, const double* info, const double* init_poses,
                           double max_correspondence_distance, double edge_prune_threshold, double preference_loop_closure,
                           double* poses, double* confidence, int32_t* kept, int32_t* iterations, int32_t* status,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APR_HIP_H */

"""Host oracle of APG aggregation and the ground-truth pairs (apr_amd/csrc/apg.hip, points.hip's k_radius through
apr_amd/fcgf/lib/apg.py): numpy only.

Two kinds of statement, kept apart:
  * float64 with an error BAND -- what any correct float32 evaluation must satisfy whatever its operation order or use of
    FMA (transform64's componentwise bound, crop_decision's must_keep / must_drop outside the band);
  * the float32 statement bit for bit -- keep_f32 and radius_pairs_f32 spell out one operation order, every product and sum
    rounded, (x + y) + z, which numpy's float32 element-wise arithmetic reproduces.  The crop's kernels compute exactly this
    (csrc/apg.hip: sqnorm_rn, contraction off; sqnorm_contracted below restates what a fused build computes instead, and
    tests/apg_cases.py plants rows on which the two differ).  k_radius and d2_rn write the same order with the __f*_rn
    intrinsics, which this toolchain compiles to plain operators that may fuse into an FMA: for the pairs the bit-for-bit
    comparison holds on inputs where no d2 is within an ulp of r^2 or of another candidate's d2 of the same query, and
    tests/test_apg_oracle_cpu.py asserts that of every pair input (the fused variants of d2 give the same list).  The
    planted pairs use exactly representable values, on which all variants agree.

`u` is the float32 unit round-off 2^-24 throughout."""
import numpy as np

U = 2.0 ** -24


def _rows_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == 3, a.shape
    return a


# ------------------------------------------------------------------------------------------------------ transform
def transform64(pts_f32, T):
    """pts @ R.T + t in float64, T rounded to float32 first as apg.apply_transform does.
    -> (out [n,3] float64, bound [n,3]): |fl32(result) - out| <= bound componentwise for a four-term float32 dot product
    evaluated in any order, with or without FMA (gamma_4 = 4u / (1 - 4u) < 5u)."""
    p = _rows_f32(pts_f32).astype(np.float64)
    T32 = np.asarray(T).astype(np.float32).reshape(4, 4)
    R, t = T32[:3, :3].astype(np.float64), T32[:3, 3].astype(np.float64)
    out = p @ R.T + t
    bound = 5 * U * (np.abs(p) @ np.abs(R).T + np.abs(t))
    return out, bound


# ----------------------------------------------------------------------------------------------------------- crop
def sqnorm_f32(p):
    """((x*x + y*y) + z*z) with every operation rounded to float32."""
    p = _rows_f32(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return (x * x + y * y) + z * z


def sqnorm_contracted(p, how):
    """What a build that fuses the squared norm computes: "fma1" = fma(x, x, y*y) + z*z, "fma2" = fma(z, z, fma(y, y, x*x))
    (the two forms the compiler chose for x*x + y*y + z*z written plainly).  A float32 square is exact in float64 and the sum
    with a float32 of similar size too, so one rounding to float32 restates the FMA."""
    p = _rows_f32(p)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    f32 = lambda a: a.astype(np.float32)
    if how == "fma1":
        return f32(x * x + f32(y * y).astype(np.float64)) + f32(z * z)
    if how == "fma2":
        return f32(z * z + f32(y * y + f32(x * x).astype(np.float64)).astype(np.float64))
    raise KeyError(how)


def crop_decision(key_f32, pts_f32):
    """The crop `|p|^2 < max |key|^2` (complement_data_loader.py:620-628) decided in float64.
    -> must_keep, must_drop, band (bool [n]) and keep_f32 (bool [n]).
    Three float32 squares summed in any order err by at most 3u relative, on both sides of the comparison: a row whose
    float64 |s - L| exceeds 8u (s + L) has one right answer (must_keep / must_drop); the others form the band.
    keep_f32 is the float32 statement sqnorm_f32(p) < max sqnorm_f32(key)."""
    key, pts = _rows_f32(key_f32), _rows_f32(pts_f32)
    s = (pts.astype(np.float64) ** 2).sum(1)
    L = float((key.astype(np.float64) ** 2).sum(1).max())
    band = np.abs(s - L) <= 8 * U * (s + L)
    must_keep = (s < L) & ~band
    must_drop = (s >= L) & ~band
    keep_f32 = sqnorm_f32(pts) < sqnorm_f32(key).max() if len(pts) else np.zeros(0, bool)
    return must_keep, must_drop, band, keep_f32


def _row_hash(rows):
    b = np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 3).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (b[:, 0] * np.uint64(0x9E3779B97F4A7C15)) ^ (b[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F))
        h = (h ^ (h >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9) ^ (b[:, 2] * np.uint64(0x94D049BB133111EB))
    return h


def match_rows(out_rows, in_rows):
    """Source index in `in_rows` of every row of `out_rows`, by the rows' 12 bytes (-> int64 [len(out_rows)]).
    The input rows must be bitwise unique (asserted); an output row that is no bitwise copy of an input row raises."""
    out_rows, in_rows = _rows_f32(out_rows), _rows_f32(in_rows)
    ib = in_rows.view(np.uint32).reshape(-1, 3)
    ob = out_rows.view(np.uint32).reshape(-1, 3)
    h = _row_hash(in_rows)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    same = np.flatnonzero(hs[1:] == hs[:-1])
    if len(same):                                   # equal hashes: equal rows, or (never seen) a 64-bit collision
        dup = (ib[order[same]] == ib[order[same + 1]]).all(1)
        assert not dup.any(), f"match_rows: input rows {order[same][dup][:4]} and {order[same + 1][dup][:4]} are bit-equal"
        raise AssertionError("match_rows: 64-bit hash collision between distinct input rows; change the hash constants")
    if len(out_rows) == 0:
        return np.zeros(0, np.int64)
    assert len(in_rows), "match_rows: output rows but no input rows"
    pos = np.minimum(np.searchsorted(hs, _row_hash(out_rows)), len(hs) - 1)
    src = order[pos].astype(np.int64)
    bad = np.flatnonzero((ib[src] != ob).any(1))
    assert len(bad) == 0, (f"match_rows: {len(bad)} output rows are no bitwise copy of an input row, first at output "
                           f"row {bad[0]}: {out_rows[bad[0]]!r}")
    return src


def check_crop(key_f32, pts_f32, out_rows, max_band=None, planted=(), exact=False):
    """Every property a cropped cloud must have, unconditionally: each output row is a bitwise copy of an input row, the
    source indices are strictly increasing (order kept, no row twice), every must_keep row is there and no must_drop row.
    max_band: largest number of band rows (planted ones aside) the input may have -- a degenerate input cannot hide a
    failure behind its band.  exact: the kept mask equals keep_f32 on every row.
    -> (src indices int64, number of band rows outside `planted`)."""
    pts = _rows_f32(pts_f32)
    must_keep, must_drop, band, keep_f32 = crop_decision(key_f32, pts)
    src = match_rows(out_rows, pts)
    assert (np.diff(src) > 0).all(), f"crop: source rows not strictly increasing at output row {np.argmin(np.diff(src) > 0)}"
    kept = np.zeros(len(pts), bool)
    kept[src] = True
    miss = np.flatnonzero(must_keep & ~kept)
    assert len(miss) == 0, f"crop: {len(miss)} rows inside the radius are missing, first input row {miss[0]}"
    extra = np.flatnonzero(must_drop & kept)
    assert len(extra) == 0, f"crop: {len(extra)} rows outside the radius were kept, first input row {extra[0]}"
    free = band.copy()
    free[np.asarray(planted, dtype=np.int64)] = False
    n_band = int(free.sum())
    if max_band is not None:
        assert n_band <= max_band, f"crop: {n_band} undecided rows, the input allows {max_band}"
    if exact:
        diff = np.flatnonzero(kept != keep_f32)
        assert len(diff) == 0, (f"crop: kept mask differs from the float32 statement on {len(diff)} rows, first input row "
                                f"{diff[0]} (kept {kept[diff[0]]})")
    return src, n_band


def band_limit(n):
    """Most band rows a test input of n rows may have: max(8, 1e-4 n)."""
    return max(8, int(1e-4 * n))


# ------------------------------------------------------------------------------------------------------ GT pairs
def d2_f32(src_rows, tgt, fused=None):
    """[len(src_rows), len(tgt)] float32: ((dx*dx + dy*dy) + dz*dz), dx = src - tgt, every operation rounded.
    fused = "fma1" / "fma2": the same sum as sqnorm_contracted would fuse it (for the tie check of the pair inputs)."""
    dx = src_rows[:, None, 0] - tgt[None, :, 0]
    dy = src_rows[:, None, 1] - tgt[None, :, 1]
    dz = src_rows[:, None, 2] - tgt[None, :, 2]
    if fused is not None:
        d = np.stack(np.broadcast_arrays(dx, dy, dz), -1).reshape(-1, 3)
        return sqnorm_contracted(d, fused).reshape(dx.shape[0], -1)
    return (dx * dx + dy * dy) + dz * dz


def radius_pairs_f32(src_f32, tgt_f32, r, chunk=512, fused=None):
    """k_radius' statement: the pairs (i, j) with d2_f32 < float32(r) * float32(r), sorted by (i, d2, j) -> int64 [M,2]."""
    src, tgt = _rows_f32(src_f32), _rows_f32(tgt_f32)
    r2 = np.float32(r) * np.float32(r)
    out = [np.zeros((0, 2), np.int64)]
    for i0 in range(0, len(src), chunk):
        d2 = d2_f32(src[i0:i0 + chunk], tgt, fused)
        i, j = np.nonzero(d2 < r2)
        o = np.lexsort((j, d2[i, j], i))
        out.append(np.stack([i[o] + i0, j[o]], 1).astype(np.int64))
    return np.concatenate(out, 0)


def radius_decided64(src_f32, tgt_f32, r, chunk=512):
    """float64 brute force with a band: a pair is decided when |d2 - r2| > 8u (d2 + r2), r2 = float32(r)^2.
    -> (inside, outside): sorted int64 codes i * len(tgt) + j of the decided pairs inside, and of the UNDECIDED pairs
    (everything else is decided outside)."""
    src, tgt = _rows_f32(src_f32).astype(np.float64), _rows_f32(tgt_f32).astype(np.float64)
    r2 = float(np.float32(r) * np.float32(r))
    inside, open_ = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for i0 in range(0, len(src), chunk):
        d2 = ((src[i0:i0 + chunk, None, :] - tgt[None]) ** 2).sum(-1)
        band = np.abs(d2 - r2) <= 8 * U * (d2 + r2)
        for mask, dst in (((d2 < r2) & ~band, inside), (band, open_)):
            i, j = np.nonzero(mask)
            dst.append((i + i0).astype(np.int64) * len(tgt) + j)
    return np.concatenate(inside), np.concatenate(open_)


def first_pair_per_source(pairs):
    """The rows of a (i, d2, j)-sorted pair list that open a new i: get_matching_indices(K=1)."""
    if len(pairs) == 0:
        return pairs
    return pairs[np.r_[True, pairs[1:, 0] != pairs[:-1, 0]]]


# -------------------------------------------------------------------------------------------------------- chamfer
def chamfer_sum64(a_f32, b_f32, chunk=256):
    """sum_i min_j |a_i - b_j|^2 in float64."""
    a, b = _rows_f32(a_f32).astype(np.float64), _rows_f32(b_f32).astype(np.float64)
    s = 0.0
    for i0 in range(0, len(a), chunk):
        s += float(((a[i0:i0 + chunk, None, :] - b[None]) ** 2).sum(-1).min(1).sum())
    return s


# ---------------------------------------------------------------------------------- crop behind a float32 transform
def crop_decision_through_transform(key_f32, frames, poses):
    """The crop of cat(transform(frame, pose)) when the transform itself is only known to its float32 bound: a row's squared
    norm lies between those of |p| - b and |p| + b (p, b = transform64's value and bound), widened by the crop's own 8u.
    -> (must_keep, must_drop, open): two correct float32 pipelines may differ on the `open` rows only."""
    key = _rows_f32(key_f32)
    L = float((key.astype(np.float64) ** 2).sum(1).max())
    lo, hi = [], []
    for f, M in zip(frames, poses):
        p, b = transform64(f, M)
        lo.append((np.maximum(np.abs(p) - b, 0.0) ** 2).sum(1))
        hi.append(((np.abs(p) + b) ** 2).sum(1))
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    must_keep = hi * (1 + 8 * U) < L * (1 - 8 * U)
    must_drop = lo * (1 - 8 * U) > L * (1 + 8 * U)
    return must_keep, must_drop, ~(must_keep | must_drop)


def check_same_crop(src_a, src_b, open_rows):
    """Two crops' source indices differ on the open rows at most."""
    diff = np.setxor1d(src_a, src_b)
    bad = diff[~open_rows[diff]]
    assert len(bad) == 0, f"crop: the two pipelines disagree on {len(bad)} decided rows, first input row {bad[0]}"


def check_aggregation(key_f32, frames, poses, moved_gpu, got_rows, ref_rows, atol):
    """transform + crop of several frames against the numpy restatement of complement_data_loader.py:65-70, 620-628, with no
    escape clause.  moved_gpu: the device's own transformed rows (the crop's input), got_rows: the device's crop,
    ref_rows: the restatement's (or a recorded fixture's) crop.
      * ref_rows is the restated crop of the restated transform, row for row within atol, and passes check_crop itself;
      * got_rows passes check_crop on moved_gpu, float32 statement included;
      * the two crops keep the same input rows, except rows the transform's rounding leaves open (at most band_limit);
      * got_rows equals the restated transform of the rows it kept within atol.
    -> (src of got_rows, src of ref_rows)."""
    key = _rows_f32(key_f32)
    cat = np.concatenate([_rows_f32(f) @ np.asarray(M).astype(np.float32)[:3, :3].T + np.asarray(M).astype(np.float32)[:3, 3]
                          for f, M in zip(frames, poses)], 0).astype(np.float32)
    n = len(cat)
    assert moved_gpu.shape == cat.shape
    ref_idx = np.flatnonzero((cat ** 2).sum(-1) < np.max((key ** 2).sum(-1)))
    assert len(ref_idx) == len(ref_rows), (len(ref_idx), len(ref_rows))
    assert np.allclose(ref_rows, cat[ref_idx], rtol=0, atol=atol)
    check_crop(key, cat, cat[ref_idx], max_band=band_limit(n))
    src, _ = check_crop(key, moved_gpu, got_rows, max_band=band_limit(n), exact=True)
    must_keep, must_drop, open_rows = crop_decision_through_transform(key, frames, poses)
    assert open_rows.sum() <= band_limit(n), int(open_rows.sum())
    check_same_crop(src, ref_idx, open_rows)
    kept = np.zeros(n, bool)
    kept[src] = True
    assert kept[must_keep].all() and not kept[must_drop].any()
    assert np.allclose(got_rows, cat[src], rtol=0, atol=atol)
    return src, ref_idx

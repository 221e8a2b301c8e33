"""Float64 NumPy restatement of apr_voxel_down_sample (include/apr_hip.h): open3d's voxel_down_sample as
Predator_APR's loaders call it (datasets/kitti.py:464-475).  open3d is not installed, so this text and the kernel restate
the same contract and are compared bit for bit:

  per cloud and axis   lo = min (fp32, exact);  origin = float64(lo) - voxel * 0.5
  per row and axis     index = floor((float64(p) - origin) / voxel)
  per voxel            s = 0.0;  s += float64(p) over its rows in ASCENDING ROW ORDER;  centroid = s / float64(count)
  output rows          clouds in batch order; inside a cloud, voxels by ascending first row (dict insertion order)

np.add.at applies its additions one by one in index order, every one rounded: the same sums as the dict loop
(`voxel_down_sample_dict`, kept for the small cases and checked against the vectorised form on the CPU).

The keyword arguments select the MUTANTS tests/test_voxel_oracle_cpu.py pairs with the cases, to show that every case can
tell a wrong implementation from a right one: fp32 index arithmetic, fp32 sums, an origin without the half voxel, and
sums in descending row order.
"""
import numpy as np

MAX_INDEX = 131071


class VoxelRangeError(ValueError):
    """What the library answers with APR_ERANGE: a non-finite row, or a voxel index above MAX_INDEX."""


def _indices(p, voxel, index_dtype, half):
    t = np.dtype(index_dtype).type
    lo = p.min(0)
    origin = lo.astype(t) - (t(voxel) * t(0.5) if half else t(0.0))
    return np.floor((p.astype(t) - origin) / t(voxel))


def voxel_down_sample(points, lengths, voxel, index_dtype=np.float64, sum_dtype=np.float64, half=True, reverse=False):
    """-> dict(centroid f64 [m,3], centroid32 f32 [m,3], count i32 [m], first i32 [m], index i32 [m,3], lengths i32 [nb])."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    out = {k: [] for k in ("centroid", "centroid32", "count", "first", "index")}
    lens, row0 = [], 0
    if not np.isfinite(points).all():
        raise VoxelRangeError("non-finite row")
    for n in lengths:
        p = points[row0:row0 + n]
        q = _indices(p, voxel, index_dtype, half)
        if not ((q >= 0) & (q <= MAX_INDEX)).all():
            raise VoxelRangeError("voxel index outside [0, %d]" % MAX_INDEX)
        q = q.astype(np.int64)
        key = (q[:, 0] << 36) | (q[:, 1] << 18) | q[:, 2]
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")            # unique() sorts by key: renumber by first row
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        cell = rank[inv.reshape(-1)]
        first = first[order]
        m = len(first)
        s = np.zeros((m, 3), sum_dtype)
        rows = np.arange(n)[::-1] if reverse else np.arange(n)
        np.add.at(s, cell[rows], p[rows].astype(sum_dtype))
        count = np.bincount(cell, minlength=m)
        c = s.astype(np.float64) / count[:, None].astype(np.float64)
        out["centroid"].append(c)
        out["centroid32"].append(c.astype(np.float32))
        out["count"].append(count.astype(np.int32))
        out["first"].append((first + row0).astype(np.int32))
        out["index"].append(q[first].astype(np.int32))
        lens.append(m)
        row0 += n
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["lengths"] = np.asarray(lens, np.int32)
    return res


def voxel_down_sample_dict(points, lengths, voxel):
    """The same with open3d's own structure: a dict of accumulators filled by one loop over the rows."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    cen, cnt, fst, idx, lens, row0 = [], [], [], [], [], 0
    for n in lengths:
        p = points[row0:row0 + n]
        q = _indices(p, voxel, np.float64, True).astype(np.int64)
        acc = {}
        for i in range(n):
            k = tuple(q[i])
            if k not in acc:
                acc[k] = [np.zeros(3, np.float64), 0, row0 + i]
            a = acc[k]
            a[0] += p[i].astype(np.float64)
            a[1] += 1
        for k, (s, c, f) in acc.items():
            cen.append(s / np.float64(c))
            cnt.append(c)
            fst.append(f)
            idx.append(k)
        lens.append(len(acc))
        row0 += n
    c = np.asarray(cen, np.float64).reshape(-1, 3)
    return dict(centroid=c, centroid32=c.astype(np.float32), count=np.asarray(cnt, np.int32), first=np.asarray(fst, np.int32),
                index=np.asarray(idx, np.int32).reshape(-1, 3), lengths=np.asarray(lens, np.int32))


MUTANTS = {
    "fp32_index": dict(index_dtype=np.float32),
    "fp32_sums": dict(sum_dtype=np.float32),
    "no_half_voxel": dict(half=False),
    "reversed_sums": dict(reverse=True),
}


def differs(a, b):
    """True when two results are not the same bits in every array."""
    return any(a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]) for k in a)

"""Independent reference for voxel hashing, coordinate maps and kernel maps (apr_amd/csrc/hash.hip and the front end of
encoder.hip).  numpy and plain Python only; shares no key arithmetic with the library or with oracle/me_oracle.py:

* rows are looked up as 4-tuples: uniqueness by lexicographic np.unique(axis=0); neighbour search per batch index over a
  packed (x, y, z) with 21 bits per axis.  A probed coordinate is c + offset * scale with |c| <= 2^17, |offset| <= 3 and
  |scale| <= 8, so |probe| + 1 < 2^19 and no field can carry into its neighbour (`_pack3` asserts it);
* the range test is an explicit comparison on the coordinates (`in_range`), made BEFORE anything is packed.

Conventions as include/apr_hip.h states them: rows int32 [n, 4] = (batch, x, y, z); kernel offsets x fastest;
nbr[j, o] = i with in[i] == out[j] + offset(o) * scale, else -1.
"""
import numpy as np

AXIS_LO, AXIS_HI = -(1 << 17), 1 << 17      # apr_amd/csrc/common.h: 18 bits per axis, biased by 2^17
BATCH_HI = 1023                             # batch index 1023 is reserved
_BIAS = np.int64(1) << 20


def voxelize(xyz, vs, batch):
    """(batch, floor(xyz / vs)) with the float32 division numpy does; `batch`: an int or one int per row."""
    q = np.floor(np.asarray(xyz, np.float32).reshape(-1, 3) / np.float32(vs))
    assert q.dtype == np.float32
    b = np.broadcast_to(np.asarray(batch, np.int32), (len(q),))
    return np.concatenate([b[:, None], q.astype(np.int32)], 1)


def in_range(rows):
    r = np.asarray(rows).astype(np.int64).reshape(-1, 4)
    ok = (r[:, 0] >= 0) & (r[:, 0] < BATCH_HI)
    for a in (1, 2, 3):
        ok &= (r[:, a] >= AXIS_LO) & (r[:, a] < AXIS_HI)
    return ok


def floor_rows(rows, floor_to):
    r = np.asarray(rows).astype(np.int64).reshape(-1, 4).copy()
    if floor_to > 0:
        r[:, 1:] = np.floor_divide(r[:, 1:], floor_to) * floor_to      # towards minus infinity
    return r


def build_map(rows, floor_to=0, n_live=None):
    """-> (unique rows int32 [m, 4] in first-occurrence order, their first input indices int64 [m], status).  Only rows
    [0, n_live) exist; a live row that is out of range after flooring sets status 1 and belongs to no voxel."""
    r = floor_rows(rows, floor_to)
    if n_live is not None:
        r = r[:max(0, min(int(n_live), len(r)))]
    ok = in_range(r)
    status = 0 if bool(ok.all()) else 1
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int64), status
    _, first = np.unique(r[idx], axis=0, return_index=True)
    first = np.sort(idx[first]).astype(np.int64)
    return r[first].astype(np.int32), first, status


def kernel_offsets(ks):
    h = ks // 2
    return [(ox, oy, oz) for oz in range(-h, h + 1) for oy in range(-h, h + 1) for ox in range(-h, h + 1)]


def _pack3(c):
    c = c.astype(np.int64)
    assert bool((np.abs(c) < _BIAS).all()), "a coordinate would carry into the next field"
    c = c + _BIAS
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def kernel_map(out_rows, in_rows, ks, scale):
    """`scale` is signed: negative = the coarse-to-fine probe of the transposed path.  in_rows: the rows of a map (unique,
    in range).  A probe that leaves the range finds nothing, whatever its packed form would alias."""
    out_rows = np.asarray(out_rows).astype(np.int64).reshape(-1, 4)
    in_rows = np.asarray(in_rows).astype(np.int64).reshape(-1, 4)
    offs = np.array(kernel_offsets(ks), np.int64) * int(scale)
    nbr = np.full((len(out_rows), len(offs)), -1, np.int32)
    if len(out_rows) == 0 or len(in_rows) == 0:
        return nbr
    assert bool(in_range(in_rows).all())
    for b in np.unique(out_rows[:, 0]):
        if not 0 <= b < BATCH_HI:
            continue
        oj = np.flatnonzero(out_rows[:, 0] == b)
        ii = np.flatnonzero(in_rows[:, 0] == b)
        if len(ii) == 0:
            continue
        keys = _pack3(in_rows[ii, 1:])
        order = np.argsort(keys, kind="stable")
        skeys = keys[order]
        base = out_rows[oj, 1:]
        for o, off in enumerate(offs):
            q = base + off
            ok = ((q >= AXIS_LO) & (q < AXIS_HI)).all(1)
            kq = _pack3(np.where(ok[:, None], q, 0))
            pos = np.minimum(np.searchsorted(skeys, kq), len(skeys) - 1)
            hit = ok & (skeys[pos] == kq)
            nbr[oj[hit], o] = ii[order[pos[hit]]]
    return nbr


def transpose_map(nbr, n_in):
    """nbr_t[i, k] = j for every nbr[j, k] = i >= 0; -1 elsewhere."""
    nbr = np.asarray(nbr)
    out = np.full((n_in, nbr.shape[1]), -1, np.int32)
    j, k = np.nonzero(nbr >= 0)
    out[nbr[j, k], k] = j
    return out


def segment_counts(first, offsets):
    first = np.asarray(first, np.int64)
    return np.array([int(((first >= offsets[b]) & (first < offsets[b + 1])).sum()) for b in range(len(offsets) - 1)], np.int32)


def bbox(rows):
    """min x, y, z, max x, y, z, max batch index, 0 (apr_coords_bbox)."""
    r = np.asarray(rows).astype(np.int64).reshape(-1, 4)
    return [int(v) for v in (*r[:, 1:].min(0), *r[:, 1:].max(0), r[:, 0].max(), 0)]


def pyramid(clouds, vs):
    """The front end of a step over frames (list of f32 [n_b, 3]): voxelise with the frame index as batch, de-duplicate,
    three floored levels.  -> dict(rows {1, 2, 4, 8}, first, counts per frame, bbox, pts, offsets, raw)."""
    offsets = [0]
    for c in clouds:
        offsets.append(offsets[-1] + len(c))
    xyz = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])
    batch = np.concatenate([np.full(len(c), b, np.int32) for b, c in enumerate(clouds)])
    raw = voxelize(xyz, vs, batch)
    rows, first, status = build_map(raw)
    lv = {1: rows}
    for ts in (2, 4, 8):
        lv[ts], _, st = build_map(lv[ts // 2], floor_to=ts)
        status |= st
    return dict(rows=lv, first=first, counts=segment_counts(first, offsets), bbox=bbox(raw), pts=xyz[first],
                offsets=offsets, raw=raw, status=status)

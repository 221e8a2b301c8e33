"""Host oracle of the point-set kernels (apr_amd/csrc/points.hip: grid subsample, radius neighbours, kNN): numpy only, no
GPU, nothing from oracle/.

Two kinds of statement, kept apart (as tests/apg_oracle.py does):
  * float32 bit for bit -- grid_subsample and radius_neighbors spell out ONE operation order with every operation rounded to
    float32, which numpy's element-wise float32 arithmetic reproduces (no FMA):
      subsample  origin = floor(min * (1 / dl)) * dl per cloud, cell = floor((p - origin) / dl), barycentre = the sequential
                 sum in input order times float32(1.0 / count), features = the sequential sum divided by float32(count)
                 (k_cell_coords mode 0, k_barycentre; the reference's grid_subsampling.cpp:60-89);
      radius     d2 = ((dx*dx) + dy*dy) + dz*dz, hit if d2 < fl(r * r), rows ordered by (d2, support index), padded with the
                 number of supports, width = min(largest count, limit) (k_radius; nanoflann's L2_Simple_Adaptor).
    The kernels compute exactly this: d2_rn / cell_index / sub_origin switch contraction off.
  * float64 with a BAND -- kNN.  k_knn writes dx*dx + dy*dy + dz*dz plainly and the compiler may fuse it, so two float32
    evaluations can order two candidates differently when their distances are a few ulp apart: knn_banded accepts any order
    inside runs of candidates whose float64 distances are within 8 float32 ulp of each other and demands the oracle's entry
    everywhere else; knn_exact is for inputs on which every product and sum is exact in float32 (is_exact_lattice), where
    all evaluations agree and the comparison is bit for bit, ties by index included.
"""
import numpy as np

F32 = np.float32


def _rows_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.shape[1] == 3, a.shape
    return a


def _starts(lengths):
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    return np.concatenate([[0], np.cumsum(lengths)])


# ------------------------------------------------------------------------------------------------- grid subsample
def subsample_cells(points, lengths, dl):
    """-> (cloud [n], cell [n,3] int64): every point's cloud and cell, each step a separately rounded float32 operation."""
    pts = _rows_f32(points)
    dl = F32(dl)
    inv = F32(1.0) / dl
    st = _starts(lengths)
    assert st[-1] == len(pts), (st[-1], len(pts))
    cloud = np.zeros(len(pts), np.int64)
    cell = np.zeros((len(pts), 3), np.int64)
    for b in range(len(st) - 1):
        p = pts[st[b]:st[b + 1]]
        origin = np.floor(p.min(0) * inv) * dl                    # float32 throughout
        cell[st[b]:st[b + 1]] = np.floor((p - origin) / dl).astype(np.int64)
        cloud[st[b]:st[b + 1]] = b
    return cloud, cell


def sequential_sum_f32(rows):
    """Sum of the rows of a float32 [m, c] array in row order, one rounded addition per row, starting from 0."""
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = acc + r
    return acc


def grid_subsample(points, lengths, dl, features=None, split=None):
    """-> (rows [M,3] float32, lengths int64 [B], counts int64 [M][, feature rows [M,f] float32]).  The rows of a cloud are
    in order of each cell's first point; compare through canonical().  split: a test hook, maps (cloud, cell, index) ids."""
    pts = _rows_f32(points)
    cloud, cell = subsample_cells(pts, lengths, dl)
    key = np.concatenate([cloud[:, None], cell], 1)
    if split is not None:
        key = split(key)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order_of_cell = np.argsort(first, kind="stable")              # cells by their first point: clouds stay contiguous
    rank = np.empty_like(order_of_cell)
    rank[order_of_cell] = np.arange(len(order_of_cell))
    cid = rank[inv]                                               # cell id of every point
    m = len(first)
    counts = np.bincount(cid, minlength=m).astype(np.int64)
    by_cell = np.argsort(cid, kind="stable")                      # points grouped by cell, input order inside a cell
    start = np.concatenate([[0], np.cumsum(counts)])
    feats = None if features is None else np.ascontiguousarray(features, dtype=np.float32)
    acc = np.zeros((m, 3), np.float32)
    facc = None if feats is None else np.zeros((m, feats.shape[1]), np.float32)
    live = np.arange(m)
    for k in range(int(counts.max())):                            # the k-th point of every cell that has one: sequential
        live = live[counts[live] > k]
        idx = by_cell[start[live] + k]
        acc[live] = acc[live] + pts[idx]
        if facc is not None:
            facc[live] = facc[live] + feats[idx]
    rows = acc * (1.0 / counts.astype(np.float64)).astype(np.float32)[:, None]
    lens = np.bincount(cloud[first[order_of_cell]], minlength=len(_starts(lengths)) - 1).astype(np.int64)
    if facc is None:
        return rows, lens, counts
    return rows, lens, counts, facc / counts.astype(np.float32)[:, None]


def canonical(rows, lengths, feats=None, counts=None):
    """Every cloud's rows sorted lexicographically (x, then y, then z) -> uint32 view [M,3] (and the features / counts
    carried along, features as uint32 too)."""
    rows = _rows_f32(rows)
    st = _starts(lengths)
    assert st[-1] == len(rows), (st[-1], len(rows))
    perm = np.concatenate([st[b] + np.lexsort((rows[st[b]:st[b + 1], 2], rows[st[b]:st[b + 1], 1], rows[st[b]:st[b + 1], 0]))
                           for b in range(len(st) - 1)] or [np.zeros(0, np.int64)]).astype(np.int64)
    out = [rows[perm].view(np.uint32)]
    if feats is not None:
        out.append(np.ascontiguousarray(feats, dtype=np.float32)[perm].view(np.uint32))
    if counts is not None:
        out.append(np.asarray(counts)[perm])
    return out[0] if len(out) == 1 else tuple(out)


def assert_subsample_equal(got_rows, got_lens, want_rows, want_lens, got_feats=None, want_feats=None):
    """Lengths equal, canonical rows (and features) equal bit for bit."""
    got_lens, want_lens = np.asarray(got_lens, np.int64), np.asarray(want_lens, np.int64)
    assert np.array_equal(got_lens, want_lens), f"subsample: lengths {got_lens.tolist()} != {want_lens.tolist()}"
    assert (got_feats is None) == (want_feats is None)
    g = canonical(got_rows, got_lens, got_feats)
    w = canonical(want_rows, want_lens, want_feats)
    if got_feats is None:
        g, w = (g,), (w,)
    bad = np.flatnonzero((g[0] != w[0]).any(1))
    assert len(bad) == 0, (f"subsample: {len(bad)} of {len(w[0])} canonical rows differ, first row {bad[0]}: "
                           f"{g[0][bad[0]].view(np.float32)!r} != {w[0][bad[0]].view(np.float32)!r}")
    if got_feats is not None:
        bad = np.flatnonzero((g[1] != w[1]).any(1))
        assert len(bad) == 0, (f"subsample: features of {len(bad)} rows differ, first row {bad[0]}: "
                               f"{g[1][bad[0]].view(np.float32)!r} != {w[1][bad[0]].view(np.float32)!r}")


# ----------------------------------------------------------------------------------------------- radius neighbours
def d2_f32(q_rows, s_rows):
    """[len(q), len(s)] float32: ((dx*dx) + dy*dy) + dz*dz, dx = q - s, every operation rounded to float32."""
    dx = q_rows[:, None, 0] - s_rows[None, :, 0]
    dy = q_rows[:, None, 1] - s_rows[None, :, 1]
    dz = q_rows[:, None, 2] - s_rows[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def radius_hits(queries, supports, q_lengths, s_lengths, radius, chunk=256, slab=False):
    """All (query, support, d2) with d2_f32 < fl(r * r) inside each cloud pair, sorted by (query, d2, support).
    slab=False: brute force over every pair of the cloud pair.  slab=True (large clouds): the queries are taken in order of
    x, a chunk at a time, against the supports whose x lies within 1.001 r + 1e-6 of the chunk's x range -- a superset of the
    hits (fl(dx*dx) <= d2 < fl(r*r) bounds |dx| by r (1 + 2^-22)); the decision itself is the same float32 statement, and
    tests/test_points_oracle_cpu.py compares the two routes."""
    q, s = _rows_f32(queries), _rows_f32(supports)
    r = F32(radius)
    r2 = r * r
    qs, ss = _starts(q_lengths), _starts(s_lengths)
    assert len(qs) == len(ss) and qs[-1] == len(q) and ss[-1] == len(s)
    I, J, D = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for b in range(len(qs) - 1):
        qb, sb = q[qs[b]:qs[b + 1]], s[ss[b]:ss[b + 1]]
        if slab:
            qo = np.argsort(qb[:, 0], kind="stable")
            so = np.argsort(sb[:, 0], kind="stable")
            sx = sb[so, 0].astype(np.float64)
            margin = 1.001 * float(r) + 1e-6
        else:
            qo, so = np.arange(len(qb)), np.arange(len(sb))
        for i0 in range(0, len(qb), chunk):
            qi = qo[i0:i0 + chunk]
            sj = so
            if slab:
                x = qb[qi, 0].astype(np.float64)
                sj = so[np.searchsorted(sx, x.min() - margin, "left"):np.searchsorted(sx, x.max() + margin, "right")]
            if len(sj) == 0:
                continue
            d2 = d2_f32(qb[qi], sb[sj])
            i, j = np.nonzero(d2 < r2)
            I.append(qi[i] + qs[b])
            J.append(sj[j] + ss[b])
            D.append(d2[i, j])
    I, J, D = np.concatenate(I), np.concatenate(J), np.concatenate(D)
    o = np.lexsort((J, D, I))
    return I[o], J[o], D[o]


def radius_neighbors(queries, supports, q_lengths, s_lengths, radius, limit=0, slab=False):
    """-> (table int32 [nq, width], counts int64 [nq]): rows ordered by (d2, support index), padded with len(supports),
    width = min(largest count, limit) (limit <= 0: the largest count)."""
    nq, ns = len(queries), len(supports)
    I, J, _ = radius_hits(queries, supports, q_lengths, s_lengths, radius, slab=slab)
    counts = np.bincount(I, minlength=nq).astype(np.int64)
    width = int(counts.max()) if nq else 0
    if limit > 0:
        width = min(width, int(limit))
    start = np.concatenate([[0], np.cumsum(counts)])
    rank = np.arange(len(I)) - start[I]
    table = np.full((nq, width), ns, np.int32)
    keep = rank < width
    table[I[keep], rank[keep]] = J[keep]
    return table, counts


def table_d2(table, queries, supports):
    """float32 d2 of every table entry by the oracle's statement; padding -> +inf."""
    q, s = _rows_f32(queries), _rows_f32(supports)
    sp = np.concatenate([s, np.zeros((1, 3), np.float32)])
    d = q[:, None, :] - sp[table]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.where(table == len(s), np.float32(np.inf), d2).astype(np.float32)


def assert_table_equal(got, want, what="radius"):
    """Entry for entry, width included."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: table shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} entries in {len(np.unique(bad[:, 0]))} rows differ, first at row {bad[0][0]} "
                           f"column {bad[0][1]}: {got[bad[0][0], bad[0][1]]} != {want[bad[0][0], bad[0][1]]}")


def assert_matches_reference(got, ref_full, queries, supports, limit=0):
    """A table against the reference binary's full table (REF.batch_query, unsorted inside ties): the same width, the same
    float32 distance in every position, and every row of `got` made of distinct entries of the reference's row.  Positions
    can therefore differ only inside runs of bit-equal d2 (nanoflann's sort is unstable there), and with limit = 0 the
    neighbour sets are equal.  No share of mismatches is allowed."""
    got, ref_full = np.asarray(got), np.asarray(ref_full)
    ns = len(supports)
    w = ref_full.shape[1] if limit <= 0 else min(ref_full.shape[1], int(limit))
    assert got.shape == (len(queries), w), f"reference: table shape {got.shape} != {(len(queries), w)}"
    dg = table_d2(got, queries, supports).view(np.uint32)
    dr = table_d2(ref_full[:, :w], queries, supports).view(np.uint32)
    bad = np.argwhere(dg != dr)
    assert len(bad) == 0, f"reference: {len(bad)} distances differ, first at row {bad[0][0]} column {bad[0][1]}"
    sg = np.sort(got, axis=1)
    dup = (sg[:, 1:] == sg[:, :-1]) & (sg[:, 1:] != ns)
    assert not dup.any(), f"reference: a neighbour appears twice in row {np.argwhere(dup)[0][0]}"
    if w == ref_full.shape[1]:
        rows = np.flatnonzero((sg != np.sort(ref_full, axis=1)).any(1))
        assert len(rows) == 0, f"reference: neighbour sets differ in {len(rows)} rows, first {rows[0]}"
    else:
        for i in np.flatnonzero((got != ref_full[:, :w]).any(1)):
            assert np.isin(got[i], ref_full[i]).all(), f"reference: row {i} holds an entry the reference's row lacks"


class counted_calls:
    """with counted_calls(lib, "apr_x") as c: ...; c.n = how often lib.apr_x was called inside the block.  The wrappers
    choose between entry points by conditions of their own (a kept grid is searched only if it still fits the call): equal
    tables cannot tell which one ran, so a test of the regrid route counts the calls of its entry point."""

    def __init__(self, obj, name):
        self.obj, self.name, self.n = obj, name, 0

    def __enter__(self):
        self.fn = getattr(self.obj, self.name)

        def wrapper(*args):
            self.n += 1
            return self.fn(*args)
        setattr(self.obj, self.name, wrapper)
        return self

    def __exit__(self, *exc):
        setattr(self.obj, self.name, self.fn)
        return False


# ------------------------------------------------------------------------------------------------------------ kNN
def knn_sorted(points, m):
    """float64 distances max(|pi - pj|^2, 1e-12) of every point to all points; -> (index [n, m'], d [n, m']) of the m' =
    min(m, n) nearest ordered by (d, index)."""
    p = _rows_f32(points).astype(np.float64)
    d = np.maximum(((p[:, None, :] - p[None]) ** 2).sum(-1), 1e-12)
    order = np.argsort(d, axis=1, kind="stable")[:, :m]            # stable: equal d in index order
    return order, np.take_along_axis(d, order, 1)


def knn(points, k, skip_first=True):
    """int32 [n, k]: the k nearest by (d, index) after dropping the FIRST of the order when skip_first (by position, not by
    identity); rows with n < k + skip are filled with the query's own index."""
    n, skip = len(points), 1 if skip_first else 0
    order, _ = knn_sorted(points, k + skip)
    out = np.repeat(np.arange(n, dtype=np.int32)[:, None], k, 1)
    got = order[:, skip:]
    out[:, :got.shape[1]] = got
    return out


def is_exact_lattice(points):
    """Every coordinate an integer and every dx*dx + dy*dy + dz*dz below 2^24: exact in float32, fused or not."""
    p = _rows_f32(points).astype(np.float64)
    ext = (p.max(0) - p.min(0)) if len(p) else np.zeros(3)
    return bool((p == np.round(p)).all() and np.abs(p).max(initial=0) < 2 ** 22 and (ext ** 2).sum() < 2 ** 24)


def assert_knn_exact(got, points, k, skip_first=True):
    assert is_exact_lattice(points), "knn_exact: the input is no exact lattice"
    assert_table_equal(got, knn(points, k, skip_first), "knn")


def knn_banded(got, points, k, skip_first=True, ulps=8):
    """General inputs.  The band is `ulps` float32 ulp of d, taken PER TABLE POSITION and never chained: the candidate a
    position holds must lie, in float64, within the band of the oracle's distance AT THAT POSITION (the ulp of the larger
    of the two), and a row's entries must be distinct.  So an entry outside the band of its position can only be the
    oracle's own, candidates within the band of each other may come in any order, and nothing farther than the band from
    the distance the oracle has there is accepted however many near-ties lie between.  Rows none of whose positions has
    another candidate within the band must equal the oracle's outright.  Asserts that, and -> the share of rows that have
    such a position (the rows that touched the band)."""
    got = np.asarray(got)
    n, skip = len(points), 1 if skip_first else 0
    assert got.shape == (n, k), f"knn: table shape {got.shape} != {(n, k)}"
    want = knn(points, k, skip_first)
    if n == 0:
        return 0.0
    order, d = knn_sorted(points, n)                     # the whole order: a tie may reach past the table
    last = min(n, k + skip)                              # the table covers order positions skip .. last-1
    ncol = max(last - skip, 0)
    band = ulps * np.spacing(d[:, 1:].astype(np.float32)).astype(np.float64)
    tied = (d[:, 1:] - d[:, :-1]) <= band                # [n, n-1]: order position p within the band of p + 1
    touched = tied[:, :max(last, 1)][:, max(skip - 1, 0):].any(1) if n > 1 else np.zeros(n, bool)
    assert_table_equal(got[~touched], want[~touched], "knn (rows without a tie)")
    assert np.array_equal(got[:, ncol:], want[:, ncol:]), "knn: filler columns"
    g = got[:, :ncol]
    assert ((g >= 0) & (g < n)).all(), "knn: an entry is no point index"
    by_index = np.empty_like(d)
    np.put_along_axis(by_index, order, d, 1)             # d of every candidate by its index
    dg, dw = np.take_along_axis(by_index, g.astype(np.int64), 1), d[:, skip:last]
    width = ulps * np.spacing(np.maximum(dg, dw).astype(np.float32)).astype(np.float64)
    off = np.argwhere((np.abs(dg - dw) > width) & (g != want[:, :ncol]))
    assert len(off) == 0, (f"knn: {len(off)} entries differ from the oracle's outside the {ulps}-ulp band of their position, "
                           f"first row {off[0][0]} column {off[0][1]}: {g[off[0][0], off[0][1]]} != {want[off[0][0], off[0][1]]}")
    sg = np.sort(g, axis=1)
    dup = np.flatnonzero((sg[:, 1:] == sg[:, :-1]).any(1))
    assert len(dup) == 0, f"knn: row {dup[0]} holds a neighbour twice"
    return float(touched.mean())

"""Planted inputs for the point-set kernels, each with the facts it claims (tests/test_points_oracle_cpu.py asserts them
on the host, so a case that stops hitting its edge fails there and not on the GPU).  numpy only.

Kernel constants the cases are built around (apr_amd/csrc/points.hip): k_barycentre sorts cells of up to 1024 points per
wave and stages a cell's points in LDS while 3 m <= 1024 (m <= 341); larger cells go to k_barycentre_big, 64 workgroups,
LDS sort up to 8192 points and a global-memory sort beyond; the cell scan takes 4096 counts per workgroup and 16 per
thread; at most 64 clouds; k_radius ranks up to 1024 hits per query, takes candidates 256 at a time (4 x 64) and runs 4
queries per workgroup; the search grids refuse cell indices from 40960 on."""
import numpy as np

import points_oracle as O

F32 = np.float32
CELL_CAP, STAGE_CAP, BIG_LDS, SCAN_BLOCK, MAX_CLOUDS, HIT_CAP, BIG_GROUPS = 1024, 341, 8192, 4096, 64, 1024, 64
GRID_MARGIN_CELLS = 40960


# ------------------------------------------------------------------------------------------------- grid subsample
def _cell_slots(n, rng, lo=-40, hi=40):
    """n distinct integer cells (some negative), in random order."""
    side = hi - lo
    flat = rng.choice(side ** 3, size=n, replace=False)
    return np.stack([flat // side ** 2, (flat // side) % side, flat % side], 1).astype(np.int64) + lo


def blob_cells(sizes_per_cloud, dl, seed, fdim=3, on_face=True):
    """Blobs inside single cells, one blob of every given size, scattered over the cloud's index range by a fixed
    permutation.  dl must be a power of two when on_face: the first point of every blob then sits exactly on the corner of
    its cell (three faces at once) and still belongs to it.  Every cloud also gets one point at the corner of its lowest
    cell, so the grid origin is that corner.
    -> dict(points, lengths, dl, features, sizes = per cloud the sorted cell populations claimed)."""
    rng = np.random.default_rng(seed)
    pts, lens, claimed = [], [], []
    for sizes in sizes_per_cloud:
        cells = _cell_slots(len(sizes) + 1, rng)
        cells[0] = cells.min(0) - 1                                # the anchor cell: lowest on every axis
        blobs = [(cells[0].astype(np.float64) * dl)[None]]
        for c, m in zip(cells[1:], sizes):
            u = rng.uniform(0.05, 0.95, (m, 3))
            if on_face:
                u[0] = 0.0
            blobs.append((c + u) * dl)
        cloud = np.concatenate(blobs).astype(np.float32)
        cloud = cloud[rng.permutation(len(cloud))]
        pts.append(cloud)
        lens.append(len(cloud))
        claimed.append(sorted([1] + list(sizes)))
    points = np.concatenate(pts)
    feats = rng.standard_normal((len(points), fdim)).astype(np.float32) if fdim else None
    return dict(points=points, lengths=np.array(lens, np.int32), dl=dl, features=feats, sizes=claimed)


POPULATIONS = [1, 2, 63, 64, 65, 341, 342, 1023, 1024, 1025, 2047, 2049, 8191, 8192, 8193, 9000]


def subsample_cases():
    """name -> builder.  Built on demand: the largest is 66 k points."""
    return {
        # every cell population of the issue's table, split over two clouds, corner points planted, dl = 2^-2
        "populations-f3": lambda: blob_cells([POPULATIONS[0::2], POPULATIONS[1::2]], 0.25, 1, fdim=3),
        "populations-f1": lambda: blob_cells([POPULATIONS[1::2], POPULATIONS[0::2]], 0.25, 2, fdim=1),
        # dl no power of two: the origin and the quotient both round
        "populations-f5-dl0.3": lambda: blob_cells([POPULATIONS[:12], POPULATIONS[12:]], 0.3, 3, fdim=5, on_face=False),
        # 65 cells of 1025 points: one more than k_barycentre_big has workgroups
        "big-cells-65": lambda: blob_cells([[1025] * 33, [1025] * 32], 0.5, 4, fdim=1),
        "no-features": lambda: blob_cells([[1, 2, 342, 1025], [65, 341]], 0.25, 5, fdim=0),
    }


CELL_COUNTS = [1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289]


def one_point_per_cell(n_cells, seed=7, dl=0.5):
    """n_cells points, each alone in its cell (the scan's block edges and the owner of start[n])."""
    rng = np.random.default_rng(seed + n_cells)
    cells = _cell_slots(n_cells, rng)
    pts = ((cells + rng.uniform(0.1, 0.9, (n_cells, 3))) * dl).astype(np.float32)
    return dict(points=pts, lengths=np.array([n_cells], np.int32), dl=dl,
                features=rng.standard_normal((n_cells, 3)).astype(np.float32), sizes=[[1] * n_cells])


def many_clouds(nb, seed=11, dl=0.5):
    """nb clouds of 3 to 9 points in 2 or 3 cells each."""
    rng = np.random.default_rng(seed)
    return blob_cells([[int(rng.integers(1, 5)), int(rng.integers(1, 5))] for _ in range(nb)], dl, seed, fdim=3)


# ----------------------------------------------------------------------------------------------- radius neighbours
def cell_f32(x, origin, cell):
    """The search grid's cell index of a coordinate: floor(fl(fl(x - origin) / cell)) in float32."""
    return np.floor((np.asarray(x, F32) - F32(origin)) / F32(cell)).astype(np.int64)


def find_straddling_pairs(r, origin, k_range):
    """Deterministic search for coordinates p < q on one axis with fl(fl(q - p)^2) < fl(r * r) whose cells in a grid of edge
    r with the given origin differ by 2: p is the largest float32 below the boundary of cell k, q the smallest float32 in
    cell k + 1 (found by nextafter from origin + k r and origin + (k + 1) r).  -> list of (p, q, k)."""
    r, origin = F32(r), F32(origin)
    r2 = r * r
    out = []
    for k in k_range:
        p = origin + F32(k) * r
        for _ in range(64):
            if cell_f32(p, origin, r) <= k - 1:
                break
            p = np.nextafter(p, F32(-np.inf))
        while cell_f32(np.nextafter(p, F32(np.inf)), origin, r) <= k - 1:
            p = np.nextafter(p, F32(np.inf))
        q = origin + F32(k + 1) * r
        for _ in range(64):
            if cell_f32(q, origin, r) >= k + 1:
                break
            q = np.nextafter(q, F32(np.inf))
        while cell_f32(np.nextafter(q, F32(-np.inf)), origin, r) >= k + 1:
            q = np.nextafter(q, F32(-np.inf))
        d = q - p
        if cell_f32(p, origin, r) == k - 1 and cell_f32(q, origin, r) == k + 1 and d * d < r2:
            out.append((float(p), float(q), k))
    return out


STRADDLE_SEARCH = [(F32(0.3 * 4.25), -37.123), (F32(0.6 * 4.25), -37.123), (1.0, -3.7), (0.1, 12.3), (2.55, -101.7)]


def straddling_case(max_pairs_per_setting=4):
    """One cloud pair per (radius, origin) setting that yields pairs: a support at the minimum corner (origin on every
    axis), the p of every pair as a support and its q as a query, along x, y and z in turn, the other coordinates at the
    origin.  -> list of dict(queries, supports, radius, pairs = [(query row, support row)], axis)."""
    cases = []
    for r, origin in STRADDLE_SEARCH:
        found = find_straddling_pairs(r, origin, range(2, 400))[:max_pairs_per_setting]
        if not found:
            continue
        o = F32(origin)
        sup, qry, pairs = [np.array([o, o, o], F32)], [], []
        for n, (p, q, _) in enumerate(found):
            ax = n % 3
            s_row, q_row = np.array([o, o, o], F32), np.array([o, o, o], F32)
            s_row[ax], q_row[ax] = p, q
            pairs.append((len(qry), len(sup), ax))
            sup.append(s_row)
            qry.append(q_row)
        cases.append(dict(queries=np.stack(qry), supports=np.stack(sup), radius=float(F32(r)), origin=float(o), pairs=pairs))
    return cases


def hit_buffer_case(counts=(1023, 1024, 1025, 2600), r=1.0, seed=21, cuts=(1, 48, 1024)):
    """One cluster of exactly `count` supports inside 0.8 r of a centre, the centres 10 r apart; the queries are the centres
    (rows 0..), then the first 6 supports of every cluster.  Around every cut c (a column limit) that the cluster can
    reach, the supports ranked c - 3 .. c + 4 by distance from the centre are made exact duplicates of one point, so a run of
    bit-equal d2 crosses the cut and the index rule decides; the supports are then shuffled.
    -> dict(queries, supports, radius, centre_counts)."""
    rng = np.random.default_rng(seed)
    sup, centres = [], []
    for n, m in enumerate(counts):
        c = np.array([10.0 * r * n, -3.0 * r * n, 2.5], np.float64)
        d = rng.standard_normal((m, 3))
        d *= (0.8 * r * rng.uniform(0.05, 1.0, (m, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        pts = (c + d).astype(np.float32)
        cf = c.astype(np.float32)
        order = np.argsort(O.d2_f32(cf[None], pts)[0], kind="stable")
        for cut in cuts:
            lo, hi = max(cut - 3, 0), min(cut + 4, m - 1)
            if cut < m:
                pts[order[lo:hi + 1]] = pts[order[lo]]
        sup.append(pts)
        centres.append(cf)
    supports = np.concatenate(sup)
    supports = supports[rng.permutation(len(supports))]
    starts = np.concatenate([[0], np.cumsum(counts)])
    queries = np.concatenate([np.stack(centres)] + [s[:6] for s in sup]).astype(np.float32)
    return dict(queries=queries, supports=supports, radius=r, centre_counts=list(counts), starts=starts)


def candidate_total(query, supports, radius, cell_factor=F32(1.01)):
    """Supports in the 27 cells around the query's in the kernel's grid: cell edge fl(1.01f * r), origin = the minimum."""
    s = O._rows_f32(supports)
    cell = F32(cell_factor) * F32(radius)
    mn = s.min(0)
    cs = np.stack([cell_f32(s[:, d], mn[d], cell) for d in range(3)], 1)
    cq = np.array([cell_f32(query[d], mn[d], cell) for d in range(3)])
    return int((np.abs(cs - cq) <= 1).all(1).sum())


def candidate_case(total, nq, r=0.5, seed=31):
    """nq queries (nq = 1, 3, 4, 5: a workgroup takes 4) in the middle cell of a 3^3 block of cells that holds `total`
    supports, the one at the minimum corner included: every query has exactly `total` candidates, a sixth of them hits."""
    rng = np.random.default_rng(seed + total)
    cell = float(F32(1.01) * F32(r))
    anchor = np.array([-5.0, 3.0, 7.0])
    blob = anchor + rng.uniform(0.05, 2.95, (total - 1, 3)) * cell
    sup = np.concatenate([anchor[None], blob]).astype(np.float32)
    qry = (anchor + rng.uniform(1.3, 1.7, (nq, 3)) * cell).astype(np.float32)
    return dict(queries=qry, supports=sup, radius=r, total=total)


def outside_box_case(r=0.75, seed=41):
    """Supports fill [0, 6]^3; queries lie outside the box beyond every face, edge and corner, within r of it or not:
    their cells are negative or past the last occupied one."""
    rng = np.random.default_rng(seed)
    sup = rng.uniform(0, 6, (1500, 3)).astype(np.float32)
    sup[0] = 0.0
    q = rng.uniform(-0.9 * r, 6 + 0.9 * r, (600, 3))
    side = rng.integers(0, 3, 600)
    far = rng.random(600) < 0.5
    q[np.arange(600), side] = np.where(far, -rng.uniform(0.01, 0.9 * r, 600), 6 + rng.uniform(0.01, 0.9 * r, 600))
    corners = np.array([[a, b, c] for a in (-0.3, 6.3) for b in (-0.3, 6.3) for c in (-0.3, 6.3)])
    beyond = np.array([[-3 * r, 3, 3], [6 + 3 * r, 3, 3], [3, -40.0, 3], [3, 3, 1e4], [-1e5, -1e5, -1e5]])
    return dict(queries=np.concatenate([q, corners, beyond]).astype(np.float32), supports=sup, radius=r,
                n_outside=600 + 8 + 5)


def no_neighbour_case():
    rng = np.random.default_rng(51)
    sup = rng.uniform(0, 3, (70, 3)).astype(np.float32)
    qry = (rng.uniform(0, 3, (9, 3)) + np.array([50.0, 0, 0])).astype(np.float32)
    return dict(queries=qry, supports=sup, radius=0.5)


def ragged_clouds_case(nb=5, r=0.6, seed=61):
    """nb clouds of different sizes, origins hundreds of metres apart; clouds 1 and 2 have IDENTICAL coordinates."""
    rng = np.random.default_rng(seed)
    ns = [257, 64, 64, 1, 700][:nb]
    nq = [5, 64, 64, 3, 300][:nb]
    S, Q = [], []
    for b in range(nb):
        o = np.array([400.0 * b, -250.0 * b, 30.0 * b])
        S.append((o + rng.uniform(0, 3.5, (ns[b], 3))).astype(np.float32))
        Q.append((o + rng.uniform(-0.3, 3.8, (nq[b], 3))).astype(np.float32))
        if ns[b] == 1:                                             # the one-support cloud: its queries right next to it
            Q[b] = (S[b] + rng.uniform(-0.2, 0.2, (nq[b], 3))).astype(np.float32)
    S[2], Q[2] = S[1].copy(), Q[1].copy()
    return dict(queries=np.concatenate(Q), supports=np.concatenate(S), q_lengths=np.array(nq, np.int32),
                s_lengths=np.array(ns, np.int32), radius=r, twins=(1, 2))


def grid_range_case(r=0.01):
    """Two supports 500 m apart at r = 1 cm: 49 505 cells of 1.01 r, beyond the 40 960 the search grid vouches for."""
    sup = np.array([[0, 0, 0], [500.0, 0, 0], [0.005, 0, 0]], np.float32)
    qry = np.array([[0.001, 0, 0], [500.0, 0.001, 0]], np.float32)
    return dict(queries=qry, supports=sup, radius=r)


# ------------------------------------------------------------------------------------------------------------ kNN
KNN_N = [1, 3, 11, 63, 64, 65, 257, 700]
KNN_K = [(1, True), (1, False), (10, True), (10, False), (15, True), (15, False), (16, False)]


def knn_lattice(n, seed=71):
    """n integer points in [-6, 6]^3 with clusters of exact duplicates: many exact ties, broken by index."""
    rng = np.random.default_rng(seed + n)
    p = rng.integers(-6, 7, (n, 3)).astype(np.float32)
    if n >= 11:
        p[n // 2:n // 2 + 4] = p[0]                    # a duplicate cluster that includes point 0
        p[-3:] = p[n // 3]
    return p


KNN_UNIFORM = [(700, 0, 20.0), (1500, 1, 35.0), (65, 2, 5.0)]    # (n, seed, half extent)


def knn_uniform(n, seed, half):
    return np.random.default_rng(seed).uniform(-half, half, (n, 3)).astype(np.float32)

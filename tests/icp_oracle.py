"""A host restatement of open3d >= 0.12 `registration_icp` with `TransformationEstimationPointToPoint` (RegistrationICP,
GetRegistrationResultAndCorrespondences, Eigen::umeyama without scaling) in NumPy float64 + scipy's cKDTree: the yardstick
of csrc/icp.hip.  open3d itself is not installed, so this is a restatement of its sources, not a recording of its output.

    T = init; evaluate: nearest target of every p = T s with d^2 < max_dist^2 (strictly), ties -> smallest row
    repeat max_iteration times: U = umeyama(p -> q); T = U T; evaluate; stop when |d fitness| < relative_fitness and
    |d rmse| < relative_rmse

`fp32_round=True` follows the arithmetic contract of apr_icp_batch, so that the association can be compared bit for bit:
p = ((T0 x + T1 y) + T2 z) + T3 in float64 from the ORIGINAL float32 row, rounded to float32 once; d^2 = (dx^2 + dy^2) + dz^2
in float32 with every operation rounded; the bound is float32(max_dist)^2 as a float32 product.  `fp32_round=False` keeps
everything in float64 (open3d's own precision).  The two differ only in which of two nearly equidistant targets a handful
of points pick, and in whether a point at the rim of max_dist counts.
"""
import numpy as np
from scipy.spatial import cKDTree

K_CAND = 8      # candidates per query taken from the tree; the float32 arg-min is chosen among them


def transform(T, s, fp32_round):
    s = s.astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    p = np.stack([((T[d, 0] * x + T[d, 1] * y) + T[d, 2] * z) + T[d, 3] for d in range(3)], 1)
    return p.astype(np.float32) if fp32_round else p


def associate(p, tgt, tree, max_dist, fp32_round):
    """-> (corr int64 [n] (target row or -1), d2 float64 [n] (the distance the kernel would sum; 0 where corr < 0))."""
    m = len(tgt)
    k = min(K_CAND, m)
    _, idx = tree.query(p.astype(np.float64), k=k, distance_upper_bound=float(max_dist) * 1.001 + 1e-6)
    idx = idx.reshape(len(p), k)
    ok = idx < m
    cand = tgt[np.where(ok, idx, 0)]
    if fp32_round:
        d = p[:, None, :].astype(np.float32) - cand.astype(np.float32)
        dx2, dy2, dz2 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
        d2 = (dx2 + dy2) + dz2
        assert d2.dtype == np.float32
        r = np.float32(max_dist)
        r2 = r * r
    else:
        d = p[:, None, :].astype(np.float64) - cand.astype(np.float64)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        r2 = float(max_dist) * float(max_dist)
    d2 = np.where(ok, d2, np.inf)
    best = d2.min(1)
    row = np.where(d2 == best[:, None], np.where(ok, idx, m), m).min(1)
    hit = (best < r2) & (row < m)
    return np.where(hit, row, -1).astype(np.int64), np.where(hit, best, 0.0).astype(np.float64)


def umeyama(p, q):
    """Eigen::umeyama(p, q, with_scaling=false): 4x4 U with q ~= U p."""
    U4 = np.eye(4)
    if len(p) == 0:
        return U4
    p, q = p.astype(np.float64), q.astype(np.float64)
    mp, mq = p.mean(0), q.mean(0)
    S = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(S)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    U4[:3, :3] = R
    U4[:3, 3] = mq - R @ mp
    return U4


def evaluate(T, src, tgt, tree, max_dist, fp32_round):
    p = transform(T, src, fp32_round)
    corr, d2 = associate(p, tgt, tree, max_dist, fp32_round)
    n = int((corr >= 0).sum())
    return dict(p=p, corr=corr, n_corr=n, fitness=n / len(src), rmse=float(np.sqrt(d2.sum() / n)) if n else 0.0)


def icp(src, tgt, init=None, max_dist=0.2, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, fp32_round=True,
        tree=None):
    """src / tgt [n,3] / [m,3] (float32 data; rounded to it when fp32_round).  -> dict(T float64 [4,4], fitness, rmse, n_corr, iterations, corr int64 [n])."""
    dt = np.float32 if fp32_round else np.float64          # float64 inputs stay float64 in the all-float64 variant
    src, tgt = np.ascontiguousarray(src, dtype=dt), np.ascontiguousarray(tgt, dtype=dt)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    tree = cKDTree(tgt.astype(np.float64)) if tree is None else tree
    ev = evaluate(T, src, tgt, tree, max_dist, fp32_round)
    it = 0
    for i in range(int(max_iteration)):
        sel = ev["corr"] >= 0
        U = umeyama(ev["p"][sel], tgt[ev["corr"][sel]])
        T = U @ T
        prev, ev = ev, evaluate(T, src, tgt, tree, max_dist, fp32_round)
        it = i + 1
        if abs(prev["fitness"] - ev["fitness"]) < relative_fitness and abs(prev["rmse"] - ev["rmse"]) < relative_rmse:
            break
    return dict(T=T, fitness=ev["fitness"], rmse=ev["rmse"], n_corr=ev["n_corr"], iterations=it, corr=ev["corr"])


def voxel_first_rows(xyz, voxel_size):
    """ME.utils.sparse_quantize(xyz / voxel_size, return_index=True): first row of every voxel, ascending."""
    c = np.floor(xyz.astype(np.float32) / np.float32(voxel_size)).astype(np.int64)
    _, first = np.unique(c, axis=0, return_index=True)
    return np.sort(first)


def apply_transform(pts, trans):
    """FCGF_APR/lib/complement_data_loader.py:65-70."""
    trans = np.asarray(trans).astype(np.float32)
    return pts.astype(np.float32) @ trans[:3, :3].T + trans[:3, 3]


def refine_pose(xyz_curr, xyz_next, M, icp_voxel_size=0.05, max_dist=0.2, max_iteration=200, fp32_round=True, tree=None):
    """_get_icp (complement_data_loader.py:376-388): -> (pose float64 [4,4] = reg.transformation @ M, the icp() dict)."""
    curr = xyz_curr[voxel_first_rows(xyz_curr, icp_voxel_size)]
    nxt = apply_transform(xyz_next[voxel_first_rows(xyz_next, icp_voxel_size)], M)
    reg = icp(nxt, curr, np.eye(4), max_dist, max_iteration, fp32_round=fp32_round, tree=tree)
    return reg["T"] @ np.asarray(M, dtype=np.float64), reg


def pose_error(T_a, T_b):
    """(metres, degrees) between two poses, as registration.rte_rre."""
    T_a, T_b = np.asarray(T_a, dtype=np.float64), np.asarray(T_b, dtype=np.float64)
    c = (np.trace(T_a[:3, :3].T @ T_b[:3, :3]) - 1) / 2
    return float(np.linalg.norm(T_a[:3, 3] - T_b[:3, 3])), float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def perturbation(trans_m, rot_deg, seed):
    """A rigid motion of `trans_m` metres along and `rot_deg` degrees about seeded random directions."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    t = rng.normal(size=3)
    t *= trans_m / np.linalg.norm(t)
    th = np.deg2rad(rot_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    P = np.eye(4)
    P[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    P[:3, 3] = t
    return P


def synthetic_frames(xs, seed=3):
    """Full-size scans of synth.make_scene(seed) taken at (x, 0, 0) for x in xs, each in its own sensor frame, and the
    poses that move every frame into the first one."""
    from apr_amd import synth
    scene = synth.make_scene(seed)
    rng = np.random.default_rng(seed)
    frames = [synth.raycast(scene, (float(x), 0.0, 0.0), 0.0, rng) for x in xs]
    poses = []
    for x in xs:
        T = np.eye(4)
        T[0, 3] = float(x) - float(xs[0])
        poses.append(T)
    return frames, poses


def icp_case(trans_m, rot_deg, seed=3):
    """The input of the converged / fixed-count GPU tests: synth.make_scene(3) frames at x = 0 and 6 m reduced to one point
    per 5 cm voxel, the second moved into the first by its planted pose perturbed by (trans_m, rot_deg).
    The perturbation's directions come from `seed`.  open3d's stopping rule needs the correspondence count to repeat
    exactly, so the iteration count is sensitive to rounding: of the seeds 1 .. 8 tried on the CPU, the float32-rounded and
    the all-float64 variant stop at the same iteration for both (trans_m, rot_deg) pairs of the tests on 3 .. 8 and at
    different ones on 1 and 2 (28 / 34 and 41 / 35 iterations, poses 5e-4 m apart).  Seed 3 is the first that is stable.
    -> (src float32 [n,3], tgt float32 [m,3])."""
    (f0, f1), (_, T1) = synthetic_frames([0.0, 6.0])
    tgt = f0[voxel_first_rows(f0, 0.05)]
    src = apply_transform(f1[voxel_first_rows(f1, 0.05)], perturbation(trans_m, rot_deg, seed) @ T1)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


# ---- small seeded clouds for the batch-layout tests (tests/test_icp_batch_gpu.py, checked on the CPU in test_icp_cpu.py) ----
BOX_LO = np.array([-4.0, -2.5, -1.0])      # a 12 x 8 x 3 m box off centre: coordinates of both signs on every axis
BOX_HI = np.array([8.0, 5.5, 2.0])


def box_cloud(m, seed, shift=(0.0, 0.0, 0.0)):
    """m points spread evenly over the six faces of the box, 1 cm noise, moved by `shift`.  -> float32 [m,3]."""
    rng = np.random.default_rng(seed)
    ext = BOX_HI - BOX_LO
    area = np.array([ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[1]]).repeat(2)
    face = rng.choice(6, size=m, p=area / area.sum())
    p = BOX_LO + rng.uniform(size=(m, 3)) * ext
    axis, far = face // 2, face % 2 == 1
    p[np.arange(m), axis] = np.where(far, BOX_HI[axis], BOX_LO[axis])
    p += rng.normal(0.0, 0.01, size=(m, 3))
    return np.ascontiguousarray((p + np.asarray(shift, dtype=np.float64)).astype(np.float32))


def box_source(tgt, n, i, seed):
    """n rows of tgt (without repetition) with 5 mm noise, moved by the inverse of perturbation(0.05 + 0.04 i, 0.5 + 0.4 i,
    seed): ICP from the identity has to find that perturbation.  -> float32 [n,3]."""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(tgt), size=n, replace=False)
    s = tgt[rows].astype(np.float64) + rng.normal(0.0, 0.005, size=(n, 3))
    inv = np.linalg.inv(perturbation(0.05 + 0.04 * i, 0.5 + 0.4 * i, seed))
    return np.ascontiguousarray((s @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))


RAGGED_TGT_ROWS = (3000, 700, 1900)
RAGGED_TGT_SEEDS = (100, 101, 102)
RAGGED_SRC_ROWS = (1, 255, 256, 257, 513, 600, 64, 300)
RAGGED_SRC_SEEDS = (200, 201, 202, 203, 204, 205, 212, 207)
RAGGED_TGT_OF_PROBLEM = (2, 0, 2, 1, 0, 1, 2, 0)


def ragged_batch():
    """Case (a): three target segments of different sizes, eight sources whose lengths sit on either side of the 256-row
    workgroup (1, 255, 256, 257, 513, ...), a non-monotone problem -> segment table.
    -> (targets [3], sources [8], tgt_of_problem [8])."""
    tgts = [box_cloud(m, s) for m, s in zip(RAGGED_TGT_ROWS, RAGGED_TGT_SEEDS)]
    srcs = [box_source(tgts[RAGGED_TGT_OF_PROBLEM[i]], n, i, s)
            for i, (n, s) in enumerate(zip(RAGGED_SRC_ROWS, RAGGED_SRC_SEEDS))]
    return tgts, srcs, list(RAGGED_TGT_OF_PROBLEM)


FULL_SEED = 300


def full_batch(nb=64):
    """Case (c): nb problems on nb segments of their own, every length different (targets 200 .. 400 rows, sources
    40 .. 300 rows).  The default mapping pairs problem i with segment i.  -> (targets [nb], sources [nb])."""
    tgts = [box_cloud(200 + (i * 37) % 201, FULL_SEED + i) for i in range(nb)]
    srcs = [box_source(tgts[i], min(40 + (i * 53) % 261, len(tgts[i])), i % 4, FULL_SEED + 1000 + i) for i in range(nb)]
    return tgts, srcs


CHUNK_TGT_SEED = 400
CHUNK_FIXED = (600, 5, 205)             # (rows, i, seed) of the fixed-count problem
CHUNK_BATCH = ((255, 1, 201), (600, 5, 205), (300, 7, 205))    # the oracle stops below 8, in 9 .. 15, at 16 or later


def chunk_target():
    return box_cloud(3000, CHUNK_TGT_SEED)


def chunk_sources():
    """Case (d): -> (the 600-row source of the fixed-count runs, the three sources of the batch that stops in three
    different chunks of 8 rounds)."""
    tgt = chunk_target()
    return box_source(tgt, *CHUNK_FIXED), [box_source(tgt, *c) for c in CHUNK_BATCH]


FAR_SHIFT = (1000.0, -2000.0, 50.0)
FACE_MAX_DIST = 0.2


def geometry_cases():
    """Case (e): name -> (src, tgt, max_dist), all float32.
    one_cell    max_dist = 50 m on the 12 m box: one grid cell holds every target, every source row has a partner.
    far         both clouds moved by (1000, -2000, 50) m, where a float32 ulp is 1.2e-4 m.
    outside     the last 8 source rows lie 5 m outside the target's bounding box: beyond the minimum on one axis each (3),
                beyond the maximum on one axis each (3), beyond both corners (2).  No partner for any of them.
    cell_faces  targets ON the faces of the search grid's cells, origin + k * (float32(max_dist) * 1.01f) in float32 as
                the kernel builds them; sources max_dist / 2 on either side of every face, the outermost ones outside the
                target's bounding box."""
    cases = {}
    tgt = box_cloud(3000, 500)
    cases["one_cell"] = (box_source(tgt, 600, 2, 501), tgt, 50.0)
    tgt = box_cloud(2000, 510)
    src = box_source(tgt, 400, 1, 511)
    sh = np.asarray(FAR_SHIFT)
    cases["far"] = ((src.astype(np.float64) + sh).astype(np.float32), (tgt.astype(np.float64) + sh).astype(np.float32), 0.2)
    tgt = box_cloud(2000, 520)
    lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
    mid = (lo + hi) / 2
    out = []
    for d in range(3):
        a, b = mid.copy(), mid.copy()
        a[d], b[d] = lo[d] - 5.0, hi[d] + 5.0
        out += [a, b]
    out = [out[0], out[2], out[4], out[1], out[3], out[5], lo - 5.0, hi + 5.0]
    cases["outside"] = (np.concatenate([box_source(tgt, 300, 1, 521), np.asarray(out, dtype=np.float32)]), tgt, 0.2)
    cell = np.float32(FACE_MAX_DIST) * np.float32(1.01)
    origin = np.array([-3.7, 1.3, 0.2], dtype=np.float32)
    k = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    tgt = origin + k * cell                                     # float32 product and sum, each rounded
    assert tgt.dtype == np.float32
    half = np.float32(FACE_MAX_DIST / 2)
    src = np.concatenate([tgt + np.float32(s) * half * np.eye(3, dtype=np.float32)[d] for d in range(3) for s in (-1, 1)])
    cases["cell_faces"] = (np.ascontiguousarray(src), np.ascontiguousarray(tgt), FACE_MAX_DIST)
    return cases


RANGE_MAX_DIST = 1e-3


def range_case(gap_m):
    """Case (f): two clusters of 200 targets in 1 m cubes, `gap_m` apart along x; the sources are the targets displaced by
    2e-4 m.  The search grid needs (gap_m + 1) / (1.01 * max_dist) cells along x.  -> (src, tgt) float32."""
    rng = np.random.default_rng(600)
    c = rng.uniform(0.0, 1.0, size=(400, 3))
    c[200:, 0] += gap_m
    tgt = c.astype(np.float32)
    d = rng.normal(size=(400, 3))
    d *= 2e-4 / np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray((tgt.astype(np.float64) + d).astype(np.float32)), np.ascontiguousarray(tgt)

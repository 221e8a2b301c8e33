"""The inputs of tests/test_apg_gpu.py, shared with tests/test_apg_oracle_cpu.py (which checks the oracle on them): numpy
only, every case rebuilt from its name so that parametrised tests carry no arrays around.

Crop cases are (key [n_key,3], pts [n,3], planted).  `planted` lists the rows of `pts` put at the limit on purpose: rows whose
float32 squared norm EQUALS the limit (the key's farthest point and its mirror images: same squares, same sum, bitwise
distinct rows as match_rows needs; the strict `<` must drop them), and rows a few float32 steps away on which a fused
(FMA) evaluation of the norm decides differently from the rounded one.  The farthest key point is chosen so that the
two fused forms of its norm differ from each other and from the rounded one, and sits where k_max_sqnorm's unrolled loop body reads
it (n_key > 65536, the first or second trip of a two-trip thread) or its remainder iteration (n_key <= 65536)."""
import numpy as np

from tests import apg_oracle as O

KBLOCK = 256                                    # rows per workgroup of the crop's kernels
SCAN = 1024                                     # block counts k_scan_counts takes per trip
N_ONE_TRIP = KBLOCK * SCAN                      # 262144: 1024 blocks, the last single-trip size
N_THREE_TRIPS = 2 * N_ONE_TRIP + 257            # 524545: 2050 blocks
CROP_SIZES = (1, 63, 64, 255, 256, 257, N_ONE_TRIP, N_ONE_TRIP + 1, N_THREE_TRIPS)
LARGE_PATTERNS = ("gauss", "all", "none", "blocks", "one_first", "one_last")


def _gauss(rng, n, sigma):
    return (rng.standard_normal((n, 3)) * sigma).astype(np.float32)


def _shell(rng, n, r_lo, r_hi):
    """n points with radius in [r_lo, r_hi) (float64 radius; the margins used below are far wider than float32 rounding)."""
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(r_lo, r_hi, (n, 1))).astype(np.float32)


def mirror_images(p):
    """The 8 sign patterns of a point, the point itself first: bitwise distinct rows, one float32 squared norm."""
    s = np.array([[1, 1, 1], [-1, 1, 1], [1, -1, 1], [1, 1, -1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, -1]],
                 np.float32)
    return s * np.asarray(p, np.float32)[None]


def _norms(p):
    p = np.atleast_2d(np.asarray(p, np.float32))
    return O.sqnorm_f32(p), O.sqnorm_contracted(p, "fma1"), O.sqnorm_contracted(p, "fma2")


def telling_point(radius, rng):
    """A point of about the given radius with fma1 < fma2 and rounded != fma1 (fma1 = fma(x,x,y*y)+z*z,
    fma2 = fma(z,z,fma(y,y,x*x))): a key's farthest point on which a fused build shows -- a limit taken as fma2 keeps the
    rows that are bit-equal to the point when their norm is taken as fma1."""
    d = rng.standard_normal((4000, 3))
    cand = (d / np.linalg.norm(d, axis=1, keepdims=True) * radius).astype(np.float32)
    a, b, c = _norms(cand)
    hit = np.flatnonzero((b < c) & (a != b) & (np.abs(cand) > 0.1 * radius).all(1))
    return cand[hit[0]].copy()


def near_limit_rows(far, rng, want=8):
    """Rows within a few float32 steps of `far` on which the rounded crop decision (against the rounded limit) differs from
    a fused one: fma1 rows against the rounded limit, in both directions, against the fma1 limit (a build that fuses both
    kernels alike) and against the fma2 limit (the two kernels fused differently).  Bitwise distinct from each other and
    from far's mirror images."""
    L, L1, L2 = (v[0] for v in _norms(far))
    cand = mirror_images(far)[rng.integers(0, 8, 60000)]
    steps = rng.integers(-48, 49, cand.shape)
    bits = cand.view(np.int32) + steps                              # sign-magnitude: +k bit steps = k steps away from 0
    cand = np.ascontiguousarray(bits.astype(np.int32)).view(np.float32)
    cand = cand[(steps != 0).any(1)]
    rn, f1, _ = _norms(cand)
    kinds = [(rn < L) & ~(f1 < L), ~(rn < L) & (f1 < L), (rn < L) != (f1 < L1), (rn < L) != (f1 < L2)]
    rows, seen = [], {r.tobytes() for r in mirror_images(far)}
    for k in range(want):
        for i in np.flatnonzero(kinds[k % 4]):
            if cand[i].tobytes() not in seen:
                seen.add(cand[i].tobytes())
                rows.append(cand[i])
                break
    return np.asarray(rows, np.float32).reshape(-1, 3)


def plant_farthest(key, pts, rng):
    """Overwrite rows of pts at block and wave boundaries with the key's farthest point and its mirror images (norm == the
    limit), and their neighbours with near_limit_rows.  -> the planted rows' indices."""
    n = len(pts)
    far = key[np.argmax(O.sqnorm_f32(key))]
    where = sorted({i for i in (0, 63, 64, 255, 256, 257, n - 2, n - 1) if 0 <= i < n})
    pts[where] = mirror_images(far)[: len(where)]
    beside = [i for i in (1, 2, 62, 65, 254, 258, 259, n - 3) if 0 <= i < n and i not in where]
    beside = sorted(set(beside))
    near = near_limit_rows(far, rng)[: len(beside)]
    beside = beside[: len(near)]
    pts[beside] = near
    return sorted(where + beside)


def at_limit(key, pts, planted):
    """The planted rows whose rounded squared norm EQUALS the limit: the strict < drops them."""
    planted = np.asarray(planted, np.int64)
    return planted[O.sqnorm_f32(pts[planted]) == O.sqnorm_f32(key).max()] if len(planted) else planted


def crop_case(pattern, n, seed=0):
    """-> (key, pts, planted)."""
    rng = np.random.default_rng([seed, n, LARGE_PATTERNS.index(pattern)])
    planted = []
    if pattern == "gauss":                       # ~85 % kept at the large sizes
        key = _gauss(rng, 70001, 20.0)
        far = int(np.argmax((key.astype(np.float64) ** 2).sum(1)))
        key[[0, far]] = key[[far, 0]]            # row 0: the first of thread 0's two trips, k_max_sqnorm's unrolled body
        key[0] = telling_point(1.001 * np.linalg.norm(key[0].astype(np.float64)), rng)
        pts = _gauss(rng, n, 45.0)
        planted = plant_farthest(key, pts, rng)
    elif pattern == "all":
        key = np.array([[600.0, -500.0, 400.0]], np.float32)
        pts = _gauss(rng, n, 45.0)
    elif pattern == "none":                      # limit 0: the strict < drops rows AT the origin too
        key = np.zeros((1, 3), np.float32)
        pts = _gauss(rng, n, 45.0)
        zeros = mirror_images([0.0, 0.0, 0.0])   # +-0 in every combination: 8 bitwise distinct rows of norm 0
        where = sorted({i for i in (0, 1, 255, 256, n // 2, n - 2, n - 1) if 0 <= i < n})
        pts[where] = zeros[: len(where)]
        planted = where
    elif pattern == "blocks":                    # whole 256-row blocks alternately inside / outside: counts 0 or 256
        key = np.array([[33.0, -44.0, 0.5]], np.float32)            # |key| ~ 55
        inside = (np.arange(n) // KBLOCK) % 2 == 0
        pts = np.where(inside[:, None], _shell(rng, n, 1.0, 50.0), _shell(rng, n, 60.0, 100.0))
    elif pattern in ("one_first", "one_last"):
        key = np.array([[33.0, -44.0, 0.5]], np.float32)
        pts = _shell(rng, n, 60.0, 100.0)
        pts[0 if pattern == "one_first" else n - 1] = [3.0, -4.0, 1.0]
    else:
        raise KeyError(pattern)
    return key, np.ascontiguousarray(pts, np.float32), planted


def crop_case_list():
    """(pattern, n) of every crop case."""
    out = [("gauss", n) for n in CROP_SIZES]
    for n in CROP_SIZES[-3:]:
        out += [(p, n) for p in LARGE_PATTERNS[1:]]
    out += [("none", 1), ("all", 1), ("none", 257), ("all", 257), ("one_last", 257)]
    return out


KEY_CASES = ((1, 0), (65536, 0), (65537, 65536), (70001, 70000))   # (n_key, index of the farthest key point)


def key_case(n_key, far_at, n=1537):
    """A key whose farthest point (radius ~80) sits at `far_at`, the others within 30; points spread over both sides, so a
    maximum that misses `far_at` drops rows that must be kept."""
    rng = np.random.default_rng([7, n_key])
    key = _shell(rng, n_key, 0.0, 30.0)
    key[far_at] = telling_point(80.0, rng)                         # inexact squares: the fused norms differ from the rounded
    pts = _gauss(rng, n, 45.0)
    planted = plant_farthest(key, pts, rng)
    return key, pts, planted


# ------------------------------------------------------------------------------------------------------ transform
TRANSFORM_SIZES = (1, 255, 256, 257, 100003)
POSES = ("identity", "general", "far")


def pose(name):
    """float64 [4,4]."""
    T = np.eye(4)
    if name == "identity":
        return T
    a, b, c = (0.7, -0.4, 1.9) if name == "general" else (-2.6, 0.3, 0.05)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [31.0, -38.0, 9.0] if name == "general" else [1500.0, -1320.0, 40.0]      # |t| ~ 50 m / ~ 2000 m
    return T


def transform_points(n, name):
    rng = np.random.default_rng([11, n])
    lim = 120.0 if name == "far" else 60.0
    return (rng.uniform(-1, 1, (n, 3)) * [lim, lim, 6.0]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ GT pairs
PAIR_CASES = ("synthetic", "planted", "far_queries", "1x1", "1x3000", "3x1", "3x3000", "2500x1", "2500x3000", "no_pairs")


def pair_case(name):
    """-> (source [n,3] f32, target [m,3] f32, T float64 [4,4], radius)."""
    rng = np.random.default_rng([13, PAIR_CASES.index(name)])
    I = np.eye(4)
    if name == "synthetic":                      # the pair of test_get_matching_indices_matches_bruteforce
        from apr_amd import synth
        a, b, T = synth.make_pair(2, n_beams=8, n_azimuth=400)
        return np.ascontiguousarray(a[::2]), np.ascontiguousarray(b[::2]), T, 0.45
    box = lambda m: rng.uniform(-5, 5, (m, 3)).astype(np.float32)
    if name == "planted":                        # identity pose, r = 0.5: r^2 = 0.25 exactly
        inside = np.nextafter(np.float32(0.5), np.float32(0))
        tgt = box(3000)
        tgt = tgt[(np.abs(tgt).max(1) > 1.5)]                       # keep the surroundings of the origin clear
        plant = np.array([[0.5, 0, 0],                              # 0: d2 == r2, excluded by the strict <
                          [inside, 0, 0],                           # 1: one float32 step inside, included
                          [0, -0.5, 0], [0, 0, -inside],            # 2 excluded, 3 included: the negative side
                          [0.25, 0.25, 0.25],                       # 4, 5, 6: duplicates -- ties go to the smaller index,
                          [0.25, 0.25, 0.25], [0.25, 0.25, 0.25],   #          and 7 (the same d2 = 0.1875, other point) after
                          [-0.25, 0.25, -0.25],
                          [0, 0, 0]], np.float32)                   # 8: d2 = 0 first of all
        tgt = np.concatenate([plant[:4], tgt[:100], plant[4:6], tgt[100:], plant[6:]], 0)
        src = np.concatenate([np.zeros((1, 3), np.float32), box(40)], 0)
        return src, tgt, I, 0.5
    if name == "far_queries":                    # many cells outside the target's box on every side, and 1e4 m away
        tgt = box(3000)
        far = []
        for ax in range(3):
            for sgn in (-1.0, 1.0):
                for dist in (6.0, 50.0, 1000.0, 1e4):
                    p = rng.uniform(-4, 4, 3)
                    p[ax] = sgn * dist
                    far.append(p)
        far += [[1e4, 1e4, 1e4], [-1e4, -1e4, -1e4], [-1e4, 1e4, -1e4]]
        far = np.asarray(far, np.float32)
        near = box(60)
        src = np.concatenate([near[:30], far, near[30:]], 0)       # far rows in between: a stray hit would show in place
        return src, tgt, I, 0.5
    if name == "no_pairs":
        return box(50) + np.float32(40.0), box(3000), I, 0.5
    ns, nt = (int(v) for v in name.split("x"))
    tgt = box(nt)
    src = box(ns)
    if nt == 1:
        src[0] = tgt[0] + np.float32(0.1)                           # one pair at least
    T = pose("general")
    Tinv = np.linalg.inv(T)
    src = (src.astype(np.float64) @ Tinv[:3, :3].T + Tinv[:3, 3]).astype(np.float32)    # T src lands in the box again
    return src, tgt, T, 0.5


# ---------------------------------------------------------------------------------------------------------- chain
def chain_case():
    """-> (key, frames, poses, voxel size): four small frames, about half of their points beyond the key's radius."""
    rng = np.random.default_rng(17)
    key = _gauss(rng, 3000, 12.0)
    frames, poses = [], []
    for k in range(4):
        frames.append(_gauss(rng, 4000 + 37 * k, 14.0))
        M = pose("general").copy()
        M[:3, 3] = [52.0 * np.cos(1.3 * k), 52.0 * np.sin(1.3 * k), 1.0 - 0.5 * k]
        poses.append(M)
    return key, frames, poses, 0.3


CHAMFER_N = (1, 255, 257, 3000)
CHAMFER_M = (1, 511, 512, 513, 5000)


def chamfer_case(n, m):
    rng = np.random.default_rng([19, n, m])
    return rng.uniform(-5, 5, (n, 3)).astype(np.float32), rng.uniform(-5, 5, (m, 3)).astype(np.float32)

"""Inputs for the voxel_down_sample tests: built once, shared by the CPU test (which shows that each of them can tell a
mutant oracle from the right one) and the GPU test (which holds the kernel to the oracle bit for bit)."""
import functools

import numpy as np

# the kernel's internal capacities (apr_amd/csrc/voxel.hip): a voxel's rows are staged kVoxStage at a time by the wave
# kernel, which sorts up to kVoxWaveCap of them; fuller voxels go to the workgroup kernel, which sorts up to kVoxBigLds
# rows in LDS (more: in global memory) and stages kVoxBigStage at a time
K_VOX_STAGE, K_VOX_WAVE_CAP, K_VOX_BIG_LDS, K_VOX_BIG_STAGE = 341, 1024, 8192, 1024
CROWDED_COUNTS = (K_VOX_STAGE - 1, K_VOX_STAGE, K_VOX_STAGE + 1, 2 * K_VOX_STAGE, 2 * K_VOX_STAGE + 1,
                  K_VOX_WAVE_CAP - 1, K_VOX_WAVE_CAP, K_VOX_WAVE_CAP + 1, 2 * K_VOX_BIG_STAGE, 2 * K_VOX_BIG_STAGE + 1,
                  K_VOX_BIG_LDS - 1, K_VOX_BIG_LDS, K_VOX_BIG_LDS + 1)


def case(points, lengths, voxel):
    points = np.ascontiguousarray(points, dtype=np.float32)
    lengths = np.asarray(lengths, np.int32)
    assert lengths.sum() == len(points)
    return dict(points=points, lengths=lengths, voxel=float(voxel))


@functools.lru_cache(None)
def boundary_rows(voxel):
    """lo = fl32(-37.123); for k = 1..200 the fp32 value nearest origin + k voxel and its two fp32 neighbours, on each
    axis in turn (the other two coordinates stay at lo): 1 + 3 * 200 * 3 = 1801 rows."""
    lo = np.float32(-37.123)
    origin = np.float64(lo) - voxel * 0.5
    rows = [np.full(3, lo, np.float32)]
    for axis in range(3):
        for k in range(1, 201):
            v = np.float32(origin + k * voxel)
            for x in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
                r = np.full(3, lo, np.float32)
                r[axis] = x
                rows.append(r)
    pts = np.stack(rows)
    assert pts.shape == (1801, 3)
    return case(pts, [len(pts)], voxel)


@functools.lru_cache(None)
def order_sensitive():
    """Sums in which a float64 addition rounds: ordinary coordinates next to values of 1e-30 .. 1e-8 in one voxel."""
    rng = np.random.default_rng(1)
    head = np.full((1, 3), -0.1, np.float32)
    a = rng.uniform(-0.1, 0.15, (40, 3)).astype(np.float32)
    b = (rng.standard_normal((40, 3)) * 10.0 ** rng.uniform(-30, -8, (40, 3))).astype(np.float32)
    rest = np.concatenate([a, b])
    rest = rest[rng.permutation(len(rest))]
    return case(np.concatenate([head, rest]), [81], 0.3)


@functools.lru_cache(None)
def crowded():
    """One voxel per entry of CROWDED_COUNTS, stacked along y; the x coordinates mix ordinary values with tiny ones (the
    voxels straddle x = 0), so every voxel's x sum depends on the order of its rows.  Rows shuffled across voxels."""
    rng = np.random.default_rng(7)
    voxel = 0.3
    lo = np.array([-0.1, -3.0, 1.0], np.float32)
    parts = []
    for j, m in enumerate(CROWDED_COUNTS):
        x = np.where(rng.random(m) < 0.5, rng.uniform(-0.1, 0.04, m), rng.standard_normal(m) * 10.0 ** rng.uniform(-30, -8, m))
        y = np.float64(lo[1]) - 0.15 + voxel * (j + 1) + rng.uniform(0.01, 0.29, m)
        z = np.float64(lo[2]) + rng.uniform(0.0, 0.1, m)
        parts.append(np.stack([x, y, z], 1))
    rest = np.concatenate(parts).astype(np.float32)
    rest = rest[rng.permutation(len(rest))]
    return case(np.concatenate([lo[None], rest]), [1 + len(rest)], voxel)


def cloud(seed, n, scale=2.0, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * scale + np.asarray(shift)).astype(np.float32)


@functools.lru_cache(None)
def shapes():
    """name -> case: small and odd sizes, degenerate clouds, batches."""
    out = {f"n{n}": case(cloud(n, n), [n], 0.3) for n in (1, 63, 65, 257)}
    out["one_voxel"] = case(np.random.default_rng(3).uniform(5.0, 5.1, (100, 3)), [100], 0.3)
    a, b, c = cloud(11, 300, 3.0, (-50.0, 20.0, -7.0)), cloud(12, 1), cloud(13, 517, 5.0, (100.0, -80.0, 3.0))
    out["batch_of_three"] = case(np.concatenate([a, b, c]), [300, 1, 517], 0.3)
    out["twice_in_a_batch"] = case(np.concatenate([a, c, a]), [300, 517, 300], 0.3)
    out["shuffled"] = case(a[np.random.default_rng(5).permutation(len(a))], [300], 0.7)
    return out

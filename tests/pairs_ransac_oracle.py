"""NumPy float64 restatement of the pair-list RANSAC (apr_ransac_pose_pairs_geometric): open3d <= 0.11
RegistrationRANSACBasedOnCorrespondence as Predator_APR/lib/benchmark_utils.py:205-210 calls it.  PARITY UNPINNED (open3d
is not part of this build); restated from the open3d 0.10 source:

    result = identity, fitness 0, rmse 0
    fewer than 4 pairs: return result
    for it < min(max_iter, max_validation):
        4 entries of the pair list, drawn with the kernels' counter RNG (seed, it, slot)
        T = Kabsch without scale, no checker
        inliers = transformed source points whose nearest target point lies within max_dist; rmse over them
        result = this if it has more inliers, or as many and a strictly lower rmse

Kabsch, the splitmix64 sampling and the inlier rule (float32 transformed point, float32 d^2 < float32(max_dist^2)) are those of
oracle/match_pose_oracle.py.  `nn="brute"` replaces the KD-tree by the full O(n * m) distance matrix.
"""
import numpy as np

from oracle import match_pose_oracle as MO


def _nearest(q32, xyz1_32, tree):
    """float64 distance of every row of q32 to its nearest target (inf: none), through the KD-tree or brute force."""
    if tree is not None:
        d, _ = tree.query(q32, k=1)
        return d
    diff = q32.astype(np.float64)[:, None, :] - xyz1_32.astype(np.float64)[None, :, :]
    return np.sqrt((diff ** 2).sum(2).min(1))


def ransac_pairs_geometric(xyz0, xyz1, pairs, max_dist, max_iter=50000, max_validation=1000, seed=0, nn="kdtree"):
    """-> (T [4,4] float64, info); info also carries the per-hypothesis inlier counts and rmse (`counts`, `rmses`) and the
    sampled list positions (`samples` [n_iter, 4])."""
    x0 = np.asarray(xyz0, dtype=np.float32).astype(np.float64)
    x1_32 = np.asarray(xyz1, dtype=np.float32)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_iter = int(min(max_iter, max_validation))
    best = (0, 0.0, -1, np.eye(4))
    info = dict(inliers=0, rmse=0.0, best_iteration=-1, n_valid=0, fitness=0.0, n_pairs=len(pairs),
                counts=np.zeros(0, np.int64), rmses=np.zeros(0), samples=np.zeros((0, 4), np.int64))
    if len(pairs) < 4:
        return best[3].copy(), info
    tree = None
    if nn == "kdtree":
        from scipy.spatial import cKDTree
        tree = cKDTree(x1_32)
    idx = MO.sample_indices(seed, 0, n_iter, len(pairs))
    T = MO.kabsch(x0[pairs[idx, 0]], x1_32.astype(np.float64)[pairs[idx, 1]])
    counts, rmses = np.zeros(n_iter, np.int64), np.zeros(n_iter)
    md2 = np.float32(max_dist * max_dist)
    for h in range(n_iter):
        q = (x0 @ T[h, :3, :3].T + T[h, :3, 3]).astype(np.float32)
        d = _nearest(q, x1_32, tree)
        inl = np.isfinite(d) & (d.astype(np.float32) ** 2 < md2)
        cnt = int(inl.sum())
        rmse = float(np.sqrt((d[inl].astype(np.float64) ** 2).sum() / cnt)) if cnt else 0.0
        counts[h], rmses[h] = cnt, rmse
        if cnt > best[0] or (cnt == best[0] and rmse < best[1]):
            best = (cnt, rmse, h, T[h])
    info.update(inliers=best[0], rmse=best[1], best_iteration=best[2], n_valid=n_iter, fitness=best[0] / max(len(x0), 1),
                counts=counts, rmses=rmses, samples=idx)
    return best[3].copy(), info

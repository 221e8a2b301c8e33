"""Feature-matching RANSAC registration: the GPU stand-in for the open3d call at
FCGF_APR/scripts/test_apr.py:148-156 (and Predator_APR/lib/benchmark_utils.py:213-225).

    T = ransac_feature_matching(xyz0, xyz1, F0, F1, distance_threshold,
                                ransac_n=4, edge_length=0.9, max_iteration=4_000_000)

returns T [4,4] float64 with xyz1 ~= xyz0 @ R.T + t, like
`ransac_result.transformation`.  Semantics follow the open3d >= 0.12 API the call
site is written against (5th positional arg `mutual_filter=False`;
`RANSACConvergenceCriteria(4000000, 10000)` -> max_iteration 4 M, confidence
clamped to 1.0 so there is no early exit): correspondences = feature-space
nearest neighbour of every source point, 4-point samples, edge-length + distance
checkers, Kabsch without scaling, hypotheses scored on the correspondence set.
open3d's RNG is unseeded / thread dependent; here the hypothesis stream is a
counter-based RNG of (seed, iteration) so runs are reproducible and the CPU
oracle can replay it.  open3d is absent from this image: parity unpinned.
`max_validation=None` (default) is that reading; an integer selects the open3d <= 0.11 reading of the same criteria
object (stop after max_validation validated hypotheses, geometric inlier scoring), as `ops.ransac_pose_geometric`.
"""
import numpy as np
import torch

from .. import ops


def _dev(t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    return t.to(device=torch.device('cuda', torch.cuda.current_device()), dtype=torch.float32).contiguous()


def feature_correspondences(F0, F1):
    return ops.feature_nn(_dev(F0), _dev(F1))


def ransac_feature_matching(xyz0, xyz1, F0, F1, distance_threshold, ransac_n=4, edge_length=0.9,
                            max_iteration=4000000, max_validation=None, seed=0, return_info=False):
    if ransac_n != 4:
        raise NotImplementedError("the HIP RANSAC kernel is specialised for ransac_n = 4 (both call sites)")
    x0, x1 = _dev(xyz0), _dev(xyz1)
    corr = feature_correspondences(F0, F1)
    if max_validation is not None:
        # open3d <= 0.11 reading of RANSACConvergenceCriteria(max_iteration, max_validation): the loop stops after
        # `max_validation` hypotheses have passed both checkers, and a hypothesis is scored by the source points that have a
        # target point within distance_threshold after the transform (not on the correspondence set) -- the flavour
        # Predator_APR's tester pins (requirements.txt: open3d 0.10; lib/benchmark_utils.py:213-225), on the same kernels
        if int(max_validation) < 1:
            raise ValueError("ransac_feature_matching: max_validation must be >= 1 (None: open3d >= 0.12 semantics)")
        T, info = ops.ransac_pose_geometric(x0, x1, corr, distance_threshold, edge_length, max_iteration,
                                            int(max_validation), seed)
    else:
        T, info = ops.ransac_pose(x0, x1, corr, distance_threshold, edge_length, max_iteration, seed)
    return (T, info) if return_info else T


def rte_rre(T_est, T_gt):
    """Translation / rotation error as FCGF_APR/scripts/test_apr.py:162-163 (metres, degrees)."""
    T_est, T_gt = np.asarray(T_est, dtype=np.float64), np.asarray(T_gt, dtype=np.float64)
    rte = np.linalg.norm(T_est[:3, 3] - T_gt[:3, 3])
    c = (np.trace(T_est[:3, :3].T @ T_gt[:3, :3]) - 1) / 2
    rre = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    return float(rte), float(rre)


# ---- point-to-point ICP: the open3d call at FCGF_APR/lib/complement_data_loader.py:384-387 (and data_loaders.py:460-463,
# Predator_APR/datasets/kitti.py:424-426) on the HIP kernels of csrc/icp.hip.  open3d is absent from this image, so the
# algorithm is restated from its >= 0.12 sources (RegistrationICP) and parity with it is unpinned.

class TransformationEstimationPointToPoint:
    """Rotation + translation, no scaling: the only estimation method the HIP kernel implements."""

    def __init__(self, with_scaling=False):
        if with_scaling:
            raise NotImplementedError("registration_icp: point-to-point with scaling is not implemented on the HIP path")
        self.with_scaling = False


class ICPConvergenceCriteria:
    """open3d's defaults; both reference call sites pass max_iteration=200 and keep the two thresholds."""

    def __init__(self, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
        self.relative_fitness = float(relative_fitness)
        self.relative_rmse = float(relative_rmse)
        self.max_iteration = int(max_iteration)


class RegistrationResult:
    """transformation float64 [4,4] (target ~= source @ R.T + t), fitness, inlier_rmse, correspondence_set int64 [K,2]
    (source row, target row); `iterations` is this port's addition."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set, iterations):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.correspondence_set = correspondence_set
        self.iterations = iterations

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, and "
                f"correspondence_set size of {len(self.correspondence_set)}")


def icp_results(rec, corr=None, src_offsets=None):
    """Records of ops.icp_batch (one device -> host copy) -> list of RegistrationResult."""
    host = rec.cpu().numpy()
    corr_host = None if corr is None else corr.cpu().numpy()
    out = []
    for i, r in enumerate(host):
        cs = np.empty((0, 2), dtype=np.int64)
        if corr_host is not None:
            c = corr_host[src_offsets[i]:src_offsets[i + 1]]
            rows = np.nonzero(c >= 0)[0]
            cs = np.stack([rows, c[rows]], 1).astype(np.int64)
        out.append(RegistrationResult(r[:16].reshape(4, 4).copy(), float(r[ops.ICP_FITNESS]), float(r[ops.ICP_RMSE]), cs,
                                      int(r[ops.ICP_ITERATIONS])))
    return out


def registration_icp(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """o3d.pipelines.registration.registration_icp(source, target, max_correspondence_distance, init, estimation_method,
    criteria) for [N,3] arrays / tensors in place of open3d point clouds.  Synchronises."""
    if estimation_method is None:
        estimation_method = TransformationEstimationPointToPoint()
    if not isinstance(estimation_method, TransformationEstimationPointToPoint):
        raise NotImplementedError("registration_icp: only TransformationEstimationPointToPoint runs on the HIP kernels "
                                  f"(got {type(estimation_method).__name__}); point-to-plane ICP is out of scope")
    if criteria is None:
        criteria = ICPConvergenceCriteria()
    src, tgt = _dev(source), _dev(target)
    init = np.eye(4) if init is None else np.asarray(init, dtype=np.float64)
    rec, corr = ops.icp_batch(src, [0, len(src)], tgt, [0, len(tgt)], init.reshape(1, 4, 4), max_correspondence_distance,
                              criteria.max_iteration, criteria.relative_fitness, criteria.relative_rmse, want_corr=True)
    return icp_results(rec, corr, [0, len(src)])[0]

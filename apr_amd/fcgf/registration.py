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


# ---- multiway registration: the open3d calls of FCGF_APR/lib/complement_data_loader.py:417-419 and :425-461 (and
# Predator_APR/datasets/kitti.py:206-251) on the HIP kernels of csrc/posegraph.hip, with arrays in place of open3d objects.
# Restated, not recorded: parity with open3d is unpinned.

def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation):
    """o3d.pipelines.registration.get_information_matrix_from_point_clouds -> float64 [6,6] numpy.  Synchronises."""
    src, tgt = _dev(source), _dev(target)
    T = np.asarray(transformation, dtype=np.float64).reshape(1, 4, 4)
    info, _, _ = ops.information_batch(src, [0, len(src)], tgt, [0, len(tgt)], T, max_correspondence_distance)
    return info[0].cpu().numpy()


class PoseGraphNode:
    def __init__(self, pose=None):
        self.pose = np.eye(4) if pose is None else np.array(pose, dtype=np.float64).reshape(4, 4)


class PoseGraphEdge:
    def __init__(self, source_node_id=-1, target_node_id=-1, transformation=None, information=None, uncertain=False,
                 confidence=1.0):
        self.source_node_id = int(source_node_id)
        self.target_node_id = int(target_node_id)
        self.transformation = np.eye(4) if transformation is None else np.array(transformation, dtype=np.float64).reshape(4, 4)
        self.information = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self.uncertain = bool(uncertain)
        self.confidence = float(confidence)


class PoseGraph:
    def __init__(self):
        self.nodes = []
        self.edges = []


class GlobalOptimizationOption:
    def __init__(self, max_correspondence_distance=0.03, edge_prune_threshold=0.25, preference_loop_closure=1.0,
                 reference_node=-1):
        self.max_correspondence_distance = float(max_correspondence_distance)
        self.edge_prune_threshold = float(edge_prune_threshold)
        self.preference_loop_closure = float(preference_loop_closure)
        self.reference_node = int(reference_node)


class GlobalOptimizationConvergenceCriteria:
    """open3d's defaults, the only values the HIP kernel takes (both reference call sites pass none)."""
    DEFAULTS = dict(max_iteration=100, min_relative_increment=1e-6, min_relative_residual_increment=1e-6,
                    min_right_term=1e-6, min_residual=1e-6, max_iteration_lm=20, upper_scale_factor=2.0 / 3.0,
                    lower_scale_factor=1.0 / 3.0)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError(f"GlobalOptimizationConvergenceCriteria: unknown field {sorted(unknown)}")
        for name, value in self.DEFAULTS.items():
            setattr(self, name, type(value)(kw.get(name, value)))

    def is_default(self):
        return all(getattr(self, name) == value for name, value in self.DEFAULTS.items())


class GlobalOptimizationLevenbergMarquardt:
    """The only method on the HIP kernel; open3d's Gauss-Newton optimiser is out of scope."""


def global_optimization(pose_graph, method=None, criteria=None, option=None):
    """o3d.pipelines.registration.global_optimization(pose_graph, method, criteria, option): Levenberg-Marquardt with the
    default criteria on the device, two passes with pruning in between.  As open3d does, it updates `pose_graph` in place:
    node poses, edge confidences (after the first pass) and the pruned uncertain edges removed.  The node poses are NOT
    compensated for option.reference_node (P_0^-1 P_i, what the reference uses, does not depend on it).  Synchronises.
    -> dict(iterations (first, second pass), status)."""
    method = GlobalOptimizationLevenbergMarquardt() if method is None else method
    criteria = GlobalOptimizationConvergenceCriteria() if criteria is None else criteria
    option = GlobalOptimizationOption() if option is None else option
    if not isinstance(method, GlobalOptimizationLevenbergMarquardt):
        raise NotImplementedError(f"global_optimization: only GlobalOptimizationLevenbergMarquardt runs on the HIP kernel "
                                  f"(got {type(method).__name__}); Gauss-Newton is out of scope")
    if not isinstance(criteria, GlobalOptimizationConvergenceCriteria) or not criteria.is_default():
        raise NotImplementedError("global_optimization: the HIP kernel takes the default "
                                  "GlobalOptimizationConvergenceCriteria only")
    if option.reference_node not in (-1, 0):
        raise NotImplementedError("global_optimization: reference_node other than 0 (or -1, none) is not implemented")
    n = len(pose_graph.nodes)
    if n > ops.POSEGRAPH_MAX_NODES:
        raise NotImplementedError(f"global_optimization: graphs with more than {ops.POSEGRAPH_MAX_NODES} nodes are out of scope")
    if any(e.confidence != 1.0 for e in pose_graph.edges):
        raise NotImplementedError("global_optimization: the HIP kernel starts every confidence at 1")
    if not pose_graph.edges:
        return dict(iterations=(0, 0), status=ops.POSEGRAPH_NO_WEIGHT)
    layout = ops.PoseGraphLayout([(n, [(e.source_node_id, e.target_node_id, e.uncertain) for e in pose_graph.edges])])
    T = np.stack([e.transformation for e in pose_graph.edges])
    info = np.stack([e.information for e in pose_graph.edges])
    init = np.stack([nd.pose for nd in pose_graph.nodes])
    poses, conf, kept, iters, status = ops.posegraph_optimize(layout, T, info, init, option.max_correspondence_distance,
                                                              option.edge_prune_threshold, option.preference_loop_closure)
    poses, conf, kept = poses.cpu().numpy(), conf.cpu().numpy(), kept.cpu().numpy()
    status = int(status.cpu()[0])
    if status == ops.POSEGRAPH_MALFORMED:
        raise ValueError("global_optimization: malformed pose graph")
    for nd, P in zip(pose_graph.nodes, poses):
        nd.pose = P.copy()
    for e, c in zip(pose_graph.edges, conf):
        e.confidence = float(c)
    pose_graph.edges = [e for e, k in zip(pose_graph.edges, kept) if k]
    return dict(iterations=tuple(int(v) for v in iters.cpu().numpy()[0]), status=status)


# ---- voxel centroids: open3d's PointCloud.voxel_down_sample as Predator_APR's loaders call it (datasets/kitti.py:464-475,
# 588-589, the same lines of nuscenes.py) on the HIP kernels of csrc/voxel.hip.  Restated, not recorded (DESIGN section
# 20): the contract is exact against tests/voxel_oracle.py, parity with open3d itself is unpinned.

def voxel_down_sample(points, voxel_size):
    """o3d.geometry.PointCloud(points).voxel_down_sample(voxel_size).points for an [N,3] array / tensor: the float64
    centroids [M,3] on the GPU, voxels in ascending order of their first row.  Synchronises."""
    out, _ = ops.voxel_down_sample(_dev(points), [len(points)], voxel_size, want=("centroid",))
    return out["centroid"]

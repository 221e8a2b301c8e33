"""APG aggregation, GT correspondences and the NPR reconstruction loss on the GPU.

  aggregate_frames   <- FCGF_APR/lib/complement_data_loader.py:576-628,671-674 (transform the 2k complement
                        frames into the key frame, crop to the key frame's radius, voxel-quantise)
  refine_pose / refine_complement_poses <- complement_data_loader.py:369-405 (_get_icp, _get_neighbourhood_icp: the
                        odometry pose of every complement frame goes through point-to-point ICP first)
  pairwise_init / full_registration / multiway_registration <- complement_data_loader.py:408-516 (the loader's default:
                        ICP on every pair of a side, information matrices, open3d's pose-graph optimisation)
  get_matching_indices <- FCGF_APR/util/pointcloud.py:53-66 ; Predator_APR/lib/benchmark_utils.py:121-135
  chamfer_distance   <- FCGF_APR/lib/complement_trainer.py:188-196 (chamferdist 1-NN sums, both directions)
  GenerativeMLP*     <- FCGF_APR/model/mlp.py:6-37 (same module / parameter names: `mlp.0.weight` ...)
  npr_reconstruction_loss <- complement_trainer.py:424-449 (differentiable: GEMM / BN / Chamfer forward and backward on
                        the HIP kernels, apr_amd/npr.py)
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from ... import _lib, npr, ops
from ..._lib import check, ptr, stream
from ...predator import kp_ops, point_ops


def _dev():
    return torch.device('cuda', torch.cuda.current_device())


def _f32(a):
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return a.to(device=_dev(), dtype=torch.float32).contiguous()


def apply_transform(pts, trans):
    """pts @ R.T + t in float32 (complement_data_loader.py:65-70)."""
    pts = _f32(pts)
    T = _f32(np.asarray(trans, dtype=np.float32).reshape(16) if not torch.is_tensor(trans) else trans.reshape(16))
    out = torch.empty_like(pts)
    check(_lib.load().apr_transform_points(ptr(pts), pts.shape[0], ptr(T), ptr(out), stream()))
    return out


def crop_to_radius(key_xyz, pts):
    """Rows of `pts` with |p|^2 < max |key|^2, order preserved."""
    key_xyz, pts = _f32(key_xyz), _f32(pts)
    lib = _lib.load()
    n = pts.shape[0]
    out = torch.empty_like(pts)
    cnt = torch.empty(1, dtype=torch.int32, device=pts.device)
    sb = int(lib.apr_crop_scratch_bytes(n))
    scratch = torch.empty(sb, dtype=torch.uint8, device=pts.device)
    check(lib.apr_crop_to_radius(ptr(key_xyz), key_xyz.shape[0], ptr(pts), n, ptr(out), ptr(cnt), ptr(scratch), sb,
                                 stream()))
    return out[: int(cnt.item())]


def voxel_first_rows(clouds, voxel_size):
    """Per cloud, the rows of ME.utils.sparse_quantize(xyz / voxel_size, return_index=True): the FIRST row of every occupied
    voxel, ascending (int64 on the GPU).  One host synchronisation for all the row counts."""
    maps = [ops.build_map(ops.voxelize(x, voxel_size, 0), want_first=True) for x in clouds]
    ops.finalize_maps(maps)
    return [torch.sort(m.first[: m.n]).values for m in maps]


def refine_complement_poses(xyz_curr, xyz_cmpls, Ms, icp_voxel_size=0.05, max_dist=0.2, max_iteration=200,
                            relative_fitness=1e-6, relative_rmse=1e-6, return_results=False):
    """_get_neighbourhood_icp (complement_data_loader.py:401-405) as ONE apr_icp_batch call with the key frame as the shared
    target.  Per complement frame, _get_icp's recipe (:376-388): both clouds reduced to the first row of every
    `icp_voxel_size` voxel, the odometry pose M applied to the frame (pts @ R.T + t in float32, :65-70), ICP of the moved
    frame onto the key frame from the identity with open3d's default thresholds, and the two poses composed.
    icp_voxel_size=None skips the reduction (Predator_APR's loader registers the full clouds).

    The composition returned is reg.transformation @ M in the column-vector form every consumer here uses
    (apply_transform, aggregate_frames): M first, then ICP's correction, i.e. the pose ICP actually found.  The reference
    writes `M @ reg.transformation` (:388) on transforms it handles transposed (:379-380); the two agree wherever the
    correction commutes with M, which is the reference's regime (a correction of millimetres).

    -> list of float64 [4,4] numpy poses (and the RegistrationResults when return_results)."""
    from .. import registration
    clouds = [_f32(xyz_curr)] + [_f32(x) for x in xyz_cmpls]
    if icp_voxel_size is not None:
        clouds = [x[sel].contiguous() for x, sel in zip(clouds, voxel_first_rows(clouds, icp_voxel_size))]
    tgt = clouds[0]
    Ms = [np.asarray(M, dtype=np.float64) for M in Ms]
    moved = [apply_transform(x, M) for x, M in zip(clouds[1:], Ms)]
    off = np.concatenate([[0], np.cumsum([len(m) for m in moved])]).astype(np.int64)
    nb = len(moved)
    rec, _ = ops.icp_batch(torch.cat(moved, 0), off, tgt, [0, len(tgt)], np.tile(np.eye(4), (nb, 1, 1)), max_dist,
                           max_iteration, relative_fitness, relative_rmse, tgt_of_problem=[0] * nb)
    results = registration.icp_results(rec)
    poses = [r.transformation @ M for r, M in zip(results, Ms)]
    return (poses, results) if return_results else poses


def refine_pose(xyz_curr, xyz_next, M, icp_voxel_size=0.05, max_dist=0.2, max_iteration=200):
    """_get_icp (complement_data_loader.py:369-399) without its disk cache: `next` registered onto `curr`, starting from
    the odometry pose M.  -> float64 [4,4] numpy (see refine_complement_poses)."""
    return refine_complement_poses(xyz_curr, [xyz_next], [M], icp_voxel_size, max_dist, max_iteration)[0]


def pairwise_init(pos_source, pos_target, velo2cam):
    """The ICP init of pairwise_registration (complement_data_loader.py:410-411): the odometry pose that moves the source
    frame into the target frame, float64 [4,4]."""
    pos_source, pos_target = np.asarray(pos_source, dtype=np.float64), np.asarray(pos_target, dtype=np.float64)
    velo2cam = np.asarray(velo2cam, dtype=np.float64)
    return (velo2cam @ pos_source.T @ np.linalg.inv(pos_target.T) @ np.linalg.inv(velo2cam)).T


def pairwise_inits(poses, velo2cam):
    """full_registration's inits for one side (:429-432): {(s, t): pairwise_init(poses[s], poses[t])} for s < t."""
    return {(s, t): pairwise_init(poses[s], poses[t], velo2cam) for s in range(len(poses)) for t in range(s + 1, len(poses))}


def inits_from_key_poses(Ms):
    """The same inits from the poses M_i that move the frames of one side into the key frame (M_0 = I for the key frame
    itself, not passed): M_st = M_t^-1 M_s, which is pairwise_init(pos_s, pos_t) up to rounding."""
    Ms = [np.eye(4)] + [np.asarray(M, dtype=np.float64) for M in Ms]
    return {(s, t): np.linalg.inv(Ms[t]) @ Ms[s] for s in range(len(Ms)) for t in range(s + 1, len(Ms))}


_LAYOUTS = {}


def _side_layout(n_clouds, n_sides):
    """Complete graphs on n_clouds nodes, edges (s, t) in full_registration's order, t == s + 1 certain (:434-451)."""
    key = (torch.cuda.current_device(), n_clouds, n_sides)
    if key not in _LAYOUTS:
        edges = [(s, t, t != s + 1) for s in range(n_clouds) for t in range(s + 1, n_clouds)]
        _LAYOUTS[key] = ops.PoseGraphLayout([(n_clouds, edges)] * n_sides, need_chain=True)
    return _LAYOUTS[key]


def _init_of(inits, s, t):
    return np.asarray(inits[(s, t)] if isinstance(inits, dict) else inits[s][t], dtype=np.float64).reshape(4, 4)


def _register_sides(sides, max_dist, max_dist_fine, max_iteration, return_graph):
    """sides: [(reduced clouds [1 + k] on the GPU, inits)], every side with the same k.  ONE icp_batch over every edge of
    every side, ONE information_batch on its records, ONE posegraph_optimize, ONE device -> host copy.
    -> per side the list of node poses (float64 [4,4] numpy), and the graph dict when asked."""
    n_clouds = len(sides[0][0])
    if any(len(c) != n_clouds for c, _ in sides) or not 2 <= n_clouds <= ops.POSEGRAPH_MAX_NODES:
        raise ValueError(f"multiway registration: 2 .. {ops.POSEGRAPH_MAX_NODES} clouds per side, the same number on every side")
    tgts, tgt_id, srcs, top, inits = [], {}, [], [], []
    for clouds, side_inits in sides:
        for s in range(n_clouds):
            for t in range(s + 1, n_clouds):
                if id(clouds[t]) not in tgt_id:                # the key frame is only ever a source
                    tgt_id[id(clouds[t])] = len(tgts)
                    tgts.append(clouds[t])
                srcs.append(clouds[s])
                top.append(tgt_id[id(clouds[t])])
                inits.append(_init_of(side_inits, s, t))
    so = np.concatenate([[0], np.cumsum([len(x) for x in srcs])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(x) for x in tgts])]).astype(np.int64)
    src, tgt = torch.cat(srcs, 0), torch.cat(tgts, 0)
    rec, _ = ops.icp_batch(src, so, tgt, to, np.stack(inits), max_dist, max_iteration, tgt_of_problem=top)
    info, _, _ = ops.information_batch(src, so, tgt, to, rec, max_dist_fine, tgt_of_problem=top)
    layout = _side_layout(n_clouds, len(sides))
    poses, conf, kept, iters, status = ops.posegraph_optimize(layout, rec, info, None, max_dist_fine)
    host = torch.cat([poses.reshape(-1), status.to(torch.float64)]).cpu().numpy()          # the one copy
    P = host[: layout.n_nodes * 16].reshape(len(sides), n_clouds, 4, 4)
    st = host[layout.n_nodes * 16:].astype(np.int64)
    if (st != ops.POSEGRAPH_OK).any():
        raise _lib.AprHipError(f"multiway registration: pose-graph status {st.tolist()} (include/apr_hip.h: "
                               "apr_posegraph_optimize); a side without correspondences at max_dist_fine gives 1")
    out = [[P[i, j].copy() for j in range(n_clouds)] for i in range(len(sides))]
    if not return_graph:
        return out, None
    ne = n_clouds * (n_clouds - 1) // 2
    graph = dict(records=rec.cpu().numpy().reshape(len(sides), ne, -1), information=info.cpu().numpy().reshape(len(sides), ne, 6, 6),
                 confidence=conf.cpu().numpy().reshape(len(sides), ne), kept=kept.cpu().numpy().reshape(len(sides), ne) != 0,
                 iterations=iters.cpu().numpy(), status=st,
                 edges=[(s, t) for s in range(n_clouds) for t in range(s + 1, n_clouds)])
    return out, graph


def full_registration(clouds, inits, max_dist=0.2, max_dist_fine=0.075, max_iteration=200, return_graph=False):
    """full_registration (complement_data_loader.py:423-463) of one side: `clouds` are the side's 1 + k clouds as the
    reference hands them over (already voxel-reduced), inits[(s, t)] (or inits[s][t]) the odometry init of every pair s < t
    (`pairwise_inits`).  ICP of every pair, its information matrix at max_dist_fine, the pose graph (t == s + 1: odometry
    edge, else an uncertain loop closure) and open3d's global optimisation, all on the device.
    -> the 1 + k node poses, float64 [4,4] numpy (and the graph dict when return_graph)."""
    out, graph = _register_sides([([_f32(x) for x in clouds], inits)], max_dist, max_dist_fine, max_iteration, return_graph)
    return (out[0], graph) if return_graph else out[0]


def multiway_registration(xyz_curr, xyz_cmpls, inits_left, inits_right, num_complement_one_side, icp_voxel_size=0.05,
                          max_dist=0.2, max_dist_fine=0.075, max_iteration=200, return_graph=False):
    """multiway_registration (complement_data_loader.py:466-516) without its caches: the default route to the APG's poses.
    xyz_cmpls: the 2k complement frames, left side first; inits_left / inits_right: `pairwise_inits` of [pos_curr] + the
    side's positions (:497-498).  Every cloud is reduced to the first row of each `icp_voxel_size` voxel (None: as given),
    both sides go through ONE icp_batch (k (k + 1) problems on 2k target segments), ONE information_batch and ONE
    posegraph_optimize, and the poses come back in one copy.
    -> the 2k poses P_0^-1 P_i in the reference's order (:508-509), float64 [4,4] numpy."""
    k = int(num_complement_one_side)
    if len(xyz_cmpls) != 2 * k:
        raise ValueError(f"multiway_registration: {2 * k} complement frames expected, got {len(xyz_cmpls)}")
    clouds = [_f32(xyz_curr)] + [_f32(x) for x in xyz_cmpls]
    if icp_voxel_size is not None:
        clouds = [x[sel].contiguous() for x, sel in zip(clouds, voxel_first_rows(clouds, icp_voxel_size))]
    sides = [([clouds[0]] + clouds[1 + side * k: 1 + (side + 1) * k], inits) for side, inits in ((0, inits_left), (1, inits_right))]
    out, graph = _register_sides(sides, max_dist, max_dist_fine, max_iteration, return_graph)
    poses = [np.linalg.inv(P[0]) @ P[i] for P in out for i in range(1, len(P))]
    return (poses, graph) if return_graph else poses


def aggregate_frames(key_xyz, complement_xyz, complement_poses, voxel_size, refine=False, icp_voxel_size=0.05,
                     icp_max_dist=0.2, icp_max_iteration=200, icp_max_dist_fine=0.075):
    """APG: returns (xyz_nghb cropped [M,3], sel indices of its voxelised subset).  refine=True: `complement_poses` are raw
    odometry and go through refine_complement_poses first, as the reference's loader does with debug_use_old_complement
    (:567-570).  refine='multiway': they go through multiway_registration, the loader's default (:571-574); the 2k frames
    are the left side then the right side, and the pairwise inits are derived from the poses (inits_from_key_poses)."""
    if isinstance(refine, str):
        if refine != 'multiway':
            raise ValueError(f"aggregate_frames: refine must be False, True or 'multiway', got {refine!r}")
        k = len(complement_xyz) // 2
        if len(complement_xyz) != 2 * k or k < 1:
            raise ValueError("aggregate_frames: refine='multiway' needs the same number of frames on both sides")
        complement_poses = multiway_registration(key_xyz, complement_xyz, inits_from_key_poses(complement_poses[:k]),
                                                 inits_from_key_poses(complement_poses[k:]), k, icp_voxel_size, icp_max_dist,
                                                 icp_max_dist_fine, icp_max_iteration)
    elif refine:
        complement_poses = refine_complement_poses(key_xyz, complement_xyz, complement_poses, icp_voxel_size, icp_max_dist,
                                                   icp_max_iteration)
    moved = [apply_transform(x, M) for x, M in zip(complement_xyz, complement_poses)]
    nghb = crop_to_radius(key_xyz, torch.cat(moved, 0))
    coords = ops.voxelize(nghb, voxel_size, 0)
    m = ops.build_map(coords, want_first=True)
    ops.finalize_maps([m])
    return nghb, m.first


def get_matching_indices(source, target, trans, search_voxel_size, K=None):
    """(i, j) pairs with |T src_i - tgt_j| < search_voxel_size, ordered by i then distance -> int64 [M,2]."""
    src = apply_transform(source, trans)
    tgt = _f32(target)
    nbr = point_ops.radius_neighbors(src, tgt, [len(src)], [len(tgt)], float(search_voxel_size))
    if K is not None:
        nbr = nbr[:, :K]
    valid = nbr < len(tgt)
    i = torch.arange(len(src), device=nbr.device).unsqueeze(1).expand_as(nbr)[valid]
    return torch.stack([i, nbr[valid].long()], 1)


def chamfer_sum(a, b):
    """sum_i min_j |a_i - b_j|^2 (0-d float64 GPU tensor)."""
    a, b = _f32(a), _f32(b)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    scratch = torch.empty(a.shape[0] * 4, dtype=torch.uint8, device=a.device)
    check(_lib.load().apr_chamfer_sum(ptr(a), a.shape[0], ptr(b), b.shape[0], ptr(out), ptr(scratch), scratch.numel(),
                                      stream()))
    return out[0]


def chamfer_distance(array1, array2):
    """forward / n1 + backward / n2 (complement_trainer.py:188-196); differentiable (apr_amd/npr.py)."""
    return npr.chamfer_distance(array1, array2)


class GenerativeMLP(nn.Module):
    """Linear -> ReLU -> BatchNorm1d stacks, final Linear -> ReLU (FCGF_APR/model/mlp.py:6-29); HIP forward."""
    CHANNELS = [None, 512, 128, None]

    def __init__(self, in_channel=125, out_points=6, bn_momentum=0.1):
        super().__init__()
        CH = self.CHANNELS
        self.mlp = nn.Sequential(
            nn.Linear(in_channel, CH[1]), nn.ReLU(), nn.BatchNorm1d(CH[1], momentum=bn_momentum),
            nn.Linear(CH[1], CH[2]), nn.ReLU(), nn.BatchNorm1d(CH[2], momentum=bn_momentum),
            nn.Linear(CH[2], out_points * 3), nn.ReLU())

    def forward(self, x, segments=None):
        """`segments` (row offsets, optional): x stacks the rows of several calls (the clouds of a batch, both frames) --
        the BatchNorms keep one set of batch statistics per call, as separate calls would."""
        return npr.run_stack(self.mlp, x, segments)


class GenerativeMLP_98(GenerativeMLP):
    CHANNELS = [None, 512, 256, None]


class GenerativeMLP_54(GenerativeMLP):
    CHANNELS = [None, 32, 16, None]


def npr_regulariser(generated, reg_type='L2', alpha=0.1):
    """Length penalty on the generated offsets [N, 3*ratio] (complement_trainer.py:432-440)."""
    return npr.regulariser(generated, reg_type, alpha)


def npr_points(generated, enc_coords, voxel_size, ratio):
    """Generated offsets + their voxel's corner -> [N*ratio, 3] points (complement_trainer.py:441-442)."""
    return (generated + voxel_size * enc_coords.to(generated.dtype).repeat(1, ratio)).reshape(-1, 3)


def npr_reconstruction_loss(generator, enc_feats, enc_coords, pcd_nghb, voxel_size, ratio, reg_strength=0.01,
                            reg_type='L2', alpha=0.1):
    """chamfer(generated + voxel centres, APG cloud) + reg * regulariser for one cloud (complement_trainer.py:424-448)."""
    generated = generator(enc_feats) * voxel_size                                       # [N, 3*ratio]
    reg = npr_regulariser(generated, reg_type, alpha)
    mod = npr_points(generated, enc_coords, voxel_size, ratio)
    return chamfer_distance(mod, pcd_nghb) + reg * reg_strength

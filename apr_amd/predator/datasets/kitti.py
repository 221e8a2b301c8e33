"""Pose refinement of Predator_APR's KITTI loader (/root/reference/Predator_APR/datasets/kitti.py:419-428).

The loader moves frame 0 by the odometry pose M, registers it onto frame 1 with point-to-point ICP (0.2 m, 200
iterations, full clouds: "for ICP we don't voxelize") and composes the two.  That is FCGF_APR's `_get_icp` with source
and target swapped and the 5 cm reduction off, so it runs on the same code (apr_amd/fcgf/lib/apg.py, csrc/icp.hip).
Disk caches and KITTI file IO stay with the caller.

The loader's complement frames take the multiway route (kitti.py:197-297: pairwise_registration, full_registration,
multiway_registration, the same text as FCGF_APR's loader, on clouds reduced to one point per 5 cm voxel), so that too
runs on FCGF's code: `multiway_registration` below is apr_amd/fcgf/lib/apg.py's (csrc/icp.hip, csrc/posegraph.hip).

`training_sample` / `test_sample` are the rest of __getitem__ (kitti.py:406-409, 441-524 and 585-636): scans plus poses in,
the reference's 12-tuple out as device tensors, every pass over the points on the device (csrc/apg.hip, csrc/voxel.hip,
csrc/points.hip).  File IO, pose caches, pair mining and `downsample_single` stay with the caller.
"""
import random

import numpy as np
import torch

from ... import ops
from ...fcgf.lib import apg
from ...fcgf.lib.apg import (full_registration, multiway_registration, pairwise_init, pairwise_inits,  # noqa: F401
                             refine_complement_poses, refine_pose)


def refine_pair_pose(xyz_0, xyz_1, M, icp_voxel_size=None, max_dist=0.2, max_iteration=200):
    """kitti.py:419-428: float64 [4,4] pose moving frame 0 into frame 1 (xyz_1 ~= xyz_0 @ R.T + t), refined from M."""
    return refine_pose(xyz_1, xyz_0, M, icp_voxel_size, max_dist, max_iteration)


def euler_zyx_matrix(angles):
    """scipy's Rotation.from_euler('zyx', angles).as_matrix() (kitti.py:500-501): extrinsic rotations about z, then y, then
    x, i.e. Rx(angles[2]) @ Ry(angles[1]) @ Rz(angles[0]), float64 [3,3].  scipy composes quaternions; the two agree to a
    few 1e-16."""
    a, b, c = (float(v) for v in angles)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cc, -sc], [0.0, sc, cc]])
    return Rx @ Ry @ Rz


def voxelise_clouds(clouds, voxel_size):
    """ONE apr_voxel_down_sample call over the clouds that have rows -> per cloud (centroids f64 [m,3], centroids f32 [m,3]);
    a cloud without rows (a crop that kept nothing) gives two empty tensors."""
    live = [c for c in clouds if len(c)]
    dev = clouds[0].device
    out = {}
    if live:
        res, lens = ops.voxel_down_sample(torch.cat(live, 0), [len(c) for c in live], voxel_size)
        ends = np.cumsum(lens)
        for c, e, n in zip(live, ends, lens):
            out[id(c)] = (res["centroid"][e - n:e], res["centroid32"][e - n:e])
    empty = (torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev))
    return [out.get(id(c), empty) for c in clouds]


def augment_pair(src, tgt, config, rng=np.random, pyrng=random):
    """kitti.py:494-517 on the float64 centroids `src`, `tgt` (GPU) -> the two fp32 inputs of the network.

    The host draws come in the reference's order, so a seeded `np.random` / `random` stands afterwards where the reference
    leaves it: rng.rand(n0,3), rng.rand(n1,3), rng.rand(3) (euler angles 'zyx'), rng.rand(1) (> 0.5: the source rotates,
    else the target), pyrng.random() (scale), rng.uniform(-r, r, 3) twice (shifts).  The points go through
    apr_sample_augment: float64, one rounding per operation, fp32 at the end (where the reference's collate calls
    .float(), datasets/dataloader.py:163)."""
    dev = src.device
    u0 = torch.from_numpy(rng.rand(src.shape[0], 3)).to(dev)
    u1 = torch.from_numpy(rng.rand(tgt.shape[0], 3)).to(dev)
    rot_ab = euler_zyx_matrix(rng.rand(3) * np.pi * 2)
    src_rotates = rng.rand(1)[0] > 0.5
    scale = config.augment_scale_min + (config.augment_scale_max - config.augment_scale_min) * pyrng.random()
    shift_src = rng.uniform(-config.augment_shift_range, config.augment_shift_range, 3)
    shift_tgt = rng.uniform(-config.augment_shift_range, config.augment_shift_range, 3)
    a = ops.sample_augment(src, u0, config.augment_noise, rot_ab if src_rotates else None, scale, shift_src)
    b = ops.sample_augment(tgt, u1, config.augment_noise, None if src_rotates else rot_ab, scale, shift_tgt)
    return a, b


def _finish_sample(src, tgt, nghb, tsfm, config, rng, pyrng):
    """:480-524 / :593-636 from the voxelised clouds on."""
    from ..lib import benchmark_utils as BU
    (src64, src32), (tgt64, tgt32) = src, tgt
    dev = src64.device
    tsfm = np.asarray(tsfm, dtype=np.float64)
    matching_inds = BU.get_correspondences(src32, tgt32, tsfm, config.overlap_radius)
    rot = torch.from_numpy(tsfm[:3, :3].astype(np.float32)).to(dev)
    trans = torch.from_numpy(tsfm[:3, 3][:, None].astype(np.float32)).to(dev)
    if getattr(config, "data_augmentation", False):
        src_in, tgt_in = augment_pair(src64, tgt64, config, rng, pyrng)
    else:
        src_in, tgt_in = src32, tgt32
    ones = lambda p: torch.ones((len(p), 1), dtype=torch.float32, device=dev)
    return (src_in, tgt_in, ones(src64), ones(tgt64), rot, trans, matching_inds, src64, tgt64, nghb[0], nghb[1],
            torch.ones(1))


def training_sample(xyz_0, xyz_1, xyz_cmpl_0, xyz_cmpl_1, list_M_0, list_M_1, tsfm, config, rng=np.random, pyrng=random):
    """kitti.py:406-409, 441-524 for one pair with its complement frames.

    xyz_*: [N,3] scans (arrays or tensors), xyz_cmpl_*: the 2k complement scans of each key frame, list_M_*: the poses
    that move them into their key frame (from `multiway_registration` / `refine_complement_poses` / the SLAM poses, as
    the loader has them), tsfm: the refined pose of the pair (`refine_pair_pose`).  config: first_subsampling_dl,
    overlap_radius, data_augmentation and, when that is set, augment_noise / augment_scale_min / augment_scale_max /
    augment_shift_range.

    The complement frames are moved (apr_transform_points, fp32) and cropped to the key frame's largest squared norm,
    strict < (apr_crop_to_radius); ONE apr_voxel_down_sample call covers the two key frames and the two aggregated clouds;
    the correspondences are benchmark_utils.get_correspondences on the fp32 centroids; features are ones.
    -> (src_pcd_input f32, tgt_pcd_input f32, src_feats, tgt_feats, rot f32 [3,3], trans f32 [3,1], matching_inds int64
        [M,2] (CPU, as get_correspondences returns it), src_pcd f64, tgt_pcd f64, src_nghb f64, tgt_nghb f64, ones(1)),
    what collate_fn_descriptor takes.  The train split's retry (:482-483) is the dataset's business: it is due when
    matching_inds.shape[0] < config.max_points."""
    key = [apg._f32(xyz_0), apg._f32(xyz_1)]
    nghb = []
    for k, frames, Ms in ((key[0], xyz_cmpl_0, list_M_0), (key[1], xyz_cmpl_1, list_M_1)):
        if len(frames) != len(Ms):
            raise ValueError(f"training_sample: {len(frames)} complement frames but {len(Ms)} poses")
        moved = torch.cat([apg.apply_transform(x, M) for x, M in zip(frames, Ms)], 0)
        nghb.append(apg.crop_to_radius(k, moved))
    src, tgt, n0, n1 = voxelise_clouds(key + nghb, config.first_subsampling_dl)
    return _finish_sample(src, tgt, (n0[0], n1[0]), tsfm, config, rng, pyrng)


def test_sample(xyz_0, xyz_1, tsfm, config, rng=np.random, pyrng=random):
    """kitti.py:585-636: the pair without complement clouds, the same voxelisation; src_nghb / tgt_nghb are empty."""
    src, tgt = voxelise_clouds([apg._f32(xyz_0), apg._f32(xyz_1)], config.first_subsampling_dl)
    empty = torch.empty((0,), dtype=torch.float64, device=src[0].device)
    return _finish_sample(src, tgt, (empty, empty), tsfm, config, rng, pyrng)

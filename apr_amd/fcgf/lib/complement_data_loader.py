"""The body of FCGF_APR's complement loader on the device: scans plus poses in, the tuple of
KITTINMComplementPairDataset.__getitem__ out, and its collate (FCGF_APR/lib/complement_data_loader.py).

  sample_random_trans        <- :29-38
  training_sample            <- :576-579, 596-716
  pair_sample                <- :751-822 (the plain branch: no complement frames)
  collate_complement_pair_fn <- :1224-1279
  collate_debug_pair_fn      <- :1282-1333
  collate_pair_fn            <- FCGF_APR/lib/data_loaders.py:26-78

Host orchestration of kernels that exist: apr_transform_points, apr_crop_to_radius, the voxel hash (sparse_quantize's
first rows), the radius search behind get_matching_indices, and apr_cloud_mean for the one reduction the reference does in
NumPy.  File IO, pose caches, pair mining, the `transform` jitter hook and `downsample_single` stay with the caller
(DESIGN section 20).
"""
import random

import numpy as np
import torch

from ... import ops
from ...MinkowskiEngine import utils as ME_utils
from . import apg


def rotation_about(axis, theta):
    """expm(cross(eye(3), axis / |axis| * theta)) (:29-30) by Rodrigues' formula, float64 on the host."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    theta = float(theta)
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def sample_random_trans(pcd, randg, rotation_range=360):
    """:33-38: a random rotation about the cloud's mean, float64 [4,4].  Draw order: randg.rand(3) (axis), then
    randg.rand(1) (angle).  The mean is taken on the device in float64 (apr_cloud_mean, the same bits run to run) where the
    reference takes np.mean of the float32 array: any mean gives a valid sample, because the pair's ground truth
    T1 @ M2 @ inv(T0) is built from the same T0 / T1 that move the clouds."""
    axis = randg.rand(3) - 0.5
    theta = rotation_range * np.pi / 180.0 * (randg.rand(1) - 0.5)
    T = np.eye(4)
    R = rotation_about(axis, theta[0])
    T[:3, :3] = R
    T[:3, 3] = R.dot(-ops.cloud_mean(apg._f32(pcd)).cpu().numpy())
    return T


NO_MATCH_FALLBACK = ((1, 1), (2, 2), (3, 3))      # :681-685, "remember to remove this pair later"


def training_sample(xyz_0, xyz_1, xyz_cmpl_0, xyz_cmpl_1, list_M_0, list_M_1, M2, config, randg, pyrng=random,
                    random_rotation=True, random_scale=True, test_augmentation=False, return_transforms=False):
    """:596-716 for one pair.  xyz_*: [N,3] scans, xyz_cmpl_*: the 2k complement scans of each key frame, list_M_*: the
    poses that move them into their key frame (apg.multiway_registration / refine_complement_poses / SLAM poses), M2:
    the pair's pose (xyz_1 ~= xyz_0 @ R.T + t; apg.refine_pose).  config: voxel_size, min_scale, max_scale,
    positive_pair_search_voxel_size_multiplier.

    Host draws in the reference's order: sample_random_trans for frame 0 then frame 1 (randg; :600-604, with the
    reference's own `rotation_range` arguments pi / 4 and 2 pi, which sample_random_trans reads as degrees), then
    pyrng.random() < 0.95 and, if so, pyrng.random() for the scale (:656-658).

    T0 / T1 are applied to the key frames and composed onto the complement poses (one fp32 transform per complement
    frame instead of the reference's two); apg.aggregate_frames then crops against the MOVED key frame, as the reference
    does.  The scale goes to xyz_0, xyz_1, trans[:3, 3] and the matching radius only: the reference does not scale the APG
    clouds (:660-662 leave xyz_nghb_* alone), and neither does this.  Zero matches: the reference's fallback pairs.
    -> (xyz_0 f32 [n0,3], xyz_1, xyz_nghb_0, xyz_nghb_1, coords_0 int32 [n0,3], coords_1, feats_0 f32 [n0,1], feats_1,
        matches int64 [M,2], trans float64 [4,4] numpy), device tensors but for trans; with return_transforms also (T0, T1)."""
    key = [apg._f32(xyz_0), apg._f32(xyz_1)]
    M2 = np.array(M2, dtype=np.float64)
    T = [np.eye(4), np.eye(4)]
    if random_rotation or test_augmentation:
        rotation_range = np.pi * 2 if test_augmentation else np.pi / 4
        T = [sample_random_trans(key[0], randg, rotation_range), sample_random_trans(key[1], randg, rotation_range)]
        trans = T[1] @ M2 @ np.linalg.inv(T[0])
        key = [apg.apply_transform(key[0], T[0]), apg.apply_transform(key[1], T[1])]
    else:
        trans = M2
    nghb = []
    for k, Tk, frames, Ms in ((key[0], T[0], xyz_cmpl_0, list_M_0), (key[1], T[1], xyz_cmpl_1, list_M_1)):
        if len(frames) != len(Ms):
            raise ValueError(f"training_sample: {len(frames)} complement frames but {len(Ms)} poses")
        pts, sel = apg.aggregate_frames(k, frames, [Tk @ np.asarray(M, dtype=np.float64) for M in Ms], config.voxel_size)
        nghb.append(pts[sel.long()].contiguous())
    search = config.voxel_size * config.positive_pair_search_voxel_size_multiplier
    if random_scale and pyrng.random() < 0.95:
        scale = config.min_scale + (config.max_scale - config.min_scale) * pyrng.random()
        search *= scale
        key = [scale * key[0], scale * key[1]]
        trans[:3, 3] = scale * trans[:3, 3]
    sel = apg.voxel_first_rows(key, config.voxel_size)
    xyz = [k[s].contiguous() for k, s in zip(key, sel)]
    matches = apg.get_matching_indices(xyz[0], xyz[1], trans, search)
    if len(matches) == 0:
        matches = torch.tensor(NO_MATCH_FALLBACK, dtype=torch.int64, device=matches.device)
    coords = [ops.voxelize(x, config.voxel_size, 0)[:, 1:].contiguous() for x in xyz]
    feats = [torch.ones((len(x), 1), dtype=torch.float32, device=x.device) for x in xyz]
    out = (xyz[0], xyz[1], nghb[0], nghb[1], coords[0], coords[1], feats[0], feats[1], matches, trans)
    return (out, (T[0], T[1])) if return_transforms else out


def collate_complement_pair_fn(list_data):
    """:1224-1279, same keys and dtypes.  `correspondences` (int32 [sum M, 2], CPU) carry the running row counts of both
    frames; the head moves for every item, also for one that is skipped because it has no matches; `T_gt` (f32
    [4 * kept, 4]) and `len_batch` hold the kept items only, while sinput*_C / _F hold every item (batch index = position in
    list_data), as the reference's sparse_collate call does.  pcd* stay tuples of per-item tensors."""
    xyz0, xyz1, xyz_nghb0, xyz_nghb1, coords0, coords1, feats0, feats1, matching_inds, trans = list(zip(*list_data))
    matching_inds_batch, trans_batch, len_batch = [], [], []
    start = np.zeros((1, 2), np.int64)
    for b in range(len(coords0)):
        N0, N1 = int(coords0[b].shape[0]), int(coords1[b].shape[0])
        m = matching_inds[b]
        m = m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        if len(m) != 0:
            t = trans[b]
            trans_batch.append(t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t)))
            matching_inds_batch.append(torch.from_numpy(m.astype(np.int64).reshape(-1, 2) + start))
            len_batch.append([N0, N1])
        start[0, 0] += N0      # the head moves whether or not the item was kept
        start[0, 1] += N1
    coords_batch0, feats_batch0 = ME_utils.sparse_collate(coords0, feats0)
    coords_batch1, feats_batch1 = ME_utils.sparse_collate(coords1, feats1)
    return {
        'pcd0': xyz0,
        'pcd1': xyz1,
        'pcd_nghb0': xyz_nghb0,
        'pcd_nghb1': xyz_nghb1,
        'sinput0_C': coords_batch0,
        'sinput0_F': feats_batch0.float(),
        'sinput1_C': coords_batch1,
        'sinput1_F': feats_batch1.float(),
        'correspondences': torch.cat(matching_inds_batch, 0).int(),
        'T_gt': torch.cat(trans_batch, 0).float(),
        'len_batch': len_batch,
    }


def pair_sample(xyz_0, xyz_1, M2, config, randg, pyrng=random, random_rotation=True, random_scale=True):
    """:751-822 for one pair, the branch the FCGF baseline trainers' loader takes (no complement frames).  Host draws in
    the reference's order: sample_random_trans for frame 0 then frame 1 (randg; :754-755, `rotation_range` pi / 4 read as
    degrees), then pyrng.random() < 0.95 and, if so, pyrng.random() for the scale (:775-777).  Composed from what
    training_sample uses; `downsample_single` and the `transform` hook stay with the caller.
    -> (xyz_0 f32 [n0,3], xyz_1, coords_0 int32 [n0,3], coords_1, feats_0 f32 [n0,1], feats_1, matches int64 [M,2],
        trans float64 [4,4] numpy): the 8-tuple of :820-822, device tensors but for trans."""
    key = [apg._f32(xyz_0), apg._f32(xyz_1)]
    M2 = np.array(M2, dtype=np.float64)
    if random_rotation:
        T0 = sample_random_trans(key[0], randg, np.pi / 4)
        T1 = sample_random_trans(key[1], randg, np.pi / 4)
        trans = T1 @ M2 @ np.linalg.inv(T0)
        key = [apg.apply_transform(key[0], T0), apg.apply_transform(key[1], T1)]
    else:
        trans = M2
    search = config.voxel_size * config.positive_pair_search_voxel_size_multiplier
    if random_scale and pyrng.random() < 0.95:
        scale = config.min_scale + (config.max_scale - config.min_scale) * pyrng.random()
        search *= scale
        key = [scale * key[0], scale * key[1]]
        trans[:3, 3] = scale * trans[:3, 3]
    sel = apg.voxel_first_rows(key, config.voxel_size)
    xyz = [k[s].contiguous() for k, s in zip(key, sel)]
    matches = apg.get_matching_indices(xyz[0], xyz[1], trans, search)
    if len(matches) == 0:
        matches = torch.tensor(NO_MATCH_FALLBACK, dtype=torch.int64, device=matches.device)
    coords = [ops.voxelize(x, config.voxel_size, 0)[:, 1:].contiguous() for x in xyz]
    feats = [torch.ones((len(x), 1), dtype=torch.float32, device=x.device) for x in xyz]
    return (xyz[0], xyz[1], coords[0], coords[1], feats[0], feats[1], matches, trans)


def _collate_pairs(list_data, concatenate):
    xyz0, xyz1, coords0, coords1, feats0, feats1, matching_inds, trans = list(zip(*list_data))
    xyz_batch0, xyz_batch1, matching_inds_batch, trans_batch, len_batch = [], [], [], [], []
    as_tensor = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    start = np.zeros((1, 2), np.int64)
    for b in range(len(coords0)):
        N0, N1 = int(coords0[b].shape[0]), int(coords1[b].shape[0])
        m = matching_inds[b]
        m = m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
        if len(m) != 0:
            xyz_batch0.append(as_tensor(xyz0[b]))
            xyz_batch1.append(as_tensor(xyz1[b]))
            trans_batch.append(as_tensor(trans[b]))
            matching_inds_batch.append(torch.from_numpy(m.astype(np.int64).reshape(-1, 2) + start))
            len_batch.append([N0, N1])
        start[0, 0] += N0      # the head moves whether or not the item was kept
        start[0, 1] += N1
    coords_batch0, feats_batch0 = ME_utils.sparse_collate(coords0, feats0)
    coords_batch1, feats_batch1 = ME_utils.sparse_collate(coords1, feats1)
    return {
        'pcd0': torch.cat(xyz_batch0, 0).float() if concatenate else xyz0,
        'pcd1': torch.cat(xyz_batch1, 0).float() if concatenate else xyz1,
        'sinput0_C': coords_batch0,
        'sinput0_F': feats_batch0.float(),
        'sinput1_C': coords_batch1,
        'sinput1_F': feats_batch1.float(),
        'correspondences': torch.cat(matching_inds_batch, 0).int(),
        'T_gt': torch.cat(trans_batch, 0).float(),
        'len_batch': len_batch,
    }


def collate_pair_fn(list_data):
    """FCGF_APR/lib/data_loaders.py:26-78 on pair_sample's 8-tuples, same keys and dtypes: `pcd0` / `pcd1` are the KEPT
    items' points concatenated (f32), everything else as collate_complement_pair_fn."""
    return _collate_pairs(list_data, True)


def collate_debug_pair_fn(list_data):
    """:1282-1333: as collate_pair_fn, but `pcd0` / `pcd1` stay tuples of every item's tensor."""
    return _collate_pairs(list_data, False)

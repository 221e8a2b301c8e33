"""Predator_APR's training / test sample on the device (apr_amd/predator/datasets/kitti.py: training_sample, test_sample)
against an oracle composed of tests/voxel_oracle.py, tests/apg_oracle.py and the op order of DESIGN section 20, on a small
synthetic pair with one complement frame per side (k = 1).  Centroids and augmented points are compared bit for bit."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import apg_oracle as AO  # noqa: E402
import sample_cases as SC  # noqa: E402
import voxel_oracle as VO  # noqa: E402
from apr_amd import synth  # noqa: E402
from apr_amd.fcgf.lib import apg  # noqa: E402
from apr_amd.predator import point_ops  # noqa: E402
from apr_amd.predator.configs.models import kitti_config  # noqa: E402
from apr_amd.predator.datasets import kitti  # noqa: E402
from apr_amd.predator.lib import benchmark_utils as BU  # noqa: E402

pytestmark = pytest.mark.gpu
AUG = dict(overlap_radius=0.45, max_points=512, augment_noise=0.01, augment_shift_range=2.0, augment_scale_max=1.2,
           augment_scale_min=0.8)


def _call(cfg, rng=np.random, pyrng=random):
    p = SC.scene_pair()
    return kitti.training_sample(p["xyz_0"], p["xyz_1"], p["cmpl_0"], p["cmpl_1"], p["M_0"], p["M_1"], p["tsfm"], cfg, rng, pyrng)


@pytest.fixture(scope="module")
def oracle(dev):
    """The four voxelised clouds of the pair.  The moved complement rows are the device's own (apr_transform_points has no
    bit-exact statement: they are held to apg_oracle.transform64's bound), the crop is apg_oracle's float32 statement on
    them, the voxels are voxel_oracle's."""
    p = SC.scene_pair()
    clouds = [p["xyz_0"], p["xyz_1"]]
    for key, frames, Ms in ((p["xyz_0"], p["cmpl_0"], p["M_0"]), (p["xyz_1"], p["cmpl_1"], p["M_1"])):
        moved = []
        for x, M in zip(frames, Ms):
            got = apg.apply_transform(x, M).cpu().numpy()
            want, bound = AO.transform64(x, M)
            assert (np.abs(got.astype(np.float64) - want) <= bound).all()
            moved.append(got)
        moved = np.concatenate(moved)
        keep = AO.crop_decision(key, moved)[3]
        assert 0 < keep.sum() < len(keep)              # the crop drops something and keeps something
        clouds.append(moved[keep])
    v = VO.voxel_down_sample(np.concatenate(clouds), [len(c) for c in clouds], 0.3)
    ends = np.cumsum(v["lengths"])
    return [v["centroid"][e - n:e] for e, n in zip(ends, v["lengths"])]


def test_training_sample_without_augmentation(dev, oracle):
    p = SC.scene_pair()
    s = _call(kitti_config(**AUG))
    assert len(s) == 12
    for got, want in zip(s[7:11], oracle):
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
    src32, tgt32 = oracle[0].astype(np.float32), oracle[1].astype(np.float32)
    assert s[0].dtype == torch.float32 and np.array_equal(s[0].cpu().numpy(), src32)
    assert s[1].dtype == torch.float32 and np.array_equal(s[1].cpu().numpy(), tgt32)
    for f, c in ((s[2], src32), (s[3], tgt32)):
        assert f.dtype == torch.float32 and tuple(f.shape) == (len(c), 1) and bool((f == 1).all())
    assert s[4].dtype == torch.float32 and np.array_equal(s[4].cpu().numpy(), p["tsfm"][:3, :3].astype(np.float32))
    assert s[5].dtype == torch.float32 and np.array_equal(s[5].cpu().numpy(), p["tsfm"][:3, 3:].astype(np.float32))
    want = BU.get_correspondences(src32, tgt32, p["tsfm"], 0.45)
    assert s[6].dtype == torch.int64 and len(want) > 512 and torch.equal(s[6].cpu(), want)
    assert torch.equal(s[11], torch.ones(1))


def _augment_oracle(src, tgt, cfg, rng, pyrng):
    """datasets/kitti.py:494-517 with the draws in the reference's order and the op order of DESIGN section 20."""
    u0, u1 = rng.rand(len(src), 3), rng.rand(len(tgt), 3)
    euler = rng.rand(3) * np.pi * 2
    R = kitti.euler_zyx_matrix(euler)
    side = rng.rand(1)[0] > 0.5
    scale = cfg.augment_scale_min + (cfg.augment_scale_max - cfg.augment_scale_min) * pyrng.random()
    sh0 = rng.uniform(-cfg.augment_shift_range, cfg.augment_shift_range, 3)
    sh1 = rng.uniform(-cfg.augment_shift_range, cfg.augment_shift_range, 3)

    def one(p, u, rot, sh):
        q = p + (u - 0.5) * cfg.augment_noise
        if rot:
            q = np.stack([(R[j, 0] * q[:, 0] + R[j, 1] * q[:, 1]) + R[j, 2] * q[:, 2] for j in range(3)], 1)
        return (q * scale + sh).astype(np.float32)

    return one(src, u0, side, sh0), one(tgt, u1, not side, sh1), side, euler, R


@pytest.mark.parametrize("seed", [1, 3])
def test_augmentation_bits_and_generator_positions(dev, oracle, seed):
    from scipy.spatial.transform import Rotation
    cfg = kitti_config(data_augmentation=True, **AUG)
    rng, pyrng = np.random.RandomState(seed), random.Random(seed + 100)
    twin, pytwin = np.random.RandomState(seed), random.Random(seed + 100)
    s = _call(cfg, rng, pyrng)
    a, b, side, euler, R = _augment_oracle(oracle[0], oracle[1], cfg, twin, pytwin)
    assert side == (seed == 3)                                           # the two seeds rotate one side each
    assert np.abs(R - Rotation.from_euler('zyx', euler).as_matrix()).max() < 1e-15
    assert np.array_equal(s[0].cpu().numpy(), a) and np.array_equal(s[1].cpu().numpy(), b)
    assert np.array_equal(s[7].cpu().numpy(), oracle[0]) and np.array_equal(s[8].cpu().numpy(), oracle[1])   # raw clouds stay
    st, tw = rng.get_state(), twin.get_state()
    assert st[0] == tw[0] and np.array_equal(st[1], tw[1]) and st[2:] == tw[2:]
    assert pyrng.getstate() == pytwin.getstate()


def test_test_sample_has_no_complement_clouds(dev, oracle):
    p = SC.scene_pair()
    s = kitti.test_sample(p["xyz_0"], p["xyz_1"], p["tsfm"], kitti_config(**AUG))
    assert len(s) == 12 and s[9].numel() == 0 and s[10].numel() == 0
    assert np.array_equal(s[7].cpu().numpy(), oracle[0]) and np.array_equal(s[8].cpu().numpy(), oracle[1])
    assert np.array_equal(s[0].cpu().numpy(), oracle[0].astype(np.float32))
    assert torch.equal(s[6], BU.get_correspondences(s[0], s[1], p["tsfm"], 0.45))


def test_registration_voxelizer_keyword(dev):
    """'open3d' feeds the network the oracle's centroids; the default feeds it apr_grid_subsample's barycentres, as before."""
    from apr_amd.predator.models.architectures import KPFCNN
    from apr_amd.predator.pipeline import PredatorRegistration
    cfg = kitti_config()
    np.random.seed(2)
    torch.manual_seed(2)
    model = KPFCNN(cfg).to(dev).eval()
    a, b, _ = synth.make_pair(70, n_beams=32, n_azimuth=700)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    want = VO.voxel_down_sample(np.concatenate([a, b]), [len(a), len(b)], 0.3)
    n0 = int(want["lengths"][0])
    pipe = PredatorRegistration(model, cfg, [38, 36, 36, 38], max_iteration=20000, voxelizer='open3d')
    src, tgt, feats, ov, sal = pipe.encode(ta, tb)
    assert np.array_equal(src.cpu().numpy(), want["centroid32"][:n0]) and np.array_equal(tgt.cpu().numpy(), want["centroid32"][n0:])
    assert feats.shape[0] == len(src) + len(tgt) and bool(torch.isfinite(feats).all())
    many = pipe.encode_batch([(ta, tb)])[0]
    assert torch.equal(many[0], src) and torch.equal(many[1], tgt)
    default = PredatorRegistration(model, cfg, [38, 36, 36, 38], max_iteration=20000)
    assert default.voxelizer == 'grid'
    pts, lens = point_ops.grid_subsample(torch.cat([ta, tb]), np.array([len(a), len(b)], np.int32), 0.3)
    src, tgt = default.encode(ta, tb)[:2]
    assert torch.equal(src, pts[:lens[0]]) and torch.equal(tgt, pts[lens[0]:])
    with pytest.raises(ValueError):
        PredatorRegistration(model, cfg, [38, 36, 36, 38], voxelizer='octree')

"""pair_sample (apr_amd/fcgf/lib/complement_data_loader.py; FCGF_APR/lib/complement_data_loader.py:751-822) on the small
synthetic pair of tests/sample_cases.py: the draws in the reference's order, the 8-tuple as the composition of the existing
calls, equal to training_sample's key-frame half, the fallback pairs, and the trainers' step on its collated batch."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_cases as SC  # noqa: E402
from apr_amd import ops  # noqa: E402
from apr_amd.fcgf.lib import apg  # noqa: E402
from apr_amd.fcgf.lib import complement_data_loader as CDL  # noqa: E402
from apr_amd.predator.configs.models import Config  # noqa: E402

pytestmark = pytest.mark.gpu
CFG = Config(voxel_size=0.3, min_scale=0.8, max_scale=1.2, positive_pair_search_voxel_size_multiplier=1.5)


def test_pair_sample_is_the_composition_of_the_existing_calls(dev):
    p = SC.scene_pair()
    randg, pyrng = np.random.RandomState(4), random.Random(9)
    out = CDL.pair_sample(p["xyz_0"], p["xyz_1"], p["tsfm"], CFG, randg, pyrng)
    assert len(out) == 8
    twin, pytwin = np.random.RandomState(4), random.Random(9)
    T = []
    for x in (p["xyz_0"], p["xyz_1"]):
        axis, theta = twin.rand(3) - 0.5, (np.pi / 4) * np.pi / 180.0 * (twin.rand(1) - 0.5)
        Tk = np.eye(4)
        Tk[:3, :3] = CDL.rotation_about(axis, theta[0])
        Tk[:3, 3] = Tk[:3, :3].dot(-ops.cloud_mean(torch.from_numpy(x).to(dev)).cpu().numpy())
        T.append(Tk)
    assert pytwin.random() < 0.95
    scale = 0.8 + (1.2 - 0.8) * pytwin.random()
    st, tw = randg.get_state(), twin.get_state()
    assert np.array_equal(st[1], tw[1]) and st[2:] == tw[2:] and pyrng.getstate() == pytwin.getstate()
    trans = T[1] @ p["tsfm"] @ np.linalg.inv(T[0])
    trans[:3, 3] = scale * trans[:3, 3]
    assert isinstance(out[7], np.ndarray) and out[7].dtype == np.float64 and np.array_equal(out[7], trans)
    scaled = [scale * apg.apply_transform(p["xyz_0"], T[0]), scale * apg.apply_transform(p["xyz_1"], T[1])]
    sel = apg.voxel_first_rows(scaled, 0.3)
    for i in (0, 1):
        want = scaled[i][sel[i]]
        assert out[i].dtype == torch.float32 and torch.equal(out[i], want)
        floor = np.floor(want.cpu().numpy() / np.float32(0.3)).astype(np.int32)      # a true fp32 division, as :809-810
        assert out[2 + i].dtype == torch.int32 and np.array_equal(out[2 + i].cpu().numpy(), floor)
        assert out[4 + i].dtype == torch.float32 and tuple(out[4 + i].shape) == (len(want), 1) and bool((out[4 + i] == 1).all())
    want = apg.get_matching_indices(out[0], out[1], trans, 0.3 * 1.5 * scale)
    assert out[6].dtype == torch.int64 and len(want) > 1000 and torch.equal(out[6], want)
    # the same draws give training_sample's key-frame half
    full = CDL.training_sample(p["xyz_0"], p["xyz_1"], p["cmpl_0"], p["cmpl_1"], p["M_0"], p["M_1"], p["tsfm"], CFG,
                               np.random.RandomState(4), random.Random(9))
    for a, b in zip(out[:7], (full[0], full[1]) + tuple(full[4:9])):
        assert torch.equal(a, b)
    assert np.array_equal(out[7], full[9])


def test_plain_and_fallback(dev):
    p = SC.scene_pair()
    randg, pyrng = np.random.RandomState(4), random.Random(9)
    out = CDL.pair_sample(p["xyz_0"], p["xyz_1"], p["tsfm"], CFG, randg, pyrng, random_rotation=False, random_scale=False)
    assert np.array_equal(out[7], p["tsfm"]) and np.array_equal(randg.get_state()[1], np.random.RandomState(4).get_state()[1])
    assert pyrng.getstate() == random.Random(9).getstate()
    key = torch.from_numpy(p["xyz_0"]).to(dev)
    assert torch.equal(out[0], key[apg.voxel_first_rows([key], 0.3)[0]])
    far = p["tsfm"].copy()
    far[:3, 3] += [0.0, 0.0, 500.0]
    out = CDL.pair_sample(p["xyz_0"], p["xyz_1"], far, CFG, np.random.RandomState(4), random.Random(9))
    assert out[6].tolist() == [[1, 1], [2, 2], [3, 3]]


def test_collated_pair_samples_train(dev):
    """Two pair samples through collate_pair_fn into PairTrainStep (batch_size 2, the triplet trainer)."""
    from apr_amd.fcgf.lib.pair_trainer import PairTrainStep
    from apr_amd.fcgf.model import load_model
    p = SC.scene_pair()
    items = [CDL.pair_sample(p["xyz_0"], p["xyz_1"], p["tsfm"], CFG, np.random.RandomState(s), random.Random(s)) for s in (4, 5)]
    batch = CDL.collate_pair_fn(items)
    n0 = [len(it[0]) for it in items]
    assert batch["pcd0"].shape[0] == sum(n0) == batch["sinput0_C"].shape[0] and batch["len_batch"][1][0] == n0[1]
    assert torch.equal(batch["correspondences"][len(items[0][6]):, 0].long().to(dev), items[1][6][:, 0] + n0[0])
    torch.manual_seed(0)
    enc = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    before = [q.detach().clone() for q in enc.parameters()]
    st = PairTrainStep(enc, torch.optim.SGD(enc.parameters(), lr=0.05, momentum=0.8), "TripletLossTrainer", batch_size=2,
                       triplet_num_pos=64, triplet_num_rand=128)
    np.random.seed(3)
    out = st(batch)
    assert bool(torch.isfinite(out["loss"])) and float(out["loss"]) > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, enc.parameters()))

"""PairTrainStep (apr_amd/fcgf/lib/pair_trainer.py): the loop body of the four FCGF trainers on ResUNetBN2C-32, SGD with
momentum, synth.make_pair(3 / 5, 16 beams x 600), for every trainer name and iter_size 1 and 2.

  - the step's loss is, bit for bit, the loss class called on the recorded encoder outputs with the same draws;
  - dL/dF at the encoder outputs agrees with the float64 oracle (tests/fcgf_losses_oracle.py; for the hardest-contrastive
    name the same expression written out below), mined rows pinned, within the feature-gradient bar of
    tests/test_fcgf_losses_gpu.py;
  - the weights after two steps are bit-equal to the same chain composed by hand (encoder -> loss -> backward -> SGD);
  - the whole run is bit-equal on a repeat.
The encoder's own gradients are held to their oracle in tests/test_train_units_gpu.py and test_train_iteration_gpu.py.
"""
import numpy as np
import pytest
import torch

from apr_amd import MinkowskiEngine as ME
from apr_amd import ops, synth
from apr_amd.fcgf.lib import apg
from apr_amd.fcgf.lib.pair_trainer import TRAINERS, PairTrainStep
from apr_amd.fcgf.lib.trainer import ContrastiveLoss, HardestContrastiveLoss, HardestTripletLoss, TripletLoss
from apr_amd.fcgf.model import load_model
from tests import fcgf_losses_oracle as O
from tests.test_fcgf_losses_gpu import BARS

pytestmark = pytest.mark.gpu

CFG = dict(num_pos_per_batch=256, num_hn_samples_per_batch=128, triplet_num_pos=128, triplet_num_hn=64, triplet_num_rand=256)
_PAIRS = {}


def _pair(dev, seed):
    if seed not in _PAIRS:
        xyz0, xyz1, T = synth.make_pair(seed, n_beams=16, n_azimuth=600)
        out, pts = {}, []
        for tag, xyz in (("0", xyz0), ("1", xyz1)):
            key = torch.from_numpy(xyz).to(dev)
            m = ops.build_map(ops.voxelize(key, 0.3, 0), want_first=True)
            ops.finalize_maps([m])
            out[f"sinput{tag}_C"] = m.coords
            out[f"sinput{tag}_F"] = torch.ones((m.n, 1), device=dev)
            pts.append(key[m.first.long()].contiguous())
        out["correspondences"] = apg.get_matching_indices(pts[0], pts[1], torch.from_numpy(T).float().to(dev), 0.45).cpu()
        _PAIRS[seed] = out
    return _PAIRS[seed]


def _draws(trainer, d, rng_seed):
    n0, n1, pairs = int(d["sinput0_C"].shape[0]), int(d["sinput1_C"].shape[0]), d["correspondences"].numpy()
    np.random.seed(rng_seed)
    if trainer == "ContrastiveLossTrainer":
        return O.generate_rand_negative_pairs(pairs, max(n0, n1), n0, n1)
    if trainer == "HardestContrastiveLossTrainer":
        return O.draw_hardest(n0, n1, len(pairs), CFG["num_pos_per_batch"], CFG["num_hn_samples_per_batch"], 1)[:3]
    if trainer == "TripletLossTrainer":
        return O.draw_triplet(n0, n1, len(pairs), CFG["triplet_num_pos"], CFG["triplet_num_rand"])
    return O.draw_hardest(n0, n1, len(pairs), CFG["triplet_num_pos"], CFG["triplet_num_hn"], CFG["triplet_num_rand"])


def _model(dev):
    torch.manual_seed(0)
    enc = load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    return enc, torch.optim.SGD(enc.parameters(), lr=0.05, momentum=0.8, weight_decay=1e-4)


def _crit(trainer):
    return {"ContrastiveLossTrainer": ContrastiveLoss, "HardestContrastiveLossTrainer": HardestContrastiveLoss,
            "TripletLossTrainer": TripletLoss, "HardestTripletLossTrainer": HardestTripletLoss}[trainer]()


def _loss(trainer, crit, F0, F1, pairs, draws, iter_size):
    """the reference's expression of the loss to run backward on, from the loss class (:266-270, :496-498, :625)"""
    if trainer == "ContrastiveLossTrainer":
        pos, neg = crit.loss(F0, F1, pairs, draws)
        return pos / iter_size + 1 * (neg / iter_size)
    if trainer == "HardestContrastiveLossTrainer":
        pos, neg = crit.contrastive_hardest_negative_loss(F0, F1, pairs, num_pos=CFG["num_pos_per_batch"],
                                                          num_hn_samples=CFG["num_hn_samples_per_batch"], draws=draws)
        return pos / iter_size + 1 * (neg / iter_size)
    return crit.triplet_loss(F0, F1, pairs, num_pos=CFG["triplet_num_pos"], num_hn_samples=CFG["triplet_num_hn"],
                             num_rand_triplet=CFG["triplet_num_rand"], draws=draws)[0] / iter_size


def _oracle_grad(trainer, crit, F0, F1, pairs, draws):
    """dL/dF0, dL/dF1 in float64 for iter_size 1, the device's mined rows pinned"""
    f0, f1 = F0.cpu().numpy(), F1.cpu().numpy()
    if trainer == "ContrastiveLossTrainer":
        r = O.contrastive(f0, f1, pairs, draws)
        return r["gF0_pos"] + r["gF0_neg"], r["gF1_pos"] + r["gF1_neg"]
    if trainer == "TripletLossTrainer":
        r = O.triplet(f0, f1, pairs, draws)
        return r["gF0"], r["gF1"]
    if trainer == "HardestTripletLossTrainer":
        got = crit.last.mined()
        r = O.hardest_triplet(f0, f1, pairs, draws, mined=(got["D01ind"].cpu().numpy(), got["D10ind"].cpu().numpy()))
        assert np.array_equal(r["mask0"], got["mask0"].cpu().numpy().astype(bool))
        return r["gF0"], r["gF1"]
    # contrastive_hardest_negative_loss (FCGF_APR/lib/trainer.py:400-452) in float64 on the device's mined rows
    pd = crit.prepare(len(f0), len(f1), pairs, CFG["num_pos_per_batch"], CFG["num_hn_samples_per_batch"], draws, F0.device)
    with torch.no_grad():
        pos0, pos1, d01, d10, keys, seed = crit._mine_and_reduce(F0, F1, pd, mine_only=True)
    pos0, pos1, d01, d10, keys = (t.cpu() for t in (pos0, pos1, d01, d10, keys))
    a, b = torch.tensor(f0, dtype=torch.float64, requires_grad=True), torch.tensor(f1, dtype=torch.float64, requires_grad=True)
    D01 = torch.sqrt((a[pos0] - b[d01]).pow(2).sum(1) + 1e-7)
    D10 = torch.sqrt((b[pos1] - a[d10]).pow(2).sum(1) + 1e-7)
    m0 = ~torch.isin(pos0 + d01 * seed, keys)
    m1 = ~torch.isin(d10 + pos1 * seed, keys)
    pos = torch.relu((a[pos0] - b[pos1]).pow(2).sum(1) - 0.1).mean()
    neg = (torch.relu(1.4 - D01[m0]).pow(2).mean() + torch.relu(1.4 - D10[m1]).pow(2).mean()) / 2
    (pos + neg).backward()
    return a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("iter_size", [1, 2])
@pytest.mark.parametrize("trainer", TRAINERS)
def test_pair_train_step(dev, trainer, iter_size):
    dicts = [_pair(dev, s) for s in (3, 5)[:iter_size]]
    draws = [[_draws(trainer, d, 100 * step + k) for k, d in enumerate(dicts)] for step in range(2)]

    def run():
        enc, opt = _model(dev)
        st = PairTrainStep(enc, opt, trainer, iter_size=iter_size, batch_size=1, **CFG)
        outs, feats = [], None
        for step in range(2):
            outs.append(st(dicts if iter_size > 1 else dicts[0], draws=draws[step]))
            if step == 0:
                feats = [(a.detach().clone(), b.detach().clone()) for a, b in st.last_features]
        return enc, outs, feats
    enc, outs, feats = run()
    assert all(v.dim() == 0 and v.is_cuda for o in outs for v in o.values())
    assert set(outs[0]) == ({"loss", "pos_loss", "neg_loss"} if "Contrastive" in trainer else {"loss", "pos_dist", "neg_dist"})

    # the step's loss from the loss class on the recorded encoder outputs; dL/dF against the oracle
    total, worst = 0, 0.0
    for (F0, F1), d, dr in zip(feats, dicts, draws[0]):
        crit = _crit(trainer)
        a, b = F0.clone().requires_grad_(True), F1.clone().requires_grad_(True)
        loss = _loss(trainer, crit, a, b, d["correspondences"], dr, iter_size)
        total = total + loss.detach()
        (loss * iter_size).backward()                    # iter_size is 1 or 2: the product is exact
        g0, g1 = _oracle_grad(trainer, crit, F0, F1, d["correspondences"].numpy(), dr)
        for got, want in ((a.grad, g0), (b.grad, g1)):
            worst = max(worst, float(np.linalg.norm(got.cpu().double().numpy() - want) / np.linalg.norm(want)))
    assert torch.equal(total, outs[0]["loss"]), (float(total), float(outs[0]["loss"]))
    print(f"[{trainer} x{iter_size}] loss {float(total):.6f}; dL/dF rel-L2 from the oracle {worst:.2e}")
    assert worst < BARS["grad"], worst

    # the same two steps composed by hand
    enc2, opt2 = _model(dev)
    crit = _crit(trainer)
    for step in range(2):
        enc2.train()
        opt2.zero_grad()
        for d, dr in zip(dicts, draws[step]):
            frames = [ME.SparseTensor(d[f"sinput{k}_F"], coordinates=d[f"sinput{k}_C"]) for k in ("0", "1")]
            e = enc2.forward_frames(frames)
            _loss(trainer, crit, e[0].F, e[1].F, d["correspondences"], dr, iter_size).backward()
        opt2.step()
    for (name, p), q in zip(enc.named_parameters(), enc2.parameters()):
        assert torch.equal(p, q), f"{name} differs from the chain composed by hand"

    # and on a repeat
    enc3, outs3, _ = run()
    for o, o3 in zip(outs, outs3):
        for k in o:
            assert torch.equal(o[k], o3[k]), k
    for (name, p), q in zip(enc.named_parameters(), enc3.parameters()):
        assert torch.equal(p, q), f"{name} differs on a repeat"
    changed = sum(int(not torch.equal(p, q)) for p, q in zip(enc.parameters(), _model(dev)[0].parameters()))
    assert changed > 0

"""The float64 oracle of one APR training iteration (oracle/apr_step_oracle.py) and the dtype-following, pinnable encoder
oracle under it: float32 without pins gives the bits of the float32-only code it replaced, pins that repeat the oracle's own
decisions change nothing, and the pinned float64 iteration's autograd gradients agree with central finite differences."""
import copy

import numpy as np
import pytest
import torch

from apr_amd import synth
from apr_amd.fcgf.lib import apg
from oracle import apr_step_oracle as AO
from oracle import match_pose_oracle as MO
from oracle import me_oracle as OME
from oracle import resunet_oracle as OR

_RELU_SITES = OR.RELU_SITES


def _old_conv_forward(x, W, kernel_size, stride, bias=None, transpose=False):
    """me_oracle.conv_forward as it was before it followed the input dtype (float32 hard-coded)."""
    cm, ts = x.coordinate_manager, x.coordinate_map_key
    if kernel_size == 1 and stride == 1:
        out = x.F @ W
        if bias is not None:
            out = out + bias
        return x._like(out)
    if not transpose:
        ts_out = ts * stride
        nbr = cm.get_map(ts, ts_out, kernel_size)
    else:
        ts_out = ts // stride
        fwd = cm.get_map(ts_out, ts, kernel_size)
        nbr = OME.transpose_map(fwd, len(cm.get_coords(ts_out)))
    out = torch.zeros(nbr.shape[0], W.shape[2], dtype=torch.float32)
    for o in range(nbr.shape[1]):
        j = np.nonzero(nbr[:, o] >= 0)[0]
        if len(j) == 0:
            continue
        i = nbr[j, o]
        out.index_add_(0, torch.from_numpy(j), x.F[torch.from_numpy(i.astype(np.int64))] @ W[o])
    if bias is not None:
        out = out + bias
    return x._like(out, ts_out)


def _old_hardest_contrastive(F0, F1, positive_pairs, sel0, sel1, pos_sel, pos_thresh=0.1, neg_thresh=1.4):
    """match_pose_oracle.hardest_contrastive as it was before it followed the input dtype."""
    F0 = torch.as_tensor(F0, dtype=torch.float32)
    F1 = torch.as_tensor(F1, dtype=torch.float32)
    positive_pairs = np.asarray(positive_pairs, dtype=np.int64)
    hash_seed = max(len(F0), len(F1))
    sample = positive_pairs if pos_sel is None else positive_pairs[pos_sel]
    subF0, subF1 = F0[sel0], F1[sel1]
    pos_ind0, pos_ind1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[pos_ind0], F1[pos_ind1]
    D01min, D01ind = MO.pdist(posF0, subF1, 'L2').min(1)
    D10min, D10ind = MO.pdist(posF1, subF0, 'L2').min(1)
    pos_keys = MO._hash(positive_pairs, hash_seed)
    D01ind = np.asarray(sel1)[D01ind.numpy()]
    D10ind = np.asarray(sel0)[D10ind.numpy()]
    mask0 = torch.from_numpy(np.logical_not(np.isin(MO._hash([pos_ind0, D01ind], hash_seed), pos_keys)))
    mask1 = torch.from_numpy(np.logical_not(np.isin(MO._hash([D10ind, pos_ind1], hash_seed), pos_keys)))
    pos_loss = torch.relu((posF0 - posF1).pow(2).sum(1) - pos_thresh)
    neg_loss0 = torch.relu(neg_thresh - D01min[mask0]).pow(2)
    neg_loss1 = torch.relu(neg_thresh - D10min[mask1]).pow(2)
    return pos_loss.mean(), (neg_loss0.mean() + neg_loss1.mean()) / 2


def _coords(seed, beams=8, azimuth=200):
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    out = []
    for xyz in (xyz0, xyz1):
        c, sel = OME.sparse_quantize(xyz / np.float32(0.3), return_index=True)
        out.append((OME.batched_coordinates([c]), xyz[sel]))
    return out, T


def _encode(om, C, dtype=torch.float32, pins=None):
    x = OME.SparseTensor(torch.ones(len(C), 1, dtype=dtype), coordinates=C)
    y = om(x, pins).F
    return x, y


def _encoder(name="ResUNetBN2C", seed=0):
    torch.manual_seed(seed)
    om = OR.MODELS[name](1, 32, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3)
    OR.randomize_bn_stats(om, seed)
    return om.train()


def _grads_and_state(om, y, proj):
    om.zero_grad()
    (y * proj).sum().backward()
    return ([p.grad.clone() for p in om.parameters()], [b.clone() for b in om.buffers()])


def test_float32_oracle_without_pins_keeps_its_bits(monkeypatch):
    """The dtype-following conv gives, in float32, the bits of the float32-only code: features, every gradient and the
    running statistics of a training step."""
    C = _coords(3)[0][0][0]
    runs = []
    for old in (False, True):
        if old:
            monkeypatch.setattr(OME, "conv_forward", _old_conv_forward)
        om = _encoder()
        _, y = _encode(om, C)
        assert y.dtype == torch.float32
        proj = torch.from_numpy(np.random.default_rng(0).standard_normal(tuple(y.shape)).astype(np.float32))
        runs.append((y.detach(),) + _grads_and_state(om, y, proj))
    (ya, ga, ba), (yb, gb, bb) = runs
    assert torch.equal(ya, yb)
    assert all(torch.equal(u, v) for u, v in zip(ga, gb)) and all(torch.equal(u, v) for u, v in zip(ba, bb))
    # numpy features stay float32, whatever their dtype (the HIP path's input type)
    assert OME.SparseTensor(np.ones((3, 1)), coordinates=C[:3]).F.dtype == torch.float32


def test_hardest_contrastive_keeps_float32_bits_follows_float64_and_takes_pins():
    rng = np.random.default_rng(1)
    F0 = rng.standard_normal((400, 16)).astype(np.float32)
    F1 = rng.standard_normal((380, 16)).astype(np.float32)
    pos = np.stack([rng.permutation(400)[:150], rng.permutation(380)[:150]], 1).astype(np.int64)
    F1[pos[:, 1]] = F0[pos[:, 0]] + 0.3 * rng.standard_normal((150, 16)).astype(np.float32)
    F0 /= np.linalg.norm(F0, axis=1, keepdims=True)         # unit rows, as the encoder's: negatives within neg_thresh
    F1 /= np.linalg.norm(F1, axis=1, keepdims=True)
    sel0, sel1, pos_sel = rng.choice(400, 96, replace=False), rng.choice(380, 96, replace=False), rng.choice(150, 60, replace=False)
    for a, b in ((F0, F1), (torch.from_numpy(F0), torch.from_numpy(F1)), (F0.astype(np.float64), F1.astype(np.float64))):
        new, old = MO.hardest_contrastive(a, b, pos, sel0, sel1, pos_sel), _old_hardest_contrastive(a, b, pos, sel0, sel1, pos_sel)
        assert all(u.dtype == torch.float32 and torch.equal(u, v) for u, v in zip(new, old))
    d0, d1 = torch.from_numpy(F0).double(), torch.from_numpy(F1).double()
    p64, n64 = MO.hardest_contrastive(d0, d1, pos, sel0, sel1, pos_sel)
    assert p64.dtype == n64.dtype == torch.float64 and float(n64) > 0
    # pinning the hardest negatives to the oracle's own arg-mins changes nothing
    sample = pos[pos_sel]
    D01ind = sel1[MO.pdist(d0[sample[:, 0]], d1[sel1]).argmin(1).numpy()]
    D10ind = sel0[MO.pdist(d1[sample[:, 1]], d0[sel0]).argmin(1).numpy()]
    pp, npin = MO.hardest_contrastive(d0, d1, pos, sel0, sel1, pos_sel, hardest=(D01ind, D10ind))
    assert float(pp) == float(p64) and abs(float(npin) - float(n64)) <= 1e-14 * abs(float(n64))
    # another (wrong) negative: another value
    _, nw = MO.hardest_contrastive(d0, d1, pos, sel0, sel1, pos_sel, hardest=(np.roll(D01ind, 1), D10ind))
    assert float(nw) != float(n64)


def _own_pins(om, C):
    """The oracle's own ReLU decisions at every site, by module name, each with its rows shuffled (coordinates travel with
    them: the pins must be matched by coordinates, not by row position)."""
    seen = []
    real = OME.relu

    def spy(x, pin=None):
        seen.append((x.coordinate_manager.get_coords(x.coordinate_map_key), (x.F > 0).detach()))
        return real(x, pin)
    OME.relu = spy
    try:
        with torch.no_grad():
            _encode(om, C, torch.float64)
    finally:
        OME.relu = real
    assert len(seen) == len(_RELU_SITES)
    pins, rng = {}, np.random.default_rng(5)
    for name, (coords, mask) in zip(_RELU_SITES, seen):
        if name not in pins:
            p = rng.permutation(len(coords))
            pins[name] = (coords[p], mask[torch.from_numpy(p)])
    return pins


def test_pinning_every_encoder_mask_to_its_own_decision_changes_nothing():
    C = _coords(4)[0][0][0]
    om = _encoder("ResUNetBN2C", 1).double()
    state = copy.deepcopy(om.state_dict())
    pins = _own_pins(om, C)
    assert set(pins) == set(_RELU_SITES)
    runs = []
    for p in (None, pins):
        om.load_state_dict(state)
        _, y = _encode(om, C, torch.float64, p)
        proj = torch.from_numpy(np.random.default_rng(2).standard_normal(tuple(y.shape)))
        runs.append((y.detach(),) + _grads_and_state(om, y, proj))
    (ya, ga, ba), (yb, gb, bb) = runs
    assert torch.equal(ya, yb)
    assert all(torch.equal(u, v) for u, v in zip(ga, gb)) and all(torch.equal(u, v) for u, v in zip(ba, bb))
    # a pin that differs from the sign does change the result (the pins are applied, not ignored)
    coords, mask = pins["block3.conv1"]
    flipped = dict(pins, **{"block3.conv1": (coords, ~mask)})
    om.load_state_dict(state)
    _, y = _encode(om, C, torch.float64, flipped)
    assert not torch.equal(y.detach(), ya)


def _small_iteration(seed=3):
    """Two frames of one small pair, their stand-in APG clouds and GT pairs, all on the host."""
    frames, T = _coords(seed)
    rng = np.random.default_rng(seed)
    coords, feats, clouds = [], [], []
    for C, pts in frames:
        coords.append(C)
        feats.append(np.ones((len(C), 1), np.float32))
        clouds.append([torch.from_numpy((np.repeat(pts, 2, 0) + rng.normal(0, 0.1, (2 * len(pts), 3))).astype(np.float32))])
    p0 = frames[0][1].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    j, d2 = AO.argmin_rows(p0, frames[1][1])
    keep = d2 < 0.45 ** 2
    pairs = np.stack([np.nonzero(keep)[0], j[keep]], 1).astype(np.int64)
    draws = (rng.choice(len(coords[0]), 128, replace=False), rng.choice(len(coords[1]), 128, replace=False),
             rng.choice(len(pairs), 96, replace=False))
    return coords, feats, clouds, pairs, draws


def _models(reg_type="L2"):
    om = _encoder("ResUNetBN2C", 2).double()
    torch.manual_seed(2)
    mlp = AO.generator_copy(apg.GenerativeMLP_54(in_channel=32, out_points=4, bn_momentum=0.05).mlp)
    return om, mlp, AO.StepConfig(ratio=4, reg_type=reg_type, loss_ratio=2e-3)


def _own_iteration_pins(om, mlp, data, cfg):
    """Pins that repeat every decision of an unpinned float64 iteration."""
    coords, feats, clouds, pairs, draws = data
    it = AO.iteration(om, mlp, *data, cfg)
    pins = AO.Pins(enc=[_own_pins(om, C) for C in coords], gen=[[(p > 0) for p in pre] for pre in it.pre_relu],
                   chamfer=list(it.argmin))
    sel0, sel1, pos_sel = draws
    sample = pairs[pos_sel]
    F0, F1 = (f.detach() for f in it.F)
    pins.hardest = (sel1[MO.pdist(F0[sample[:, 0]], F1[sel1]).argmin(1).numpy()],
                    sel0[MO.pdist(F1[sample[:, 1]], F0[sel0]).argmin(1).numpy()])
    return pins


def test_pinning_every_decision_of_an_iteration_to_its_own_changes_nothing():
    data = _small_iteration()
    om, mlp, cfg = _models()
    state, gstate = copy.deepcopy(om.state_dict()), copy.deepcopy(mlp.state_dict())
    pins = _own_iteration_pins(om, mlp, data, cfg)
    assert len(pins.gen) == 2 and all(len(g) == 3 for g in pins.gen) and len(pins.chamfer) == 2
    runs = []
    for p in (None, pins):
        om.load_state_dict(state)
        mlp.load_state_dict(gstate)
        opt = AO.make_optimizer(om, mlp, lr=0.05, momentum=0.8, weight_decay=1e-4)
        it = AO.step(om, mlp, opt, *data, cfg, pins=p)
        runs.append(([v.item() for v in [it.loss, it.pos_loss, it.neg_loss] + it.cham + it.reg],
                     [f.grad.clone() for f in it.F], [t.detach().clone() for t in list(om.state_dict().values())
                                                      + list(mlp.state_dict().values())]))
    (la, fa, sa), (lb, fb, sb) = runs
    assert np.allclose(la, lb, rtol=1e-13, atol=0), (la, lb)
    assert all(torch.allclose(u, v, rtol=1e-12, atol=1e-15) for u, v in zip(fa, fb))
    assert all(torch.allclose(u.double(), v.double(), rtol=1e-12, atol=1e-15) for u, v in zip(sa, sb))


@pytest.mark.parametrize("reg_type", ["L2", "RepelL2", "RepelL1"])
def test_pinned_float64_iteration_matches_finite_differences(reg_type):
    """With every decision pinned the iteration's loss is smooth in the parameters: its autograd gradient at a few
    parameters of the encoder (first conv, a residual block, a transposed stage, the final bias, a BatchNorm gamma) and of
    the generator equals the central difference."""
    data = _small_iteration(seed=5)
    om, mlp, cfg = _models(reg_type)
    pins = _own_iteration_pins(om, mlp, data, cfg)

    def loss():
        return AO.iteration(om, mlp, *data, cfg, pins=pins).loss

    om.zero_grad(); mlp.zero_grad()
    loss().backward()
    named = dict(om.named_parameters())
    named.update({f"mlp.{k}": v for k, v in mlp.named_parameters()})
    probes = [("conv1.kernel", (60, 0, 3)), ("block2.conv1.kernel", (13, 5, 7)), ("conv3_tr.kernel", (4, 100, 2)),
              ("block1.norm2.bn.weight", (9,)), ("final.bias", (0, 11)), ("mlp.0.weight", (3, 17)),
              ("mlp.2.bias", (5,)), ("mlp.6.weight", (7, 2))]
    h = 1e-6
    for name, idx in probes:
        p = named[name]
        g = float(p.grad[idx])
        with torch.no_grad():
            v = float(p[idx])
            p[idx] = v + h
            up = float(loss())
            p[idx] = v - h
            dn = float(loss())
            p[idx] = v
        fd = (up - dn) / (2 * h)
        assert abs(fd - g) <= 1e-6 * abs(g) + 1e-9, (name, idx, g, fd)

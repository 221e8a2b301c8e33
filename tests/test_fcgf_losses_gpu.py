"""ContrastiveLoss, TripletLoss and HardestTripletLoss on the pair-list kernels (apr_amd/fcgf/lib/trainer.py,
csrc/pair_loss.hip) against the fp64 leg of the reference's own text (tests/golden/fcgf_losses_ref.npz).

Per loss and fixture case: the returned values and the feature gradients within BARS (relative; relative L2 for gradients;
rows the reference leaves at zero are exactly zero), the masks of the key filter and the mined rows EQUAL to the
reference's (the generator keeps the yardstick clear of every decision: no exclusion list), the same bits on a second
call, from `prepare()` called before the features exist, and from the default NumPy stream replayed from the seed.

Measured on an MI355X against the fp64 leg, worst over the three losses and both cases: returned values 2.0e-7 (the
contrastive negative mean at c = 32; the loss of the triplets 1.1e-7), feature gradients 1.98e-7 relative L2 (contrastive,
c = 32) -- the reference's own fp32 leg is 1.96e-7 from its fp64 leg there, the kernels are nowhere worse than 1.15x that
leg.  Bars at 5x the measured worst (the results are bit-stable: the margin covers regenerated inputs), both far below
the project's ceilings of 1e-5 on loss values and 8e-6 on feature gradients.  tests/test_fcgf_losses_edges_gpu.py and
tests/test_pair_train_step_gpu.py use the same bars (worst there: values 1.2e-7, dL/dF 9.9e-8).
Every run prints its measured values (`pytest -s`).
"""
import numpy as np
import pytest
import torch

from tests import fcgf_losses_oracle as O

pytestmark = pytest.mark.gpu

BARS = {"value": 1e-6, "grad": 1e-6}
SEED = 77
Z = O.load_fixture()


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _inputs(tag, dev):
    F0 = torch.from_numpy(Z[f"{tag}_F0"]).to(dev).requires_grad_(True)
    F1 = torch.from_numpy(Z[f"{tag}_F1"]).to(dev).requires_grad_(True)
    return F0, F1, Z[f"{tag}_pairs"], [int(v) for v in Z[f"{tag}_args"]]


def _grad_err(F, key):
    g = F.grad.cpu().double().numpy()
    want = O.fixture_grad(Z, key, len(g))
    untouched = np.setdiff1d(np.arange(len(g)), Z[key + "_rows"])
    assert not g[untouched].any(), f"{key}: a row outside every term has a gradient"
    return float(np.linalg.norm(g - want) / np.linalg.norm(want))


def _check(tag, kind, worst):
    print(f"[{tag} {kind}] measured:", {k: f"{v:.2e}" for k, v in worst.items()},
          "fp32 reference leg, gradients:", [f"{v:.2e}" for v in Z[f"{tag}_{kind}_grad32_rel"]])
    for k, v in worst.items():
        assert v < BARS["grad" if k.startswith("g") else "value"], (k, v)


def _same_bits(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.detach(), y.detach()) or (bool(torch.isnan(x)) and bool(torch.isnan(y)))


@pytest.mark.parametrize("tag", O.CASES)
def test_contrastive(dev, tag):
    from apr_amd.fcgf.lib.trainer import ContrastiveLoss
    m = ContrastiveLoss()
    neg = Z[f"{tag}_con_neg_pairs"]

    def run(how):
        F0, F1, pairs, _ = _inputs(tag, dev)
        if how == "draws":
            out = m.loss(F0, F1, torch.from_numpy(pairs), neg)
        elif how == "prepared":
            out = m.loss(F0, F1, None, draws=m.prepare(len(F0), len(F1), pairs, draws=neg, device=dev))
        else:
            np.random.seed(SEED)
            out = m.loss(F0, F1, torch.from_numpy(pairs))
            assert np.random.rand() == float(Z[f"{tag}_con_next"])
        (out[0] + m.neg_weight * out[1]).backward()
        return out, F0, F1
    out, F0, F1 = run("draws")
    assert all(o.dim() == 0 and o.is_cuda for o in out)
    worst = {"pos": _rel(float(out[0].detach()), Z[f"{tag}_con_values"][0]),
             "neg": _rel(float(out[1].detach()), Z[f"{tag}_con_values"][1]),
             "gF0": _grad_err(F0, f"{tag}_con_gF0"), "gF1": _grad_err(F1, f"{tag}_con_gF1")}
    _check(tag, "con", worst)
    np.random.seed(SEED)
    assert np.array_equal(m.generate_rand_negative_pairs(Z[f"{tag}_pairs"], max(len(F0), len(F1)), len(F0), len(F1)), neg)
    for how in ("draws", "prepared", "rng"):
        out2, G0, G1 = run(how)
        _same_bits(out, out2)
        assert torch.equal(F0.grad, G0.grad) and torch.equal(F1.grad, G1.grad), how


@pytest.mark.parametrize("kind", ["tri", "hard"])
@pytest.mark.parametrize("tag", O.CASES)
def test_triplet_losses(dev, tag, kind):
    from apr_amd.fcgf.lib.trainer import HardestTripletLoss, TripletLoss
    m = TripletLoss() if kind == "tri" else HardestTripletLoss()
    draws = O.fixture_draws(Z, tag, kind)

    def run(how):
        F0, F1, pairs, (num_pos, num_hn, num_rand) = _inputs(tag, dev)
        kw = dict(num_pos=num_pos, num_hn_samples=num_hn, num_rand_triplet=num_rand)
        if how == "draws":
            out = m.triplet_loss(F0, F1, torch.from_numpy(pairs), draws=draws, **kw)
        elif how == "prepared":
            out = m.triplet_loss(F0, F1, None, draws=m.prepare(len(F0), len(F1), pairs, draws=draws, device=dev, **kw))
        else:
            np.random.seed(SEED)
            out = m.triplet_loss(F0, F1, torch.from_numpy(pairs), **kw)
            assert np.random.rand() == float(Z[f"{tag}_{kind}_next"])
        out[0].backward()
        return out, F0, F1
    out, F0, F1 = run("draws")
    assert all(o.dim() == 0 and o.is_cuda for o in out)
    got = {k: v.cpu().numpy() for k, v in m.last.mined().items()}
    names = ("rand_mask",) if kind == "tri" else ("rand_mask", "mask0", "mask1", "D01ind", "D10ind")
    assert set(got) == set(names)
    for k in names:
        assert np.array_equal(got[k].astype(Z[f"{tag}_{kind}_{k}"].dtype), Z[f"{tag}_{kind}_{k}"]), k
    want = Z[f"{tag}_{kind}_values"]
    worst = {"loss": _rel(float(out[0].detach()), want[0]), "pos_dist": _rel(float(out[1]), want[1]), "neg_dist": _rel(float(out[2]), want[2]),
             "gF0": _grad_err(F0, f"{tag}_{kind}_gF0"), "gF1": _grad_err(F1, f"{tag}_{kind}_gF1")}
    _check(tag, kind, worst)
    for how in ("draws", "prepared", "rng"):
        out2, G0, G1 = run(how)
        _same_bits(out, out2)
        assert torch.equal(F0.grad, G0.grad) and torch.equal(F1.grad, G1.grad), how

"""The 'cross_cat' layer of the overlap-attention module on the GPU against the reference's own gcn.py in float64
(tests/golden/predator_cross_cat_ref.npz, written by tests/golden/make_predator_cross_cat_ref_golden.py):

(a) GCN(4, 64, 10, ['cross_cat']), n = 37, m = 23 (head width 16: the training entry points in eval() and train()): both
    outputs at rel-L2 < 1e-4, the project's feature parity bar, and for the loss o0.sum() + (o1 ** 2).sum() the gradient of both
    descriptor inputs and of every parameter at rel-L2 < 1e-4, the bar tests/test_predator_gpu.py holds KPConv's dx / dW to.
    Four of the twelve parameter gradients are ZERO in exact arithmetic -- the key projection's bias (it shifts every score
    of a query alike: the softmax does not see it) and the biases of proj[2], merge and mlp[0] (a per-channel constant ahead
    of mlp[1]'s InstanceNorm) -- and the float64 reference holds rounding noise of relative size 1e-16 there.  A rel-L2
    against noise is not defined, so such a gradient (reference norm below 1e-9 of its layer's weight gradient) is held to
    ||g|| < 1e-4 ||d weight||, the same bar on the layer's own scale.
(b) GCN(4, 256, 10, ['self', 'cross_cat', 'self']), n = 150, m = 130, eval(): head width 64, the MFMA route (asserted), outputs
    at rel-L2 < 1e-4.
A rerun gives equal bits.  KPFCNN with nets = ['self', 'cross_cat', 'self'] on the small pair of tests/golden/predator_small.npz:
eval() is finite and equals the train path to 1e-4, one backward fills every parameter's gradient.

Measured on the MI355X (rel-L2 against float64; in brackets the reference's own float32 CPU run from the fixture):
  (a) eval and train: o0 1.25e-7 [1.47e-7], o1 1.24e-7 [1.53e-7]; gx0 6.7e-8 [7.2e-8], gx1 1.38e-7 [1.68e-7];
      distribute.weight 4.3e-7 [5.8e-7], distribute.bias 5.3e-7 [9.1e-7], proj.1.weight 3.9e-7 [5.1e-7], proj.2.weight 6.8e-7
      [8.0e-7], merge.weight 4.4e-7 [5.5e-7], mlp.0.weight 4.1e-7 [5.0e-7], mlp.3.weight 1.6e-7 [1.8e-7], mlp.3.bias 4.6e-8
      [5.6e-8]; the four zero gradients, ||g|| / ||d weight||: proj.1.bias 1.4e-8, proj.2.bias 2.8e-7, merge.bias 1.2e-9,
      mlp.0.bias 1.5e-9
  (b) o0 1.4e-6 [1.49e-6], o1 1.4e-6 [1.50e-6]
  KPFCNN, train path against eval: feats 5.3e-7, overlap 1.8e-7, saliency 1.6e-7
"""
import os

import numpy as np
import pytest
import torch

from apr_amd import _lib
from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
from apr_amd.predator.models import gcn
from apr_amd.predator.models.architectures import KPFCNN
from helpers import rel_l2

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLD, "predator_cross_cat_ref.npz")))


def _model_a(g, dev):
    m = gcn.GCN(4, 64, 10, ['cross_cat'])
    m.load_state_dict({k[len("a_sd/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("a_sd/")}, strict=True)
    return m.to(dev)


def _inputs_a(g, dev):
    return [torch.from_numpy(g[k]).to(dev) for k in ("a_c0", "a_c1", "a_x0", "a_x1")]


def test_fixture_a_eval(g, dev):
    m = _model_a(g, dev).eval()
    c0, c1, x0, x1 = _inputs_a(g, dev)
    with torch.no_grad():
        o0, o1 = m(c0, c1, x0, x1)
        p0, p1 = m(c0, c1, x0, x1)
    assert m.layers[0].attn.last_route == 'train' and not o0.requires_grad
    assert torch.equal(o0, p0) and torch.equal(o1, p1), "a rerun must give equal bits"
    r0, r1 = rel_l2(o0.cpu(), g["a_o0"]), rel_l2(o1.cpu(), g["a_o1"])
    print(f"(a) eval: o0 {r0:.3g} [{float(g['a_f32/o0']):.3g}]  o1 {r1:.3g} [{float(g['a_f32/o1']):.3g}]")
    assert r0 < BAR and r1 < BAR


def _train_run(m, c0, c1, x0, x1):
    m.zero_grad(set_to_none=True)
    a, b = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
    o0, o1 = m(c0, c1, a, b)
    (o0.sum() + (o1 ** 2).sum()).backward()
    return o0.detach(), o1.detach(), a.grad, b.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


def test_fixture_a_train_with_gradients(g, dev):
    m = _model_a(g, dev).train()
    c0, c1, x0, x1 = _inputs_a(g, dev)
    o0, o1, gx0, gx1, grads = _train_run(m, c0, c1, x0, x1)
    assert m.layers[0].attn.last_route == 'train'
    again = _train_run(m, c0, c1, x0, x1)
    assert torch.equal(o0, again[0]) and torch.equal(o1, again[1]) and torch.equal(gx0, again[2]) and torch.equal(gx1, again[3])
    assert all(torch.equal(grads[k], again[4][k]) for k in grads), "a rerun must give equal bits"
    figures = {"o0": rel_l2(o0.cpu(), g["a_o0"]), "o1": rel_l2(o1.cpu(), g["a_o1"]), "gx0": rel_l2(gx0.cpu(), g["a_gx0"]),
               "gx1": rel_l2(gx1.cpu(), g["a_gx1"])}
    for key, val in figures.items():
        print(f"(a) train: {key} {val:.3g} [{float(g['a_f32/' + key]):.3g}]")
    assert set(grads) == {k[len("a_g/"):] for k in g if k.startswith("a_g/")}
    zero = []
    for k, got in grads.items():
        ref = g["a_g/" + k].astype(np.float64)
        wref = float(np.linalg.norm(g["a_g/" + k.rsplit(".", 1)[0] + ".weight"].astype(np.float64)))
        assert wref > 0 and bool(torch.isfinite(got).all())
        if np.linalg.norm(ref) < 1e-9 * wref:                       # zero in exact arithmetic (module docstring)
            assert k.endswith(".bias")
            zero.append(k)
            figures["g/" + k] = float(got.double().norm()) / wref
            print(f"(a) train: g/{k} ||g|| / ||d weight|| {figures['g/' + k]:.3g} (zero in exact arithmetic)")
        else:
            figures["g/" + k] = rel_l2(got.cpu(), ref)
            print(f"(a) train: g/{k} {figures['g/' + k]:.3g} [{float(g['a_f32/g/' + k]):.3g}]")
    assert sorted(zero) == sorted("layers.0." + k for k in ("attn.proj.1.bias", "attn.proj.2.bias", "attn.merge.bias", "mlp.0.bias"))
    bad = {k: v for k, v in figures.items() if not v < BAR}
    assert not bad, bad


def test_fixture_b_eval_takes_the_mfma_route(g, dev, monkeypatch):
    torch.manual_seed(int(g["b_seed"]))
    m = gcn.GCN(4, 256, 10, ['self', 'cross_cat', 'self']).to(dev).eval()
    c0, c1 = torch.from_numpy(g["b_c0"]).to(dev), torch.from_numpy(g["b_c1"]).to(dev)
    x0, x1 = (torch.from_numpy(g[k].astype(np.float32) / np.float32(1024)).to(dev) for k in ("b_x0q", "b_x1q"))
    lib = _lib.load()
    called = []
    for fname in ("apr_mha_cat_headmajor", "apr_mha_cat_train_forward", "apr_gcn_forward"):
        real = getattr(lib, fname)
        monkeypatch.setattr(lib, fname, lambda *args, _n=fname, _f=real: (called.append(_n), _f(*args))[1], raising=False)
    with torch.no_grad():
        o0, o1 = m(c0, c1, x0, x1)
    assert called == ["apr_mha_cat_headmajor"] * 2 and m.layers[1].attn.last_route == 'mfma', called
    with torch.no_grad():
        p0, p1 = m(c0, c1, x0, x1)
    assert torch.equal(o0, p0) and torch.equal(o1, p1), "a rerun must give equal bits"
    r0, r1 = rel_l2(o0.cpu(), g["b_o0"]), rel_l2(o1.cpu(), g["b_o1"])
    print(f"(b) eval: o0 {r0:.3g} [{float(g['b_f32/o0']):.3g}]  o1 {r1:.3g} [{float(g['b_f32/o1']):.3g}]")
    assert r0 < BAR and r1 < BAR


def test_kpfcnn_with_cross_cat_runs_and_trains(dev):
    small = np.load(os.path.join(GOLD, "predator_small.npz"))
    cfg = kitti_config(nets=['self', 'cross_cat', 'self'])
    np.random.seed(3)
    torch.manual_seed(3)
    model = KPFCNN(cfg).to(dev)
    src, tgt = small["src"], small["tgt"]
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg,
                                  [int(v) for v in small["limits"]])
    model.eval()
    feats, ov, sal = model(batch)
    assert model.gnn.layers[1].attn.last_route == 'mfma'
    assert all(bool(torch.isfinite(t).all()) for t in (feats, ov, sal)) and feats.shape[1] == cfg.final_feats_dim
    model.train()
    tf, tov, tsal = model(batch)
    assert tf.requires_grad and model.gnn.layers[1].attn.last_route == 'train'
    figures = [rel_l2(a.detach().cpu(), b.cpu()) for a, b in ((tf, feats), (tov, ov), (tsal, sal))]
    print("KPFCNN with cross_cat, train path vs eval: feats %.3g  overlap %.3g  saliency %.3g" % tuple(figures))
    assert max(figures) < BAR
    weights = torch.from_numpy(np.random.default_rng(4).standard_normal(tuple(tf.shape)).astype(np.float32)).to(dev)
    ((tf * weights).sum() + tov.sum() + tsal.sum()).backward()
    missing = [n for n, p in model.named_parameters() if p.requires_grad and (p.grad is None or not bool(torch.isfinite(p.grad).all()))]
    assert not missing, missing
    cat = [n for n, p in model.named_parameters() if n.startswith("gnn.layers.1.") and p.grad is not None]
    assert len(cat) == 12

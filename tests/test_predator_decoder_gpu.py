"""KPFCNNDecoder, the symmetric generator of Predator_APR, on the GPU against the fixture the reference itself wrote
(tests/golden/predator_decoder_ref.npz + predator_decoder_ref_features.npz, made by make_predator_decoder_ref_golden.py:
the reference's KPFCNN and KPFCNNDecoder under seeds 0 on tests/predator_loss_fixture.small_pair()), and one symmetric
PredatorPairTrainStep iteration.

Bars.  Output: relative L2 < 1e-4, the bar of the predator_small.npz test.  Gradients (the two stored in full, and the L2
norm of every parameter's): 2e-2, the bar of test_kpfcnn_training_path_gradients (fp32 through ~40 layers of KPConv and
instance norms, GPU vs CPU reductions).  regularization_loss: every generated row has unit length, so each frame's
mean(sum(offset^2)) over its 4 points per row is 1/4 up to rounding; 1e-5 of 0.5 for the two frames.

Measured on an MI355X (records, not thresholds): output 5.5e-6 in train(), 6.4e-6 in eval(); the two full gradients 1.26e-2
and 6.3e-6; the worst of the 38 gradient norms 3.5e-3; the two routes of the first layer give the same output bits;
regularization_loss 0.5.
"""
import os

import numpy as np
import pytest
import torch

from apr_amd.predator import kp_ops
from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
from apr_amd.predator.lib.trainer import PredatorPairTrainStep
from apr_amd.predator.lib.validation import PredatorPairValidStep
from apr_amd.predator.models.architectures import KPFCNN, KPFCNNDecoder
from oracle import predator_points_oracle as PREF
from tests.helpers import rel_l2
from tests.predator_loss_fixture import collated, small_pair, train_config

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LIMITS = [30, 30, 30, 30]
LR, MOMENTUM, WD = 0.01, 0.98, 1e-6                       # as tests/test_predator_iteration_gpu.py
OUT_BAR, GRAD_BAR = 1e-4, 2e-2


def _pair_of_models(cfg, seed):
    """main.py:52-63: KPFCNN with switch_to_decoder = False, then the decoder with it set"""
    np.random.seed(seed)
    torch.manual_seed(seed)
    cfg.symmetric, cfg.switch_to_decoder = True, False
    enc = KPFCNN(cfg)
    cfg.switch_to_decoder = True
    return enc, KPFCNNDecoder(cfg)


@pytest.fixture(scope="module")
def world(dev):
    """the fixture, the reference's parameters (same seeds: pinned by the fixture's key list and weight sum) loaded strictly
    into a decoder built under other seeds, and the pair collated by apr_amd's own collate on the GPU"""
    g = dict(np.load(os.path.join(GOLD, "predator_decoder_ref.npz")))
    g["second_features"] = np.load(os.path.join(GOLD, "predator_decoder_ref_features.npz"))["second_features"]
    cfg = kitti_config()
    _, seeded = _pair_of_models(cfg, 0)
    sd = seeded.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["dec_keys"]]
    wsum = float(sum(v.double().abs().sum() for v in sd.values()))
    assert abs(wsum - float(g["dec_weight_abs_sum"])) <= 1e-9 * wsum, "same seeds must give the reference's parameters"
    _, dec = _pair_of_models(cfg, 5)
    res = dec.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    dec = dec.to(dev)
    src, tgt = g["src"], g["tgt"]
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg,
                                  [int(v) for v in g["limits"]])
    batch["second_features"] = torch.from_numpy(g["second_features"]).to(dev)
    return dict(g=g, cfg=cfg, dec=dec, batch=batch)


def _train_forward(world, dev):
    dec = world["dec"].train()
    dec.zero_grad(set_to_none=True)
    out = dec(world["batch"])
    assert out.requires_grad
    return out


def test_forward_matches_the_reference(world, dev):
    g, dec, batch = world["g"], world["dec"], world["batch"]
    out = _train_forward(world, dev)
    r_train = rel_l2(out.detach().cpu(), g["out"])
    dec.eval()
    out_eval = dec(batch)
    assert not out_eval.requires_grad and tuple(out_eval.shape) == tuple(g["out"].shape)
    r_eval = rel_l2(out_eval.cpu(), g["out"])
    with torch.no_grad():
        r_nograd = rel_l2(dec.train()(batch).cpu(), g["out"])
    print(f"decoder output vs the reference: train {r_train:.3g}  eval {r_eval:.3g}  train under no_grad {r_nograd:.3g}")
    assert r_train < OUT_BAR and r_eval < OUT_BAR and r_nograd < OUT_BAR
    assert float((out_eval.norm(dim=1) - 1).abs().max()) < 1e-5
    assert batch["second_features"].grad is None and not batch["second_features"].requires_grad


def test_gradients_match_the_reference(world, dev):
    g, dec = world["g"], world["dec"]
    out = _train_forward(world, dev)
    (out * torch.from_numpy(g["G"]).to(dev)).sum().backward()
    params = dict(dec.named_parameters())
    without = [n for n, p in params.items() if p.grad is None]
    assert without == ["epsilon"] + [n for n in params if n.endswith("kernel_points")]
    r_first = rel_l2(params["encoder_blocks.0.KPConv.weights"].grad.cpu(), g["grad_first_kpconv"])
    r_last = rel_l2(params["decoder_blocks.5.mlp.weight"].grad.cpu(), g["grad_last_unary"])
    print(f"full gradients: encoder_blocks.0.KPConv.weights {r_first:.3g}  decoder_blocks.5.mlp.weight {r_last:.3g}")
    names = [str(n) for n in g["grad_names"]]
    assert names == [n for n in params if n not in without]
    worst = ("", 0.0)
    for n, ref in zip(names, g["grad_norms"]):
        r = abs(float(params[n].grad.norm()) - float(ref)) / float(ref)
        worst = max(worst, (n, r), key=lambda t: t[1])
    print(f"gradient norms: {len(names)} parameters, worst relative difference {worst[1]:.3g} ({worst[0]})")
    assert r_first < GRAD_BAR and r_last < GRAD_BAR
    assert worst[1] < GRAD_BAR, worst


def test_both_routes_of_the_first_layer_agree(world, dev):
    g, dec, batch = world["g"], world["dec"].eval(), world["batch"]
    saved = kp_ops.KPCONV_C32
    outs = {}
    try:
        for on in (False, True):
            kp_ops.KPCONV_C32 = on
            outs[on] = dec(batch).cpu()
    finally:
        kp_ops.KPCONV_C32 = saved
    r = rel_l2(outs[True], outs[False])
    print(f"apr_kpconv_weighted_c32 vs the generic kernel, decoder output: {r:.3g}; vs the reference "
          f"{rel_l2(outs[True], g['out']):.3g} / {rel_l2(outs[False], g['out']):.3g}")
    assert r < OUT_BAR and rel_l2(outs[True], g["out"]) < OUT_BAR and rel_l2(outs[False], g["out"]) < OUT_BAR


# ------------------------------------------------------------------------------------------------ one iteration
def _iteration(dev, loss_ratio=None):
    """a fresh symmetric step (the builders and the pair of tests/test_predator_iteration_gpu.py), one iteration ->
    everything the checks below read"""
    cfg = train_config()
    if loss_ratio is not None:
        cfg.loss_ratio = loss_ratio
    model, gen = _pair_of_models(cfg, 7)
    model, gen = model.to(dev), gen.to(dev)
    opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=LR, momentum=MOMENTUM,
                          weight_decay=WD)
    step = PredatorPairTrainStep(model, gen, opt, cfg)
    assert step.symmetric
    batch = collated(small_pair(), cfg, LIMITS, dev)
    before = {n: p.detach().clone() for n, p in gen.named_parameters()}
    grads = {}
    opt_step = opt.step

    def spy_step(*a, **k):                                 # the gradients the optimizer is about to consume
        grads.update({"enc." + n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        grads.update({"gen." + n: p.grad.detach().clone() for n, p in gen.named_parameters() if p.grad is not None})
        return opt_step(*a, **k)
    opt.step = spy_step
    np.random.seed(99)
    stats, invalid = step(batch)
    return dict(stats=stats, invalid=invalid, grads=grads, before=before, batch=batch, cfg=cfg,
                gen={n: p.detach().clone() for n, p in gen.named_parameters()},
                enc={n: p.detach().clone() for n, p in model.named_parameters()})


@pytest.fixture(scope="module")
def iteration(dev):
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    return _iteration(dev)


def test_one_symmetric_iteration(iteration):
    it = iteration
    stats = it["stats"]
    assert not it["invalid"] and len(stats) == 10
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    print("stats:", {k: float(v) for k, v in stats.items()})
    assert abs(stats["regularization_loss"] - 0.5) < 1e-5, stats["regularization_loss"]
    assert "second_features" in it["batch"] and tuple(it["batch"]["second_features"].shape)[1] == it["cfg"].final_feats_dim
    still = [n for n in it["gen"] if torch.equal(it["gen"][n], it["before"][n])]
    assert still == ["epsilon"] + [n for n in it["gen"] if n.endswith("kernel_points")], still
    assert not any(k == "gen.epsilon" or k.endswith("kernel_points") for k in it["grads"])


def test_the_generator_sends_nothing_into_the_encoder(iteration, dev):
    """the detach: the encoder's gradients are those of the same iteration with loss_ratio = 0, bit for bit"""
    zero = _iteration(dev, loss_ratio=0.0)
    enc = [k for k in iteration["grads"] if k.startswith("enc.")]
    assert len(enc) > 50 and enc == [k for k in zero["grads"] if k.startswith("enc.")]
    for k in enc:
        assert torch.equal(iteration["grads"][k], zero["grads"][k]), k


def test_two_fresh_runs_give_the_same_bits(iteration, dev):
    again = _iteration(dev)
    for k, v in iteration["stats"].items():
        assert float(v) == float(again["stats"][k]), k
    for part in ("enc", "gen"):
        for n, p in iteration[part].items():
            assert torch.equal(p, again[part][n]), (part, n)
    assert list(iteration["grads"]) == list(again["grads"])
    for k, v in iteration["grads"].items():
        assert torch.equal(v, again["grads"][k]), k


def test_validation_still_refuses_the_symmetric_config(dev):
    """the reference's val branch cannot run (trainer.py:238-239): the config build_models leaves behind is refused"""
    from apr_amd.predator.lib.learned import build_models
    cfg = train_config()
    model, gen, opt, _ = build_models(dev, cfg, seed=7, symmetric=True)
    assert cfg.symmetric and cfg.switch_to_decoder and isinstance(gen, KPFCNNDecoder)
    assert tuple(model.decoder_blocks[5].mlp.weight.shape) == (cfg.final_feats_dim + 2, 320)      # built before the switch
    assert [len(grp["params"]) for grp in opt.param_groups] == [len(list(model.parameters())), len(list(gen.parameters()))]
    with pytest.raises(NotImplementedError):
        PredatorPairValidStep(model, gen, cfg)

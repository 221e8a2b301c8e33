"""One whole Predator_APR training iteration (apr_amd/predator/lib/trainer.py::PredatorPairTrainStep: KPFCNN in train(), the
NPR loss of both frames, MetricLoss, one backward, SGD) on the small pair synth.make_pair(13, 16 x 400), against a chain of
oracles: oracle/kpfcnn_oracle.py's `kpfcnn_forward.__wrapped__` under autograd (as test_kpfcnn_training_path_gradients uses
it: the reference's formulation on the CPU), then tests/predator_loss_oracle.py and the NPR statements in float64.  The HIP
iteration's own arg-maxes, arg-min and `choice` are pinned in the chain.

Bars and where they come from.  Parameter gradients: 2e-2, the bar of the existing whole-network gradient test (fp32
through ~40 layers, GPU vs CPU reductions).  Loss-valued stats: the network's outputs agree with the oracle's to 1e-4
(the bar of that same test); the circle loss multiplies feature distances by log_scale = 16 before exponentials, the BCE
terms take logs of scores: 2e-3 relative.  Count-valued stats are ratios of a few hundred to a few thousand decisions on
features that differ by 1e-4: at most 1 % of the decisions may flip (0.01 absolute).

Measured on an MI355X: the ten stats agree to 5.1e-8, 64 parameter gradients to 1.07e-2 relative L2, c_loss falls
2.162 -> 1.640 over 5 iterations, two fresh runs give identical bits.
"""
import copy

import numpy as np
import pytest
import torch

from apr_amd.predator.lib.trainer import PredatorPairTrainStep
from apr_amd.predator.models.architectures import KPFCNN
from apr_amd.predator.models.mlp import GenerativeMLP_98
from oracle import apr_step_oracle as AO
from oracle import kpfcnn_oracle as KO
from oracle import predator_points_oracle as PREF
from tests import predator_loss_oracle as O
from tests.helpers import rel_l2
from tests.predator_loss_fixture import TRAIN, collated, small_pair, train_config

pytestmark = pytest.mark.gpu

LIMITS = [30, 30, 30, 30]
LR, MOMENTUM, WD = 0.01, 0.98, 1e-6                       # momentum / weight decay: configs/train/kitti.yaml:59-60
BARS = {"loss": 2e-3, "count": 0.01, "grad": 2e-2}
LOSSES = ("circle_loss", "overlap_loss", "saliency_loss", "chamfer_loss", "regularization_loss")
COUNTS = ("recall", "overlap_recall", "overlap_precision", "saliency_recall", "saliency_precision")


def _build(dev, seed=7):
    np.random.seed(seed)
    torch.manual_seed(seed)
    cfg = train_config()
    model = KPFCNN(cfg).to(dev)
    gen = GenerativeMLP_98(in_channel=cfg.final_feats_dim, out_points=cfg.point_generation_ratio, radius=None,
                           bn_momentum=cfg.batch_norm_momentum).to(dev)
    opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=LR, momentum=MOMENTUM,
                          weight_decay=WD)
    step = PredatorPairTrainStep(model, gen, opt, cfg)
    step.desc_loss.keep_intermediates = True
    return cfg, model, gen, opt, step


def _total(stats):
    return stats["circle_loss"] * TRAIN["w_circle_loss"] + stats["overlap_loss"] * TRAIN["w_overlap_loss"] \
        + stats["saliency_loss"] * TRAIN["w_saliency_loss"] \
        + (stats["chamfer_loss"] + stats["regularization_loss"] * TRAIN["regularization_strength"]) * TRAIN["loss_ratio"]


def test_one_iteration_matches_the_oracle_chain(dev):
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    cfg, model, gen, opt, step = _build(dev)
    pair = small_pair()
    batch = collated(pair, cfg, LIMITS, dev)
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    gen0 = copy.deepcopy(gen).cpu().double().train()
    grads = {}
    opt_step = opt.step
    def spy_step(*a, **k):                                 # the gradients the optimizer is about to consume
        grads.update({n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
        grads.update({"gen." + n: p.grad.detach().cpu().clone() for n, p in gen.named_parameters() if p.grad is not None})
        return opt_step(*a, **k)
    opt.step = spy_step
    np.random.seed(99)
    stats, invalid = step(batch)
    assert not invalid and set(stats) == set(LOSSES) | set(COUNTS)
    assert all(isinstance(stats[k], float) for k in LOSSES)
    last = step.desc_loss.last
    ns, nt = int(last["counts"][0]), int(last["counts"][1])

    # ---- the chain
    sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd0.items()}
    f, ov, sal = KO.kpfcnn_forward.__wrapped__(sd, cfg, KO.collate(pair["src"], pair["tgt"], cfg, LIMITS))
    n_src = len(pair["src"])
    d = lambda v: torch.from_numpy(np.asarray(v, np.float64))
    f64, ov64, sal64 = f.double(), ov.double(), sal.double()
    pins = {"row_arg": last["row_arg"][:ns].cpu().long(), "col_arg": last["col_arg"][:nt].cpu().long(),
            "nn": last["nn"].cpu().long()}
    choice = last["choice"].cpu().numpy()
    ref = O.forward(d(pair["src"]), d(pair["tgt"]), f64[:n_src], f64[n_src:], torch.from_numpy(pair["corr"]), d(pair["rot"]),
                    d(pair["trans"]), ov64, sal64, choice=choice, pins=pins)
    mods = [m for block in gen0.list_modules for m in block]
    cham = reg = gl = 0
    for feats, pcd, nghb in ((f64[:n_src], pair["src"], pair["src_nghb"]), (f64[n_src:], pair["tgt"], pair["tgt_nghb"])):
        generated = AO.run_generator(mods, feats)
        r = torch.mean(torch.sum(generated.reshape(-1, 3) ** 2, axis=-1))
        mod = (generated + d(pcd).repeat(1, cfg.point_generation_ratio)).reshape(-1, 3)
        c, _ = AO.chamfer(mod, d(nghb))
        cham, reg, gl = cham + c, reg + r, gl + (c + r * TRAIN["regularization_strength"]) * TRAIN["loss_ratio"]
    ref = dict(ref, chamfer_loss=cham, regularization_loss=reg)
    total = ref["circle_loss"] * TRAIN["w_circle_loss"] + ref["overlap_loss"] * TRAIN["w_overlap_loss"] \
        + ref["saliency_loss"] * TRAIN["w_saliency_loss"] + gl
    total.backward()

    worst = {}
    for k in LOSSES:
        worst[k] = abs(stats[k] - float(ref[k])) / abs(float(ref[k]))
    for k in COUNTS:
        worst[k] = abs(float(stats[k]) - float(ref[k]))
    print("stats (hip, chain):", {k: (float(stats[k]), float(ref[k])) for k in LOSSES + COUNTS})
    print("measured:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in LOSSES:
        assert worst[k] < BARS["loss"], (k, worst[k])
    for k in COUNTS:
        assert worst[k] <= BARS["count"], (k, worst[k])
    checked, gworst = 0, 0.0
    for name, p in model.named_parameters():
        g_ref = sd[name].grad
        if g_ref is None or name not in grads:
            continue
        if float(g_ref.norm()) < 1e-3:                      # analytically zero (biases in front of an instance norm)
            assert float((grads[name] - g_ref).norm()) < 1e-4, name
            continue
        gworst = max(gworst, rel_l2(grads[name], g_ref))
        checked += 1
    for name, p in gen0.named_parameters():
        gworst = max(gworst, rel_l2(grads["gen." + name], p.grad))
        checked += 1
    print(f"parameter gradients: {checked} checked, worst relative L2 {gworst:.2e}")
    assert checked > 50 and gworst < BARS["grad"], (checked, gworst)


def test_loss_falls_and_two_fresh_runs_give_the_same_bits(dev):
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    pair = small_pair()
    runs = []
    for _ in range(2):
        cfg, model, gen, opt, step = _build(dev)
        batch = collated(pair, cfg, LIMITS, dev)
        np.random.seed(5)
        hist = [step(batch)[0] for _ in range(5)]
        runs.append((hist, [p.detach().clone() for p in list(model.parameters()) + list(gen.parameters())]))
    totals = [_total(s) for s in runs[0][0]]
    print("c_loss over 5 iterations:", [f"{v:.4f}" for v in totals])
    assert totals[-1] < totals[0]
    for a, b in zip(runs[0][0], runs[1][0]):
        for k in a:
            assert float(a[k]) == float(b[k]), k
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)

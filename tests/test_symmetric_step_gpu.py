"""Whole SYMMETRIC APR training iterations (GenerativePairTrainStep(symmetric=True): both encodes, hardest-contrastive loss, a
second ResUNetFatBN(128, 12) as generator on the encoder's output tensor -- its 5^3 conv1 over 128 -> 32 channels and that
layer's input gradient back into the encoder --, regulariser, Chamfer, one backward, SGD) against the float64 oracle chain of
tests/symmetric_oracle.py, two iterations per case, with the harness of tests/test_train_iteration_gpu.py: before each
iteration the oracle takes the HIP models' parameters, running statistics and momentum buffers; the ReLU masks of both
networks' fused nodes, the mined hardest negatives and the Chamfer arg-mins are pinned and each checked to be legitimate.

Measured on an MI355X, worst over the three cases and both iterations (relative L2 unless noted), and the bar BARS holds
each to (the measured value times a margin inside the 3.7 - 7x band of tests/test_train_iteration_gpu.py):
  loss terms (pos, neg, each cloud's Chamfer and regulariser, total; relative)     1.84e-7   bar 1e-6    (5.4x)
  dL/dF at the encoder outputs (contrastive + the generator conv1's input gradient) 9.32e-7   bar 5e-6    (5.4x)
  encoder parameter gradients                                                      2.00e-6   bar 1e-5    (5.0x)
  generator parameter gradients (23 more conv units behind the encoder)            5.08e-6   bar 2.5e-5  (4.9x)
  SGD momentum buffers after the step                                              5.08e-6   bar 2.5e-5  (4.9x)
  SGD step of every parameter (beyond one fp32 ulp of the stored value)            5.02e-6   bar 2.5e-5  (5.0x)
  running means / variances, max |hip - ref| / (|ref| + 1e-3 max |ref|)            2.01e-4   bar 1e-3    (5.0x)
  pinned ReLU decisions the float64 sign disagrees with: |z| / layer RMS           1.84e-6   bar 1e-5    (5.4x)
  their count: 1 - 3 in 5.9 M (one pair), 1 - 3 in 10.7 M (two pairs); cap max(4, 1e-5 x watched)
  num_batches_tracked                                                              exact
"""
import numpy as np
import pytest
import torch

from apr_amd.fcgf.lib.complement_trainer import GenerativePairTrainStep
from apr_amd.fcgf.model import load_model
from oracle import apr_step_oracle as AO
from tests import symmetric_oracle as SO
from tests import test_train_iteration_gpu as TI
from tests.helpers import ReluSpy, oracle_copy, rel_l2, stat_err

pytestmark = pytest.mark.gpu

BARS = {"loss": 1e-6, "dF": 5e-6, "grad_enc": 1e-5, "grad_gen": 2.5e-5, "running": 1e-3, "update": 2.5e-5,
        "momentum": 2.5e-5, "flip_z/rms": 1e-5}
assert set(BARS) == set(TI.BARS)
LR, MOMENTUM, WD = TI.LR, TI.MOMENTUM, TI.WD
N_OUT, RATIO = 128, 4

CASES = {"one-pair-stacked": ("one", True), "one-pair-per-call": ("one", False), "two-pairs-stacked": ("two", True)}


def _batch(dev, which):
    return TI._two_pairs(dev, 8, 200) if which == "two" else TI._pair(dev, 3, 8, 200)


def _models(dev, lr=LR):
    torch.manual_seed(0)
    enc = load_model("ResUNetFatBN")(1, N_OUT, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    gen = load_model("ResUNetFatBN")(N_OUT, RATIO * 3, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    opt = torch.optim.SGD([{'params': enc.parameters()}, {'params': gen.parameters()}], lr=lr, momentum=MOMENTUM,
                          weight_decay=WD)
    return enc, gen, opt


def _step(dev, nb, stack, symmetric=True, gen=None):
    enc, g, opt = _models(dev)
    if gen is not None:
        g = gen(dev)
        opt = torch.optim.SGD([{'params': enc.parameters()}, {'params': g.parameters()}], lr=LR, momentum=MOMENTUM,
                              weight_decay=WD)
    kw = {"symmetric": True} if symmetric else {}
    st = GenerativePairTrainStep(enc, g, opt, point_generation_ratio=RATIO, regularization_strength=0.01,
                                 regularization_type="L2", loss_ratio=2e-3, num_pos_per_batch=256,
                                 num_hn_samples_per_batch=128, batch_size=nb, **kw)
    st.stack_frames = stack
    return st


class _Recorder(TI._StepRecorder):
    """The step recorder with the generator's fused nodes and forward_train calls next to the encoder's."""

    def __init__(self, monkeypatch, st):
        super().__init__(monkeypatch, st)
        gen = st.generator_model
        self.names.update({id(m): n for n, m in gen.named_modules()})
        self.gen_calls, self.gen_inputs = [], []
        real = gen.forward_train

        def forward_train(x, frame_rows=None):
            self.gen_calls.append((x.coordinate_manager, len(self.nodes), frame_rows))
            x.F.retain_grad()      # the encoder's output where BOTH losses meet (stacked: the walk's own tensor, whose
            self.gen_inputs.append(x.F)      # per-frame slices feed the contrastive loss)
            return real(x, frame_rows=frame_rows)
        monkeypatch.setattr(gen, "forward_train", forward_train)

    def reset(self):
        super().reset()
        self.gen_calls.clear()
        self.gen_inputs.clear()


def _draws(rng, st, n0, n1, n_pairs):
    sel0 = rng.choice(n0, min(n0, st.num_hn), replace=False)
    sel1 = rng.choice(n1, min(n1, st.num_hn), replace=False)
    pos_sel = rng.choice(n_pairs, st.num_pos, replace=False) if n_pairs > st.num_pos else None
    return sel0, sel1, pos_sel


@pytest.mark.parametrize("case", list(CASES))
def test_symmetric_iteration_matches_fp64_oracle(dev, case, monkeypatch):
    which, stack = CASES[case]
    batch = _batch(dev, which)
    nb = len(batch["len_batch"])
    st = _step(dev, nb, stack)
    enc, gen, opt = st.encoder_model, st.generator_model, st.optimizer
    cfg = AO.StepConfig(voxel_size=st.voxel_size, ratio=RATIO, reg_strength=0.01, reg_type="L2", alpha=st.alpha,
                        loss_ratio=2e-3, neg_weight=st.neg_weight)
    rec = _Recorder(monkeypatch, st)
    coords = [batch["sinput0_C"].cpu().numpy(), batch["sinput1_C"].cpu().numpy()]
    feats = [batch["sinput0_F"].cpu(), batch["sinput1_F"].cpu()]
    clouds = [[c.cpu() for c in batch["pcd_nghb0"]], [c.cpu() for c in batch["pcd_nghb1"]]]
    pairs = batch["correspondences"].numpy()
    n0, n1 = (int(c.shape[0]) for c in coords)
    rng = np.random.default_rng(7)
    hip_named = dict({f"enc.{k}": v for k, v in enc.named_parameters()}, **{f"gen.{k}": v for k, v in gen.named_parameters()})
    worst, fails = {}, []
    spy = ReluSpy(monkeypatch)

    def note(q, v, it):
        worst[q] = max(worst.get(q, 0.0), v)
        if not v <= BARS[q]:
            fails.append((it, q, f"{v:.2e}"))

    for it in range(2):
        om = oracle_copy("ResUNetFatBN", enc.state_dict(), N_OUT)
        og = SO.generator_copy("ResUNetFatBN", gen.state_dict(), N_OUT, RATIO * 3)
        opt_o = AO.make_optimizer(om, og, LR, MOMENTUM, WD)
        o_named = dict({f"enc.{k}": v for k, v in om.named_parameters()}, **{f"gen.{k}": v for k, v in og.named_parameters()})
        assert set(o_named) == set(hip_named)
        for n, p in hip_named.items():
            buf = opt.state.get(p, {}).get("momentum_buffer")
            assert (buf is None) == (it == 0), n
            if buf is not None:
                opt_o.state[o_named[n]]["momentum_buffer"] = buf.detach().cpu().double().clone()
        before = {n: p.detach().cpu().double().clone() for n, p in hip_named.items()}
        draws = _draws(rng, st, n0, n1, len(pairs))

        rec.reset()
        r = st(batch, draws=draws)
        torch.cuda.synchronize()

        # both networks ran as fused nodes: one walk each when stacked (the generator on the encoder's stacked tensor and
        # coordinate manager), one per frame otherwise, generator calls after the encoder's, frame 0 first
        assert len(rec.nodes) == (46 if stack else 92), len(rec.nodes)
        assert len(rec.calls) == len(rec.gen_calls) == (1 if stack else 2)
        assert all(g[0] is e[0] for g, e in zip(rec.gen_calls, rec.calls))      # the encoder's coordinate manager, reused
        assert rec.gen_calls[0][1] == (23 if stack else 46)
        gen_nodes = rec.nodes[rec.gen_calls[0][1]:]
        g1 = gen_nodes[0]
        assert tuple(g1["kernel"].shape) == (125, N_OUT, 32) and g1["x_grad"] and g1["fwd"] == {"tile"} and g1["bwd"] == {"tile"}
        assert rec.nn_batch and not rec.nn

        pos0, pos1, d01, d10 = rec.mined[-1]
        F0h, F1h = (f.detach().cpu().double().numpy() for f in rec.F)
        TI._check_hardest(F0h, F1h, pos0, pos1, draws[0], draws[1], d01, d10)
        cham_pairs = rec.chamfer_pairs()
        assert len(cham_pairs) == 2 * nb
        for s, (a, b, i_ab, i_ba) in enumerate(cham_pairs):
            TI._check_argmin(a, b, i_ab, f"cloud {s} a->b")
            TI._check_argmin(b, a, i_ba, f"cloud {s} b->a")
        pins = AO.Pins(enc=rec.pins(coords), hardest=(d01, d10), chamfer=[(i_ab, i_ba) for _, _, i_ab, i_ba in cham_pairs])
        gen_pins = rec.pins(coords, calls=rec.gen_calls)
        assert len(pins.enc) == len(gen_pins) == 2
        spy.reset()
        ref = SO.step(om, og, opt_o, coords, feats, clouds, pairs, draws, cfg, pins=pins, gen_pins=gen_pins)
        flips, flip_z, watched = spy.summary()
        note("flip_z/rms", flip_z, it)
        if not flips <= max(4, 1e-5 * watched):
            fails.append((it, "mask flips", flips, watched))

        terms = [("pos", r["pos_loss"], ref.pos_loss), ("neg", r["neg_loss"], ref.neg_loss), ("loss", r["loss"], ref.loss)]
        assert len(rec.cham) == len(ref.cham) == len(rec.reg) == len(ref.reg) == 2 * nb
        terms += [(f"cham{s}", h, o) for s, (h, o) in enumerate(zip(rec.cham, ref.cham))]
        terms += [(f"reg{s}", h, o) for s, (h, o) in enumerate(zip(rec.reg, ref.reg))]
        for t, h, o in terms:
            note("loss", abs(float(h) - float(o.detach())) / abs(float(o.detach())), (it, t))
        dF = torch.cat([f.grad for f in rec.gen_inputs], 0).cpu()
        for k, (a, b) in enumerate(((0, n0), (n0, n0 + n1))):
            note("dF", rel_l2(dF[a:b], ref.F[k].grad), (it, k))
        for n, p in hip_named.items():
            assert p.grad is not None and o_named[n].grad is not None, n
            note("grad_gen" if n.startswith("gen.") else "grad_enc", rel_l2(p.grad.cpu(), o_named[n].grad), (it, n))
            note("update", TI._update_err(p, o_named[n], before[n]), (it, n))
            note("momentum", rel_l2(opt.state[p]["momentum_buffer"].cpu(), opt_o.state[o_named[n]]["momentum_buffer"]), (it, n))
        for hs, os_ in ((enc.state_dict(), om.state_dict()), (gen.state_dict(), og.state_dict())):
            for n, v in hs.items():
                if n.endswith("num_batches_tracked"):
                    assert int(v) == int(os_[n]) == 2 * (it + 1), (n, int(v), int(os_[n]))
                elif "running" in n:
                    note("running", stat_err(v, os_[n]), (it, n))
        print(f"[{case} it{it}] flips {flips}/{watched} (worst |z|/rms {flip_z:.1e})")
    print(f"[{case}] worst: " + ", ".join(f"{q} {v:.2e}" for q, v in sorted(worst.items())))
    assert not fails, fails[:20]


def _run(dev, which, stack, symmetric, iters=2, gen=None):
    """`iters` iterations from the seeded models -> (per-iteration loss terms, gradients of the last one, final parameters)."""
    batch = _batch(dev, which)
    st = _step(dev, len(batch["len_batch"]), stack, symmetric=symmetric, gen=gen)
    n0, n1, npairs = batch["sinput0_C"].shape[0], batch["sinput1_C"].shape[0], len(batch["correspondences"])
    rng = np.random.default_rng(7)
    out = []
    for it in range(iters):
        r = st(batch, draws=_draws(rng, st, n0, n1, npairs))
        out.append({k: r[k].clone() for k in ("loss", "pos_loss", "neg_loss")})
    named = dict({f"enc.{k}": v for k, v in st.encoder_model.named_parameters()},
                 **{f"gen.{k}": v for k, v in st.generator_model.named_parameters()})
    stats = dict({f"enc.{k}": v for k, v in st.encoder_model.state_dict().items() if "running" in k},
                 **{f"gen.{k}": v for k, v in st.generator_model.state_dict().items() if "running" in k})
    return out, {n: p.grad.clone() for n, p in named.items()}, {n: p.detach().clone() for n, p in named.items()}, stats


def test_stacked_and_per_call_runs_agree(dev):
    """APR_TRAIN_STACK_FRAMES on / off: the same iteration as one walk per network or one per frame.  Compared directly
    where the iteration is continuous in its inputs -- the loss terms and the running statistics of both networks, at the
    single bar.  The gradients depend on which negatives were mined and which arg-mins the Chamfer searches took, and two
    fp32 runs may decide a tie differently: they are held to the bars through the float64 chain, each run under its own
    pinned decisions (the cases "one-pair-stacked" and "one-pair-per-call" above: same pair, same draws)."""
    (la, _, _, sa), (lb, _, _, sb) = _run(dev, "one", True, True, iters=1), _run(dev, "one", False, True, iters=1)
    for k in la[0]:
        assert abs(float(la[0][k]) - float(lb[0][k])) / abs(float(lb[0][k])) <= BARS["loss"], k
    assert len(sa) == len(sb) == 2 * 2 * 21      # two networks, 21 BatchNorms each, mean and variance
    for n in sa:
        assert stat_err(sa[n], sb[n]) <= BARS["running"], n


def test_mlp_branch_is_untouched(dev, monkeypatch):
    """symmetric=False (passed or left at its default) runs the MLP branch as before: the same bits, loss terms, gradients,
    parameters and running statistics after two iterations, as the step built without the argument, and never enters the
    symmetric code."""
    from apr_amd.fcgf.lib import apg
    mlp = lambda dev: apg.GenerativeMLP_98(in_channel=N_OUT, out_points=RATIO, bn_momentum=0.05).to(dev)
    ref = _run(dev, "one", True, False, gen=mlp)

    def never(*a, **k):
        raise AssertionError("symmetric code on the MLP branch")
    monkeypatch.setattr(GenerativePairTrainStep, "_recon_symmetric", never)
    real = GenerativePairTrainStep.__init__
    monkeypatch.setattr(GenerativePairTrainStep, "__init__", lambda self, *a, **k: real(self, *a, symmetric=False, **k))
    got = _run(dev, "one", True, False, gen=mlp)
    for a, b in zip(ref[0], got[0]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    for a, b in zip(ref[1:], got[1:]):
        assert set(a) == set(b) and all(torch.equal(a[n], b[n]) for n in a)

"""One whole APR training iteration (GenerativePairTrainStep.__call__: both encodes, hardest-contrastive loss, the NPR branch
of both frames -- generator, regulariser, Chamfer -- one backward, SGD) against the float64 oracle chain of the reference's
loop body (oracle/apr_step_oracle.py), two iterations per case.  Before each iteration the oracle takes the HIP model's
parameters, running statistics and momentum buffers in float64, so iteration 2 is judged on weights SGD changed in place
(and on every weight pack rebuilt from them).

Every data-dependent decision the HIP iteration took is recorded and pinned in the oracle: the encoder's ReLU masks per
fused node (matched by coordinates, split per frame for the stacked encode), the generator's ReLU masks, the mined hardest
negatives and the Chamfer arg-mins.  Each decision is checked to be legitimate: where a float64 pre-activation disagrees
with the HIP mask it is within fp32 noise of 0; every arg-min is a float64 arg-min up to fp32 rounding of the distances.

Measured on an MI355X, worst over the six cases and both iterations (relative L2 unless noted; BARS holds each bar, 3.7 - 7x
its measured value):
  loss terms (pos, neg, each cloud's Chamfer and regulariser, total; relative)   6.8e-7
  dL/dF0, dL/dF1 at the encoder outputs                                          1.2e-6   (FatBN)
  encoder parameter gradients (all 23 kernels, final.bias, BatchNorm gamma/beta)  3.8e-6   (FatBN)
  generator parameter gradients                                                  1.4e-5   (GenerativeMLP_98)
  SGD momentum buffers after the step                                            1.1e-5
  SGD step of every parameter (beyond one fp32 ulp of the stored value)          1.1e-5
  running means / variances, max |hip - ref| / (|ref| + 1e-3 max |ref|)          1.1e-4
  num_batches_tracked                                                            exact
Pinned decisions where the float64 sign disagrees with the HIP mask: encoder 0 - 2 in 4.9 M (BN2C-32), 2 - 7 in 24 M
(FatBN-128); generator 0 - 1 in the GenerativeMLP_54 cases, 3 - 6 in 26 M (GenerativeMLP_98); all of them within 1.3e-6 of
their layer's RMS of 0.  Every Chamfer arg-min and every mined hardest negative is a float64 arg-min up to fp32 rounding.
"""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from apr_amd import npr, ops, synth
from apr_amd.fcgf.lib import apg
from apr_amd.fcgf.lib.complement_trainer import GenerativePairTrainStep
from apr_amd.fcgf.model import load_model
from apr_amd.predator import kp_ops
from oracle import apr_step_oracle as AO
from tests.helpers import EncoderRecorder, ReluSpy, oracle_copy, rel_l2, stat_err

pytestmark = pytest.mark.gpu

BARS = {"loss": 5e-6, "dF": 6e-6, "grad_enc": 2e-5, "grad_gen": 6e-5, "running": 4e-4, "update": 5e-5,
        "momentum": 5e-5, "flip_z/rms": 1e-5}

LR, MOMENTUM, WD = 0.05, 0.8, 1e-4


def _pair(dev, seed, beams, azimuth):
    """input_dict of one pair with a stand-in APG cloud per frame (the frame's own voxel points jittered and doubled) and
    the GT correspondences within 1.5 voxels (as tests/test_train_step_gpu.py builds it)."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    out, pts = {}, []
    rng = np.random.default_rng(seed)
    for tag, xyz in (("0", xyz0), ("1", xyz1)):
        key = torch.from_numpy(xyz).to(dev)
        m = ops.build_map(ops.voxelize(key, 0.3, 0), want_first=True)
        ops.finalize_maps([m])
        out[f"sinput{tag}_C"] = m.coords
        out[f"sinput{tag}_F"] = torch.ones((m.n, 1), device=dev)
        p = key[m.first.long()].contiguous()
        pts.append(p)
        jit = torch.from_numpy(rng.normal(0, 0.1, (2 * m.n, 3)).astype(np.float32)).to(dev)
        out[f"pcd_nghb{tag}"] = [(p.repeat(2, 1) + jit).contiguous()]
    out["correspondences"] = apg.get_matching_indices(pts[0], pts[1], torch.from_numpy(T).float().to(dev), 0.45).cpu()
    out["len_batch"] = [[int(out["sinput0_C"].shape[0]), int(out["sinput1_C"].shape[0])]]
    return out


def _two_pairs(dev, beams, azimuth):
    """batch_size 2: each frame tensor holds two clouds, correspondences carry the collate's row offsets."""
    b0, b1 = _pair(dev, 3, beams, azimuth), _pair(dev, 5, beams, azimuth)
    shift = lambda C, k: torch.cat((C[:, :1] + k, C[:, 1:]), 1)
    batch = {}
    for tag in ("0", "1"):
        batch[f"sinput{tag}_C"] = torch.cat((b0[f"sinput{tag}_C"], shift(b1[f"sinput{tag}_C"], 1)), 0).contiguous()
        batch[f"sinput{tag}_F"] = torch.cat((b0[f"sinput{tag}_F"], b1[f"sinput{tag}_F"]), 0)
        batch[f"pcd_nghb{tag}"] = b0[f"pcd_nghb{tag}"] + b1[f"pcd_nghb{tag}"]
    off = torch.tensor([[b0["sinput0_C"].shape[0], b0["sinput1_C"].shape[0]]])
    batch["correspondences"] = torch.cat((b0["correspondences"], b1["correspondences"] + off), 0)
    batch["len_batch"] = b0["len_batch"] + b1["len_batch"]
    return batch


# case: (encoder, features, generator, pairs as (seed, beams, azimuth) or "two", stack_frames, regulariser,
#        routes that must run in backward, a launch that must run)
CASES = {
    "a-BN2C-stacked": ("ResUNetBN2C", 32, apg.GenerativeMLP_54, (3, 16, 600), True, "L2", {"ws3", "tile"}, None),
    "b-BN2C-per-call": ("ResUNetBN2C", 32, apg.GenerativeMLP_54, (3, 16, 600), False, "L2", {"ws3", "tile"}, None),
    # stacked rows >= 32768 (the dense-rows threshold): conv1_tr and final on apr_dense_rows_bf3
    "c-FatBN-stacked": ("ResUNetFatBN", 128, apg.GenerativeMLP_98, (3, 64, 2400), True, "L2", {"ws3", "ws", "tile"},
                        "apr_dense_rows_bf3"),
    "d-BN2C-two-pairs": ("ResUNetBN2C", 32, apg.GenerativeMLP_54, "two", True, "L2", {"ws3", "tile"}, None),
    "e-BN2C-RepelL2": ("ResUNetBN2C", 32, apg.GenerativeMLP_54, (3, 16, 600), True, "RepelL2", {"ws3", "tile"}, None),
    "e-BN2C-RepelL1": ("ResUNetBN2C", 32, apg.GenerativeMLP_54, (3, 16, 600), True, "RepelL1", {"ws3", "tile"}, None),
}


class _StepRecorder(EncoderRecorder):
    """EncoderRecorder plus the rest of the iteration's decisions and per-term values."""

    def __init__(self, monkeypatch, st):
        super().__init__(monkeypatch, st.encoder_model)
        self.gen_masks, self.nn_batch, self.nn, self.mined, self.F, self.cham, self.reg = [], [], [], [], [], [], []
        rec = self
        base = kp_ops.LinearReluFunction

        class LinearRelu(base):
            @staticmethod
            def forward(ctx, x, weight, wp_info, bias):
                y = base.forward(ctx, x, weight, wp_info, bias)
                rec.gen_masks.append((y > 0).cpu())
                return y
        monkeypatch.setattr(kp_ops, "LinearReluFunction", LinearRelu)
        nn3_batch, nn3 = npr.nn3_batch, npr.nn3

        def rec_nn3_batch(a, ao, b, bo, *args, **kw):
            out = nn3_batch(a, ao, b, bo, *args, **kw)
            rec.nn_batch.append((a.detach().cpu(), list(ao), b.detach().cpu(), list(bo), out[0].cpu()))
            return out

        def rec_nn3(a, b, *args, **kw):
            out = nn3(a, b, *args, **kw)
            rec.nn.append((a.detach().cpu(), b.detach().cpu(), out[0].cpu()))
            return out
        monkeypatch.setattr(npr, "nn3_batch", rec_nn3_batch)
        monkeypatch.setattr(npr, "nn3", rec_nn3)
        mine = st.crit._mine_and_reduce

        def rec_mine(F0, F1, pd, mine_only):
            res = mine(F0, F1, pd, mine_only)
            if mine_only:
                rec.mined.append(tuple(t.cpu().numpy() for t in res[:4]))
            return res
        monkeypatch.setattr(st.crit, "_mine_and_reduce", rec_mine)
        loss = st.crit.contrastive_hardest_negative_loss

        def rec_loss(F0, F1, *args, **kw):
            F0.retain_grad()
            F1.retain_grad()
            rec.F[:] = [F0, F1]
            return loss(F0, F1, *args, **kw)
        monkeypatch.setattr(st.crit, "contrastive_hardest_negative_loss", rec_loss)
        cdb, cd, reg = npr.chamfer_distance_batch, npr.chamfer_distance, apg.npr_regulariser

        def rec_cdb(*args):
            out = cdb(*args)
            rec.cham.extend(out.detach().cpu().double().unbind(0))
            return out

        def rec_cd(*args):
            out = cd(*args)
            rec.cham.append(out.detach().cpu().double())
            return out

        def rec_reg(*args):
            out = reg(*args)
            rec.reg.append(out.detach().cpu().double())
            return out
        monkeypatch.setattr(npr, "chamfer_distance_batch", rec_cdb)
        monkeypatch.setattr(npr, "chamfer_distance", rec_cd)
        monkeypatch.setattr(apg, "npr_regulariser", rec_reg)

    def reset(self):
        for lst in (self.nodes, self.calls, self.gen_masks, self.nn_batch, self.nn, self.mined, self.cham, self.reg,
                    self.proxy.log):
            lst.clear()

    def chamfer_pairs(self):
        """Per cloud, in call order: (generated points, cloud points, i_ab, i_ba), local indices, HIP fp32 inputs."""
        out = []
        if self.nn_batch:
            assert len(self.nn_batch) == 2 and not self.nn
            (a, ao, b, bo, i_ab), (b2, bo2, a2, ao2, i_ba) = self.nn_batch
            assert ao == ao2 and bo == bo2 and torch.equal(a, a2) and torch.equal(b, b2)
            for s in range(len(ao) - 1):
                out.append((a[ao[s]:ao[s + 1]], b[bo[s]:bo[s + 1]], (i_ab[ao[s]:ao[s + 1]] - bo[s]).numpy(),
                            (i_ba[bo[s]:bo[s + 1]] - ao[s]).numpy()))
        else:
            assert len(self.nn) % 2 == 0
            for (a, b, i_ab), (b2, a2, i_ba) in zip(self.nn[0::2], self.nn[1::2]):
                assert torch.equal(a, a2) and torch.equal(b, b2)
                out.append((a, b, i_ab.numpy(), i_ba.numpy()))
        return out

    def generator_pins(self, offs):
        """Per cloud (global row offsets `offs`): the masks of the generator's three ReLUs."""
        assert len(self.gen_masks) % 3 == 0 and self.gen_masks
        layers = [torch.cat(self.gen_masks[k::3], 0) for k in range(3)]
        assert all(m.shape[0] == offs[-1] for m in layers), ([m.shape for m in layers], offs[-1])
        return [[m[a:b] for m in layers] for a, b in zip(offs[:-1], offs[1:])]


def _update_err(hip, ref, before):
    """The SGD step of one parameter: |hip - ref| beyond one float32 ulp of the stored parameter (the HIP parameter is
    fp32), relative to the float64 step's size."""
    h = hip.detach().cpu()
    ulp = (torch.nextafter(h, torch.full_like(h, float("inf"))) - h).double()
    excess = ((h.double() - ref.detach()).abs() - ulp).clamp_min(0)
    return float(excess.norm() / (ref.detach() - before).norm().clamp_min(1e-30))


def _check_argmin(a, b, idx, tag):
    """idx[i] is a float64 arg-min of |a_i - b_j|^2 over j, up to fp32 rounding of the distances (a, b: the fp32 points the
    HIP search saw)."""
    a64, b64 = a.double().numpy(), b.double().numpy()
    dmin = cKDTree(b64).query(a64)[0] ** 2
    d = ((a64 - b64[idx]) ** 2).sum(1)
    bad = d > dmin * (1 + 1e-6) + 1e-12
    assert not bad.any(), (tag, int(bad.sum()), float((d - dmin).max()))
    return int((d > dmin * (1 + 1e-12)).sum())


def _check_hardest(F0, F1, pos0, pos1, sel0, sel1, d01, d10):
    """The mined negatives are float64 arg-mins over the sampled rows up to fp32 rounding (HIP features, unit rows)."""
    for P, S, F, ind in ((F0[pos0], sel1, F1, d01), (F1[pos1], sel0, F0, d10)):
        D = ((P[:, None, :] - F[S][None, :, :]) ** 2).sum(-1)
        d = ((P - F[ind]) ** 2).sum(-1)
        assert (d <= D.min(1) + 1e-5).all(), float((d - D.min(1)).max())
        assert np.isin(ind, S).all()


@pytest.mark.parametrize("case", list(CASES))
def test_train_iteration_matches_fp64_oracle(dev, case, monkeypatch):
    enc_name, out_ch, gen_cls, pair, stack, reg_type, need_bwd, need_launch = CASES[case]
    batch = _two_pairs(dev, 16, 600) if pair == "two" else _pair(dev, *pair)
    nb = len(batch["len_batch"])
    torch.manual_seed(0)
    enc = load_model(enc_name)(1, out_ch, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    gen = gen_cls(in_channel=out_ch, out_points=4, bn_momentum=0.05).to(dev)
    opt = torch.optim.SGD([{'params': enc.parameters()}, {'params': gen.parameters()}], lr=LR, momentum=MOMENTUM,
                          weight_decay=WD)
    st = GenerativePairTrainStep(enc, gen, opt, point_generation_ratio=4, regularization_strength=0.1,
                                 regularization_type=reg_type, loss_ratio=2e-3, num_pos_per_batch=256,
                                 num_hn_samples_per_batch=128, batch_size=nb)
    st.stack_frames = stack
    cfg = AO.StepConfig(voxel_size=st.voxel_size, ratio=4, reg_strength=0.1, reg_type=reg_type, alpha=st.alpha,
                        loss_ratio=2e-3, neg_weight=st.neg_weight)
    rec = _StepRecorder(monkeypatch, st)
    coords = [batch["sinput0_C"].cpu().numpy(), batch["sinput1_C"].cpu().numpy()]
    feats = [batch["sinput0_F"].cpu(), batch["sinput1_F"].cpu()]
    clouds = [[c.cpu() for c in batch["pcd_nghb0"]], [c.cpu() for c in batch["pcd_nghb1"]]]
    pairs = batch["correspondences"].numpy()
    offs = [0]
    for k in range(2):
        for r in batch["len_batch"]:
            offs.append(offs[-1] + int(r[k]))
    n0, n1 = (int(c.shape[0]) for c in coords)
    if need_launch == "apr_dense_rows_bf3":
        assert n0 + n1 >= 32768 and n0 < 32768 and n1 < 32768, (n0, n1)
    rng = np.random.default_rng(7)
    enc_named = dict(enc.named_parameters())
    hip_named = dict(enc_named, **{f"mlp.{k}": v for k, v in gen.mlp.named_parameters()})
    worst, fails = {}, []
    spy = ReluSpy(monkeypatch)

    def note(q, v, it):
        worst[q] = max(worst.get(q, 0.0), v)
        if not v <= BARS[q]:
            fails.append((it, q, f"{v:.2e}"))

    for it in range(2):
        # the oracle starts from the HIP model's state: parameters, running statistics, momentum buffers
        om = oracle_copy(enc_name, enc.state_dict(), out_ch)
        mlp = AO.generator_copy(gen.mlp).train()
        opt_o = AO.make_optimizer(om, mlp, LR, MOMENTUM, WD)
        o_named = dict(om.named_parameters(), **{f"mlp.{k}": v for k, v in mlp.named_parameters()})
        for n, p in hip_named.items():
            buf = opt.state.get(p, {}).get("momentum_buffer")
            assert (buf is None) == (it == 0), n
            if buf is not None:
                opt_o.state[o_named[n]]["momentum_buffer"] = buf.detach().cpu().double().clone()
        before = {n: p.detach().cpu().double().clone() for n, p in hip_named.items()}
        sel0 = rng.choice(n0, min(n0, st.num_hn), replace=False)
        sel1 = rng.choice(n1, min(n1, st.num_hn), replace=False)
        pos_sel = rng.choice(len(pairs), st.num_pos, replace=False) if len(pairs) > st.num_pos else None
        draws = (sel0, sel1, pos_sel)

        rec.reset()
        r = st(batch, draws=draws)
        torch.cuda.synchronize()

        # routes of this iteration's encoder (forward and backward) and the number of fused nodes
        assert len(rec.nodes) == (23 if stack else 46), len(rec.nodes)
        fwd, bwd = rec.routes()
        assert need_bwd <= bwd, (need_bwd, bwd)
        assert "tile" in fwd or "ws3" in fwd, fwd
        if need_launch is not None:
            assert need_launch in rec.proxy.log
        if stack:
            assert rec.nn_batch and not rec.nn
        else:
            assert rec.nn and not rec.nn_batch

        # pins, each checked to be a legitimate decision
        pos0, pos1, d01, d10 = rec.mined[-1]
        F0h, F1h = (f.detach().cpu().double().numpy() for f in rec.F)
        _check_hardest(F0h, F1h, pos0, pos1, sel0, sel1, d01, d10)
        cham_pairs = rec.chamfer_pairs()
        assert len(cham_pairs) == 2 * nb
        inexact = 0
        for s, (a, b, i_ab, i_ba) in enumerate(cham_pairs):
            inexact += _check_argmin(a, b, i_ab, f"cloud {s} a->b") + _check_argmin(b, a, i_ba, f"cloud {s} b->a")
        pins = AO.Pins(enc=rec.pins(coords), gen=rec.generator_pins(offs), hardest=(d01, d10),
                       chamfer=[(i_ab, i_ba) for _, _, i_ab, i_ba in cham_pairs])
        spy.reset()
        ref = AO.step(om, mlp, opt_o, coords, feats, clouds, pairs, draws, cfg, pins=pins)
        flips, flip_z, watched = spy.summary()
        gflips, gworst, gwatched = 0, 0.0, 0
        for pre, masks in zip(ref.pre_relu, pins.gen):
            for z, m in zip(pre, masks):
                bad = (z > 0) != m
                gflips += int(bad.sum())
                gwatched += bad.numel()
                if bad.any():
                    gworst = max(gworst, float(z[bad].abs().max() / z.pow(2).mean().sqrt()))
        note("flip_z/rms", max(flip_z, gworst), it)
        if not (flips <= max(4, 1e-5 * watched) and gflips <= max(4, 1e-5 * gwatched)):
            fails.append((it, "mask flips", flips, watched, gflips, gwatched))

        # values
        terms = [("pos", r["pos_loss"], ref.pos_loss), ("neg", r["neg_loss"], ref.neg_loss), ("loss", r["loss"], ref.loss)]
        assert len(rec.cham) == len(ref.cham) == len(rec.reg) == len(ref.reg) == 2 * nb
        terms += [(f"cham{s}", h, o) for s, (h, o) in enumerate(zip(rec.cham, ref.cham))]
        terms += [(f"reg{s}", h, o) for s, (h, o) in enumerate(zip(rec.reg, ref.reg))]
        for t, h, o in terms:
            o = float(o)
            note("loss", abs(float(h) - o) / abs(o), (it, t))
        for k in range(2):
            note("dF", rel_l2(rec.F[k].grad.cpu(), ref.F[k].grad), (it, k))
        for n, p in hip_named.items():
            assert p.grad is not None and o_named[n].grad is not None, n
            note("grad_gen" if n.startswith("mlp.") else "grad_enc", rel_l2(p.grad.cpu(), o_named[n].grad), (it, n))
            note("update", _update_err(p, o_named[n], before[n]), (it, n))
            note("momentum", rel_l2(opt.state[p]["momentum_buffer"].cpu(), opt_o.state[o_named[n]]["momentum_buffer"]),
                 (it, n))
        for hs, os_ in ((enc.state_dict(), om.state_dict()), (gen.mlp.state_dict(), mlp.state_dict())):
            for n, v in hs.items():
                if n.endswith("num_batches_tracked"):
                    assert int(v) == int(os_[n]), (n, int(v), int(os_[n]))
                elif "running" in n:
                    note("running", stat_err(v, os_[n]), (it, n))
        nbt = int(enc.state_dict()["norm1.bn.num_batches_tracked"])
        assert nbt == 2 * (it + 1), nbt
        assert int(gen.mlp.state_dict()["2.num_batches_tracked"]) == 2 * nb * (it + 1)
        print(f"[{case} it{it}] enc flips {flips}/{watched}, gen flips {gflips}/{gwatched}, chamfer arg-mins within fp32 rounding of the fp64 one but not it {inexact}, routes fwd {sorted(fwd)} "
              f"bwd {sorted(bwd)}")
    print(f"[{case}] worst: " + ", ".join(f"{q} {v:.2e}" for q, v in sorted(worst.items())))
    assert not fails, fails[:20]

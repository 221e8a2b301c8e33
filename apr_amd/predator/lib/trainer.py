"""Predator_APR's training iteration on the HIP kernels: the NPR reconstruction loss and `PredatorPairTrainStep`.

Mirrors /root/reference/Predator_APR/lib/trainer.py: `chamfer_distance` (:131-140) and, per frame, the statements
:175-183 / :199-207 of `Trainer.inference_one_batch` -- offsets from the generative model, mean-of-squares
regulariser, `generated + pcd.repeat(1, ratio)` reshaped to points, Chamfer distance to the aggregated neighbour
cloud, `(chamfer + regulariser * strength) * loss_ratio`.  Differentiable end to end (apr_amd/npr.py); the circle /
overlap / saliency losses of the descriptor branch are in lib/loss.py (`MetricLoss`, on HIP kernels as well).

`PredatorPairTrainStep` is the train branch of `inference_one_batch` (:147-221), for the MLP generator and -- with
`config.symmetric` -- for the symmetric one (a KPFCNNDecoder on the encoder's descriptors, :160-164), plus the
optimizer step and `zero_grad` of `inference_one_epoch` (:316-322): KPFCNN forward in train(), the NPR loss of both
frames, MetricLoss, `circle * w_circle + overlap * w_overlap + saliency * w_saliency + generative_loss`, backward unless a
Chamfer value is NaN.  The epoch loop, loader, logging and checkpoints around it stay the reference's own host code.
"""
import numpy as np
import torch

from ... import npr
from .loss import MetricLoss


def chamfer_distance(array1, array2):
    """forward_cd / n1 + backward_cd / n2 (lib/trainer.py:131-140)."""
    return npr.chamfer_distance(array1, array2)


def npr_frame_loss(generative_model, feats, pcd, nghb, point_generation_ratio, regularization_strength, loss_ratio):
    """One frame's share of `generative_loss` (lib/trainer.py:175-183): returns (loss, chamfer_loss_raw, regularize_loss,
    mod_generated)."""
    generated = generative_model(feats)
    if isinstance(generated, tuple):          # a model built with a radius returns (x, radius): models/mlp.py:140-143
        generated = generated[0]
    return npr_generated_loss(generated, pcd, nghb, point_generation_ratio, regularization_strength, loss_ratio)


def npr_generated_loss(generated, pcd, nghb, point_generation_ratio, regularization_strength, loss_ratio):
    """`npr_frame_loss` from ready `generated` rows [n, ratio * 3] (lib/trainer.py:176-183): the symmetric generator makes
    both frames' rows in one call."""
    regularize_loss = torch.mean(torch.sum((generated.reshape(-1, 3)) ** 2, axis=-1))
    mod_generated = (generated + pcd.to(generated.device).repeat(1, point_generation_ratio)).reshape(-1, 3)
    chamfer_loss_raw = chamfer_distance(mod_generated, nghb)
    loss = (chamfer_loss_raw + regularize_loss * regularization_strength) * loss_ratio
    return loss, chamfer_loss_raw, regularize_loss, mod_generated


def npr_loss(generative_model, src_feats, tgt_feats, src_pcd, tgt_pcd, src_nghb, tgt_nghb, point_generation_ratio,
             regularization_strength, loss_ratio):
    """Both frames (lib/trainer.py:166-211): -> dict(generative_loss, chamfer_loss, regularization_loss, invalid)."""
    l0, c0, r0, _ = npr_frame_loss(generative_model, src_feats, src_pcd, src_nghb, point_generation_ratio,
                                   regularization_strength, loss_ratio)
    l1, c1, r1, _ = npr_frame_loss(generative_model, tgt_feats, tgt_pcd, tgt_nghb, point_generation_ratio,
                                   regularization_strength, loss_ratio)
    return {"generative_loss": l0 + l1, "chamfer_loss": c0 + c1, "regularization_loss": r0 + r1,
            "invalid": bool(torch.isnan(c0) or torch.isnan(c1))}


class PredatorPairTrainStep:
    """One training iteration on one collated pair (`collate_fn_descriptor` output with the keys rot, trans,
    correspondences, src_pcd_raw, tgt_pcd_raw, src_nghb, tgt_nghb).  -> (stats, invalid_flag): the reference's ten keys
    (the eight of MetricLoss, chamfer_loss, regularization_loss), the five loss terms as Python floats (:274-278), the
    metrics as 0-d device tensors.

    One host round trip per iteration: the count of filtered correspondences (for the draw of loss.py:157) and the two
    Chamfer NaN flags (:186, :209) come back in ONE 12-byte fetch, so the NaN test adds no synchronisation to the one
    MetricLoss already has; the loss itself then runs with `choice` given and does not synchronise.  The closing
    `float()` conversions are the reference's own (:274-278).  `validate_gradient` (:317) is a per-parameter host loop in
    the reference; here it is one fused device reduction, opt-in (`validate_gradient=True`), because it synchronises."""

    def __init__(self, model, generative_model, optimizer, config, validate_gradient=False):
        self.model, self.generative_model, self.optimizer = model, generative_model, optimizer
        self.desc_loss = MetricLoss(config)
        self.w_circle_loss, self.w_overlap_loss = config.w_circle_loss, config.w_overlap_loss
        self.w_saliency_loss = config.w_saliency_loss
        self.point_generation_ratio = config.point_generation_ratio
        self.regularization_strength, self.loss_ratio = config.regularization_strength, config.loss_ratio
        self.validate_gradient = validate_gradient
        # :160-164: `generative_model` is a KPFCNNDecoder fed the whole batch dict with the encoder's descriptors in it
        self.symmetric = bool(getattr(config, "symmetric", False))

    def __call__(self, inputs):
        self.model.train()
        self.generative_model.train()
        feats, scores_overlap, scores_saliency = self.model(inputs)
        dev = feats.device
        on = lambda v, dt=torch.float32: torch.as_tensor(v).to(dev, dt).contiguous()
        len_src = int(inputs['stack_lengths'][0][0])
        rot, trans = on(inputs['rot']), on(inputs['trans']).reshape(3, 1)
        corr = on(inputs['correspondences'], torch.int64)
        src_pcd, tgt_pcd = on(inputs['src_pcd_raw']), on(inputs['tgt_pcd_raw'])
        src_feats, tgt_feats = feats[:len_src], feats[len_src:]

        if self.symmetric:                        # :160-164: one generator call for the stacked pair, split at len_src
            inputs['second_features'] = feats     # written into the caller's dict, as the reference does
            generated = self.generative_model(inputs)
            l0, c0, r0, _ = npr_generated_loss(generated[:len_src], src_pcd, on(inputs['src_nghb']),
                                               self.point_generation_ratio, self.regularization_strength, self.loss_ratio)
            l1, c1, r1, _ = npr_generated_loss(generated[len_src:], tgt_pcd, on(inputs['tgt_nghb']),
                                               self.point_generation_ratio, self.regularization_strength, self.loss_ratio)
        else:
            l0, c0, r0, _ = npr_frame_loss(self.generative_model, src_feats, src_pcd, on(inputs['src_nghb']),
                                           self.point_generation_ratio, self.regularization_strength, self.loss_ratio)
            l1, c1, r1, _ = npr_frame_loss(self.generative_model, tgt_feats, tgt_pcd, on(inputs['tgt_nghb']),
                                           self.point_generation_ratio, self.regularization_strength, self.loss_ratio)
        generative_loss, chamfer_loss, regularization_loss = l0 + l1, c0 + c1, r0 + r1

        _, count = self.desc_loss.select(src_pcd, tgt_pcd, corr, rot, trans)
        host = torch.stack((count[0].to(torch.float32), torch.isnan(c0.detach()).float(),
                            torch.isnan(c1.detach()).float())).cpu()               # the iteration's one fetch
        invalid_flag = bool(host[1] > 0 or host[2] > 0)
        choice = torch.from_numpy(np.ascontiguousarray(self.desc_loss.draw_choice(int(host[0])), dtype=np.int64)).to(dev)
        stats = self.desc_loss(src_pcd, tgt_pcd, src_feats, tgt_feats, corr, rot, trans, scores_overlap, scores_saliency,
                               choice=choice)
        c_loss = stats['circle_loss'] * self.w_circle_loss + stats['overlap_loss'] * self.w_overlap_loss \
            + stats['saliency_loss'] * self.w_saliency_loss
        c_loss = c_loss + generative_loss
        if not invalid_flag:                      # :220-221; an invalid pair raises in the epoch loop: no step (:311-312)
            c_loss.backward()
            ok = True
            if self.validate_gradient:
                grads = [p.grad for g in self.optimizer.param_groups for p in g['params'] if p.grad is not None]
                ok = bool(torch.isfinite(torch.stack([g.abs().max() for g in grads])).all())
            if ok:
                self.optimizer.step()
            self.optimizer.zero_grad()
        stats = dict(stats)
        for k in ('circle_loss', 'overlap_loss', 'saliency_loss'):
            stats[k] = float(stats[k].detach())
        stats['chamfer_loss'] = float(chamfer_loss.detach())
        stats['regularization_loss'] = float(regularization_loss.detach())
        return stats, invalid_flag

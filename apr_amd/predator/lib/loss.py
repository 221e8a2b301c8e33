"""Predator_APR's descriptor loss on the HIP kernels (csrc/metric_loss.hip).

Mirrors `MetricLoss`, Predator_APR/lib/loss.py:16-178: the circle loss and feature-match recall on at most `max_points`
filtered correspondences, the weighted BCE of the overlap scores against labels made from the correspondences, and
the weighted BCE of the saliency scores, in the overlap region, against labels made from the mutual arg-max of the
feature inner products.  The same eight `stats` keys come back.

Deviations from the reference, all listed in INTEGRATION.md:
  * the unique index lists of :114-115 are ascending (Python's `set` order is unspecified; only the order in which the
    saliency BCE terms are summed depends on it);
  * arg-max / arg-min ties go to the lowest index;
  * the five metrics are 0-d device tensors (`float()` works on them), not Python / NumPy scalars: no host round trip;
  * `forward` takes one more keyword, `choice`.  None: the count of filtered correspondences is fetched once (4 bytes)
    and, above `max_points`, `np.random.permutation(count)[:max_points]` is drawn exactly as :157, so the global NumPy
    stream ends where the reference's does.  An int64 GPU tensor: the anchors are `filtered[choice]`, entries outside
    the filtered list are absent anchors, and the call does not synchronise at all (`torch.arange(max_points)` keeps
    every correspondence of a short list, as the reference does).

GPU tensors only: there is no CPU fallback.
"""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ..._lib import AprHipError


class WeightedBCEFunction(torch.autograd.Function):
    """get_weighted_bce_loss (:79-97) -> f32 [8]: loss, w_negative, precision, recall, tp, fp, fn, n.  Only element 0 is
    differentiable.  `pred` is `scores` itself, or its entries at `pos` (the gather of :142-144), `n_dev` of them."""

    @staticmethod
    def forward(ctx, scores, pred, gt, n_dev, pos):
        pred = scores if pred is None else pred
        out = ops.weighted_bce(pred, gt, n_dev)
        ctx.save_for_backward(pred, gt, out)
        ctx.n_dev, ctx.pos, ctx.shape = n_dev, pos, scores.shape
        return out

    @staticmethod
    def backward(ctx, g):
        pred, gt, out = ctx.saved_tensors
        d = torch.zeros(ctx.shape, dtype=torch.float32, device=pred.device)
        ops.weighted_bce_backward(pred.contiguous(), gt.contiguous(), out, g.contiguous(), ctx.n_dev, ctx.pos, d)
        return d, None, None, None, None


class CircleLossFunction(torch.autograd.Function):
    """:156-176 on the anchors `filtered[choice]` -> f32 [4]: circle_loss, recall, #row_sel, #col_sel (element 0
    differentiable with respect to the two feature matrices)."""

    @staticmethod
    def forward(ctx, src_feats, tgt_feats, src_pcd, tgt_pcd, corr, rot, trans, filt, count, choice, params, keep):
        g = ops.circle_gather(corr, filt, count, choice, src_pcd, tgt_pcd, src_feats, tgt_feats, rot, trans)
        out, st_a, st_b, nn_idx = ops.circle_forward(params, anchors=g)
        ctx.g, ctx.params, ctx.st, ctx.out = g, params, (st_a, st_b), out
        ctx.rows = (src_feats.shape[0], tgt_feats.shape[0])
        if keep is not None:
            keep.update(g, nn=nn_idx, st_a=st_a, st_b=st_b)
        return out

    @staticmethod
    def backward(ctx, grad):
        d_a, d_b = ops.circle_backward(ctx.params, ctx.st[0], ctx.st[1], ctx.out, grad.contiguous(), anchors=ctx.g)
        d_src = ops.circle_scatter(d_a, ctx.g["a_row"], ctx.rows[0])
        d_tgt = ops.circle_scatter(d_b, ctx.g["b_row"], ctx.rows[1])
        return (d_src, d_tgt) + (None,) * 10


class DenseCircleLossFunction(torch.autograd.Function):
    """get_circle_loss / get_recall (:34-77) on dense [n, m] distance matrices, n, m <= 512."""

    @staticmethod
    def forward(ctx, coords_dist, feats_dist, params):
        out, st_a, st_b, _ = ops.circle_forward(params, coords_dist=coords_dist, feats_dist=feats_dist)
        ctx.save_for_backward(coords_dist, feats_dist, st_a, st_b, out)
        ctx.params = params
        return out

    @staticmethod
    def backward(ctx, grad):
        cd, fd, st_a, st_b, out = ctx.saved_tensors
        return None, ops.circle_backward(ctx.params, st_a, st_b, out, grad.contiguous(), coords_dist=cd, feats_dist=fd), None


def _gpu(t, dtype, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise AprHipError(f"MetricLoss: {name} must be a GPU tensor (the HIP path has no CPU fallback)")
    return t.to(dtype).contiguous()


class MetricLoss(nn.Module):
    """
    We evaluate both contrastive loss and circle loss
    """

    def __init__(self, configs, log_scale=16, pos_optimal=0.1, neg_optimal=1.4):
        super(MetricLoss, self).__init__()
        self.log_scale = log_scale
        self.pos_optimal = pos_optimal
        self.neg_optimal = neg_optimal

        self.pos_margin = configs.pos_margin
        self.neg_margin = configs.neg_margin
        self.max_points = configs.max_points

        self.safe_radius = configs.safe_radius
        self.matchability_radius = configs.matchability_radius
        self.pos_radius = configs.pos_radius  # just to take care of the numeric precision
        self.keep_intermediates = False       # True: `last` holds the forward's device-side decisions (index lists,
        self.last = {}                        # arg-maxes, anchors) until the next call; for tests and oracle chains

    def _params(self):
        return (self.pos_radius, self.safe_radius, self.pos_optimal, self.neg_optimal, self.pos_margin, self.neg_margin,
                self.log_scale)

    def get_circle_loss(self, coords_dist, feats_dist):
        return DenseCircleLossFunction.apply(_gpu(coords_dist, torch.float32, "coords_dist"),
                                             _gpu(feats_dist, torch.float32, "feats_dist"), self._params())[0]

    def get_recall(self, coords_dist, feats_dist):
        """
        Get feature match recall, divided by number of true inliers
        """
        out, _, _, _ = ops.circle_forward(self._params(), coords_dist=_gpu(coords_dist, torch.float32, "coords_dist"),
                                          feats_dist=_gpu(feats_dist.detach(), torch.float32, "feats_dist"))
        return out[1]

    def get_weighted_bce_loss(self, prediction, gt):
        out = WeightedBCEFunction.apply(_gpu(prediction, torch.float32, "prediction"), None, _gpu(gt, torch.float32, "gt"),
                                        None, None)
        return out[0], out[2].detach(), out[3].detach()

    def select(self, src_pcd, tgt_pcd, correspondence, rot, trans):
        """:153-155 -> (filt, count): the correspondences closer than pos_radius - 0.001, count on the device."""
        with torch.no_grad():
            return ops.circle_select(correspondence, src_pcd, tgt_pcd, rot, trans, self.pos_radius - 0.001)

    def draw_choice(self, n):
        """:156-157 for `n` filtered correspondences (a host integer): the reference's draw from the global NumPy stream
        above max_points, every correspondence otherwise."""
        if n > self.max_points:
            return np.random.permutation(n)[:self.max_points]
        return np.arange(max(n, 1))

    def forward(self, src_pcd, tgt_pcd, src_feats, tgt_feats, correspondence, rot, trans, scores_overlap, scores_saliency,
                choice=None):
        """
        Circle loss for metric learning, here we feed the positive pairs only
        Input:
            src_pcd:        [N, 3]
            tgt_pcd:        [M, 3]
            rot:            [3, 3]
            trans:          [3, 1]
            src_feats:      [N, C]
            tgt_feats:      [M, C]
        """
        f32 = torch.float32
        src_pcd, tgt_pcd = _gpu(src_pcd, f32, "src_pcd"), _gpu(tgt_pcd, f32, "tgt_pcd")
        src_feats, tgt_feats = _gpu(src_feats, f32, "src_feats"), _gpu(tgt_feats, f32, "tgt_feats")
        corr = _gpu(correspondence, torch.int64, "correspondence")
        rot, trans = _gpu(rot, f32, "rot"), _gpu(trans, f32, "trans")
        scores_overlap, scores_saliency = _gpu(scores_overlap, f32, "scores_overlap"), _gpu(scores_saliency, f32, "scores_saliency")
        n_src, n_tgt = src_pcd.shape[0], tgt_pcd.shape[0]
        stats = dict()
        keep = {} if self.keep_intermediates else None

        #######################
        # BCE loss for overlap: labels from the correspondences (:114-128)
        with torch.no_grad():
            gt, src_idx, tgt_idx, counts = ops.overlap_labels(corr, n_src, n_tgt)
        o = WeightedBCEFunction.apply(scores_overlap, None, gt, None, None)
        stats['overlap_loss'] = o[0]
        stats['overlap_recall'] = o[3].detach()
        stats['overlap_precision'] = o[2].detach()

        #######################
        # BCE loss for saliency, points of the overlap region only (:132-149)
        with torch.no_grad():
            row_arg, col_arg = ops.gathered_argmax(src_feats.detach(), src_idx, counts[0:1], tgt_feats.detach(), tgt_idx,
                                                   counts[1:2])
            labels, sel, pos, dist = ops.saliency_labels(src_pcd, tgt_pcd, rot, trans, src_idx, tgt_idx, counts, row_arg,
                                                         col_arg, scores_saliency.detach(), self.matchability_radius)
        s = WeightedBCEFunction.apply(scores_saliency, sel, labels, counts[2:3], pos)
        stats['saliency_loss'] = s[0]
        stats['saliency_recall'] = s[3].detach()
        stats['saliency_precision'] = s[2].detach()

        #######################################
        # filter the correspondences, keep at most max_points of them (:153-162)
        filt, count = self.select(src_pcd, tgt_pcd, corr, rot, trans)
        if choice is None:
            choice = self.draw_choice(int(count.item()))       # the one host round trip of the call: 4 bytes
        if not torch.is_tensor(choice):
            choice = torch.from_numpy(np.ascontiguousarray(choice, dtype=np.int64)).to(corr.device)
        choice = _gpu(choice, torch.int64, "choice")

        ##############################
        # get FMR and circle loss (:166-176)
        c = CircleLossFunction.apply(src_feats, tgt_feats, src_pcd, tgt_pcd, corr, rot, trans, filt, count, choice,
                                     self._params(), keep)
        stats['circle_loss'] = c[0]
        stats['recall'] = c[1].detach()

        self.last = keep if keep is not None else {}
        if keep is not None:
            keep.update(gt=gt, src_idx=src_idx, tgt_idx=tgt_idx, counts=counts, row_arg=row_arg, col_arg=col_arg,
                        saliency_labels=labels, saliency_dist=dist, saliency_pos=pos, filt=filt, count=count,
                        choice=choice, overlap=o.detach(), saliency=s.detach())
        return stats

"""The validation pass of Predator_APR's trainer on the HIP kernels, device-resident.

Mirrors the non-symmetric branch of `Trainer.inference_one_batch(inputs, 'val')` (Predator_APR/lib/trainer.py:223-280) and
`inference_one_epoch(epoch, 'val')` (:283-350): per held-out pair the KPFCNN in eval() under no_grad, the NPR terms of both
frames, `MetricLoss`; per epoch the ten `AverageMeter.avg` values, which the reference's `train()` uses to switch the
saliency loss on (`recall.avg > 0.3`, :370-374) and to select its snapshots (:363-368).

The reference hands five values to the host per pair (`float(...)`, :274-278) behind about ten elementwise launches.  Here
a pair leaves ONE 16-float record on the device (`apr_predator_valid_record`, csrc/predator_valid.hip) and an epoch reads
all records back with one copy.

What still talks to the host, once per pair and cached across epochs by `PredatorValidEpoch`: `prepare` uploads the pair
and fetches the count of filtered correspondences (4 bytes), which decides whether the reference draws
`np.random.permutation(count)[:max_points]` (lib/loss.py:156-157).  The step itself, given a prepared pair and a `choice`
tensor, enqueues without a host synchronisation.

Not mirrored: the epoch loop's blanket `try / except` (:306-330; an exception propagates), `torch.cuda.empty_cache()`,
logging, tensorboard, snapshots.  The symmetric generator's val branch cannot run in the reference itself (:238-239 writes
`second_feature`, the module reads `second_features`, and one tensor is unpacked into three): `config.symmetric` raises.
"""
import numpy as np
import torch

from ... import ops
from .loss import MetricLoss
from .trainer import npr_frame_loss

KEYS = ops.PVALID_STATS + ("chamfer_loss", "regularization_loss")      # the reference's ten stats, record columns 0-9


class PreparedPair:
    """One validation pair with everything that needs the host done: the collate's dict, the trainer's tensors on the
    device in the loss's dtypes, the filtered correspondences and their count (device and host)."""

    __slots__ = ("inputs", "len_src", "rot", "trans", "corr", "src_pcd", "tgt_pcd", "src_nghb", "tgt_nghb", "filt",
                 "count", "n_filtered")


def saliency_weight(recall_avg):
    """trainer.py:370-374: the saliency loss joins in once the validation recall is above 0.3 (strictly)."""
    return 1.0 if recall_avg > 0.3 else 0.0


class PredatorPairValidStep:
    """`step(prepared_or_inputs, records, slot, choice=None)` enqueues the validation of one pair into `records[slot]`
    (float32 [pairs, 16] on the GPU, columns `ops.PVALID_*`).  `inputs`: `collate_fn_descriptor`'s dict with the trainer's
    keys rot, trans, correspondences, src_pcd_raw, tgt_pcd_raw, src_nghb, tgt_nghb -- or a `PreparedPair` from
    `prepare(inputs)`; with that and a `choice` int64 GPU tensor the call does not synchronise.  `choice=None` draws as the
    reference does (`draw_choice`).

    The generator's mode: the reference never calls `generative_model.eval()` (only `self.model.eval()`, :224), so during
    validation the generator's BatchNorm1d layers normalise with batch statistics and update their running statistics,
    under no_grad.  `strict_reference=True` (default) leaves the generator's mode alone, running-statistics update
    included; `False` puts it in eval() for the call.  Both models are left in the mode they were in (the reference leaves
    `model` in eval() and lets the next train call reset it)."""

    def __init__(self, model, generative_model, config, strict_reference=True):
        if getattr(config, "symmetric", False):
            raise NotImplementedError("the symmetric val branch cannot run in the reference itself (trainer.py:238-239)")
        self.model, self.generative_model = model, generative_model
        self.desc_loss = MetricLoss(config)
        self.point_generation_ratio = config.point_generation_ratio
        self.strict_reference = strict_reference
        self.keep_intermediates = False       # True: `last` holds the step's device-side decisions, for oracle chains
        self.last = {}

    # ------------------------------------------------------------------ host half, once per pair
    def prepare(self, inputs):
        """Uploads, then `MetricLoss.select` (it depends on the data alone); its count comes back in the call's one fetch."""
        dev = torch.device('cuda', torch.cuda.current_device())
        on = lambda v, dt=torch.float32: torch.as_tensor(v).to(dev, dt).contiguous()
        p = PreparedPair()
        p.inputs = inputs
        p.len_src = int(inputs['stack_lengths'][0][0])
        p.rot, p.trans = on(inputs['rot']), on(inputs['trans']).reshape(3, 1)
        p.corr = on(inputs['correspondences'], torch.int64)
        p.src_pcd, p.tgt_pcd = on(inputs['src_pcd_raw']), on(inputs['tgt_pcd_raw'])
        p.src_nghb, p.tgt_nghb = on(inputs['src_nghb']), on(inputs['tgt_nghb'])
        p.filt, p.count = self.desc_loss.select(p.src_pcd, p.tgt_pcd, p.corr, p.rot, p.trans)
        p.n_filtered = int(p.count.cpu()[0])
        return p

    def draw_choice(self, prepared):
        """lib/loss.py:156-157: `np.random.permutation(count)[:max_points]` from the GLOBAL NumPy stream above max_points, no
        draw otherwise -> int64 NumPy array."""
        return np.ascontiguousarray(self.desc_loss.draw_choice(prepared.n_filtered), dtype=np.int64)

    # ------------------------------------------------------------------ device half
    def _metric_vectors(self, p, src_feats, tgt_feats, scores_overlap, scores_saliency, choice):
        """`MetricLoss.forward` launch for launch, without the autograd wrappers, keeping the kernels' result vectors whole
        -> (overlap f32 [8], saliency f32 [8], circle f32 [4])."""
        L = self.desc_loss
        n_src, n_tgt = p.src_pcd.shape[0], p.tgt_pcd.shape[0]
        gt, src_idx, tgt_idx, counts = ops.overlap_labels(p.corr, n_src, n_tgt)
        o = ops.weighted_bce(scores_overlap, gt)
        row_arg, col_arg = ops.gathered_argmax(src_feats, src_idx, counts[0:1], tgt_feats, tgt_idx, counts[1:2])
        labels, sel, pos, dist = ops.saliency_labels(p.src_pcd, p.tgt_pcd, p.rot, p.trans, src_idx, tgt_idx, counts, row_arg,
                                                     col_arg, scores_saliency, L.matchability_radius)
        s = ops.weighted_bce(sel, labels, counts[2:3])
        g = ops.circle_gather(p.corr, p.filt, p.count, choice, p.src_pcd, p.tgt_pcd, src_feats, tgt_feats, p.rot, p.trans)
        c, _, _, nn_idx = ops.circle_forward(L._params(), anchors=g)
        if self.keep_intermediates:
            self.last = dict(g, nn=nn_idx, counts=counts, row_arg=row_arg, col_arg=col_arg, choice=choice, overlap=o,
                             saliency=s, circle=c, src_idx=src_idx, tgt_idx=tgt_idx)
        return o, s, c

    def step(self, prepared_or_inputs, records, slot, choice=None):
        p = prepared_or_inputs if isinstance(prepared_or_inputs, PreparedPair) else self.prepare(prepared_or_inputs)
        if choice is None:
            choice = self.draw_choice(p)
        if not torch.is_tensor(choice):
            choice = torch.from_numpy(np.ascontiguousarray(choice, dtype=np.int64)).to(p.corr.device)
        modes = (self.model.training, self.generative_model.training)
        _set_training(self.model, False)                                # :224
        if not self.strict_reference:
            self.generative_model.eval()
        try:
            with torch.no_grad():
                feats, scores_overlap, scores_saliency = self.model(p.inputs)
                f32 = lambda t: t.to(torch.float32).contiguous()
                src_feats, tgt_feats = f32(feats[:p.len_src]), f32(feats[p.len_src:])
                # :252-264 (`invalid_flag` is always False in this branch, :265): no loss ratio, no NaN test
                _, c0, r0, _ = npr_frame_loss(self.generative_model, src_feats, p.src_pcd, p.src_nghb,
                                              self.point_generation_ratio, 0.0, 1.0)
                _, c1, r1, _ = npr_frame_loss(self.generative_model, tgt_feats, p.tgt_pcd, p.tgt_nghb,
                                              self.point_generation_ratio, 0.0, 1.0)
                o, s, c = self._metric_vectors(p, src_feats, tgt_feats, f32(scores_overlap), f32(scores_saliency), choice)
                ops.predator_valid_record(o, s, c, p.count, f32(c0), f32(c1), f32(r0), f32(r1), p.src_pcd.shape[0],
                                          p.tgt_pcd.shape[0], records, slot)
        finally:
            _set_training(self.model, modes[0])
            self.generative_model.train(modes[1])

    __call__ = step


def _set_training(module, mode):
    """What `nn.Module.train(mode)` does, flag by flag.  `KPFCNN.train` also drops the network's cached host temperature
    (it guards against parameters rewritten behind the cache's back); a mode switch rewrites nothing, and refetching the
    temperature in every validated pair would be the host synchronisation this step exists to avoid.  The cache still
    follows the parameter's version: the first pair after an optimizer step fetches it once."""
    for m in module.modules():
        m.training = mode


def reduce_records(rec):
    """The ten `AverageMeter.avg` values of an epoch (:326-327) from its records (float32 [pairs, 16], host): plain float64
    means over the pairs of the float32 columns, under the reference's keys, plus `pairs`.  NaN stays NaN."""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, ops.PVALID_RECORD_FLOATS)
    if len(rec) == 0:
        raise ValueError("reduce_records: no pairs")
    out = {k: float(np.mean(rec[:, i].astype(np.float64))) for i, k in enumerate(KEYS)}
    out["pairs"] = len(rec)
    return out


class PredatorValidEpoch:
    """Owns the [pairs, 16] record buffer.  `epoch()` draws the `choice`s in pair order (the reference's draws from the
    global NumPy stream), enqueues every pair, copies the records back ONCE and returns (the reference's ten averages plus
    `pairs`, the per-pair records as a float32 NumPy array).  The pairs are prepared on the first epoch and kept
    (`cache=True`): the reference's val split has no augmentation; a caller whose pairs change says `cache=False`."""

    def __init__(self, step, pairs, cache=True):
        self.step, self.pairs, self.cache = step, list(pairs), cache
        self._prepared = [None] * len(self.pairs)
        self.records = None

    def _pair(self, i):
        p = self._prepared[i]
        if p is None:
            p = self.pairs[i] if isinstance(self.pairs[i], PreparedPair) else self.step.prepare(self.pairs[i])
            if self.cache:
                self._prepared[i] = p
        return p

    def __call__(self):
        if not self.pairs:
            raise ValueError("PredatorValidEpoch: no pairs")
        dev = torch.device('cuda', torch.cuda.current_device())
        if self.records is None:
            self.records = torch.empty((len(self.pairs), ops.PVALID_RECORD_FLOATS), dtype=torch.float32, device=dev)
        self.records.zero_()
        for i in range(len(self.pairs)):
            p = self._pair(i)
            self.step(p, self.records, i, choice=self.step.draw_choice(p))
        host = self.records.cpu().numpy()              # the epoch's one device-to-host copy
        return reduce_records(host), host

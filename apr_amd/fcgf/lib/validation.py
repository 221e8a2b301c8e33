"""The validation pass of APR's FCGF trainer on the HIP kernels, device-resident.

Mirrors `GenerativePairTrainer._valid_epoch` (FCGF_APR/lib/complement_trainer.py:514-681; `GenerativePairValidStep`: the
non-symmetric branch, `SymmetricPairValidStep`: the symmetric one): per held-out pair both frames through the encoder in eval mode, `find_corr(..., subsample_size=5000)`, `est_quad_linear_robust`,
`corr_dist`, RTE, RRE, hit ratio (:555-572) and the NPR validation terms (:583-653); per epoch the seven averages of
:673-681, which `best_val_metric` selects checkpoints by.

The reference hands a value to the host after every one of these (`find_nn_gpu(...).cpu()`, the IRLS result, `.item()`
of the hit ratio, of the Chamfer term, of the regulariser ...).  Here a pair leaves ONE 24-float record on the device
(`apr_valid_pair`, csrc/valid.hip, plus the two NPR terms written into the record's spare floats) and an epoch reads all
records back with one copy.

What still talks to the host: building a pair's voxel pyramid fetches the map sizes (the sizes of the next allocations
depend on them).  The validation set is fixed (`reset_seed(0)`, :518), so `GenerativePairValidStep.prepare` does that
once per pair and `ValidEpoch` keeps the prepared pairs across epochs; the step itself, given a prepared pair, enqueues
without a host synchronisation.

Out of scope, as in the training step: the data loader, logging, checkpoints.  The `SimpleNet*` families of
model/simpleunet.py are not mirrored (`load_model` refuses them): no shipped script selects them -- the symmetric recipe's
generator is a ResUNetFatBN (scripts/train_apr_nuscenes.sh).
"""
import numpy as np
import torch

from ... import MinkowskiEngine as ME
from ... import ops
from . import apg
from .trainer import _Staging

FEAT_MATCH_THRESH = 0.05        # complement_trainer.py:571


class PreparedPair:
    """One validation pair with everything that needs the host done: sparse inputs whose coordinate pyramids are built,
    clouds, ground truth and APG clouds on the device, per-cloud row counts."""

    __slots__ = ("sinput", "coords", "xyz", "T_gt", "nghb", "rows")


class GenerativePairValidStep:
    """`step(input_dict, records, slot)` enqueues the validation of one pair into `records[slot]` (float32 [pairs, 24] on
    the GPU, columns `ops.VALID_*`).  `input_dict`: the collate's keys `sinput{0,1}_{C,F}`, `pcd0`, `pcd1`, `T_gt`,
    `pcd_nghb{0,1}`, optional `len_batch` -- or a `PreparedPair` from `prepare(input_dict)`, with which the call does
    not synchronise.

    `strict_reference=True` (default: parity with the reference is the contract) mirrors two things in the reference's
    text that look unintended; `False` does the evident thing:
      * frame 1's generated points are compared with `pcd_nghb0[i]`, not `pcd_nghb1[i]` (:643);
      * with `RepelL1` the regulariser is ASSIGNED per cloud (`raw_reg_loss =`, :603, :635) where `L2` / `RepelL2`
        accumulate, so only the last cloud of frame 1 counts.
    Both models are put into eval() for the call and left in the mode they were in.

    This class is the non-symmetric branch and refuses `symmetric=True`; the symmetric branch (the generator is a sparse
    network on the encoder's output tensor) is `SymmetricPairValidStep`."""

    def __init__(self, encoder_model, generator_model, voxel_size=0.3, point_generation_ratio=6,
                 regularization_strength=0.1, regularization_type='L2', alpha=0.1, hit_ratio_thresh=0.1,
                 subsample_size=5000, strict_reference=True, symmetric=False):
        if symmetric:
            raise NotImplementedError("the symmetric (SimpleNet) generator branch of _valid_epoch is out of scope")
        if regularization_type not in ('L2', 'RepelL2', 'RepelL1'):
            raise ValueError(regularization_type)
        self.encoder_model, self.generator_model = encoder_model, generator_model
        self.voxel_size, self.point_generation_ratio = voxel_size, point_generation_ratio
        self.regularization_strength, self.regularization_type, self.alpha = regularization_strength, regularization_type, alpha
        self.hit_ratio_thresh, self.subsample_size = hit_ratio_thresh, subsample_size
        self.strict_reference = strict_reference
        self._staging = _Staging()

    # ------------------------------------------------------------------ host half, once per pair
    def prepare(self, input_dict):
        """Uploads, sparse inputs and their coordinate pyramids (synchronises: the map sizes come back to the host)."""
        dev = torch.device('cuda', torch.cuda.current_device())
        f32 = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
        p = PreparedPair()
        p.coords = [input_dict[f'sinput{k}_C'].to(dev) for k in ("0", "1")]
        p.sinput = [ME.SparseTensor(input_dict[f'sinput{k}_F'].to(dev), coordinates=c) for k, c in zip(("0", "1"), p.coords)]
        for s in p.sinput:
            s.coordinate_manager.build_pyramid([2, 4, 8])
        p.xyz = [f32(input_dict['pcd0'][0]), f32(input_dict['pcd1'][0])]
        p.T_gt = f32(input_dict['T_gt']).reshape(-1)[:16].contiguous()
        p.nghb = [[f32(c) for c in input_dict[f'pcd_nghb{k}']] for k in ("0", "1")]
        lens = input_dict.get('len_batch')
        n = [int(c.shape[0]) for c in p.coords]
        p.rows = ([int(l[0]) for l in lens], [int(l[1]) for l in lens]) if lens else ([n[0]], [n[1]])
        for k in (0, 1):
            if sum(p.rows[k]) != n[k] or len(p.rows[k]) != len(p.nghb[k]):
                raise ValueError("validation pair: len_batch / pcd_nghb do not describe the frame's rows")
            if p.xyz[k].shape[0] != p.rows[k][0]:
                raise ValueError(f"validation pair: pcd{k}[0] has {p.xyz[k].shape[0]} rows, its features {p.rows[k][0]}")
        return p

    def draw_subsample(self, n0, n1):
        """find_corr's two draws in the reference's order (source, then target; lib/eval.py:find_corr) -> (inds0, inds1)
        NumPy int64, or (None, None) when the reference does not subsample."""
        s = self.subsample_size
        if s > 0 and n0 > s:
            inds0 = np.random.choice(n0, min(n0, s), replace=False)
            inds1 = np.random.choice(n1, min(n1, s), replace=False)
            return inds0.astype(np.int64), inds1.astype(np.int64)
        return None, None

    # ------------------------------------------------------------------ device half
    def _npr_terms(self, enc, pair):
        """:583-653 -> (chamfer, raw regulariser), both 0-d float32 on the device, divided by 2 * len(clouds)."""
        ratio, vs = self.point_generation_ratio, self.voxel_size
        reg, cham, n_clouds = 0, 0, 1
        for k in (0, 1):
            rows, F, C = pair.rows[k], enc[k].F, pair.coords[k]
            n_clouds, r0 = len(rows), 0
            for i, r in enumerate(rows):
                generated = self.generator_model(F[r0:r0 + r]) * vs
                term = apg.npr_regulariser(generated, self.regularization_type, self.alpha)
                if self.regularization_type == 'RepelL1' and self.strict_reference:
                    reg = term
                else:
                    reg = reg + term
                points = apg.npr_points(generated, C[r0:r0 + r, 1:], vs, ratio)
                target = pair.nghb[0 if self.strict_reference else k][i]
                cham = cham + apg.chamfer_distance(points, target)
                r0 += r
        return cham / (2 * n_clouds), reg / (2 * n_clouds)

    def __call__(self, input_dict, records, slot, draws=None):
        """-> dict of device tensors (sel0, sel1, nn) for inspection; the results are in `records[slot]`.
        `draws`: (inds0, inds1) overrides the NumPy RNG."""
        pair = input_dict if isinstance(input_dict, PreparedPair) else self.prepare(input_dict)
        dev = pair.xyz[0].device
        # find_corr pairs pcd0[0] with ALL rows of F0: as in the reference, that only fits one cloud per frame tensor
        if len(pair.rows[0]) != 1 or len(pair.rows[1]) != 1:
            raise NotImplementedError("validation runs with batch size 1 (find_corr pairs pcd0[0] with all feature rows)")
        n0, n1 = pair.rows[0][0], pair.rows[1][0]
        inds0, inds1 = self.draw_subsample(n0, n1) if draws is None else draws
        sel0 = sel1 = None
        if inds0 is not None:
            sel0, sel1 = self._staging.upload([np.asarray(inds0, dtype=np.int64), np.asarray(inds1, dtype=np.int64)], dev)
        modes = (self.encoder_model.training, self.generator_model.training)
        self.encoder_model.eval()
        self.generator_model.eval()
        try:
            with torch.no_grad():
                enc = [self.encoder_model(s) for s in pair.sinput]
                F0, F1 = enc[0].F, enc[1].F
                if sel0 is not None:
                    F0, F1 = F0.index_select(0, sel0), F1.index_select(0, sel1)
                nn = ops.feature_nn(F0, F1)
                ops.valid_pair(pair.xyz[0], pair.xyz[1], nn, pair.T_gt, records, slot, sel0=sel0, sel1=sel1,
                               hit_thresh=self.hit_ratio_thresh)
                cham, reg = self._npr_terms(enc, pair)
                records[slot, ops.VALID_CHAMFER:ops.VALID_REG + 1] = torch.stack((cham.float(), reg.float()))
        finally:
            self.encoder_model.train(modes[0])
            self.generator_model.train(modes[1])
        return {"sel0": sel0, "sel1": sel1, "nn": nn}


class SymmetricPairValidStep(GenerativePairValidStep):
    """The symmetric branch of `_valid_epoch` (:575-581, :590-591, :622-623; scripts/train_apr_nuscenes.sh): the generator
    is a sparse network (the script's: ResUNetFatBN, 128 channels in, point_generation_ratio * 3 out) called once per frame
    on the encoder's output tensor, and a cloud's rows of its output are the cloud's generated offsets.  Everything else,
    both `strict_reference` behaviours included, is the base class."""

    def __init__(self, encoder_model, generator_model, **kw):
        kw.pop("symmetric", None)
        super().__init__(encoder_model, generator_model, **kw)
        self.symmetric = True

    def _npr_terms(self, enc, pair):
        ratio, vs = self.point_generation_ratio, self.voxel_size
        gens = [self.generator_model(e) for e in enc]            # :576-577: frame 0, then frame 1
        reg, cham, n_clouds = 0, 0, 1
        for k in (0, 1):
            rows, G, C = pair.rows[k], gens[k].F, pair.coords[k]
            n_clouds, r0 = len(rows), 0
            for i, r in enumerate(rows):
                generated = G[r0:r0 + r] * vs
                term = apg.npr_regulariser(generated, self.regularization_type, self.alpha)
                if self.regularization_type == 'RepelL1' and self.strict_reference:
                    reg = term
                else:
                    reg = reg + term
                points = apg.npr_points(generated, C[r0:r0 + r, 1:], vs, ratio)
                target = pair.nghb[0 if self.strict_reference else k][i]
                cham = cham + apg.chamfer_distance(points, target)
                r0 += r
        return cham / (2 * n_clouds), reg / (2 * n_clouds)


def reduce_records(rec, regularization_strength):
    """The seven averages of :673-681 from the records of an epoch (float32 [pairs, 24], host).

    `loss` is the mean of TWO updates per pair: `corr_dist` (:560), then `chamfer + regulariser * strength` (:651, float32
    arithmetic as on the device there); `rre` averages the pairs whose angle is not NaN (:565); `feat_match_ratio` is the
    share of pairs with `hit_ratio > 0.05`, strictly, compared in the record's float32 (the reference widens its float32
    ratio to a double first, so there a ratio that rounds to float32(0.05), e.g. 250 hits of 5000, counts as matched)."""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, ops.VALID_RECORD_FLOATS)
    if len(rec) == 0:
        raise ValueError("reduce_records: no pairs")
    bad = rec[:, ops.VALID_N_CORR] < 0
    if bad.any():
        raise ValueError(f"validation pair {int(np.flatnonzero(bad)[0])}: subsample / nearest-neighbour index out of range")
    mean = lambda v: float(np.mean(np.asarray(v, dtype=np.float64))) if len(v) else 0.0      # AverageMeter.avg of no update: 0
    cham, reg = rec[:, ops.VALID_CHAMFER], rec[:, ops.VALID_REG]
    second = cham + reg * np.float32(regularization_strength)
    rre = rec[:, ops.VALID_RRE]
    hit = rec[:, ops.VALID_HIT_RATIO]
    return {
        "loss": mean(np.stack((rec[:, ops.VALID_CORR_DIST], second), 1).reshape(-1)),
        "rre": mean(rre[~np.isnan(rre)]),
        "rte": mean(rec[:, ops.VALID_RTE]),
        "feat_match_ratio": mean(hit > np.float32(FEAT_MATCH_THRESH)),
        "hit_ratio": mean(hit),
        "chamfer_distance": mean(cham),
        "regularize_loss": mean(reg),
    }


class ValidEpoch:
    """Owns the [pairs, 24] record buffer: calls the step once per pair, copies the buffer back ONCE and returns
    (the reference's dict, the per-pair records as a float32 NumPy array).  The pairs are prepared on the first epoch and
    kept (`cache=True`): the validation set does not change between epochs."""

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
            raise ValueError("ValidEpoch: no pairs")
        dev = torch.device('cuda', torch.cuda.current_device())
        if self.records is None:
            self.records = torch.empty((len(self.pairs), ops.VALID_RECORD_FLOATS), dtype=torch.float32, device=dev)
        self.records.zero_()
        for i in range(len(self.pairs)):
            self.step(self._pair(i), self.records, i)
        host = self.records.cpu().numpy()              # the epoch's one device-to-host copy
        return reduce_records(host, self.step.regularization_strength), host

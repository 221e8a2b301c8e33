"""One training iteration of the FCGF baseline trainers on the HIP kernels: the loop body of the four `_train_epoch`s of
FCGF_APR/lib/trainer.py (:224-277 ContrastiveLossTrainer, :465-505 HardestContrastiveLossTrainer, :596-631
TripletLossTrainer and, inherited, HardestTripletLossTrainer), selected as the reference does with `--trainer`
(config.py:21).

`zero_grad` once; per input dict of the `iter_size` accumulated ones both frames through the encoder in train mode (per-call
BatchNorm statistics), the named loss divided by `iter_size`, `backward`; one `optimizer.step()`.  The host half of every
loss (draws, keys, one pinned upload) runs before the encoder is enqueued, from the row counts alone, and nothing reads the
device between the encoder and the optimizer: the logged scalars come back as device tensors.  The epoch loop, the data
loader, logging and checkpoints around it are the reference's own host code and stay out of scope.
"""
import torch

from ... import MinkowskiEngine as ME
from .trainer import ContrastiveLoss, HardestContrastiveLoss, HardestTripletLoss, TripletLoss

TRAINERS = ("ContrastiveLossTrainer", "HardestContrastiveLossTrainer", "TripletLossTrainer", "HardestTripletLossTrainer")


class PairTrainStep:
    def __init__(self, model, optimizer, trainer='HardestContrastiveLossTrainer', iter_size=1, batch_size=1,
                 num_pos_per_batch=1024, num_hn_samples_per_batch=256, neg_thresh=1.4, pos_thresh=0.1, neg_weight=1,
                 triplet_num_pos=256, triplet_num_hn=512, triplet_num_rand=1024):
        # defaults: FCGF_APR/config.py:30-36, :63-65, :93
        if trainer not in TRAINERS:
            raise ValueError(f"PairTrainStep: trainer {trainer!r} is none of {TRAINERS}")
        self.model, self.optimizer, self.trainer, self.iter_size = model, optimizer, trainer, int(iter_size)
        self.neg_weight = neg_weight
        if trainer == "ContrastiveLossTrainer":
            self.crit, self.args = ContrastiveLoss(neg_thresh, pos_thresh, neg_weight), {}
        elif trainer == "HardestContrastiveLossTrainer":       # :492-494
            self.crit = HardestContrastiveLoss(pos_thresh, neg_thresh)
            self.args = dict(num_pos=num_pos_per_batch * batch_size, num_hn_samples=num_hn_samples_per_batch * batch_size)
        else:                                                   # :622-624
            self.crit = (TripletLoss if trainer == "TripletLossTrainer" else HardestTripletLoss)(neg_thresh)
            self.args = dict(num_pos=triplet_num_pos * batch_size, num_hn_samples=triplet_num_hn * batch_size,
                             num_rand_triplet=triplet_num_rand * batch_size)
        self.last_features = []       # the encoder outputs (F0, F1) of the latest call, per input dict

    def prepare(self, input_dict, draws=None, device=None):
        """The host half of the loss for one input dict, from the row counts of its coordinates."""
        n0, n1 = int(input_dict['sinput0_C'].shape[0]), int(input_dict['sinput1_C'].shape[0])
        return self.crit.prepare(n0, n1, input_dict['correspondences'], draws=draws, device=device, **self.args)

    def encode(self, input_dict, dev):
        sinputs = [ME.SparseTensor(input_dict[f'sinput{k}_F'].to(dev), coordinates=input_dict[f'sinput{k}_C'].to(dev))
                   for k in ("0", "1")]
        if hasattr(self.model, "forward_frames"):
            enc = self.model.forward_frames(sinputs)        # both encoder calls in one walk, per-call BN statistics
        else:
            enc = [self.model(t) for t in sinputs]
        return enc[0].F, enc[1].F

    def loss(self, F0, F1, prepared):
        """-> (loss to run backward on, the other two logged scalars) of one input dict, divided by iter_size where the
        reference divides (:266-270, :496-498, :625)."""
        if self.trainer.endswith("ContrastiveLossTrainer"):
            if self.trainer == "ContrastiveLossTrainer":
                pos, neg = self.crit.loss(F0, F1, None, draws=prepared)
            else:
                pos, neg = self.crit.contrastive_hardest_negative_loss(F0, F1, None, draws=prepared, **self.args)
            pos, neg = pos / self.iter_size, neg / self.iter_size
            return pos + self.neg_weight * neg, pos, neg
        loss, pos_dist, neg_dist = self.crit.triplet_loss(F0, F1, None, draws=prepared)
        return loss / self.iter_size, pos_dist / self.iter_size, neg_dist / self.iter_size

    def __call__(self, input_dicts, draws=None):
        """`input_dicts`: one collated batch or a list of `iter_size` of them; `draws`: per dict the loss's draws (tests).
        -> the reference's logged scalars as 0-d device tensors: loss / pos_loss / neg_loss for the contrastive trainers
        (:273-275, :501-503: sums over the accumulated dicts of the terms already divided by iter_size), loss / pos_dist /
        neg_dist for the triplet trainers (:627-629: the distances are the meters' averages over the dicts)."""
        if isinstance(input_dicts, dict):
            input_dicts = [input_dicts]
        if len(input_dicts) != self.iter_size:
            raise ValueError(f"PairTrainStep: iter_size is {self.iter_size}, got {len(input_dicts)} input dicts")
        draws = [None] * self.iter_size if draws is None else draws
        dev = torch.device('cuda', torch.cuda.current_device())
        self.model.train()
        self.optimizer.zero_grad()
        self.last_features = []
        contrastive = self.trainer.endswith("ContrastiveLossTrainer")
        total = [0, 0, 0]
        for input_dict, dr in zip(input_dicts, draws):
            prepared = self.prepare(input_dict, dr, dev)
            F0, F1 = self.encode(input_dict, dev)
            self.last_features.append((F0, F1))
            loss, a, b = self.loss(F0, F1, prepared)
            loss.backward()
            total = [t + v.detach() for t, v in zip(total, (loss, a, b))]
        self.optimizer.step()
        names = ("loss", "pos_loss", "neg_loss") if contrastive else ("loss", "pos_dist", "neg_dist")
        return dict(zip(names, total))

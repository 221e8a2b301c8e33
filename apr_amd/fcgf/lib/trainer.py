"""Hardest-contrastive mining of the FCGF/APR trainers on the GPU (forward value of the loss).

`contrastive_hardest_negative_loss(F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048)` keeps the
signature and sampling of HardestContrastiveLossTrainer (FCGF_APR/lib/trainer.py:400-452; identical copy at
lib/complement_trainer.py:296-348): the three `np.random.choice` draws stay on the host RNG in the same
order, everything after them (gathers, two nearest-negative searches, the positive-pair filter, both hinge
terms and their means) runs in HIP kernels with no host round trip until the two scalars come back.

Training: when the features take part in autograd the mining (gathers + the two
nearest-negative searches) still runs on the HIP kernels under no_grad, and the loss itself is rebuilt from the
mined indices with differentiable torch ops — the same expression as the reference, whose `min` passes gradients
only to the arg-min element, i.e. to exactly the rows gathered here.
"""
import numpy as np
import torch

from ... import _lib, ops
from ..._lib import check, ptr, stream
from ...predator import kp_ops


def _hash(arr, M):
    """Pair key i + j*M (FCGF_APR/util/misc.py:6-18)."""
    if isinstance(arr, np.ndarray):
        N, D = arr.shape
    else:
        N, D = len(arr[0]), len(arr)
    h = np.zeros(N, dtype=np.int64)
    for d in range(D):
        h += (arr[:, d] if isinstance(arr, np.ndarray) else arr[d]) * M ** d
    return h


class PreparedDraws:
    """The host half of one loss evaluation done ahead of the encoder: the three np.random.choice draws (the reference's
    order, trainer.py:413-420), the sampled pairs, the sorted positive keys -- uploaded from pinned memory without
    blocking the host, so that nothing synchronises between the encode and the backward."""

    __slots__ = ("sel0_d", "sel1_d", "pos0_d", "pos1_d", "keys_d", "hash_seed", "N0", "N1")


class _Staging:
    """Two pinned host buffers used in turn for the per-iteration index upload: ONE asynchronous copy per loss evaluation
    and no pinned allocation in the loop (hipHostMalloc / hipHostFree synchronise the device: with the host an iteration
    ahead of the GPU, a fresh `pin_memory()` per array cost a 60-80 ms stall every few iterations)."""

    def __init__(self):
        self.buf, self.ev, self.turn = [None, None], [None, None], 0

    def upload(self, arrays, dev):
        sizes = [int(a.size) for a in arrays]
        total = sum(sizes)
        t = self.turn
        self.turn ^= 1
        if self.buf[t] is None or self.buf[t].numel() < total:
            self.buf[t] = torch.empty(max(total, 1 << 16), dtype=torch.int64).pin_memory()
            self.ev[t] = None
        if self.ev[t] is not None:
            self.ev[t].synchronize()                     # the copy that last read this buffer (two evaluations ago) is done
        host = self.buf[t].numpy()
        pos = 0
        for a, n in zip(arrays, sizes):
            host[pos:pos + n] = a
            pos += n
        d = self.buf[t][:total].to(dev, non_blocking=True)
        self.ev[t] = torch.cuda.Event()
        self.ev[t].record()
        out, pos = [], 0
        for n in sizes:
            out.append(d[pos:pos + n])
            pos += n
        return out


class HardestContrastiveLoss:
    def __init__(self, pos_thresh=0.1, neg_thresh=1.4):   # config.py:34-35
        self.pos_thresh, self.neg_thresh = pos_thresh, neg_thresh
        self._staging = _Staging()

    def prepare(self, N0, N1, positive_pairs, num_pos=5192, num_hn_samples=2048, draws=None, device=None):
        """Everything of contrastive_hardest_negative_loss that does not need the features (trainer.py:408-423): the row
        counts N0 / N1 are known from the coordinates, so a trainer can call this BEFORE the encoder runs."""
        dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        if not isinstance(positive_pairs, np.ndarray):
            positive_pairs = (positive_pairs.detach().cpu().numpy() if torch.is_tensor(positive_pairs)
                              else np.asarray(positive_pairs)).astype(np.int64)
        positive_pairs = positive_pairs.astype(np.int64)
        N_pos_pairs = len(positive_pairs)
        hash_seed = max(N0, N1)
        if draws is None:
            sel0 = np.random.choice(N0, min(N0, num_hn_samples), replace=False)
            sel1 = np.random.choice(N1, min(N1, num_hn_samples), replace=False)
            pos_sel = np.random.choice(N_pos_pairs, num_pos, replace=False) if N_pos_pairs > num_pos else None
        else:
            sel0, sel1, pos_sel = draws
        sample = positive_pairs if pos_sel is None else positive_pairs[pos_sel]
        pd = PreparedDraws()
        pd.sel0_d, pd.sel1_d, pd.pos0_d, pd.pos1_d, pd.keys_d = self._staging.upload(
            [np.asarray(sel0, dtype=np.int64), np.asarray(sel1, dtype=np.int64), sample[:, 0], sample[:, 1],
             np.sort(_hash(positive_pairs, hash_seed))], dev)
        pd.hash_seed, pd.N0, pd.N1 = int(hash_seed), int(N0), int(N1)
        return pd

    def contrastive_hardest_negative_loss(self, F0, F1, positive_pairs, num_pos=5192, num_hn_samples=2048, thresh=None,
                                          draws=None):
        """-> (pos_loss, neg_loss).  Under no_grad: 0-d CPU tensors (forward value only).  With features that
        require grad: differentiable 0-d GPU tensors.  `draws`: (sel0, sel1, pos_sel) overrides the RNG (tests), or a
        PreparedDraws from `prepare` (then `positive_pairs` is not looked at again)."""
        track = torch.is_grad_enabled() and (F0.requires_grad or F1.requires_grad)
        pd = draws if isinstance(draws, PreparedDraws) else \
            self.prepare(len(F0), len(F1), positive_pairs, num_pos, num_hn_samples, draws, F0.device)
        if pd.N0 != len(F0) or pd.N1 != len(F1):
            raise ValueError("contrastive_hardest_negative_loss: the prepared draws belong to other clouds")
        with torch.no_grad():
            res = self._mine_and_reduce(F0, F1, pd, mine_only=track)
        if not track:
            return res
        pos0_d, pos1_d, d01ind, d10ind, keys_d, hash_seed = res
        posF0, posF1 = F0[pos0_d], F1[pos1_d]
        d01 = torch.sqrt((posF0 - F1[d01ind]).pow(2).sum(1) + 1e-7)      # lib/metrics.py:pdist 'L2'
        d10 = torch.sqrt((posF1 - F0[d10ind]).pow(2).sum(1) + 1e-7)
        mask0 = ~torch.isin(pos0_d + d01ind * hash_seed, keys_d, assume_unique=False)
        mask1 = ~torch.isin(d10ind + pos1_d * hash_seed, keys_d, assume_unique=False)
        pos_loss = torch.relu((posF0 - posF1).pow(2).sum(1) - self.pos_thresh)
        neg0 = torch.relu(self.neg_thresh - d01).pow(2)
        neg1 = torch.relu(self.neg_thresh - d10).pow(2)
        # masked means without boolean indexing (which would synchronise to learn its output size): NaN for an empty
        # mask, as torch.mean() of an empty tensor
        m0, m1 = mask0.to(neg0.dtype), mask1.to(neg1.dtype)
        return pos_loss.mean(), ((neg0 * m0).sum() / m0.sum() + (neg1 * m1).sum() / m1.sum()) / 2

    def _mine_and_reduce(self, F0, F1, pd, mine_only):
        dev = F0.device
        sel0_d, sel1_d, pos0_d, pos1_d, keys_d, hash_seed = pd.sel0_d, pd.sel1_d, pd.pos0_d, pd.pos1_d, pd.keys_d, pd.hash_seed
        F0, F1 = F0.detach().contiguous(), F1.detach().contiguous()
        gather = lambda F, idx: kp_ops.gather_pool(F, idx.view(-1, 1), "closest")
        posF0, posF1 = gather(F0, pos0_d), gather(F1, pos1_d)
        subF0, subF1 = gather(F0, sel0_d), gather(F1, sel1_d)
        lib = _lib.load()
        p, c = posF0.shape
        if mine_only:       # indices into the sub-samples -> row indices of the full clouds
            nn01 = ops.feature_nn(posF0, subF1)         # exact arg-min (bf16-MFMA filter + fp32 refine for c in 32 / 64 / 128)
            nn10 = ops.feature_nn(posF1, subF0)
            return (pos0_d, pos1_d, sel1_d[nn01], sel0_d[nn10], keys_d, int(hash_seed))
        nn01 = torch.empty(p, dtype=torch.int64, device=dev)
        nn10 = torch.empty(p, dtype=torch.int64, device=dev)
        check(lib.apr_feature_nn(ptr(posF0), p, ptr(subF1), subF1.shape[0], c, ptr(nn01), stream()))
        check(lib.apr_feature_nn(ptr(posF1), p, ptr(subF0), subF0.shape[0], c, ptr(nn10), stream()))
        out = torch.empty(6, dtype=torch.float64, device=dev)
        check(lib.apr_contrastive_reduce(ptr(posF0), ptr(posF1), p, c, ptr(nn01), ptr(nn10), ptr(sel0_d), ptr(sel1_d),
                                         ptr(pos0_d), ptr(pos1_d), ptr(keys_d), keys_d.shape[0], int(hash_seed),
                                         float(self.pos_thresh), float(self.neg_thresh), ptr(out), stream()))
        o = out.cpu()
        pos_loss = o[0] / o[1]
        neg_loss = (o[2] / o[3] + o[4] / o[5]) / 2     # NaN when every mined negative was a positive, as torch.mean()
        return pos_loss.float(), neg_loss.float()


# ---------------------------------------------------------------------------------------------------------------------
# Random-negative contrastive, triplet and hardest-triplet losses (FCGF_APR/lib/trainer.py:172-300, :530-731) on the pair-
# list kernels of csrc/pair_loss.hip: forward and backward on the device, nothing read back.
# ---------------------------------------------------------------------------------------------------------------------
_STAT, _SQ, _NEG, _TRIPLET = 0, 1, 2, 3        # APR_PAIR_TERM_* (include/apr_hip.h)


def _as_pairs(positive_pairs):
    if torch.is_tensor(positive_pairs):
        positive_pairs = positive_pairs.detach().cpu().numpy()
    return np.asarray(positive_pairs).astype(np.int64).reshape(-1, 2)


def _terms(kind, group, pa=None, pb=None, kp=None):
    n = len(pa if pa is not None else pb)
    t = np.full((n, 4), -1, dtype=np.int32)
    for col, v in enumerate((pa, pb, kp)):
        if v is not None:
            t[:, col] = v
    t[:, 3] = kind | (group << 8)
    return t


class PreparedPairLoss:
    """The host half of one pair-list loss done ahead of the encoder: the draws, the pair list (mined rows left open), the
    term table and the sorted positive keys on the device, from ONE pinned upload."""

    __slots__ = ("N0", "N1", "hash_seed", "n", "n_plain", "eps", "margin", "n_groups", "n_gout", "r0", "r1", "terms", "keys",
                 "sel0", "sel1", "pos0", "pos1", "mine", "slices", "d", "kept", "owner")

    def mined(self):
        """After the loss ran: the mined rows and the masks of the key filter, as device tensors (tests)."""
        out = {}
        for name, (which, a, b) in self.slices.items():
            out[name] = {"r0": self.r0, "r1": self.r1, "kept": self.kept}[which][a:b]
        return out


def _upload_plan(staging, dev, N0, N1, r0, r1, terms, keys, extra=()):
    """r0 / r1 / terms travel as int32 packed into the int64 staging buffer, first, so that the term table stays 16-byte
    aligned; `extra`: int64 arrays (sub-sample rows for the mining gathers)."""
    n, T = len(r0), len(terms)
    if (len(r0) and (r0.min() < 0 or r0.max() >= N0)) or (len(r1) and (r1.min() < 0 or r1.max() >= N1)):
        raise ValueError("pair loss: a pair names a row outside its cloud")
    n4 = (n + 3) // 4 * 4
    packed = np.zeros(2 * n4 + 4 * T, dtype=np.int32)
    packed[:n], packed[n4:n4 + n], packed[2 * n4:] = r0, r1, terms.reshape(-1)
    up = staging.upload([packed.view(np.int64), keys] + [np.asarray(e, dtype=np.int64) for e in extra], dev)
    p32 = up[0].view(torch.int32)
    return p32[:n], p32[n4:n4 + n], p32[2 * n4:].view(-1, 4), up[1], up[2:]


class _PairLossFn(torch.autograd.Function):
    """means f32 [n_groups] of a PreparedPairLoss; differentiable in its first n_gout entries."""

    @staticmethod
    def forward(ctx, F0, F1, plan):
        lib, dev = _lib.load(), F0.device
        F0c, F1c = F0.contiguous(), F1.contiguous()
        n, T, G, c = plan.n, plan.terms.shape[0], plan.n_groups, F0.shape[1]
        d = torch.empty(n, dtype=torch.float32, device=dev)
        coef = torch.empty(n, dtype=torch.float32, device=dev)
        grp = torch.empty(n, dtype=torch.int32, device=dev)
        red = torch.empty(2 * G, dtype=torch.float64, device=dev)
        mean = torch.empty(G, dtype=torch.float32, device=dev)
        kept = torch.empty(T, dtype=torch.uint8, device=dev)
        check(lib.apr_pair_dist(ptr(F0c), plan.N0, ptr(F1c), plan.N1, c, ptr(plan.r0), ptr(plan.r1), n, plan.n_plain,
                                float(plan.eps), ptr(d), ptr(coef), ptr(grp), stream()))
        sb = int(lib.apr_pair_terms_scratch_bytes(T))
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
        check(lib.apr_pair_terms_reduce(ptr(d), ptr(plan.r0), ptr(plan.r1), n, ptr(plan.terms), T, ptr(plan.keys),
                                        plan.keys.shape[0], plan.hash_seed, float(plan.margin), G, ptr(red), ptr(mean),
                                        ptr(coef), ptr(grp), ptr(kept), ptr(scratch), sb, stream()))
        plan.d, plan.kept = d, kept
        ctx.plan = plan
        ctx.save_for_backward(F0c, F1c, coef, grp, red, plan.r0, plan.r1)
        return mean

    @staticmethod
    def backward(ctx, gmean):
        F0, F1, coef, grp, red, r0, r1 = ctx.saved_tensors
        plan, lib = ctx.plan, _lib.load()
        gout = gmean.contiguous().float()
        dF0, dF1 = torch.empty_like(F0), torch.empty_like(F1)
        sb = int(lib.apr_pair_grad_scratch_bytes(plan.n, plan.N0, plan.N1))
        scratch = torch.empty(sb, dtype=torch.uint8, device=F0.device)
        check(lib.apr_pair_grad(ptr(F0), plan.N0, ptr(F1), plan.N1, F0.shape[1], ptr(r0), ptr(r1), plan.n, ptr(coef), ptr(grp),
                                ptr(red), ptr(gout), plan.n_gout, ptr(dF0), ptr(dF1), ptr(scratch), sb, stream()))
        return dF0, dF1, None


class _PairLoss:
    def __init__(self):
        self._staging = _Staging()
        self.last = None        # the PreparedPairLoss of the latest evaluation (mined rows, masks)

    @staticmethod
    def _features(F0, F1, name):
        for F, tag in ((F0, "F0"), (F1, "F1")):
            if not torch.is_tensor(F) or not F.is_cuda or F.dtype != torch.float32 or F.dim() != 2:
                raise _lib.AprHipError(f"{name}: {tag} must be a float32 [N, c] GPU tensor (the HIP path has no CPU fallback)")
        c = F0.shape[1]
        if F1.shape[1] != c or c % 4 != 0 or c > 256 or c <= 0:
            raise _lib.AprHipError(f"{name}: needs equal channel counts with c % 4 == 0 and c <= 256, got {c} and {F1.shape[1]}")

    def _plan(self, dev, N0, N1, hash_seed, r0, r1, terms, keys, n_plain, eps, n_groups, n_gout, extra=(), slices=None):
        pl = PreparedPairLoss()
        pl.r0, pl.r1, pl.terms, pl.keys, rest = _upload_plan(self._staging, dev, N0, N1, r0, r1, terms, keys, extra)
        pl.sel0, pl.sel1, pl.pos0, pl.pos1 = rest if rest else (None,) * 4
        pl.N0, pl.N1, pl.hash_seed, pl.n, pl.n_plain, pl.eps = int(N0), int(N1), int(hash_seed), len(r0), int(n_plain), eps
        pl.margin, pl.n_groups, pl.n_gout, pl.slices, pl.mine, pl.owner = self.neg_thresh, n_groups, n_gout, slices or {}, None, self
        pl.d = pl.kept = None
        return pl

    def _run(self, F0, F1, pl, name):
        if pl.owner is not self or pl.N0 != len(F0) or pl.N1 != len(F1):
            raise ValueError(f"{name}: the prepared draws belong to other clouds or another loss")
        if pl.mine is not None:
            with torch.no_grad():
                self._mine(F0.detach().contiguous(), F1.detach().contiguous(), pl)
        self.last = pl
        return _PairLossFn.apply(F0, F1, pl)


class ContrastiveLoss(_PairLoss):
    """ContrastiveLossTrainer's loss (FCGF_APR/lib/trainer.py:192-206, :254-267)."""

    def __init__(self, neg_thresh=1.4, pos_thresh=0.1, neg_weight=1):    # config.py:34-36; pos_thresh is unused at :260
        super().__init__()
        self.neg_thresh, self.pos_thresh, self.neg_weight = neg_thresh, pos_thresh, neg_weight

    @staticmethod
    def generate_rand_negative_pairs(positive_pairs, hash_seed, N0, N1, N_neg=0):
        """trainer.py:192-206 (== complement_trainer.py:280), on the host: the same array for the same NumPy state."""
        positive_pairs = _as_pairs(positive_pairs)
        if N_neg < 1:
            N_neg = positive_pairs.shape[0] * 2
        pos_keys = _hash(positive_pairs, hash_seed)
        neg_pairs = np.floor(np.random.rand(int(N_neg), 2) * np.array([[N0, N1]])).astype(np.int64)
        neg_keys = _hash(neg_pairs, hash_seed)
        return neg_pairs[np.logical_not(np.isin(neg_keys, pos_keys, assume_unique=False))]

    def prepare(self, N0, N1, positive_pairs, draws=None, device=None):
        """`draws`: the negative pairs [Nn, 2]; None: generate_rand_negative_pairs with hash_seed = max(N0, N1) (:250)."""
        dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        pos = _as_pairs(positive_pairs)
        neg = self.generate_rand_negative_pairs(pos, max(N0, N1), N0, N1) if draws is None else _as_pairs(draws)
        P, Nn = len(pos), len(neg)
        if P + Nn == 0:
            raise ValueError("ContrastiveLoss: no pair at all")
        r0, r1 = np.concatenate([pos[:, 0], neg[:, 0]]), np.concatenate([pos[:, 1], neg[:, 1]])
        terms = np.concatenate([_terms(_SQ, 0, pa=np.arange(P)), _terms(_NEG, 1, pb=P + np.arange(Nn))])
        return self._plan(dev, N0, N1, max(N0, N1), r0, r1, terms, np.zeros(0, np.int64), P, 1e-4, 2, 2)

    def loss(self, F0, F1, pos_pairs, neg_pairs=None, draws=None):
        """-> (pos_loss_mean, neg_loss_mean), 0-d device tensors (:254-267 before the division by iter_size)."""
        self._features(F0, F1, "ContrastiveLoss.loss")
        pl = draws if isinstance(draws, PreparedPairLoss) else \
            self.prepare(len(F0), len(F1), pos_pairs, neg_pairs if draws is None else draws, F0.device)
        mean = self._run(F0, F1, pl, "ContrastiveLoss.loss")
        return mean[0], mean[1]


class TripletLoss(_PairLoss):
    """TripletLossTrainer.triplet_loss (FCGF_APR/lib/trainer.py:532-579)."""

    def __init__(self, neg_thresh=1.4):
        super().__init__()
        self.neg_thresh = neg_thresh

    @staticmethod
    def _draw_random_triplets(num_pos_pairs, N1, num_rand_triplet):
        rand_inds = np.random.choice(num_pos_pairs, min(num_pos_pairs, num_rand_triplet), replace=False)
        negatives = np.random.choice(N1, min(N1, num_rand_triplet), replace=False)
        return rand_inds, negatives

    @staticmethod
    def _random_triplets(pairs, rand_inds, negatives):
        rand_inds, negatives = np.asarray(rand_inds, dtype=np.int64), np.asarray(negatives, dtype=np.int64)
        if len(rand_inds) != len(negatives):        # the reference's _hash fails to broadcast at :569
            raise ValueError(f"triplet_loss: operands could not be broadcast together with shapes ({len(rand_inds)},) "
                             f"({len(negatives)},): min(len(pairs), num_rand_triplet) != min(N1, num_rand_triplet)")
        return pairs[rand_inds], negatives

    def prepare(self, N0, N1, positive_pairs, num_pos=1024, num_hn_samples=None, num_rand_triplet=1024, draws=None, device=None):
        """`draws`: (pos_sel or None, rand_inds, negatives), the reference's order of np.random.choice calls (:547-566)."""
        dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        pairs = _as_pairs(positive_pairs)
        if draws is None:
            pos_sel = np.random.choice(len(pairs), num_pos, replace=False) if len(pairs) > num_pos else None
            rand_inds, negatives = self._draw_random_triplets(len(pairs), N1, num_rand_triplet)
        else:
            pos_sel, rand_inds, negatives = draws
        rand_pairs, negatives = self._random_triplets(pairs, rand_inds, negatives)
        sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
        R, p = len(rand_pairs), len(sample)
        if R == 0 or p == 0:
            raise ValueError("triplet_loss: no positive pair")
        r0 = np.concatenate([rand_pairs[:, 0], rand_pairs[:, 0], sample[:, 0]])
        r1 = np.concatenate([rand_pairs[:, 1], negatives, sample[:, 1]])
        ar = np.arange(R)
        terms = np.concatenate([_terms(_TRIPLET, 0, pa=ar, pb=R + ar, kp=R + ar), _terms(_STAT, 1, pa=2 * R + np.arange(p)),
                                _terms(_STAT, 2, pa=R + ar, kp=R + ar)])
        hash_seed = max(N0, N1)
        return self._plan(dev, N0, N1, hash_seed, r0, r1, terms, np.sort(_hash(pairs, hash_seed)), 0, 1e-7, 3, 1,
                          slices={"rand_mask": ("kept", 0, R)})

    def triplet_loss(self, F0, F1, positive_pairs, num_pos=1024, num_hn_samples=None, num_rand_triplet=1024, draws=None):
        """-> (loss, pos_dist.mean(), rand_neg_dist.mean()): 0-d device tensors, the last two carry no gradient."""
        self._features(F0, F1, "triplet_loss")
        pl = draws if isinstance(draws, PreparedPairLoss) else \
            self.prepare(len(F0), len(F1), positive_pairs, num_pos, num_hn_samples, num_rand_triplet, draws, F0.device)
        mean = self._run(F0, F1, pl, "triplet_loss")
        return mean[0], mean[1].detach(), mean[2].detach()


class HardestTripletLoss(TripletLoss):
    """HardestTripletLossTrainer.triplet_loss (FCGF_APR/lib/trainer.py:658-731)."""

    def prepare(self, N0, N1, positive_pairs, num_pos=1024, num_hn_samples=512, num_rand_triplet=1024, draws=None, device=None):
        """`draws`: (sel0, sel1, pos_sel or None, rand_inds, negatives) (:671-675, :710-713)."""
        dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        pairs = _as_pairs(positive_pairs)
        if draws is None:
            sel0 = np.random.choice(N0, min(N0, num_hn_samples), replace=False)
            sel1 = np.random.choice(N1, min(N1, num_hn_samples), replace=False)
            pos_sel = np.random.choice(len(pairs), num_pos, replace=False) if len(pairs) > num_pos else None
            rand_inds, negatives = self._draw_random_triplets(len(pairs), N1, num_rand_triplet)
        else:
            sel0, sel1, pos_sel, rand_inds, negatives = draws
        rand_pairs, negatives = self._random_triplets(pairs, rand_inds, negatives)
        sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel, dtype=np.int64)]
        R, p = len(rand_pairs), len(sample)
        if R == 0 or p == 0 or len(sel0) == 0 or len(sel1) == 0:
            raise ValueError("triplet_loss: no positive pair or an empty sub-sample")
        # pairs: random (positive | negative), then the sampled positives twice, each copy followed by its mined negatives
        # (a pair carries the gradient of one term only); the mined rows are written by the device before the distances
        open_rows = np.zeros(p, dtype=np.int64)
        r0 = np.concatenate([rand_pairs[:, 0], rand_pairs[:, 0], sample[:, 0], sample[:, 0], sample[:, 0], open_rows])
        r1 = np.concatenate([rand_pairs[:, 1], negatives, sample[:, 1], open_rows, sample[:, 1], sample[:, 1]])
        ar, ap, b = np.arange(R), np.arange(p), 2 * R
        terms = np.concatenate([_terms(_TRIPLET, 0, pa=ar, pb=R + ar, kp=R + ar),
                                _terms(_TRIPLET, 0, pa=b + ap, pb=b + p + ap, kp=b + p + ap),
                                _terms(_TRIPLET, 0, pa=b + 2 * p + ap, pb=b + 3 * p + ap, kp=b + 3 * p + ap),
                                _terms(_STAT, 1, pa=b + ap), _terms(_STAT, 2, pa=b + p + ap), _terms(_STAT, 3, pa=b + 3 * p + ap)])
        hash_seed = max(N0, N1)
        pl = self._plan(dev, N0, N1, hash_seed, r0, r1, terms, np.sort(_hash(pairs, hash_seed)), 0, 1e-7, 4, 1,
                        extra=(sel0, sel1, sample[:, 0], sample[:, 1]),
                        slices={"rand_mask": ("kept", 0, R), "mask0": ("kept", R, R + p), "mask1": ("kept", R + p, R + 2 * p),
                                "D01ind": ("r1", b + p, b + 2 * p), "D10ind": ("r0", b + 3 * p, b + 4 * p)})
        pl.mine = (b + p, b + 3 * p, p)
        return pl

    def _mine(self, F0, F1, pl):
        """Both nearest-negative searches over the sub-samples (:687-699): exact arg-min, lowest index on a tie."""
        lib, dev = _lib.load(), F0.device
        at01, at10, p = pl.mine
        c = F0.shape[1]
        gather = lambda F, idx: kp_ops.gather_pool(F, idx.view(-1, 1), "closest")
        posF0, posF1, subF0, subF1 = gather(F0, pl.pos0), gather(F1, pl.pos1), gather(F0, pl.sel0), gather(F1, pl.sel1)
        best = torch.empty(2, p, dtype=torch.int64, device=dev)
        check(lib.apr_feature_nn(ptr(posF0), p, ptr(subF1), subF1.shape[0], c, ptr(best[0]), stream()))
        check(lib.apr_feature_nn(ptr(posF1), p, ptr(subF0), subF0.shape[0], c, ptr(best[1]), stream()))
        check(lib.apr_pair_rows_from_nn(ptr(best[0]), p, ptr(pl.sel1), pl.sel1.shape[0], ptr(pl.r1[at01:at01 + p]), stream()))
        check(lib.apr_pair_rows_from_nn(ptr(best[1]), p, ptr(pl.sel0), pl.sel0.shape[0], ptr(pl.r0[at10:at10 + p]), stream()))

    def triplet_loss(self, F0, F1, positive_pairs, num_pos=1024, num_hn_samples=512, num_rand_triplet=1024, draws=None):
        """-> (loss, pos_dist.mean(), (D01min.mean() + D10min.mean()) / 2): 0-d device tensors; the reference's `.item()` on
        the third (:731) is not reproduced.  The last two carry no gradient."""
        self._features(F0, F1, "triplet_loss")
        pl = draws if isinstance(draws, PreparedPairLoss) else \
            self.prepare(len(F0), len(F1), positive_pairs, num_pos, num_hn_samples, num_rand_triplet, draws, F0.device)
        mean = self._run(F0, F1, pl, "triplet_loss")
        return mean[0], mean[1].detach(), ((mean[2] + mean[3]) / 2).detach()

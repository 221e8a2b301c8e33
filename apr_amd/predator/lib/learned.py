"""Train a Predator_APR model on some synthetic pairs, validating after every epoch, then test what it learned: the body
of the reference's `Trainer.train()` (Predator_APR/lib/trainer.py:353-377) followed by its tester's epoch, on the HIP
kernels.  The Predator counterpart of apr_amd/fcgf/lib/learned.py: every Predator throughput figure before it used a
random-init KPFCNN.

    per epoch:  PredatorPairTrainStep over the training pairs -> scheduler.step() -> PredatorValidEpoch ->
                best circle loss / best recall (the epoch is recorded, no file is written) ->
                w_saliency_loss = saliency_weight(valid['recall'])
    then:       PredatorTestEpoch on the test split

Pairs come from `synth.make_pair` with complement scans from `synth.raycast`, as `fcgf.lib.learned.synthetic_pair` builds
them; samples from `datasets.kitti.training_sample` (train, validation) and `test_sample` (test), with disjoint seed ranges
per split; neighbour limits from `calibrate_neighbors` on the training items; KPFCNN(kitti_config) + GenerativeMLP_98;
SGD(lr 0.01, momentum 0.98, weight_decay 1e-6) with ExponentialLR(gamma 0.99) (configs/train/kitti.yaml:55-64).
"""
import time

import numpy as np
import torch

from ... import synth
from ..configs.models import kitti_config
from ..datasets import kitti
from ..datasets.dataloader import calibrate_neighbors, collate_fn_descriptor
from ..models.architectures import KPFCNN, KPFCNNDecoder
from ..models.mlp import GenerativeMLP_98
from .tester import PredatorTestEpoch
from .trainer import PredatorPairTrainStep
from .validation import KEYS, PredatorPairValidStep, PredatorValidEpoch, saliency_weight

SEED_STRIDE, VAL_SEED_OFFSET, TEST_SEED_OFFSET = 100000, 50000, 75000
# configs/train/kitti.yaml:40-53 (log_scale is MetricLoss's own default, as the reference's trainer constructs it)
LOSS = dict(pos_margin=0.1, neg_margin=1.4, pos_radius=0.21, safe_radius=0.75, overlap_radius=0.45, matchability_radius=0.3,
            w_circle_loss=1.0, w_overlap_loss=1.0, w_saliency_loss=0.0, max_points=512, loss_ratio=0.001,
            regularization_strength=0.01)
LR, MOMENTUM, WEIGHT_DECAY, GAMMA = 0.01, 0.98, 1e-6, 0.99


def split_seeds(n_train, n_val, n_test, seed=0):
    """-> (train, validation, test) seeds for synth.make_pair: three disjoint ranges, disjoint across `seed` values too."""
    if not (0 < n_train <= VAL_SEED_OFFSET and 0 < n_val <= TEST_SEED_OFFSET - VAL_SEED_OFFSET
            and 0 < n_test <= SEED_STRIDE - TEST_SEED_OFFSET):
        raise ValueError("split_seeds: 1 .. 50000 training, 1 .. 25000 validation and test pairs")
    base = int(seed) * SEED_STRIDE
    return (list(range(base, base + n_train)), list(range(base + VAL_SEED_OFFSET, base + VAL_SEED_OFFSET + n_val)),
            list(range(base + TEST_SEED_OFFSET, base + TEST_SEED_OFFSET + n_test)))


def synthetic_sample(dev, seed, config, split, n_beams=64, n_azimuth=1875, k=5, spacing=6.0):
    """One pair of `synth.make_pair(seed)` as the loader's tuple: `training_sample` with 2k complement scans per key frame
    (`split` 'train' / 'val'), `test_sample` without them ('test')."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=n_beams, n_azimuth=n_azimuth)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    if split == 'test':
        return kitti.test_sample(up(xyz0), up(xyz1), T, config)
    R1 = T[:3, :3].T
    d = float((-R1 @ T[:3, 3])[0])
    yaw = float(np.arctan2(R1[1, 0], R1[0, 0]))
    scene = synth.make_scene(seed)
    cmpl, poses = [], []
    for ox, yw in ((0.0, 0.0), (d, yaw)):
        rng = np.random.default_rng(seed + 1000 + int(ox * 7))
        c, s = np.cos(yw), np.sin(yw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        frames, Ms = [], []
        for j in list(range(-k, 0)) + list(range(1, k + 1)):
            frames.append(up(synth.raycast(scene, (ox + j * spacing, 0.0, 0.0), yw, rng, n_beams, n_azimuth)))
            M = np.eye(4)
            M[:3, 3] = R.T @ np.array([j * spacing, 0.0, 0.0])
            Ms.append(M)
        cmpl.append(frames)
        poses.append(Ms)
    return kitti.training_sample(up(xyz0), up(xyz1), cmpl[0], cmpl[1], poses[0], poses[1], T, config)


def build_models(dev, config, seed=0, symmetric=False):
    """KPFCNN + GenerativeMLP_98 + the yaml's optimizer and scheduler, seeded.  `symmetric`: the generator is a
    KPFCNNDecoder built as the reference's main.py:52-63 builds it -- `config.switch_to_decoder` is False for the KPFCNN
    and set to True (with `config.symmetric`) on the caller's config afterwards, so PredatorPairTrainStep(.., config) takes
    the symmetric branch.  The optimizer gets the same two parameter groups."""
    np.random.seed(seed)                    # the KPConv kernel points are placed with NumPy's global stream
    torch.manual_seed(seed)
    if symmetric:
        config.symmetric, config.switch_to_decoder = True, False
    model = KPFCNN(config).to(dev)
    if symmetric:
        config.switch_to_decoder = True
        gen = KPFCNNDecoder(config).to(dev)
    else:
        gen = GenerativeMLP_98(in_channel=config.final_feats_dim, out_points=config.point_generation_ratio, radius=None,
                               bn_momentum=config.batch_norm_momentum).to(dev)
    opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=LR, momentum=MOMENTUM,
                          weight_decay=WEIGHT_DECAY)
    return model, gen, opt, torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)


def _total(stats, step):
    """The loss the iteration optimised (trainer.py:217-219), from its stats and the step's weights at that time."""
    return stats['circle_loss'] * step.w_circle_loss + stats['overlap_loss'] * step.w_overlap_loss \
        + stats['saliency_loss'] * step.w_saliency_loss \
        + (stats['chamfer_loss'] + stats['regularization_loss'] * step.regularization_strength) * step.loss_ratio


def train_and_test(dev, n_train, n_val, n_test, epochs, n_beams=64, n_azimuth=1875, k=5, seed=0, n_points=5000,
                   max_iteration=50000, max_points=None, strict_reference=True, validate_first=True):
    """-> dict: `train` (per epoch the means of the ten stats and of `total` over its valid iterations), `iterations` (per
    iteration the ten stats and `total` as floats), `valid` / `valid_records` (per epoch; with `validate_first` index 0 is
    the untrained model and epoch e is at e + 1), `w_saliency_history` (the weight each epoch's validation set for the
    next), `best_loss` / `best_recall` as (value, epoch), `test` (the tester's summary) and `test_records`, `invalid`
    (iterations with a NaN Chamfer value: no step, not averaged), `limits`, wall `seconds` per phase.

    The global NumPy stream is seeded once (`np.random.seed(seed)`) and then runs through the training draws, the validation
    draws and the tester's draws in order, as the reference's does.  `validate_first` (an addition: the reference's train()
    has no such pass) validates the untrained model so that a run states the held-out figures before and after."""
    t, clock = {}, time.perf_counter
    t0 = clock()
    over = dict(LOSS)
    if max_points is not None:
        over["max_points"] = max_points
    cfg = kitti_config(**over)
    s_train, s_val, s_test = split_seeds(n_train, n_val, n_test, seed)
    items = {split: [synthetic_sample(dev, s, cfg, split, n_beams, n_azimuth, k) for s in seeds]
             for split, seeds in (("train", s_train), ("val", s_val), ("test", s_test))}
    limits = [int(v) for v in calibrate_neighbors(items["train"], cfg)]
    batches = {split: [collate_fn_descriptor([it], cfg, limits) for it in items[split]] for split in ("train", "val")}
    model, gen, opt, sched = build_models(dev, cfg, seed)
    tstep = PredatorPairTrainStep(model, gen, opt, cfg)
    vepoch = PredatorValidEpoch(PredatorPairValidStep(model, gen, cfg, strict_reference=strict_reference), batches["val"])
    np.random.seed(seed)
    torch.cuda.synchronize()
    t["data"] = clock() - t0

    valid, valid_records = [], []
    t["valid"] = 0.0

    def validate():
        t1 = clock()
        d, rec = vepoch()
        valid.append(d)
        valid_records.append(rec)
        t["valid"] += clock() - t1
        return d

    if validate_first:
        validate()
    history, iterations, w_hist, invalid = [], [], [], 0
    best_loss, best_recall = (float("inf"), None), (-1.0, None)
    t["train"] = 0.0
    for epoch in range(epochs):
        t1 = clock()
        rows = []
        for batch in batches["train"]:
            stats, bad = tstep(batch)
            stats = {key: float(stats[key]) for key in KEYS}
            stats["total"] = _total(stats, tstep)
            iterations.append(stats)
            if bad:                                 # :311-312: raises in the epoch loop, the meters do not see the pair
                invalid += 1
            else:
                rows.append(stats)
        sched.step()
        history.append({key: float(np.mean([r[key] for r in rows])) if rows else float("nan") for key in KEYS + ("total",)})
        t["train"] += clock() - t1
        d = validate()
        if d["circle_loss"] < best_loss[0]:         # :363-368, without the snapshot files
            best_loss = (d["circle_loss"], epoch)
        if d["recall"] > best_recall[0]:
            best_recall = (d["recall"], epoch)
        tstep.w_saliency_loss = saliency_weight(d["recall"])
        w_hist.append(tstep.w_saliency_loss)
    t1 = clock()
    tester = PredatorTestEpoch(model, cfg, limits, n_points=n_points, max_iteration=max_iteration)
    summary, test_records = tester(items["test"])
    t["test"] = clock() - t1
    t["total"] = clock() - t0
    return {"train": history, "iterations": iterations, "valid": valid, "valid_records": valid_records,
            "w_saliency_history": w_hist, "best_loss": best_loss, "best_recall": best_recall, "test": summary,
            "test_records": test_records, "invalid": invalid, "limits": limits, "seeds": (s_train, s_val, s_test),
            "rows": [int(len(it[0])) for it in items["val"]], "seconds": t}

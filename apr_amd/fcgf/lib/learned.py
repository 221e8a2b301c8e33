"""Train on some synthetic pairs, then validate and register held-out ones: the first run of this code base in which the
features under the matcher are LEARNED (every throughput figure before it used a random-init encoder or planted
descriptors).

    validate (fresh models) -> `iterations` x GenerativePairTrainStep over the training pairs -> validate -> register

`train_and_test` trains with APR's recipe or the FCGF baseline's and then runs the reference's tester epoch
(`tester.FCGFTestEpoch`: scripts/test_apr.py / scripts/test_fcgf.py) on the held-out pairs.

Pairs come from `synth.make_pair` with disjoint train / held-out seeds, assembled with the recipe of
`complement_trainer.synthetic_batch` (voxelised key frames, APG clouds from 2k complement scans, GT correspondences
within 1.5 voxels) plus the validation keys `pcd0`, `pcd1`, `T_gt`.
"""
import time

import numpy as np
import torch

from ... import ops, synth
from ..model import load_model
from ..pipeline import PairRegistration
from ..registration import rte_rre
from . import apg
from .complement_trainer import GenerativePairTrainStep
from .pair_trainer import PairTrainStep
from .tester import FCGFTestEpoch, fmr_table
from .validation import GenerativePairValidStep, SymmetricPairValidStep, ValidEpoch

VAL_SEED_OFFSET = 50000
SEED_STRIDE = 100000
RTE_THRESH, RRE_THRESH = 2.0, 5.0          # FCGF_APR/scripts/test_apr.py:106-107 (metres, degrees)


def pair_seeds(n_train, n_val, seed=0):
    """-> (train seeds, held-out seeds) for synth.make_pair: two disjoint ranges, disjoint across `seed` values too."""
    if not (0 < n_train <= VAL_SEED_OFFSET and 0 < n_val <= SEED_STRIDE - VAL_SEED_OFFSET):
        raise ValueError("pair_seeds: 1 .. 50000 pairs per split")
    base = int(seed) * SEED_STRIDE
    return list(range(base, base + n_train)), list(range(base + VAL_SEED_OFFSET, base + VAL_SEED_OFFSET + n_val))


def synthetic_pair(dev, seed, n_beams=64, n_azimuth=1875, k=5, spacing=6.0, voxel_size=0.3):
    """`complement_trainer.synthetic_batch` at any scan size, with the validation keys: -> (input_dict, xyz0, xyz1, T)."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=n_beams, n_azimuth=n_azimuth)
    R1 = T[:3, :3].T
    d = float((-R1 @ T[:3, 3])[0])
    yaw = float(np.arctan2(R1[1, 0], R1[0, 0]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    scene = synth.make_scene(seed)
    out, pts = {}, []
    for tag, xyz, ox, yw in (("0", xyz0, 0.0, 0.0), ("1", xyz1, d, yaw)):
        key = up(xyz)
        rng = np.random.default_rng(seed + 1000 + int(ox * 7))
        c, s = np.cos(yw), np.sin(yw)
        R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        frames, poses = [], []
        for j in list(range(-k, 0)) + list(range(1, k + 1)):
            frames.append(up(synth.raycast(scene, (ox + j * spacing, 0.0, 0.0), yw, rng, n_beams, n_azimuth)))
            M = np.eye(4)
            M[:3, 3] = R.T @ np.array([j * spacing, 0.0, 0.0])
            poses.append(M)
        nghb, sel = apg.aggregate_frames(key, frames, poses, voxel_size)
        out[f"pcd_nghb{tag}"] = [nghb[sel.long()].contiguous()]
        m = ops.build_map(ops.voxelize(key, voxel_size, 0), want_first=True)
        ops.finalize_maps([m])
        out[f"sinput{tag}_C"] = m.coords
        out[f"sinput{tag}_F"] = torch.ones((m.n, 1), device=dev)
        pts.append(key[m.first.long()].contiguous())
        out[f"pcd{tag}"] = [pts[-1]]
    Tt = torch.from_numpy(T).float()
    out["T_gt"] = Tt
    out["correspondences"] = apg.get_matching_indices(pts[0], pts[1], Tt.to(dev), voxel_size * 1.5).cpu()
    out["len_batch"] = [[int(out["sinput0_C"].shape[0]), int(out["sinput1_C"].shape[0])]]
    return out, xyz0, xyz1, T


def build_models(dev, model="ResUNetFatBN", n_out=128, generator=None, ratio=4, lr=0.1, symmetric=False):
    """Encoder, generator and optimizer of scripts/train_apr_kitti.sh (as `complement_trainer.build_step`), seeded.
    `symmetric`: of scripts/train_apr_nuscenes.sh -- `generator` names a sparse network of `load_model` (default: the
    script's ResUNetFatBN) built as lib/complement_trainer.py:52-60 does, n_out channels in, ratio * 3 out."""
    torch.manual_seed(0)
    enc = load_model(model)(1, n_out, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
    if symmetric:
        gen = load_model(generator or "ResUNetFatBN")(n_out, ratio * 3, bn_momentum=0.05, normalize_feature=True,
                                                      conv1_kernel_size=5, D=3).to(dev)
        opt = torch.optim.SGD([{'params': enc.parameters()}, {'params': gen.parameters()}], lr=lr, momentum=0.8,
                              weight_decay=1e-4)
        return enc, gen, opt
    if generator is None:
        generator = "GenerativeMLP_98" if n_out >= 64 else "GenerativeMLP_54"
    gen = getattr(apg, generator)(in_channel=n_out, out_points=ratio, bn_momentum=0.05).to(dev)
    opt = torch.optim.SGD([{'params': enc.parameters()}, {'params': gen.parameters()}], lr=lr, momentum=0.8,
                          weight_decay=1e-4)
    return enc, gen, opt


def train_and_validate(dev, n_train, n_val, iterations, model="ResUNetFatBN", n_out=128, n_beams=64, n_azimuth=1875,
                       seed=0, generator=None, k=5, lr=0.1, num_pos=1024, num_hn=256, ransac_iters=200000,
                       register=True, symmetric=False):
    """`symmetric`: the recipe of scripts/train_apr_nuscenes.sh (sparse generator on the encoder's output tensor,
    regularization_strength 0.01) instead of scripts/train_apr_kitti.sh's.
    -> dict: `valid_before` / `valid_after` (the reference's seven averages on the held-out pairs), their per-pair
    `records_before` / `records_after`, `losses` (one float per iteration), `recall` and the mean RTE / RRE of the
    successes when `register`, wall `seconds` per phase.  Iteration `it` trains on pair `it % n_train` after
    `np.random.seed(it)`; every validation epoch starts from `np.random.seed(0)` (the reference's `reset_seed(0)`)."""
    ratio, vs = 4, 0.3
    t = {}
    clock = time.perf_counter
    t0 = clock()
    s_train, s_val = pair_seeds(n_train, n_val, seed)
    train = [synthetic_pair(dev, s, n_beams, n_azimuth, k)[0] for s in s_train]
    held = [synthetic_pair(dev, s, n_beams, n_azimuth, k) for s in s_val]
    enc, gen, opt = build_models(dev, model, n_out, generator, ratio, lr, symmetric=symmetric)
    reg = 0.01 if symmetric else 0.1
    tstep = GenerativePairTrainStep(enc, gen, opt, voxel_size=vs, point_generation_ratio=ratio, regularization_strength=reg,
                                    loss_ratio=2e-3, num_pos_per_batch=num_pos, num_hn_samples_per_batch=num_hn,
                                    symmetric=symmetric)
    vcls = SymmetricPairValidStep if symmetric else GenerativePairValidStep
    vstep = vcls(enc, gen, voxel_size=vs, point_generation_ratio=ratio, regularization_strength=reg)
    epoch = ValidEpoch(vstep, [h[0] for h in held])
    torch.cuda.synchronize()
    t["data"] = clock() - t0

    def validate(tag):
        t1 = clock()
        np.random.seed(0)
        d, rec = epoch()
        t[tag] = clock() - t1
        return d, rec

    before, rec_before = validate("valid_before")
    t1 = clock()
    losses = []
    for it in range(iterations):
        np.random.seed(it)
        losses.append(tstep(train[it % n_train])["loss"])
    losses = [float(v) for v in torch.stack(losses).cpu()] if losses else []
    t["train"] = clock() - t1
    after, rec_after = validate("valid_after")
    out = {"valid_before": before, "valid_after": after, "records_before": rec_before, "records_after": rec_after,
           "losses": losses, "train_seeds": s_train, "val_seeds": s_val,
           "voxels": [int(h[0]["sinput0_C"].shape[0]) for h in held]}
    if register:
        t1 = clock()
        enc.eval()
        pipe = PairRegistration(enc, vs, ransac_iters=ransac_iters)
        ok, n_valid = [], []
        with torch.no_grad():
            for i, (_, xyz0, xyz1, T) in enumerate(held):
                T_est, info = pipe(torch.from_numpy(xyz0).to(dev), torch.from_numpy(xyz1).to(dev), seed=i)
                rte, rre = rte_rre(T_est, T)
                n_valid.append(int(info["n_valid"]))
                if rte < RTE_THRESH and rre < RRE_THRESH:
                    ok.append((rte, rre))
        t["register"] = clock() - t1
        out.update(recall=len(ok) / len(held), rte_success=float(np.mean([o[0] for o in ok])) if ok else None,
                   rre_success=float(np.mean([o[1] for o in ok])) if ok else None,
                   mean_valid_hypotheses=float(np.mean(n_valid)), ransac_iters=ransac_iters)
    t["total"] = clock() - t0
    out["seconds"] = t
    return out


def train_and_test(dev, n_train, n_test, iterations, trainer='apr', symmetric=False, model="ResUNetFatBN", n_out=128,
                   n_beams=64, n_azimuth=1875, seed=0, generator=None, k=5, lr=0.1, num_pos=1024, num_hn=256,
                   ransac_iters=4000000, subsample_size=5000, n_points=5000, pairs_per_fetch=64):
    """Train, then run the reference's tester on held-out synthetic pairs.  `trainer='apr'`: APR's recipe
    (`GenerativePairTrainStep`; `symmetric` as in `train_and_validate`), tested as scripts/test_apr.py does;
    `trainer='fcgf'`: the FCGF baseline (`PairTrainStep`, hardest contrastive loss), tested as scripts/test_fcgf.py does
    (`FCGFTestEpoch(variant=trainer)`).  Iteration `it` trains on pair `it % n_train` after `np.random.seed(it)`; the test
    epoch starts from `np.random.seed(0)` with the pair index as RANSAC seed.
    -> dict: `losses` (one float per iteration), `summary` (`tester.test_summary`'s keys with `recall`, plus `n_replayed`),
    `fmr` (`tester.fmr_table`), `records` (float64 [n_test, 48]), `recall`, `n_replayed`, `train_seeds`, `test_seeds`,
    `voxels`, wall `seconds` per phase."""
    if trainer not in ("apr", "fcgf"):
        raise ValueError(f"train_and_test: trainer {trainer!r} is neither 'apr' nor 'fcgf'")
    if trainer == "fcgf" and symmetric:
        raise ValueError("train_and_test: `symmetric` is a switch of APR's recipe")
    ratio, vs = 4, 0.3
    t = {}
    clock = time.perf_counter
    t0 = clock()
    s_train, s_test = pair_seeds(n_train, n_test, seed)
    train = [synthetic_pair(dev, s, n_beams, n_azimuth, k)[0] for s in s_train]
    held = [synthetic_pair(dev, s, n_beams, n_azimuth, k)[0] for s in s_test]
    if trainer == "apr":
        enc, gen, opt = build_models(dev, model, n_out, generator, ratio, lr, symmetric=symmetric)
        tstep = GenerativePairTrainStep(enc, gen, opt, voxel_size=vs, point_generation_ratio=ratio,
                                        regularization_strength=0.01 if symmetric else 0.1, loss_ratio=2e-3,
                                        num_pos_per_batch=num_pos, num_hn_samples_per_batch=num_hn, symmetric=symmetric)
    else:
        torch.manual_seed(0)
        enc = load_model(model)(1, n_out, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev)
        opt = torch.optim.SGD(enc.parameters(), lr=lr, momentum=0.8, weight_decay=1e-4)
        tstep = PairTrainStep(enc, opt, trainer='HardestContrastiveLossTrainer', num_pos_per_batch=num_pos,
                              num_hn_samples_per_batch=num_hn)
    torch.cuda.synchronize()
    t["data"] = clock() - t0
    t1 = clock()
    losses = []
    for it in range(iterations):
        np.random.seed(it)
        losses.append(tstep(train[it % n_train])["loss"])
    losses = [float(v) for v in torch.stack(losses).cpu()] if losses else []
    t["train"] = clock() - t1
    t1 = clock()
    tester = FCGFTestEpoch(enc, variant=trainer, voxel_size=vs, ransac_iters=ransac_iters, subsample_size=subsample_size,
                           n_points=n_points, rte_thresh=RTE_THRESH, rre_thresh=RRE_THRESH, pairs_per_fetch=pairs_per_fetch)
    np.random.seed(0)
    summary, records = tester.epoch(held)
    t["test"] = clock() - t1
    t["total"] = clock() - t0
    return {"losses": losses, "summary": summary, "fmr": fmr_table(records), "records": records, "recall": summary["recall"],
            "n_replayed": summary["n_replayed"], "train_seeds": s_train, "test_seeds": s_test,
            "voxels": [int(h["sinput0_C"].shape[0]) for h in held], "ransac_iters": ransac_iters, "seconds": t}

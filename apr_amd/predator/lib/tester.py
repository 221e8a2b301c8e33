"""The epoch of Predator_APR's tester on the HIP kernels: `PredatorTestEpoch` and `test_summary`.

Mirrors `KITTITester.test` / `NUSCENESTester.test` (Predator_APR/lib/tester.py:33-141, 158-268).  The per-pair body
(:48-100: network, score-weighted sampling, feature matching, RANSAC) is `PredatorRegistration.register_samples_phases`
(apr_amd/predator/pipeline.py); behind each pair's RANSAC one launch (`apr_predator_test_pair`, csrc/predator_valid.hip)
turns the raw result, still on the device, into a 32-double record: rotation / translation error, the success flag, |t_gt|,
the two inlier shares, the pose.  An epoch reads its records back ONCE; `test_summary` is the host arithmetic the tester
runs after its loop (:104-137), quirks included.

Not mirrored: the tester's `try / except: continue` around the forward (:56-60; an exception propagates), the timers, the
logger and the files it writes (`results.npz`, `success_dists.npy`, `fail_dists.npy`: their contents are returned).
"""
import warnings

import numpy as np
import torch

from ... import ops
from ..pipeline import PredatorRegistration
from .benchmark_utils import get_angle_deviation


def test_summary(rot_est, trans_est, rot_gt, trans_gt, rot_threshold=5, trans_threshold=2):
    """lib/tester.py:104-137 in NumPy, on rot_est [B,3,3], trans_est [B,3], rot_gt [B,3,3], trans_gt [B,3] or [B,3,1] in
    the dtypes the caller has them (the reference: float64 estimates, float32 ground truth).  As the reference has it:
    the rotation statistics are taken over the pairs under the ROTATION threshold alone and the translation statistics over
    the pairs under the TRANSLATION threshold alone (not over the successes), `trans_rmse` is a mean, every figure is
    `round(., 3)`; an empty selection gives NaN.  -> dict: `recall`, `errors` (rot_mean, rot_median, trans_rmse,
    trans_rmedse, rot_std, trans_std), the per-pair `r_deviation` / `translation_errors`, `success_dists` / `fail_dists`
    (|t_gt| of the successes / the failures) and the four arrays of the reference's results.npz.  Writes no file."""
    rot_est, trans_est, rot_gt = np.asarray(rot_est), np.asarray(trans_est), np.asarray(rot_gt)
    trans_gt = np.asarray(trans_gt)
    if trans_gt.ndim == 3:
        trans_gt = trans_gt[:, :, 0]
    if rot_gt.shape[0] == 0:
        raise ValueError("test_summary: no pairs")
    r_deviation = get_angle_deviation(rot_est, rot_gt)
    translation_errors = np.linalg.norm(trans_est - trans_gt, axis=-1)
    flag_1 = r_deviation < rot_threshold
    flag_2 = translation_errors < trans_threshold
    correct = (flag_1 & flag_2).sum()
    precision = correct / rot_gt.shape[0]
    success_inds = flag_1 & flag_2
    dists = np.linalg.norm(trans_gt, axis=-1)
    r_sel, t_sel = r_deviation[flag_1], translation_errors[flag_2]
    errors = dict()
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)       # the mean / median / std of nothing: NaN, as in the reference
        errors['rot_mean'] = round(np.mean(r_sel), 3)
        errors['rot_median'] = round(np.median(r_sel), 3)
        errors['trans_rmse'] = round(np.mean(t_sel), 3)
        errors['trans_rmedse'] = round(np.median(t_sel), 3)
        errors['rot_std'] = round(np.std(r_sel), 3)
        errors['trans_std'] = round(np.std(t_sel), 3)
    return {"recall": precision, "errors": errors, "r_deviation": r_deviation, "translation_errors": translation_errors,
            "success_dists": dists[np.where(success_inds > 0)], "fail_dists": dists[np.where(success_inds < 1)],
            "rot_est": rot_est, "rot_gt": rot_gt, "trans_est": trans_est, "trans_gt": trans_gt}


def records_summary(records, rot_gt, trans_gt, rot_threshold=5, trans_threshold=2):
    """`test_summary` of an epoch's records (float64 [pairs, 32], host) and the pairs' ground truth."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, ops.PTEST_RECORD_FLOATS)
    T = records[:, ops.PTEST_T:ops.PTEST_T + 16].reshape(-1, 4, 4)
    return test_summary(T[:, :3, :3], T[:, :3, 3], rot_gt, trans_gt, rot_threshold, trans_threshold)


class PredatorTestEpoch:
    """`epoch(samples, rng=None, seeds=None)` -> (summary, records float64 [pairs, 32] on the host, columns `ops.PTEST_*`).

    `samples`: `datasets.kitti.test_sample` / `training_sample` tuples, already voxelised.  `rng=None` draws the
    score-weighted samples from the global `np.random` in the reference's order -- source then target, and only a side
    with more than `n_points` rows draws (lib/tester.py:83-92) -- so the stream ends where the reference's does; a
    `np.random.RandomState` serves the same way.  `seeds`: the RANSAC seeds (default: the pair index).  The records are
    read back once, at the end; a `corr` entry out of range in any of them raises."""

    def __init__(self, model, config, neighborhood_limits, n_points=5000, distance_threshold=0.3, max_iteration=50000,
                 max_validation=1000, rot_threshold=5, trans_threshold=2, inlier_distance_threshold=0.1, pairs_per_batch=1):
        mode = model.training
        self.pipe = PredatorRegistration(model, config, neighborhood_limits, n_points=n_points,
                                         distance_threshold=distance_threshold, max_iteration=max_iteration,
                                         max_validation=max_validation)
        self.model = model.train(mode)                      # the pipeline's constructor leaves it in eval()
        self.rot_threshold, self.trans_threshold = rot_threshold, trans_threshold
        self.inlier_distance_threshold = inlier_distance_threshold
        self.pairs_per_batch = max(1, int(pairs_per_batch))

    def __call__(self, samples, rng=None, seeds=None):
        samples = list(samples)
        if not samples:
            raise ValueError("PredatorTestEpoch: no pairs")
        seeds = list(range(len(samples))) if seeds is None else list(seeds)
        if len(seeds) != len(samples):
            raise ValueError(f"PredatorTestEpoch: {len(samples)} pairs but {len(seeds)} seeds")
        draws = np.random if rng is None else rng
        dev = samples[0][0].device
        records = torch.zeros((len(samples), ops.PTEST_RECORD_FLOATS), dtype=torch.float64, device=dev)
        mode = self.model.training
        self.model.eval()                                   # :39
        try:
            for i in range(0, len(samples), self.pairs_per_batch):
                j = i + self.pairs_per_batch
                ops.drive(self.pipe.register_samples_phases(samples[i:j], draws, seeds[i:j], records=records, slot0=i,
                                                            rot_threshold=self.rot_threshold,
                                                            trans_threshold=self.trans_threshold,
                                                            inlier_distance_threshold=self.inlier_distance_threshold))
        finally:
            self.model.train(mode)
        host = records.cpu().numpy()                        # the epoch's one copy of results
        bad = host[:, ops.PTEST_BAD_CORR] != 0
        if bad.any():
            raise ValueError(f"test pair {int(np.flatnonzero(bad)[0])}: nearest-neighbour index out of range")
        rot_gt = np.stack([s[4].detach().cpu().numpy().reshape(3, 3) for s in samples])
        trans_gt = np.stack([s[5].detach().cpu().numpy().reshape(3) for s in samples])
        return records_summary(host, rot_gt, trans_gt, self.rot_threshold, self.trans_threshold), host

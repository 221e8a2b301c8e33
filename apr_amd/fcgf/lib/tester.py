"""The tester epoch of FCGF_APR on the HIP kernels: `FCGFTestEpoch`, `test_summary`, `fmr_table`, `records_summary`.

Mirrors the per-pair loop of scripts/test_apr.py:111-196 (`variant='apr'`) and scripts/test_fcgf.py:116-205
(`variant='fcgf'`: the same loop with `random_sample` to exactly `n_points` rows a side in front of RANSAC).  Per pair both
frames go through the encoder, `find_corr(..., subsample_size=5000)` gives the correspondences `evaluate_nn_dist` is taken
on, the open3d >= 0.12 RANSAC (apr_amd/fcgf/registration.py) gives the pose; behind it one launch (`apr_fcgf_test_pair`,
csrc/fcgf_test.hip) turns the raw result, still on the device, into a 48-double record: RTE, RRE, the success flag, |t_gt|,
the float32 pose, the inlier shares and the ten hit counts of the pair's `dists_nn` row.  The records of up to
`pairs_per_fetch` pairs are read back with ONE copy; `test_summary` is the host arithmetic of the scripts (:123-124,
:162-186, :215-218), quirks included.

What still talks to the host per pair: building a frame's voxel pyramid fetches the map sizes (the sizes of the next
allocations depend on them), as in the validation pass (validation.py).  Nothing of a pair's RESULT is read back per pair.

Not mirrored: the scripts' timers, logging, `try / except ValueError` around the loader, checkpoint loading and the file
test_fcgf.py:209 writes (its five arrays are returned).  open3d is absent: parity of the RANSAC itself is unpinned.
"""
import numpy as np
import torch

from ... import MinkowskiEngine as ME
from ... import ops
from .trainer import _Staging

VARIANTS = ("apr", "fcgf")
RANSAC_CHUNK = 1 << 20          # the hypothesis list of a single RANSAC round (csrc/ransac.hip: kChunk)


def host_draws(n0, n1, variant, subsample_size=5000, n_points=5000, rng=None):
    """A pair's NumPy draws in the reference's order -> dict of int64 arrays or None: `inds0`, `inds1` (find_corr,
    test_apr.py:44-49: source then target, only when n0 > subsample_size), then for `variant='fcgf'` `choice0`, `choice1`
    (random_sample, test_fcgf.py:65-71, side 0 then side 1: a permutation's head when n > N, draws with replacement when
    n < N, nothing when equal).  `rng=None`: the global `np.random`."""
    if variant not in VARIANTS:
        raise ValueError(f"host_draws: variant {variant!r} is none of {VARIANTS}")
    rng = np.random if rng is None else rng
    out = dict(inds0=None, inds1=None, choice0=None, choice1=None)
    if subsample_size > 0 and n0 > subsample_size:
        out["inds0"] = np.asarray(rng.choice(n0, min(n0, subsample_size), replace=False), dtype=np.int64)
        out["inds1"] = np.asarray(rng.choice(n1, min(n1, subsample_size), replace=False), dtype=np.int64)
    if variant == "fcgf":
        for key, n in (("choice0", n0), ("choice1", n1)):
            if n > n_points:
                out[key] = np.asarray(rng.permutation(n)[:n_points], dtype=np.int64)
            elif n < n_points:
                out[key] = np.asarray(rng.choice(n, n_points), dtype=np.int64)
    return out


class _Meter:
    """lib/timer.py:5-24 (AverageMeter): `sum` and `sq_sum` start as Python floats and take the values in the type they
    come in; `var` = sq_sum / count - avg ** 2.  Before the first update `avg` is 0 and the reference has no `var`: NaN."""

    def __init__(self):
        self.sum, self.sq_sum, self.count, self.avg, self.var = 0.0, 0.0, 0, 0, float("nan")

    def update(self, val):
        self.sum += val
        self.count += 1
        self.avg = self.sum / self.count
        self.sq_sum += val ** 2
        self.var = self.sq_sum / self.count - self.avg ** 2


def _fma32(a, b, c):
    """float32 fused multiply-add, one rounding: the product is exact in double, the sum is rounded to odd there (the
    neighbour of the nearest double with an odd last bit when the sum is inexact), which makes the final rounding to float32
    the correct one."""
    p, c = np.float64(a) * np.float64(b), np.float64(c)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                       # s + err == p + c exactly (two-sum)
    if err != 0.0 and np.isfinite(s) and not (int(s.view(np.int64)) & 1):
        s = np.nextafter(s, np.float64(np.inf) if err > 0 else np.float64(-np.inf))
    return np.float32(s)


def pose_errors_f32(E, G):
    """(rte, rre) of scripts/test_apr.py:162-163 for float32 [4,4] poses, both np.float32, in a STATED float32 order.
    The reference writes `np.linalg.norm(t_est - t_gt)` and `np.trace(R_est.t() @ R_gt)` on float32 torch CPU tensors and
    so leaves order and fusing to the BLAS under NumPy and torch: on the machine tests/golden/fcgf_tester_ref.npz was made on
    the norm's three squares are rounded to float32, added in double and rounded once, and a matrix product entry is
    fma(a2, b2, fma(a1, b1, a0 * b0)); another machine returned 0 where that one returned NaN.  This function states
    the fixture machine's order, which there equals the reference's text bit for bit (20 000 of 20 000 random pose pairs,
    33 of the 10 000 identical ones NaN), so that the figures do not depend on where they are computed.  `np.arccos` on a
    float32 scalar is NumPy's own float32 routine, as in the reference."""
    f = np.float32
    d = [f(E[k, 3]) - f(G[k, 3]) for k in range(3)]
    sq = np.float64(d[0] * d[0]) + np.float64(d[1] * d[1]) + np.float64(d[2] * d[2])
    rte = np.sqrt(f(sq))
    diag = [_fma32(E[2, i], G[2, i], _fma32(E[1, i], G[1, i], f(E[0, i]) * f(G[0, i]))) for i in range(3)]
    with np.errstate(invalid="ignore"):
        rre = np.arccos(((diag[0] + diag[1]) + diag[2] - 1) / 2)
    return rte, rre


def test_summary(T_est, T_gt, rte_thresh=2, rre_thresh=5):
    """The host arithmetic of scripts/test_apr.py:123-124, :162-186 and :215-218 on float32 poses T_est, T_gt [pairs, 4, 4]
    (an epoch's: the records' columns `ops.FTEST_T`).  As the reference has it: both error statements run in float32
    (`pose_errors_f32`: RTE the norm of the translation difference; RRE `np.arccos` of (trace(R_est^T R_gt) - 1) / 2,
    NOT clipped, so NaN when rounding carries the argument past 1, even for an estimate bit-identical to the ground truth);
    a NaN RRE is a failure (`not np.isnan(rre)`, :174, :177); `rte_meter` takes the pairs under the RTE threshold alone and
    `rre_meter`, in degrees, the pairs under the RRE threshold alone (not the successes); both comparisons are strict.
    -> dict: `success_sum`, `success_count`, `recall`, `rte_avg`, `rte_var`, `rre_avg`, `rre_var` (AverageMeter's avg and
    var = sq_sum / count - avg ** 2; a meter without an update: avg 0, var NaN), `dists_success` / `dists_fail` (|t_gt| of
    the successes / failures), `list_rte`, `list_rre` (radians), and the five arrays of test_fcgf.py:209 (`rres`, `rtes`,
    `dists`, `T_gt`, `T_est`).  Writes no file."""
    T_est = np.ascontiguousarray(np.asarray(T_est, dtype=np.float32).reshape(-1, 4, 4))
    T_gt = np.ascontiguousarray(np.asarray(T_gt, dtype=np.float32).reshape(-1, 4, 4))
    if len(T_est) == 0 or len(T_est) != len(T_gt):
        raise ValueError(f"test_summary: {len(T_est)} estimates for {len(T_gt)} ground truth poses")
    success, rte_meter, rre_meter = _Meter(), _Meter(), _Meter()
    dists_success, dists_fail, list_rte, list_rre, trans_gt = [], [], [], [], []
    rre_limit = np.pi / 180 * rre_thresh
    with np.errstate(invalid="ignore"):
        for E, G in zip(T_est, T_gt):
            dist_gt = np.sqrt(np.sum(G[:3, 3] ** 2))
            trans_gt.append(dist_gt)
            rte, rre = pose_errors_f32(E, G)
            rre_ok = bool(not np.isnan(rre) and rre < rre_limit)
            if rte < rte_thresh:
                rte_meter.update(rte)
            if rre_ok:
                rre_meter.update(rre * 180 / np.pi)
            ok = bool(rte < rte_thresh and rre_ok)
            success.update(1 if ok else 0)
            (dists_success if ok else dists_fail).append(dist_gt)
            list_rte.append(rte)
            list_rre.append(rre)
    return {"success_sum": success.sum, "success_count": success.count, "recall": success.avg,
            "rte_avg": rte_meter.avg, "rte_var": rte_meter.var, "rre_avg": rre_meter.avg, "rre_var": rre_meter.var,
            "dists_success": np.asarray(dists_success, dtype=np.float32), "dists_fail": np.asarray(dists_fail, dtype=np.float32),
            "list_rte": np.asarray(list_rte, dtype=np.float32), "list_rre": np.asarray(list_rre, dtype=np.float32),
            "rres": np.asarray(list_rre, dtype=np.float32), "rtes": np.asarray(list_rte, dtype=np.float32),
            "dists": np.asarray(trans_gt, dtype=np.float32), "T_gt": T_gt, "T_est": T_est}


def fmr_table(records):
    """The hit-ratio and feature-match-recall tables from an epoch's records: `hit_ratios[k][pair]` = share of the pair's
    find_corr correspondences with d < (k + 1) * 0.1 (count / m0), `fmrs[j][k]` = share of pairs with
    `hit_ratios[k][pair] > (j + 1) * 0.01`, j, k = 0 .. 9 -- the block at scripts/test_apr.py:200-213 (test_fcgf.py:211-224),
    which the reference keeps COMMENTED OUT: there `np.array(dists_nn)` is ragged whenever two pairs differ in their row
    count, here `m0` may differ between pairs.  -> dict of float64 arrays `hit_ratios` [10, pairs], `fmrs` [10, 10]."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, ops.FTEST_RECORD_FLOATS)
    if len(records) == 0:
        raise ValueError("fmr_table: no pairs")
    counts = records[:, ops.FTEST_HITS:ops.FTEST_HITS + ops.FTEST_HIT_LEVELS]
    hit_ratios = (counts / records[:, ops.FTEST_M0:ops.FTEST_M0 + 1]).T.copy()
    fmrs = np.stack([np.mean((hit_ratios > j * 0.01).astype(float), axis=1) for j in range(1, 11)])
    return {"hit_ratios": hit_ratios, "fmrs": fmrs}


def records_summary(records, T_gt, rte_thresh=2, rre_thresh=5):
    """`test_summary` of an epoch's records (float64 [pairs, 48], host) and the pairs' float32 ground truth [pairs, 4, 4],
    with `fmr_table`'s two arrays added."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, ops.FTEST_RECORD_FLOATS)
    T_est = records[:, ops.FTEST_T:ops.FTEST_T + 16].astype(np.float32).reshape(-1, 4, 4)      # exact: widened float32
    out = test_summary(T_est, T_gt, rte_thresh, rre_thresh)
    out.update(fmr_table(records))
    return out


class FCGFTestEpoch:
    """`epoch(input_dicts, seeds=None, rng=None, keep_dists=False)` -> (summary, records float64 [pairs, 48] on the host,
    columns `ops.FTEST_*`).

    Every input dict is one `collate_debug_pair_fn([pair_sample(...)])` item (batch size 1, as the test loader): keys
    `sinput{0,1}_{C,F}`, `pcd0`, `pcd1`, `T_gt`.  `rng=None` draws from the global `np.random` in the reference's order
    (`host_draws`), so the stream ends where the reference's does; a `np.random.RandomState` serves the same way.
    `seeds`: the RANSAC seeds (default: the pair index).  `keep_dists`: the summary gains `dists_nn`, a list of the pairs'
    float32 `evaluate_nn_dist` rows.

    RANSAC runs as ONE round of all iterations without a host synchronisation (`ops.ransac_pose_async`).  A pair whose
    record says the hypothesis list of that round overflowed (`ops.FTEST_OVERFLOW`: more than 2^20 hypotheses passed both
    checkers) is redone at its fetch through the synchronous `ops.ransac_pose` (rounds of 2^20 iterations, which cannot
    overflow) on the correspondences kept for it, its record is issued again and that row read again; the summary counts
    such pairs in `n_replayed` and lists them in `replayed`.  A record with an index out of range raises.  The model is
    put into eval() for the call and left in the mode it was in."""

    def __init__(self, model, variant='apr', voxel_size=0.3, ransac_iters=4000000, edge_length=0.9, subsample_size=5000,
                 n_points=5000, rte_thresh=2, rre_thresh=5, pairs_per_fetch=64):
        if variant not in VARIANTS:
            raise ValueError(f"FCGFTestEpoch: variant {variant!r} is none of {VARIANTS}")
        self.model, self.variant, self.voxel_size = model, variant, voxel_size
        self.ransac_iters, self.edge_length = int(ransac_iters), edge_length
        self.subsample_size, self.n_points = int(subsample_size), int(n_points)
        self.rte_thresh, self.rre_thresh = rte_thresh, rre_thresh
        self.pairs_per_fetch = max(1, int(pairs_per_fetch))
        self.distance_threshold = voxel_size * 1.0              # test_apr.py:149
        self._staging = _Staging()

    def _record(self, p, raw, records, round_iters):
        ops.fcgf_test_pair(p["xyz0"], p["xyz1"], p["nn"], p["r0"], p["r1"], p["corr"], p["T_gt"], raw, records, p["slot"],
                           sel0=p["sel0"], sel1=p["sel1"], distance_threshold=self.distance_threshold,
                           rte_thresh=self.rte_thresh, rre_thresh=self.rre_thresh, max_iter=round_iters, dists=p["dists"])

    def _enqueue(self, d, T_gt, records, slot, seed, rng, keep_dists):
        """One pair up to its record; -> what the record depends on, to be kept until its fetch."""
        dev = records.device
        if len(d['pcd0']) != 1 or len(d['pcd1']) != 1:
            raise NotImplementedError("FCGFTestEpoch runs with batch size 1 (find_corr pairs pcd0[0] with all feature rows)")
        f32 = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
        xyz0, xyz1 = f32(d['pcd0'][0]), f32(d['pcd1'][0])
        n0, n1 = int(xyz0.shape[0]), int(xyz1.shape[0])
        F = [self.model(ME.SparseTensor(d[f'sinput{k}_F'].to(dev), coordinates=d[f'sinput{k}_C'].to(dev))).F for k in ("0", "1")]
        if F[0].shape[0] != n0 or F[1].shape[0] != n1:
            raise ValueError(f"test pair {slot}: pcd0 / pcd1 have {n0} / {n1} rows, their features {F[0].shape[0]} / {F[1].shape[0]}")
        h = host_draws(n0, n1, self.variant, self.subsample_size, self.n_points, rng)
        names = [k for k in ("inds0", "inds1", "choice0", "choice1") if h[k] is not None]
        up = dict(zip(names, self._staging.upload([h[k] for k in names], dev))) if names else {}
        sel0, sel1 = up.get("inds0"), up.get("inds1")
        take = lambda t, idx: t if idx is None else t.index_select(0, idx)
        nn = ops.feature_nn(take(F[0], sel0), take(F[1], sel1))
        if self.variant == "fcgf":
            c0, c1 = up.get("choice0"), up.get("choice1")
            r0, r1 = take(xyz0, c0), take(xyz1, c1)
            corr = ops.feature_nn(take(F[0], c0), take(F[1], c1))
        else:
            r0, r1 = xyz0, xyz1
            corr = nn if sel0 is None else ops.feature_nn(F[0], F[1])      # no draw: find_corr's search IS RANSAC's
        raw = ops.ransac_pose_async(r0, r1, corr, self.distance_threshold, self.edge_length, self.ransac_iters, seed)
        p = dict(xyz0=xyz0, xyz1=xyz1, sel0=sel0, sel1=sel1, nn=nn, r0=r0, r1=r1, corr=corr, T_gt=T_gt, raw=raw, slot=slot,
                 seed=seed, dists=torch.empty(nn.shape[0], dtype=torch.float32, device=dev) if keep_dists else None)
        self._record(p, raw, records, self.ransac_iters)
        return p

    def _fetch(self, pending, records, host, dists_out):
        """The pending pairs' records in one copy (synchronises), the overflow replays -> the slots replayed."""
        s0, s1 = pending[0]["slot"], pending[-1]["slot"] + 1
        host[s0:s1] = records[s0:s1].cpu().numpy()
        replayed = []
        for p in pending:
            row = host[p["slot"]]
            if row[ops.FTEST_BAD] != 0:
                raise ValueError(f"test pair {p['slot']}: subsample / nearest-neighbour index out of range")
            if row[ops.FTEST_OVERFLOW] != 0:
                T, info = ops.ransac_pose(p["r0"], p["r1"], p["corr"], self.distance_threshold, self.edge_length,
                                          self.ransac_iters, p["seed"])
                raw = torch.from_numpy(ops.ransac_encode(T, info)).to(records.device)
                self._record(p, raw, records, min(self.ransac_iters, RANSAC_CHUNK))      # its rounds cannot overflow
                host[p["slot"]] = records[p["slot"]].cpu().numpy()
                replayed.append(p["slot"])
        if dists_out is not None:
            flat = torch.cat([p["dists"] for p in pending]).cpu().numpy()
            pos = 0
            for p in pending:
                n = p["dists"].shape[0]
                dists_out.append(flat[pos:pos + n].copy())
                pos += n
        return replayed

    def epoch(self, input_dicts, seeds=None, rng=None, keep_dists=False):
        dicts = list(input_dicts)
        if not dicts:
            raise ValueError("FCGFTestEpoch: no pairs")
        seeds = list(range(len(dicts))) if seeds is None else list(seeds)
        if len(seeds) != len(dicts):
            raise ValueError(f"FCGFTestEpoch: {len(dicts)} pairs but {len(seeds)} seeds")
        T_host = np.stack([np.asarray(torch.as_tensor(d['T_gt']).detach().cpu().numpy(), dtype=np.float32).reshape(4, 4)
                           for d in dicts])
        dev = torch.device('cuda', torch.cuda.current_device())
        T_dev = torch.from_numpy(T_host).to(dev)                 # the ground truth of the whole epoch: one upload
        records = torch.zeros((len(dicts), ops.FTEST_RECORD_FLOATS), dtype=torch.float64, device=dev)
        host = np.zeros((len(dicts), ops.FTEST_RECORD_FLOATS), dtype=np.float64)
        dists_out = [] if keep_dists else None
        pending, replayed = [], []
        mode = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                for i, d in enumerate(dicts):
                    pending.append(self._enqueue(d, T_dev[i], records, i, seeds[i], rng, keep_dists))
                    if len(pending) == self.pairs_per_fetch or i + 1 == len(dicts):
                        replayed += self._fetch(pending, records, host, dists_out)
                        pending = []
        finally:
            self.model.train(mode)
        summary = records_summary(host, T_host, self.rte_thresh, self.rre_thresh)
        summary.update(n_replayed=len(replayed), replayed=replayed)
        if keep_dists:
            summary["dists_nn"] = dists_out
        return summary, host

    __call__ = epoch

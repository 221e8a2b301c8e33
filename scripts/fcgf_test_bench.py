"""Milliseconds per tested pair: the FCGF tester epoch (apr_amd/fcgf/lib/tester.py: FCGFTestEpoch, records on the device, one
fetch per `--fetch` pairs) against the host-chained loop of learned.train_and_validate's `register=True` tail
(PairRegistration per pair, a pose fetched per pair, registration.rte_rre on the host), full-size synthetic pairs, the same
weights, the same RANSAC seeds; prints one JSON line.

    python scripts/fcgf_test_bench.py [--pairs 8] [--repeats 5] [--ransac-iters 4000000] [--variant apr|fcgf] [--fetch 64]

These two forms do not run the same work and the figures say so: the chained loop voxelises the raw scans itself, encodes the
two frames as ONE batched tensor and searches the feature nearest neighbours once; the epoch starts from the loader's
voxelised pair, encodes the frames one after the other as the reference's tester does, searches twice when find_corr
subsamples (its correspondences are not RANSAC's), and writes the record.  A third form, `reference_chain`, is the epoch's own
work on the public functions that existed before it, one host round trip each (two encodes, eval.find_corr,
eval.evaluate_hit_ratio, random_sample for --variant fcgf, registration.ransac_feature_matching, rte_rre): the like-for-like
comparison of what the records remove.  All end in a device synchronise inside the timed window; the forms alternate,
`--repeats` windows each after one warm-up window each, and the spread is reported.
`torch_syncs_per_pair`: the synchronising torch calls of one pass (torch.cuda.set_sync_debug_mode('warn'), counted in a pass
of its own); the library's own stream synchronisations are not visible to torch and are listed in `library_syncs_per_pair`
from the code: apr_ransac_pose fetches its result once per round pass, apr_ransac_pose_async never.
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from apr_amd import MinkowskiEngine as ME  # noqa: E402
from apr_amd import ops, synth  # noqa: E402
from apr_amd.fcgf import registration  # noqa: E402
from apr_amd.fcgf.lib.eval import evaluate_hit_ratio, find_corr  # noqa: E402
from apr_amd.fcgf.lib.tester import FCGFTestEpoch  # noqa: E402
from apr_amd.fcgf.model import load_model  # noqa: E402
from apr_amd.fcgf.pipeline import PairRegistration  # noqa: E402
from apr_amd.fcgf.registration import rte_rre  # noqa: E402

VS = 0.3


def loader_pair(dev, seed, beams, azimuth):
    """What the test loader hands the tester for one pair (collate_debug_pair_fn's keys), and the raw scans."""
    xyz0, xyz1, T = synth.make_pair(seed, n_beams=beams, n_azimuth=azimuth)
    out, raw = {}, []
    for tag, xyz in (("0", xyz0), ("1", xyz1)):
        key = torch.from_numpy(xyz).to(dev)
        m = ops.build_map(ops.voxelize(key, VS, 0), want_first=True)
        ops.finalize_maps([m])
        out[f"sinput{tag}_C"] = m.coords
        out[f"sinput{tag}_F"] = torch.ones((m.n, 1), device=dev)
        out[f"pcd{tag}"] = [key[m.first.long()].contiguous()]
        raw.append(key)
    out["T_gt"] = torch.from_numpy(T).float()
    return out, raw[0], raw[1], T


def count_torch_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ransac-iters", type=int, default=4000000)
    ap.add_argument("--variant", default="apr", choices=("apr", "fcgf"))
    ap.add_argument("--fetch", type=int, default=64)
    ap.add_argument("--model", default="ResUNetBN2C")
    ap.add_argument("--n-out", type=int, default=32)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=1875)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fcgf_test_bench needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = load_model(a.model)(1, a.n_out, bn_momentum=0.05, normalize_feature=True, conv1_kernel_size=5, D=3).to(dev).eval()
    held = [loader_pair(dev, 50000 + i, a.beams, a.azimuth) for i in range(a.pairs)]
    dicts = [h[0] for h in held]
    seeds = list(range(a.pairs))
    tester = FCGFTestEpoch(model, variant=a.variant, voxel_size=VS, ransac_iters=a.ransac_iters, pairs_per_fetch=a.fetch)
    pipe = PairRegistration(model, VS, ransac_iters=a.ransac_iters)
    last = {}

    def epoch():
        np.random.seed(0)
        last["epoch"] = tester.epoch(dicts, seeds=seeds)
        torch.cuda.synchronize()

    def chained():
        out = []
        with torch.no_grad():
            for i, (_, xyz0, xyz1, T) in enumerate(held):
                T_est, info = pipe(xyz0, xyz1, seed=i)
                out.append(rte_rre(T_est, T) + (info["n_valid"],))
        torch.cuda.synchronize()
        last["chained"] = out

    def reference_chain():
        np.random.seed(0)
        out = []
        with torch.no_grad():
            for i, d in enumerate(dicts):
                F = [model(ME.SparseTensor(d[f"sinput{k}_F"], coordinates=d[f"sinput{k}_C"])).F for k in ("0", "1")]
                pts = [d["pcd0"][0], d["pcd1"][0]]
                c0, c1 = find_corr(pts[0], pts[1], F[0], F[1], subsample_size=5000)
                hit = evaluate_hit_ratio(c0, c1, d["T_gt"], 0.1)
                if a.variant == "fcgf":
                    for k in (0, 1):
                        n = len(pts[k])
                        if n != 5000:
                            choice = np.random.permutation(n)[:5000] if n > 5000 else np.random.choice(n, 5000)
                            idx = torch.from_numpy(choice).to(dev)
                            pts[k], F[k] = pts[k][idx].contiguous(), F[k][idx].contiguous()
                T_est = registration.ransac_feature_matching(pts[0], pts[1], F[0], F[1], VS, 4, 0.9, a.ransac_iters, seed=i)
                out.append(rte_rre(T_est, d["T_gt"].numpy()) + (hit,))
        torch.cuda.synchronize()
        last["reference_chain"] = out

    forms = {"epoch": epoch, "chained": chained, "reference_chain": reference_chain}
    for f in forms.values():      # warm-up: code objects, weight packs, pinned staging
        f()
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) / a.pairs * 1e3)
    syncs = {k: count_torch_syncs(f) / a.pairs for k, f in forms.items()}
    summary, rec = last["epoch"]
    # the same work must give the same pose: the epoch against reference_chain (same draws, same seeds)
    same = [bool(abs(r[ops.FTEST_RTE] - c[0]) < 1e-4) for r, c in zip(rec, last["reference_chain"])]
    stat = lambda v: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(json.dumps({
        "pairs": a.pairs, "repeats": a.repeats, "variant": a.variant, "ransac_iters": a.ransac_iters, "model": a.model,
        "n_out": a.n_out, "rays": [a.beams, a.azimuth], "pairs_per_fetch": a.fetch,
        "voxels_mean": float(np.mean([d["sinput0_C"].shape[0] for d in dicts])),
        "ms_per_pair_epoch": stat(times["epoch"]), "ms_per_pair_chained": stat(times["chained"]),
        "ms_per_pair_reference_chain": stat(times["reference_chain"]),
        "torch_syncs_per_pair": syncs,
        "library_syncs_per_pair": {"epoch": 0, "chained": "1 (apr_ransac_pose; 2 when its single round overflows)",
                                   "reference_chain": "1 (the same)"},
        "recall": summary["recall"], "n_replayed": summary["n_replayed"],
        "mean_valid_hypotheses": float(rec[:, ops.FTEST_N_VALID].mean()), "rte_agrees_with_reference_chain": same}))


if __name__ == "__main__":
    main()

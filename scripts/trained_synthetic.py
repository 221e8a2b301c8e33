"""Train on synthetic pairs, validate and register held-out ones with the learned features (apr_amd/fcgf/lib/learned.py);
prints one JSON line.

    python scripts/trained_synthetic.py [--train 8] [--val 8] [--iterations 300] [--k 1] [--model ResUNetFatBN] [--n-out 128]
                                        [--symmetric] [--test [--trainer apr|fcgf]]

--symmetric: the recipe of FCGF_APR/scripts/train_apr_nuscenes.sh (a second ResUNetFatBN as generator on the encoder's
output tensor, point_generation_ratio 4, regularization_strength 0.01, L2, loss_ratio 2e-3, num_complement_one_side 3).

--test: train, then run the reference's tester epoch (FCGFTestEpoch: scripts/test_apr.py for --trainer apr, test_fcgf.py with
its 5000-row random_sample for --trainer fcgf) on the held-out pairs instead of validating; --ransac-iters then defaults
to the scripts' 4000000.

The defaults are what fits about two minutes on one MI355X: most of it is the host ray-casting the scans (two key frames
and 4k complement scans per pair), not the GPU.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from apr_amd.fcgf.lib.learned import train_and_test, train_and_validate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=8)
    ap.add_argument("--val", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--k", type=int, default=None,
                    help="complement scans on each side of a key frame (default 1; 3 with --symmetric; the KITTI trainer uses 5)")
    ap.add_argument("--model", default="ResUNetFatBN")
    ap.add_argument("--n-out", type=int, default=128)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=1875)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ransac-iters", type=int, default=None, help="default 200000; 4000000 with --test")
    ap.add_argument("--test", action="store_true", help="train, then the tester epoch on the held-out pairs")
    ap.add_argument("--trainer", default="apr", choices=("apr", "fcgf"), help="with --test: the recipe trained and tested")
    ap.add_argument("--symmetric", action="store_true", help="the nuScenes recipe: sparse generator, 3 complement scans a side")
    a = ap.parse_args()
    if a.k is None:
        a.k = 3 if a.symmetric else 1
    if a.ransac_iters is None:
        a.ransac_iters = 4000000 if a.test else 200000
    if a.test:
        r = train_and_test(torch.device("cuda:0"), a.train, a.val, a.iterations, trainer=a.trainer, symmetric=a.symmetric,
                           model=a.model, n_out=a.n_out, n_beams=a.beams, n_azimuth=a.azimuth, seed=a.seed, k=a.k,
                           ransac_iters=a.ransac_iters)
        s = r["summary"]
        line = {"trainer": a.trainer, "symmetric": a.symmetric, "pairs_train": a.train, "pairs_test": a.val,
                "iterations": a.iterations, "model": a.model, "n_out": a.n_out, "rays": [a.beams, a.azimuth],
                "voxels_test_mean": sum(r["voxels"]) / len(r["voxels"]),
                "loss_first_last": [r["losses"][0], r["losses"][-1]] if r["losses"] else None,
                "recall_rte2m_rre5deg": r["recall"], "success": [s["success_sum"], s["success_count"]],
                "n_replayed": r["n_replayed"], "rte_avg_var": [float(s["rte_avg"]), float(s["rte_var"])],
                "rre_deg_avg_var": [float(s["rre_avg"]), float(s["rre_var"])],
                "hit_ratio_mean_at_0.1m_0.3m": [float(r["fmr"]["hit_ratios"][0].mean()), float(r["fmr"]["hit_ratios"][2].mean())],
                "fmr_tau2_0.05_at_0.1m_0.3m": [float(r["fmr"]["fmrs"][4][0]), float(r["fmr"]["fmrs"][4][2])],
                "mean_valid_hypotheses": float(r["records"][:, 26].mean()), "ransac_iters": r["ransac_iters"],
                "seconds": {k: round(v, 2) for k, v in r["seconds"].items()}}
        print(json.dumps(line))
        return
    r = train_and_validate(torch.device("cuda:0"), a.train, a.val, a.iterations, model=a.model, n_out=a.n_out,
                           n_beams=a.beams, n_azimuth=a.azimuth, seed=a.seed, k=a.k, ransac_iters=a.ransac_iters,
                           symmetric=a.symmetric)
    line = {"symmetric": a.symmetric, "pairs_train": a.train, "pairs_val": a.val, "iterations": a.iterations, "model": a.model, "n_out": a.n_out,
            "rays": [a.beams, a.azimuth], "complement_scans_per_frame": 2 * a.k, "voxels_val_mean": sum(r["voxels"]) / len(r["voxels"]),
            "valid_before": r["valid_before"], "valid_after": r["valid_after"],
            "loss_first_last": [r["losses"][0], r["losses"][-1]] if r["losses"] else None,
            "recall_rte2m_rre5deg": r["recall"], "rte_success_m": r["rte_success"], "rre_success_deg": r["rre_success"],
            "mean_valid_hypotheses": r["mean_valid_hypotheses"], "ransac_iters": r["ransac_iters"],
            "seconds": {k: round(v, 2) for k, v in r["seconds"].items()}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()

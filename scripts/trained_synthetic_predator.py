"""Train a Predator_APR model on synthetic pairs with a validation pass per epoch, then run the tester's epoch on held-out
pairs (apr_amd/predator/lib/learned.py); prints one JSON line.

    python scripts/trained_synthetic_predator.py [--train 8] [--val 4] [--test 4] [--epochs 10] [--k 1]
                                                 [--beams 64] [--azimuth 1875] [--seed 0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from apr_amd.predator.lib.learned import train_and_test  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", type=int, default=8)
    ap.add_argument("--val", type=int, default=4)
    ap.add_argument("--test", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--k", type=int, default=1, help="complement scans on each side of a key frame (the KITTI trainer uses 5)")
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=1875)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--n-points", type=int, default=5000)
    ap.add_argument("--ransac-iters", type=int, default=50000)
    a = ap.parse_args()
    r = train_and_test(torch.device("cuda:0"), a.train, a.val, a.test, a.epochs, n_beams=a.beams, n_azimuth=a.azimuth, k=a.k,
                       seed=a.seed, n_points=a.n_points, max_iteration=a.ransac_iters)
    num = lambda v: None if v != v else float(v)          # NaN has no JSON form
    line = {"pairs": [a.train, a.val, a.test], "epochs": a.epochs, "rays": [a.beams, a.azimuth],
            "complement_scans_per_frame": 2 * a.k, "rows_val": r["rows"], "neighbour_limits": r["limits"],
            "train_total_first_last": [num(r["train"][0]["total"]), num(r["train"][-1]["total"])] if r["train"] else None,
            "valid_first": {k: num(v) for k, v in r["valid"][0].items()},
            "valid_last": {k: num(v) for k, v in r["valid"][-1].items()},
            "w_saliency_history": r["w_saliency_history"], "best_loss": r["best_loss"], "best_recall": r["best_recall"],
            "invalid_iterations": r["invalid"], "test_recall_rre5deg_rte2m": float(r["test"]["recall"]),
            "test_errors": {k: num(v) for k, v in r["test"]["errors"].items()},
            "seconds": {k: round(v, 2) for k, v in r["seconds"].items()}}
    print(json.dumps(line))


if __name__ == "__main__":
    main()

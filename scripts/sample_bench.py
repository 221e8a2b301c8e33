"""Per-sample milliseconds of the device-side training samples at KITTI size: one ~118 k-point pair
with 2k complement scans per key frame, k = 3 and k = 5, on both trees; apr_voxel_down_sample alone on the sample's four
clouds, and the NumPy oracle (tests/voxel_oracle.py) on the same clouds beside it.  The poses are given (exact): pose
refinement is measured elsewhere (scripts/multiway_bench.py).

    python scripts/sample_bench.py [--reps 5] [--no-oracle]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from apr_amd import ops, synth
from apr_amd.fcgf.lib import apg
from apr_amd.fcgf.lib import complement_data_loader as CDL
from apr_amd.predator.configs.models import Config, kitti_config
from apr_amd.predator.datasets import kitti


def pose(x, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    W = np.eye(4)
    W[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    W[:3, 3] = [x, 0.0, 0.0]
    return W


def make_pair(kmax, seed=0):
    rng = np.random.default_rng(seed)
    scene = synth.make_scene(seed)
    scan = lambda W: synth.raycast(scene, W[:3, 3], np.arctan2(W[1, 0], W[0, 0]), rng)
    W = [pose(0.0, 0.0), pose(10.0, 0.1)]
    out = dict(xyz=[scan(w) for w in W], tsfm=np.linalg.inv(W[1]) @ W[0], cmpl=[], M=[])
    for w in W:
        yaw = np.arctan2(w[1, 0], w[0, 0])
        steps = [-1.0 * (j + 1) for j in range(kmax)] + [1.0 * (j + 1) for j in range(kmax)]
        Wc = [pose(w[0, 3] + d, yaw + 0.005 * d) for d in steps]
        out["cmpl"].append([scan(c) for c in Wc])
        out["M"].append([np.linalg.inv(w) @ c for c in Wc])
    return out


def side(p, i, k, kmax):
    idx = list(range(k)) + list(range(kmax, kmax + k))
    return [p["cmpl"][i][j] for j in idx], [p["M"][i][j] for j in idx]


def timed(fn, reps):
    fn()                                     # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kmax = 5
    p = make_pair(kmax)
    to = lambda a: torch.from_numpy(a).to(dev)
    xyz = [to(a) for a in p["xyz"]]
    pcfg = kitti_config(overlap_radius=0.45, max_points=512, augment_noise=0.01, augment_shift_range=2.0,
                        augment_scale_max=1.2, augment_scale_min=0.8, data_augmentation=True)
    fcfg = Config(voxel_size=0.3, min_scale=0.8, max_scale=1.2, positive_pair_search_voxel_size_multiplier=1.5)
    out = {"workload": "training sample, 2 x ~118 k-point key scans + 2k complement scans each, voxel 0.3",
           "key_points": [len(a) for a in p["xyz"]], "cpu_cores": len(os.sched_getaffinity(0)), "k": {}}
    for k in (3, 5):
        c0, M0 = side(p, 0, k, kmax)
        c1, M1 = side(p, 1, k, kmax)
        c0, c1 = [to(a) for a in c0], [to(a) for a in c1]
        rng, pyrng = np.random.RandomState(0), random.Random(0)
        row = {}
        row["predator_training_sample_ms"] = timed(
            lambda: kitti.training_sample(xyz[0], xyz[1], c0, c1, M0, M1, p["tsfm"], pcfg, rng, pyrng), args.reps)
        row["fcgf_training_sample_ms"] = timed(
            lambda: CDL.training_sample(xyz[0], xyz[1], c0, c1, M0, M1, p["tsfm"], fcfg, rng, pyrng), args.reps)
        nghb = [apg.crop_to_radius(key, torch.cat([apg.apply_transform(x, M) for x, M in zip(c, Ms)], 0))
                for key, c, Ms in ((xyz[0], c0, M0), (xyz[1], c1, M1))]
        clouds = xyz + nghb
        cat, lens = torch.cat(clouds, 0).contiguous(), [len(c) for c in clouds]
        row["cloud_points"] = lens
        row["voxel_down_sample_4_clouds_ms"] = timed(lambda: ops.voxel_down_sample(cat, lens, 0.3), args.reps)
        res, vl = ops.voxel_down_sample(cat, lens, 0.3, want=("count",))
        row["voxels"] = [int(v) for v in vl]
        row["largest_voxel_rows"] = int(res["count"].max())
        if not args.no_oracle:
            import voxel_oracle as VO
            host = cat.cpu().numpy()
            t0 = time.perf_counter()
            VO.voxel_down_sample(host, lens, 0.3)
            row["numpy_oracle_4_clouds_ms"] = (time.perf_counter() - t0) * 1e3
        out["k"][str(k)] = row
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

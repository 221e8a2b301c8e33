#!/usr/bin/env python
"""Time the ICP pose refinement (csrc/icp.hip) on synthetic frames.

Three cases, each ONE apr_icp_batch call with the reference's criteria (0.2 m, 1e-6 / 1e-6 / 200 iterations) on clouds
reduced to one point per 5 cm voxel, poses perturbed by 0.15 m / 0.5 deg:
  one      one complement frame onto the key frame
  batch10  the 2k = 10 complement frames of a key frame, the key frame as the shared target
  sample11 a training sample: batch10 plus the pair's own pose (2k + 1 = 11 problems, two target segments)
Prints one JSON line.  --cpu also times the host restatement (tests/icp_oracle.py) on the `one` input.
--assoc-only N: additionally time N rounds of association alone (relative thresholds 0, max_iteration N) on `one`, from
which the per-round cost follows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from apr_amd import ops  # noqa: E402
from tests import icp_oracle as O  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--assoc-only", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    xs = [0.0] + [float(d) for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)] + [8.0]
    frames, planted = O.synthetic_frames(xs)
    red = [f[O.voxel_first_rows(f, 0.05)] for f in frames]
    moved = [O.apply_transform(red[i], O.perturbation(0.15, 0.5, seed=20 + i) @ planted[i]) for i in range(1, 12)]
    key = torch.from_numpy(red[0]).to(dev)
    srcs = [torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in moved]
    # the pair of the sample: frame 11 (8 m ahead) is the target of the key frame moved by the inverse perturbed pose
    pair_T = np.linalg.inv(O.perturbation(0.15, 0.5, seed=19) @ planted[11])
    pair_src = torch.from_numpy(np.ascontiguousarray(O.apply_transform(red[0], pair_T))).to(dev)
    pair_tgt = torch.from_numpy(red[11]).to(dev)

    def call(src_list, tgts, tgt_of, max_it=200, rf=1e-6, rr=1e-6):
        off = np.concatenate([[0], np.cumsum([len(s) for s in src_list])])
        toff = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
        src, tgt = torch.cat(src_list, 0), torch.cat(tgts, 0)
        init = np.tile(np.eye(4), (len(src_list), 1, 1))
        return lambda: ops.icp_batch(src, off, tgt, toff, init, 0.2, max_it, rf, rr, tgt_of_problem=tgt_of)

    cases = {"one": call(srcs[:1], [key], [0]),
             "batch10": call(srcs[:10], [key], [0] * 10),
             "sample11": call(srcs[:10] + [pair_src], [key, pair_tgt], [0] * 10 + [1])}
    out = {"rows_key": len(key), "rows_src_mean": int(np.mean([len(s) for s in srcs[:10]]))}
    for name, fn in cases.items():
        ms = timed(fn, a.reps)
        rec = fn()[0].cpu().numpy()
        out[name] = {"ms": round(ms, 3), "problems": len(rec), "ms_per_problem": round(ms / len(rec), 3),
                     "iterations": rec[:, ops.ICP_ITERATIONS].astype(int).tolist(),
                     "fitness_min": round(float(rec[:, ops.ICP_FITNESS].min()), 4)}
    if a.assoc_only > 0:
        n = a.assoc_only
        ms_n = timed(call(srcs[:1], [key], [0], n, 0.0, 0.0), a.reps)
        ms_0 = timed(call(srcs[:1], [key], [0], 0, 0.0, 0.0), a.reps)
        out["round_us_one"] = round((ms_n - ms_0) / n * 1e3, 2)
        out["setup_ms_one"] = round(ms_0, 3)
        ms_n = timed(call(srcs[:10], [key], [0] * 10, n, 0.0, 0.0), a.reps)
        ms_0 = timed(call(srcs[:10], [key], [0] * 10, 0, 0.0, 0.0), a.reps)
        out["round_us_batch10"] = round((ms_n - ms_0) / n * 1e3, 2)
    if a.cpu:
        t = time.perf_counter()
        r = O.icp(moved[0], red[0], None, 0.2, 200, fp32_round=False)
        out["cpu_one"] = {"s": round(time.perf_counter() - t, 2), "iterations": r["iterations"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

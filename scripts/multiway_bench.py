#!/usr/bin/env python
"""Time the multiway registration (csrc/icp.hip + csrc/posegraph.hip) on synthetic KITTI-size frames.

Per key frame and for k = 3 (the training scripts' num_complement_one_side) and k = 5 (the config default): the 1 + 2k scans
of synth.make_scene reduced to one point per 5 cm voxel, odometry disturbed by 0.15 m / 0.5 deg, the reference's criteria
(0.2 m / 200 iterations for ICP, 0.075 m for the information matrices and the line process).
  multiway_ms      apg.multiway_registration on the reduced clouds (icp_voxel_size=None: the reduction is timed apart)
  icp_ms / information_ms / posegraph_ms   the three library calls of it, each timed alone on the same inputs
  reduce_ms        apg.voxel_first_rows of the 1 + 2k clouds
  refine_ms        apg.refine_complement_poses (the reference's "old method": 2k ICP problems onto the key frame) beside it
Prints one JSON line.
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
from apr_amd.fcgf.lib import apg  # noqa: E402
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


def case(k, dev, reps):
    xs = [0.0] + [-float(d) for d in range(1, k + 1)] + [float(d) for d in range(1, k + 1)]
    frames, planted = O.synthetic_frames(xs)
    odo = [O.perturbation(0.15, 0.5, seed=60 + i) @ planted[i] for i in range(1, 2 * k + 1)]
    full = [torch.from_numpy(f).to(dev) for f in frames]
    reduce_ms = timed(lambda: apg.voxel_first_rows(full, 0.05), reps)
    red = [x[s].contiguous() for x, s in zip(full, apg.voxel_first_rows(full, 0.05))]
    il, ir = apg.inits_from_key_poses(odo[:k]), apg.inits_from_key_poses(odo[k:])
    multiway_ms = timed(lambda: apg.multiway_registration(red[0], red[1:], il, ir, k, icp_voxel_size=None), reps)
    poses, graph = apg.multiway_registration(red[0], red[1:], il, ir, k, icp_voxel_size=None, return_graph=True)
    refine_ms = timed(lambda: apg.refine_complement_poses(red[0], red[1:], odo, icp_voxel_size=None), reps)
    refined = apg.refine_complement_poses(red[0], red[1:], odo, icp_voxel_size=None)

    # the three library calls alone, on the batch multiway_registration builds
    n = k + 1
    srcs, top, inits = [], [], []
    for side, side_inits in ((0, il), (1, ir)):
        ids = [0] + [1 + side * k + i for i in range(k)]
        for s in range(n):
            for t in range(s + 1, n):
                srcs.append(red[ids[s]])
                top.append(ids[t] - 1)
                inits.append(side_inits[(s, t)])
    so = np.concatenate([[0], np.cumsum([len(x) for x in srcs])])
    to = np.concatenate([[0], np.cumsum([len(x) for x in red[1:]])])
    src, tgt = torch.cat(srcs, 0), torch.cat(red[1:], 0)
    icp = lambda: ops.icp_batch(src, so, tgt, to, np.stack(inits), 0.2, 200, tgt_of_problem=top)   # noqa: E731
    icp_ms = timed(icp, reps)
    rec, _ = icp()
    information_ms = timed(lambda: ops.information_batch(src, so, tgt, to, rec, 0.075, tgt_of_problem=top), reps)
    info, _, _ = ops.information_batch(src, so, tgt, to, rec, 0.075, tgt_of_problem=top)
    layout = apg._side_layout(n, 2)
    posegraph_ms = timed(lambda: ops.posegraph_optimize(layout, rec, info, None, 0.075), reps)
    err = lambda ps: [round(float(np.max([O.pose_error(p, g)[j] for p, g in zip(ps, planted[1:])])), 5) for j in (0, 1)]  # noqa: E731
    return {"k": k, "problems": len(srcs), "rows_key": len(red[0]), "rows_src_total": int(so[-1]),
            "reduce_ms": round(reduce_ms, 3), "multiway_ms": round(multiway_ms, 3), "icp_ms": round(icp_ms, 3),
            "information_ms": round(information_ms, 3), "posegraph_ms": round(posegraph_ms, 3),
            "refine_ms": round(refine_ms, 3),
            "icp_iterations_max": int(graph["records"][..., ops.ICP_ITERATIONS].max()),
            "lm_iterations": graph["iterations"].tolist(), "pruned": int((~graph["kept"]).sum()),
            "confidence_min": round(float(graph["confidence"].min()), 4),
            "worst_error_m_deg": {"odometry": err(odo), "multiway": err(poses), "refine": err(refined)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, nargs="+", default=[3, 5])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({f"k{k}": case(k, dev, a.reps) for k in a.k}))


if __name__ == "__main__":
    main()

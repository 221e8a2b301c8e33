"""Times get_inlier_ratio (matrix-free, HIP kernels) against a torch restatement of the reference's path (matmul -> .cpu() ->
NumPy mutual_selection; Predator_APR/lib/benchmark_utils.py:227-295) on the same GPU in the same process.

    python scripts/mutual_bench.py [--sizes 5000 14000] [--reps 20] [--warmup 3] [--out FILE.json]

Both paths get the same seeded float32 inputs already on the host (as the tester holds them) and end with their results on
the host, so each timed call ends in a synchronising copy; the host clock brackets it.  The two paths alternate inside the
timed loop.  Per size and path: median and min / max of the call time, kernel launches per call (counted from the entry
points called, not traced), peak device bytes (torch's allocator, reset before the call) and peak host bytes of the call
(tracemalloc, which sees NumPy's and not torch's host buffers: the .cpu() copy of the score matrix is added from its shape).
There is no fall-back: without a GPU the script fails.
"""
import argparse
import json
import os
import sys
import time
import tracemalloc

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from apr_amd.predator.lib import benchmark_utils as BU  # noqa: E402

# launches per get_inlier_ratio call: 2 arg-max (rows, columns) + 1 mutual select + 1 inlier ratio; 3 result copies
OURS_LAUNCHES = 4


def make_inputs(seed, n, m):
    rng = np.random.default_rng(seed)
    unit = lambda f: (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)
    src_feat, tgt_feat = unit(rng.standard_normal((n, 32))), unit(rng.standard_normal((m, 32)))
    k = min(n, m) // 3
    pi, pj = rng.choice(n, k, replace=False), rng.choice(m, k, replace=False)
    tgt_feat[pj] = unit(src_feat[pi] + 0.03 * rng.standard_normal((k, 32)))
    src = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    tgt = rng.uniform(-40, 40, (m, 3)).astype(np.float32)
    a = np.deg2rad(12.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    trans = np.array([[1.0], [-2.0], [0.5]], np.float32)
    tgt[pj] = (src[pi] @ rot.T + trans[:, 0] + rng.normal(0, 0.02, (k, 3))).astype(np.float32)
    return src, tgt, src_feat, tgt_feat, rot, trans


def reference_mutual_selection(score_mat):
    """benchmark_utils.py:271-295 restated: three full-size host arrays besides the input."""
    mutuals = np.zeros_like(score_mat)
    for i in range(score_mat.shape[0]):
        c_mat = score_mat[i]
        flag_row, flag_column = np.zeros_like(c_mat), np.zeros_like(c_mat)
        np.put_along_axis(flag_row, np.argmax(c_mat, 1)[:, None], 1, 1)
        np.put_along_axis(flag_column, np.argmax(c_mat, 0)[None, :], 1, 0)
        mutuals[i] = flag_row.astype(bool) & flag_column.astype(bool)
    return mutuals.astype(bool)


def reference_path(src, tgt, src_feat, tgt_feat, rot, trans, thr, dev):
    """benchmark_utils.py:227-268 restated with torch: the score matrix is formed on the device and copied to the host."""
    src_t, tgt_t = torch.from_numpy(src), torch.from_numpy(tgt)
    src_t = (torch.matmul(torch.from_numpy(rot), src_t.transpose(0, 1)) + torch.from_numpy(trans)).transpose(0, 1)
    scores = torch.matmul(torch.from_numpy(src_feat).to(dev), torch.from_numpy(tgt_feat).transpose(0, 1).to(dev)).cpu()
    _, idx = scores.max(-1)
    d_wo = torch.norm(src_t - tgt_t[idx], dim=1)
    sel = reference_mutual_selection(scores[None].numpy())[0]
    row_sel, col_sel = np.where(sel)
    d_w = torch.norm(src_t[row_sel] - tgt_t[col_sel], dim=1)
    return (float((d_wo < thr).float().mean()), float((d_w < thr).float().mean()), len(row_sel))


def ours_path(src, tgt, src_feat, tgt_feat, rot, trans, thr, dev):
    r = BU.get_inlier_ratio(src, tgt, src_feat, tgt_feat, rot, trans, thr)
    return float(r["wo"]["inlier_ratio"]), float(r["w"]["inlier_ratio"]), len(r["w"]["distance"])


def measure(fn, args, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn(*args, dev)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def peaks(fn, args, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    tracemalloc.start()
    fn(*args, dev)
    torch.cuda.synchronize(dev)
    host_peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    return torch.cuda.max_memory_allocated(dev) - base, host_peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 14000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mutual_bench: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    rows = []
    for n in a.sizes:
        args = make_inputs(n, n, n) + (0.1,)
        paths = {"ours": ours_path, "reference": reference_path}
        for _ in range(a.warmup):
            outs = {k: f(*args, dev) for k, f in paths.items()}
        # random descriptors hold a few rows whose two best scores differ by less than float32 rounding, where the two
        # arithmetics may pick differently: the figures of both paths are printed side by side, not asserted
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():                     # alternating: both see the same drift of the shared host
                times[k].append(measure(f, args, dev)[0])
        for k, f in paths.items():
            dpk, hpk = peaks(f, args, dev)
            if k == "reference":
                hpk += n * n * 4                            # the .cpu() copy of the score matrix lives in torch's host allocator
            t = np.array(times[k]) * 1e3
            rows.append(dict(path=k, n_src=n, n_tgt=n, d=32, reps=a.reps, ms_median=float(np.median(t)), ms_min=float(t.min()),
                             ms_max=float(t.max()), launches=OURS_LAUNCHES if k == "ours" else None,
                             peak_device_bytes=int(dpk), peak_host_bytes=int(hpk), mutual_pairs=outs[k][2],
                             ratio_wo=outs[k][0], ratio_w=outs[k][1]))
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

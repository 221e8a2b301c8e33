"""Forward + backward milliseconds of the FCGF trainers' pair-list losses at the reference's batch-4 sizes (DESIGN section
23): two stacked frames of ~57 k rows, c = 32 and c = 128; ContrastiveLoss on every positive pair and twice as many random
negatives, TripletLoss and HardestTripletLoss at num_pos / num_hn / num_rand = 1024 / 2048 / 4096 (config.py:63-65 x
batch_size 4).  Beside each: the reference's expression (tests/fcgf_losses_oracle.py's, which restates it) in fp32 torch on
the same GPU, with the reference's own host round trips (arg-min indices to the host, np.isin, boolean indexing).

Per row: median of `--reps` timings, each a host clock around `--inner` forward + backward calls that ends in a device
synchronise, after a warm-up of the same calls; the kernels launched per call (torch.profiler, a run of its own) and the
host synchronisations per call (torch.cuda.set_sync_debug_mode: the calls torch itself knows to block; the HIP path's
library calls are enqueue-only by construction).  Prints one JSON line per row.

    python scripts/fcgf_losses_bench.py [--reps 5] [--inner 10] [--rows 57000]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from apr_amd.fcgf.lib.trainer import ContrastiveLoss, HardestTripletLoss, TripletLoss, _hash


def make_inputs(n, c, n_pairs, dev, seed=0):
    rng = np.random.default_rng(seed)
    f0 = rng.standard_normal((n, c)).astype(np.float32)
    f1 = rng.standard_normal((n - 500, c)).astype(np.float32)
    pairs = np.stack([rng.permutation(n)[:n_pairs], rng.permutation(n - 500)[:n_pairs]], 1).astype(np.int64)
    f1[pairs[:, 1]] = f0[pairs[:, 0]] + 0.3 * rng.standard_normal((n_pairs, c)).astype(np.float32)
    unit = lambda f: torch.from_numpy(f / np.linalg.norm(f, axis=1, keepdims=True)).to(dev)
    return unit(f0), unit(f1), pairs


def dist(a, b, eps):
    return torch.sqrt((a - b).pow(2).sum(1) + eps)


def torch_contrastive(F0, F1, pairs, neg):
    pos, neg = torch.from_numpy(pairs).to(F0.device), torch.from_numpy(neg).to(F0.device)
    pos_loss = (F0.index_select(0, pos[:, 0]) - F1.index_select(0, pos[:, 1])).pow(2).sum(1)
    neg_loss = F.relu(1.4 - dist(F0.index_select(0, neg[:, 0]), F1.index_select(0, neg[:, 1]), 1e-4)).pow(2)
    return pos_loss.mean() + neg_loss.mean()


def torch_random_triplets(F0, F1, pairs, keys, seed, rand_inds, negatives):
    rp = pairs[rand_inds]
    m = ~np.isin(_hash([rp[:, 0], negatives], seed), keys)
    a, p, n = rp[m, 0], rp[m, 1], negatives[m]
    return dist(F0[a], F1[p], 1e-7), dist(F0[a], F1[n], 1e-7)


def torch_triplet(F0, F1, pairs, draws):
    pos_sel, rand_inds, negatives = draws
    seed = max(len(F0), len(F1))
    rpd, rnd = torch_random_triplets(F0, F1, pairs, _hash(pairs, seed), seed, rand_inds, negatives)
    return F.relu(rpd + 1.4 - rnd).mean()


def torch_hardest(F0, F1, pairs, draws):
    sel0, sel1, pos_sel, rand_inds, negatives = draws
    seed = max(len(F0), len(F1))
    keys = _hash(pairs, seed)
    sample = pairs[pos_sel]
    posF0, posF1 = F0[sample[:, 0]], F1[sample[:, 1]]
    D01 = torch.sqrt((posF0.unsqueeze(1) - F1[sel1].unsqueeze(0)).pow(2).sum(2) + 1e-7)
    D10 = torch.sqrt((posF1.unsqueeze(1) - F0[sel0].unsqueeze(0)).pow(2).sum(2) + 1e-7)
    D01min, D01ind = D01.min(1)
    D10min, D10ind = D10.min(1)
    D01ind, D10ind = sel1[D01ind.cpu().numpy()], sel0[D10ind.cpu().numpy()]
    m0 = torch.from_numpy(~np.isin(_hash([sample[:, 0], D01ind], seed), keys))
    m1 = torch.from_numpy(~np.isin(_hash([D10ind, sample[:, 1]], seed), keys))
    pos_dist = dist(posF0, posF1, 1e-7)
    rpd, rnd = torch_random_triplets(F0, F1, pairs, keys, seed, rand_inds, negatives)
    return F.relu(torch.cat([rpd + 1.4 - rnd, pos_dist[m0] + 1.4 - D01min[m0], pos_dist[m1] + 1.4 - D10min[m1]])).mean()


def measure(fn, F0, F1, reps, inner):
    def call():
        a, b = F0.detach().requires_grad_(True), F1.detach().requires_grad_(True)
        fn(a, b).backward()
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / inner)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        call()
    torch.cuda.set_sync_debug_mode("default")
    return dict(ms=round(float(np.median(ts) * 1e3), 4), ms_min=round(float(min(ts) * 1e3), 4), ms_max=round(float(max(ts) * 1e3), 4),
                launches=launches, host_syncs=sum(1 for x in w if "synchroniz" in str(x.message).lower()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rows", type=int, default=57000)
    ap.add_argument("--pairs", type=int, default=20000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fcgf_losses_bench: needs the GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda:0")
    for c in (32, 128):
        F0, F1, pairs = make_inputs(args.rows, c, args.pairs, dev)
        n0, n1 = len(F0), len(F1)
        np.random.seed(0)
        neg = ContrastiveLoss.generate_rand_negative_pairs(pairs, max(n0, n1), n0, n1)
        sel0, sel1 = np.random.choice(n0, 2048, replace=False), np.random.choice(n1, 2048, replace=False)
        tri = (np.random.choice(len(pairs), 1024, replace=False), np.random.choice(len(pairs), 4096, replace=False),
               np.random.choice(n1, 4096, replace=False))
        con, tl, hl = ContrastiveLoss(), TripletLoss(), HardestTripletLoss()
        rows = {
            "contrastive": (lambda a, b: sum(con.loss(a, b, pairs, neg)), lambda a, b: torch_contrastive(a, b, pairs, neg)),
            "triplet": (lambda a, b: tl.triplet_loss(a, b, pairs, draws=tri)[0], lambda a, b: torch_triplet(a, b, pairs, tri)),
            "hardest_triplet": (lambda a, b: hl.triplet_loss(a, b, pairs, draws=(sel0, sel1) + tri)[0],
                                lambda a, b: torch_hardest(a, b, pairs, (sel0, sel1) + tri)),
        }
        for name, (hip, ref) in rows.items():
            with torch.no_grad():
                got, want = float(hip(F0, F1)), float(ref(F0, F1))
            out = dict(loss=name, c=c, rows=[n0, n1], value_hip=got, value_torch=want, hip=measure(hip, F0, F1, args.reps, args.inner),
                       torch_fp32=measure(ref, F0, F1, args.reps, args.inner))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

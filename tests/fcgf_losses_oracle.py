"""Float64 restatement of the FCGF trainers' random-negative contrastive, triplet and hardest-triplet losses
(FCGF_APR/lib/trainer.py:192-206, :254-267, :532-579, :658-731), on CPU torch, with autograd for the gradients.

Held to the reference's own text by tests/test_fcgf_losses_cpu.py (fixture tests/golden/fcgf_losses_ref.npz); the GPU tests
compare the HIP path with it.  Every function takes the draws explicitly (`draw_*` replays them from np.random in the
reference's order) and returns a dict of float64 / integer NumPy arrays.
"""
import numpy as np
import torch


def _hash(arr, M):
    """Pair key i + j * M (util/misc.py:6-18) for an [N, 2] array or a pair of vectors."""
    a, b = (arr[:, 0], arr[:, 1]) if isinstance(arr, np.ndarray) else arr
    return np.asarray(a, dtype=np.int64) + np.asarray(b, dtype=np.int64) * np.int64(M)


def generate_rand_negative_pairs(positive_pairs, hash_seed, N0, N1, N_neg=0):
    positive_pairs = np.asarray(positive_pairs, dtype=np.int64)
    if N_neg < 1:
        N_neg = positive_pairs.shape[0] * 2
    neg_pairs = np.floor(np.random.rand(int(N_neg), 2) * np.array([[N0, N1]])).astype(np.int64)
    mask = np.isin(_hash(neg_pairs, hash_seed), _hash(positive_pairs, hash_seed))
    return neg_pairs[~mask]


def draw_triplet(N0, N1, num_pairs, num_pos, num_rand_triplet):
    pos_sel = np.random.choice(num_pairs, num_pos, replace=False) if num_pairs > num_pos else None
    rand_inds = np.random.choice(num_pairs, min(num_pairs, num_rand_triplet), replace=False)
    negatives = np.random.choice(N1, min(N1, num_rand_triplet), replace=False)
    return pos_sel, rand_inds, negatives


def draw_hardest(N0, N1, num_pairs, num_pos, num_hn_samples, num_rand_triplet):
    sel0 = np.random.choice(N0, min(N0, num_hn_samples), replace=False)
    sel1 = np.random.choice(N1, min(N1, num_hn_samples), replace=False)
    return (sel0, sel1) + draw_triplet(N0, N1, num_pairs, num_pos, num_rand_triplet)


def _leaves(F0, F1):
    F0 = torch.tensor(np.asarray(F0, dtype=np.float64), requires_grad=True)
    F1 = torch.tensor(np.asarray(F1, dtype=np.float64), requires_grad=True)
    return F0, F1


def _grads(out, F0, F1, tag=""):
    g0, g1 = torch.autograd.grad(out, (F0, F1), retain_graph=True, allow_unused=True)
    z = lambda g, F: (torch.zeros_like(F) if g is None else g).numpy()
    return {f"gF0{tag}": z(g0, F0), f"gF1{tag}": z(g1, F1)}


def _dist(A, B, eps):
    return torch.sqrt((A - B).pow(2).sum(1) + eps)


def contrastive(F0, F1, pos_pairs, neg_pairs, neg_thresh=1.4):
    """-> pos, neg (means; NaN over nothing) and the gradient of each with respect to F0 / F1."""
    F0, F1 = _leaves(F0, F1)
    pos_pairs, neg_pairs = (torch.from_numpy(np.asarray(a, dtype=np.int64).reshape(-1, 2)) for a in (pos_pairs, neg_pairs))
    pos = (F0[pos_pairs[:, 0]] - F1[pos_pairs[:, 1]]).pow(2).sum(1).mean()
    neg = torch.relu(neg_thresh - _dist(F0[neg_pairs[:, 0]], F1[neg_pairs[:, 1]], 1e-4)).pow(2).mean()
    out = {"pos": pos.item(), "neg": neg.item()}
    out.update(_grads(pos, F0, F1, "_pos") if len(pos_pairs) else {})
    out.update(_grads(neg, F0, F1, "_neg") if len(neg_pairs) else {})
    return out


def _random_triplets(F0, F1, pairs, keys, hash_seed, rand_inds, negatives):
    rand_inds, negatives = np.asarray(rand_inds, dtype=np.int64), np.asarray(negatives, dtype=np.int64)
    if len(rand_inds) != len(negatives):
        raise ValueError(f"operands could not be broadcast together with shapes ({len(rand_inds)},) ({len(negatives)},)")
    rand_pairs = pairs[rand_inds]
    rand_mask = ~np.isin(_hash([rand_pairs[:, 0], negatives], hash_seed), keys)
    a, p, n = (torch.from_numpy(v[rand_mask]) for v in (rand_pairs[:, 0], rand_pairs[:, 1], negatives))
    return rand_mask, _dist(F0[a], F1[p], 1e-7), _dist(F0[a], F1[n], 1e-7)


def triplet(F0, F1, positive_pairs, draws, neg_thresh=1.4):
    N0, N1 = len(F0), len(F1)
    F0, F1 = _leaves(F0, F1)
    pairs = np.asarray(positive_pairs, dtype=np.int64)
    pos_sel, rand_inds, negatives = draws
    hash_seed = max(N0, N1)
    keys = _hash(pairs, hash_seed)
    sample = torch.from_numpy(pairs if pos_sel is None else pairs[np.asarray(pos_sel)])
    pos_dist = _dist(F0[sample[:, 0]], F1[sample[:, 1]], 1e-7)
    rand_mask, rpd, rnd = _random_triplets(F0, F1, pairs, keys, hash_seed, rand_inds, negatives)
    hinge = rpd + neg_thresh - rnd
    loss = torch.relu(hinge).mean()
    out = {"loss": loss.item(), "pos_dist": pos_dist.mean().item(), "neg_dist": rnd.mean().item(), "rand_mask": rand_mask,
           "hinge": hinge.detach().numpy()}
    out.update(_grads(loss, F0, F1) if rand_mask.any() else {"gF0": np.zeros(F0.shape), "gF1": np.zeros(F1.shape)})
    return out


def hardest_triplet(F0, F1, positive_pairs, draws, neg_thresh=1.4, mined=None):
    """`mined`: (D01ind, D10ind) rows of the full clouds to use in place of the float64 arg-mins (a test that pins the
    device's choice); D01 / D10, the float64 distance matrices, come back either way."""
    N0, N1 = len(F0), len(F1)
    F0, F1 = _leaves(F0, F1)
    pairs = np.asarray(positive_pairs, dtype=np.int64)
    sel0, sel1, pos_sel, rand_inds, negatives = draws
    sel0, sel1 = np.asarray(sel0, dtype=np.int64), np.asarray(sel1, dtype=np.int64)
    hash_seed = max(N0, N1)
    keys = _hash(pairs, hash_seed)
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel)]
    pos0, pos1 = sample[:, 0], sample[:, 1]
    posF0, posF1 = F0[torch.from_numpy(pos0)], F1[torch.from_numpy(pos1)]
    with torch.no_grad():
        D01 = torch.sqrt((posF0.unsqueeze(1) - F1[torch.from_numpy(sel1)].unsqueeze(0)).pow(2).sum(2) + 1e-7)
        D10 = torch.sqrt((posF1.unsqueeze(1) - F0[torch.from_numpy(sel0)].unsqueeze(0)).pow(2).sum(2) + 1e-7)
    if mined is None:
        D01ind, D10ind = sel1[D01.min(1)[1].numpy()], sel0[D10.min(1)[1].numpy()]
    else:
        D01ind, D10ind = (np.asarray(m, dtype=np.int64) for m in mined)
    D01min = _dist(posF0, F1[torch.from_numpy(D01ind)], 1e-7)
    D10min = _dist(posF1, F0[torch.from_numpy(D10ind)], 1e-7)
    mask0 = ~np.isin(_hash([pos0, D01ind], hash_seed), keys)
    mask1 = ~np.isin(_hash([D10ind, pos1], hash_seed), keys)
    pos_dist = _dist(posF0, posF1, 1e-7)
    rand_mask, rpd, rnd = _random_triplets(F0, F1, pairs, keys, hash_seed, rand_inds, negatives)
    m0, m1 = torch.from_numpy(mask0), torch.from_numpy(mask1)
    hinge = torch.cat([rpd + neg_thresh - rnd, pos_dist[m0] + neg_thresh - D01min[m0], pos_dist[m1] + neg_thresh - D10min[m1]])
    loss = torch.relu(hinge).mean()
    out = {"loss": loss.item(), "pos_dist": pos_dist.mean().item(), "neg_dist": ((D01min.mean() + D10min.mean()) / 2).item(),
           "rand_mask": rand_mask, "mask0": mask0, "mask1": mask1, "D01ind": D01ind, "D10ind": D10ind,
           "D01": D01.numpy(), "D10": D10.numpy(), "hinge": hinge.detach().numpy()}
    out.update(_grads(loss, F0, F1) if len(hinge) else {"gF0": np.zeros(F0.shape), "gF1": np.zeros(F1.shape)})
    return out


# ---- the fixture (tests/golden/fcgf_losses_ref.npz) -----------------------------------------------------------------------
CASES = ("c32", "c128")


def load_fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcgf_losses_ref.npz"))


def fixture_grad(z, key, n_rows):
    """A stored gradient: float32 + float16 remainder * 2^-30 on its non-zero rows -> float64 [n_rows, c]."""
    hi, lo = z[key + "_hi"], z[key + "_lo"]
    g = np.zeros((n_rows, hi.shape[1]))
    g[z[key + "_rows"]] = hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -30
    return g


def fixture_draws(z, tag, kind):
    """The stored draws of one loss in the order its `prepare` takes them (pos_sel of length 0 = not drawn)."""
    get = lambda k: z[f"{tag}_{kind}_{k}"]
    pos_sel = get("pos_sel") if len(get("pos_sel")) else None
    if kind == "tri":
        return pos_sel, get("rand_inds"), get("negatives")
    return get("sel0"), get("sel1"), pos_sel, get("rand_inds"), get("negatives")


# ---- the collates (FCGF_APR/lib/data_loaders.py:26-78, lib/complement_data_loader.py:1282-1333) --------------------------
def collate_items():
    """Three 8-tuples as pair_sample returns them, on the CPU: matches as a list, none at all (the item is skipped but
    moves the head), and as an array."""
    def item(n0, n1, matches, k):
        rng = np.random.default_rng(k)
        f = lambda n: torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
        c = lambda n: torch.from_numpy(rng.integers(-50, 50, (n, 3)).astype(np.int32))
        return (f(n0), f(n1), c(n0), c(n1), torch.ones((n0, 1)), torch.ones((n1, 1)), matches, np.eye(4) * (k + 1) + 0.125 * k)
    return [item(7, 9, [(0, 1), (6, 8)], 0), item(11, 13, [], 1), item(17, 19, np.array([[2, 3], [16, 18]]), 2)]


def flatten_collated(batch, prefix):
    """A collated dict as numeric arrays: tensors as they are (the dtype travels), a tuple of tensors as its concatenation
    plus `_lens` (and `_is_tuple`), len_batch as an int64 array; `_keys`: the dict's key order as indices into sorted()."""
    out = {}
    for k, v in batch.items():
        if torch.is_tensor(v):
            out[f"{prefix}_{k}"] = v.numpy()
        elif k == "len_batch":
            out[f"{prefix}_{k}"] = np.asarray(v, dtype=np.int64)
        else:
            out[f"{prefix}_{k}"] = torch.cat(list(v), 0).numpy()
            out[f"{prefix}_{k}_lens"] = np.array([len(x) for x in v], dtype=np.int64)
            out[f"{prefix}_{k}_is_tuple"] = np.array(isinstance(v, tuple))
    out[f"{prefix}_keys"] = np.array([sorted(batch).index(k) for k in batch], dtype=np.int64)
    return out

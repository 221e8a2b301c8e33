"""Reference-pinned fixture of the FCGF trainers' contrastive, triplet and hardest-triplet losses:
tests/golden/fcgf_losses_ref.npz.

Run where the reference checkout is present:   python tests/golden/make_fcgf_losses_ref_golden.py

Same rule as make_fcgf_ref_golden.py: `pdist` (FCGF_APR/lib/metrics.py:22-29), `_hash` (util/misc.py:6-18),
`generate_rand_negative_pairs` (lib/trainer.py:192-206), the statements :254-267 of ContrastiveLossTrainer._train_epoch and
both `triplet_loss` bodies (:532-579, :658-731) are cut out of the reference's files with `ast`, compiled unchanged and
executed on seeded inputs; the locals of the two bodies (masks, mined rows) are read off their frames when they return.
Two legs per case: fp32 (the text as it stands) and fp64 (the same text on float64 features, the yardstick).  Stored, as
numeric arrays only: the inputs, the draws (the seed replayed), the returned values, masks and mined rows of the fp64 leg,
its gradients' non-zero rows, the fp32 leg's values and the relative L2 distance of its gradients from the fp64 leg's, and
the next value of the NumPy stream after each call; and what the reference's two pair collates return on the items of
tests/fcgf_losses_oracle.py:collate_items.  A gradient is stored as float32 plus a float16 remainder scaled by
2^30 (`fixture_grad` in tests/fcgf_losses_oracle.py puts them together: 2^-35 relative, a quarter less file than float64).

Cases
  c32    N0 = 700, N1 = 650, 460 positive pairs of which 40 rows of F0 are paired twice; num_pos = num_rand_triplet = 256,
         num_hn_samples = 128.  Features: a smooth function of the position plus noise, unit rows.
  c128   N0 = 40, N1 = 36, 30 pairs (4 rows twice); 24 / 24 / 16.  Features linear in the position (rows on opposite sides of
         the box are further apart than 1.4 + a positive distance: with 128 channels the sine features never are).
Planted per case: two equal rows of F1 inside sel1 where one of them is a nearest negative (an exact tie: the lower index
of the sub-sample wins).  Checked here, so that the GPU test needs no exclusion list: outside that tie the top-two gap of
every nearest-negative row is above fp32 rounding, no hinge argument lies within 1e-5 of 0, the fp32 leg takes every
decision as the fp64 leg does, and on each side at least one mined negative is a true positive (mask false).
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import fcgf_losses_oracle as O  # noqa: E402
REF = "/root/reference/FCGF_APR"
SEED = 77
CASES = {"c32": dict(N0=700, N1=650, c=32, single=380, twice=40, num_pos=256, num_hn=128, num_rand=256),
         "c128": dict(N0=40, N1=36, c=128, single=22, twice=4, num_pos=24, num_hn=16, num_rand=24, linear=True)}


def _tree(rel):
    src = open(os.path.join(REF, rel), encoding="utf-8").read()
    return src, ast.parse(src)


def _defs(rel, names, ns, cls=None):
    src, tree = _tree(rel)
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    found = {n.name: textwrap.dedent("\n".join(src.splitlines()[n.lineno - 1:n.end_lineno]))
             for n in body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert set(found) == set(names), set(names) - set(found)
    out = {}
    for name in names:
        exec(compile(found[name], f"{REF}/{rel}:{name}", "exec"), ns)
        out[name] = ns[name]
    return out


def _loop_statements():
    """trainer.py:254-267: the eight assignments from `neg0 = ...` to `neg_loss_mean = ...`, first in source order."""
    src, tree = _tree("lib/trainer.py")
    lines = src.splitlines()
    out = []
    for name in ("neg0", "neg1", "pos0", "pos1", "pos_loss", "neg_loss", "pos_loss_mean", "neg_loss_mean"):
        hits = sorted((n for n in ast.walk(tree) if isinstance(n, ast.Assign) and len(n.targets) == 1 and
                       isinstance(n.targets[0], ast.Name) and n.targets[0].id == name), key=lambda n: n.lineno)
        n = hits[0]
        assert 254 <= n.lineno <= 267, (name, n.lineno)
        out.append(textwrap.dedent("\n".join(lines[n.lineno - 1:n.end_lineno])))
    return "\n".join(out)


def call_with_locals(fn, *args, **kw):
    box = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is fn.__code__:
            box.update(frame.f_locals)
    sys.setprofile(prof)
    try:
        ret = fn(*args, **kw)
    finally:
        sys.setprofile(None)
    return ret, box


def reference():
    ns = {"np": np, "torch": torch, "F": F}
    _defs("lib/metrics.py", ["pdist"], ns)
    _defs("util/misc.py", ["_hash"], ns)
    fns = _defs("lib/trainer.py", ["generate_rand_negative_pairs"], ns, cls="ContrastiveLossTrainer")
    fns["triplet"] = _defs("lib/trainer.py", ["triplet_loss"], dict(ns), cls="TripletLossTrainer")["triplet_loss"]
    fns["hardest"] = _defs("lib/trainer.py", ["triplet_loss"], dict(ns), cls="HardestTripletLossTrainer")["triplet_loss"]
    fns["loop"] = compile(_loop_statements(), f"{REF}/lib/trainer.py:254-267", "exec")
    fns["ns"] = ns
    return fns


def make_inputs(rng, N0, N1, c, single, twice, linear=False, **_):
    """Positions in a box; F1's paired rows sit next to their partner; features smooth in the position plus noise."""
    x0 = rng.uniform(-10, 10, (N0, 3))
    x1 = rng.uniform(-10, 10, (N1, 3))
    i = rng.permutation(N0)[:single + twice]
    j = rng.permutation(N1)[:single + 2 * twice]
    pairs = np.concatenate([np.stack([i, j[:single + twice]], 1), np.stack([i[:twice], j[single + twice:]], 1)])
    x1[pairs[:, 1]] = x0[pairs[:, 0]] + 0.1 * rng.standard_normal((len(pairs), 3))
    pairs = pairs[rng.permutation(len(pairs))].astype(np.int64)
    W = rng.standard_normal((3, c)) * 0.35
    ph = rng.uniform(0, 2 * np.pi, c)

    def feats(x):
        f = (x @ W / 4 if linear else np.sin(x @ W + ph)) + 0.06 * rng.standard_normal((len(x), c))
        return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)
    return feats(x0), feats(x1), pairs


def replay_triplet(N0, N1, npairs, num_pos, num_rand):
    np.random.seed(SEED)
    pos_sel = np.random.choice(npairs, num_pos, replace=False) if npairs > num_pos else np.zeros(0, np.int64)
    rand_inds = np.random.choice(npairs, min(npairs, num_rand), replace=False)
    negatives = np.random.choice(N1, min(N1, num_rand), replace=False)
    return pos_sel, rand_inds, negatives, np.random.rand()


def replay_hardest(N0, N1, npairs, num_pos, num_hn, num_rand):
    np.random.seed(SEED)
    sel0 = np.random.choice(N0, min(N0, num_hn), replace=False)
    sel1 = np.random.choice(N1, min(N1, num_hn), replace=False)
    pos_sel = np.random.choice(npairs, num_pos, replace=False) if npairs > num_pos else np.zeros(0, np.int64)
    rand_inds = np.random.choice(npairs, min(npairs, num_rand), replace=False)
    negatives = np.random.choice(N1, min(N1, num_rand), replace=False)
    return sel0, sel1, pos_sel, rand_inds, negatives, np.random.rand()


def split(g):
    hi = g.astype(np.float32)
    return hi, ((g - hi.astype(np.float64)) * 2.0 ** 30).astype(np.float16)


def store_grad(out, key, g):
    rows = np.flatnonzero(np.abs(g).sum(1) > 0)
    out[key + "_rows"] = rows.astype(np.int32)
    out[key + "_hi"], out[key + "_lo"] = split(g[rows])


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def plant_tie(F0, F1, pairs, sel1, pos_sel):
    """Make the nearest negative of one sampled positive exist twice in F1[sel1]."""
    sample = pairs[pos_sel] if len(pos_sel) else pairs
    A, B = F0[sample[:, 0]].astype(np.float64), F1[sel1].astype(np.float64)
    k = ((A[:, None, :] - B[None, :, :]) ** 2).sum(2).argmin(1)
    used = set(pairs[:, 1].tolist())
    free = [q for q in range(len(sel1)) if q not in set(k.tolist())]
    free = [q for q in free if sel1[q] not in used] or free
    row = len(sample) // 2
    F1[sel1[free[-1]]] = F1[sel1[k[row]]]
    return row, sorted((int(k[row]), free[-1]))


def run_case(ref, tag, cfg, out):
    rng = np.random.default_rng(2025 + cfg["c"])
    N0, N1 = cfg["N0"], cfg["N1"]
    F0, F1, pairs = make_inputs(rng, **cfg)
    num_pos, num_hn, num_rand = cfg["num_pos"], cfg["num_hn"], cfg["num_rand"]
    hd = replay_hardest(N0, N1, len(pairs), num_pos, num_hn, num_rand)
    tie_row, tie_cols = plant_tie(F0, F1, pairs, hd[1], hd[2])
    out[f"{tag}_F0"], out[f"{tag}_F1"], out[f"{tag}_pairs"] = F0, F1, pairs
    out[f"{tag}_args"] = np.array([num_pos, num_hn, num_rand])
    out[f"{tag}_tie"] = np.array([tie_row] + tie_cols)
    stub = types.SimpleNamespace(neg_thresh=1.4, pos_thresh=0.1, neg_weight=1)
    tpairs = torch.from_numpy(pairs)

    def legs(fn):
        res = {}
        for dt in (torch.float64, torch.float32):
            a, b = torch.tensor(F0, dtype=dt, requires_grad=True), torch.tensor(F1, dtype=dt, requires_grad=True)
            np.random.seed(SEED)
            res[dt] = fn(a, b) + (a, b, np.random.rand())
        return res[torch.float64], res[torch.float32]

    def grads(loss, a, b):
        ga, gb = torch.autograd.grad(loss, (a, b))
        return ga.double().numpy(), gb.double().numpy()

    def decisions_agree(l64, l32, names):
        for nme in names:
            x, y = l64[nme], l32[nme]
            x, y = (v.numpy() if torch.is_tensor(v) else np.asarray(v) for v in (x, y))
            assert np.array_equal(x, y), f"{tag}: the fp32 leg decides {nme} differently"

    # ---- random-negative contrastive ---------------------------------------------------------------------------------
    def contrastive(a, b):
        neg = ref["generate_rand_negative_pairs"](stub, tpairs, max(N0, N1), N0, N1)
        ns = dict(ref["ns"], F0=a, F1=b, self=stub, iter_size=1, pos_pairs=tpairs.long(), neg_pairs=torch.from_numpy(neg).long())
        exec(ref["loop"], ns)
        return (ns["pos_loss_mean"], ns["neg_loss_mean"], neg, ns["neg_loss"])
    (p64, n64, neg, nl, a, b, nxt), (p32, n32, neg32, _, a32, b32, _) = legs(contrastive)
    assert np.array_equal(neg, neg32)
    dneg = np.sqrt(((F0[neg[:, 0]].astype(np.float64) - F1[neg[:, 1]]) ** 2).sum(1) + 1e-4)
    assert np.abs(1.4 - dneg).min() > 1e-5, f"{tag}: a contrastive hinge within 1e-5 of 0"
    assert 0 < (nl > 0).sum().item() < len(neg)
    out[f"{tag}_con_neg_pairs"], out[f"{tag}_con_next"] = neg, np.array(nxt)
    out[f"{tag}_con_values"] = np.array([p64.item(), n64.item()])
    out[f"{tag}_con_values32"] = np.array([p32.item(), n32.item()], dtype=np.float32)
    g64, g32 = grads(p64 + stub.neg_weight * n64, a, b), grads(p32 + stub.neg_weight * n32, a32, b32)
    store_grad(out, f"{tag}_con_gF0", g64[0])
    store_grad(out, f"{tag}_con_gF1", g64[1])
    out[f"{tag}_con_grad32_rel"] = np.array([rel_l2(g32[0], g64[0]), rel_l2(g32[1], g64[1])])

    # ---- triplet -----------------------------------------------------------------------------------------------------------
    def trip(a, b):
        ret, loc = call_with_locals(ref["triplet"], stub, a, b, tpairs, num_pos=num_pos, num_hn_samples=None,
                                    num_rand_triplet=num_rand)
        return (ret, loc)
    (r64, l64, a, b, nxt), (r32, l32, a32, b32, _) = legs(trip)
    td = replay_triplet(N0, N1, len(pairs), num_pos, num_rand)
    assert nxt == td[3]
    decisions_agree(l64, l32, ["rand_mask", "rand_inds", "negatives"])
    assert np.array_equal(l64["rand_inds"], td[1]) and np.array_equal(l64["rand_mask"].shape, td[2].shape)
    hinge = (l64["rand_pos_dist"] + 1.4 - l64["rand_neg_dist"]).detach().numpy()
    print(tag, "triplet hinge: min abs", np.abs(hinge).min(), "active", int((hinge > 0).sum()), "of", len(hinge))
    assert np.abs(hinge).min() > 1e-5 and 0 < (hinge > 0).sum() < len(hinge), f"{tag}: triplet hinges degenerate"
    assert 0 < l64["rand_mask"].sum() <= len(td[1])
    out[f"{tag}_tri_pos_sel"], out[f"{tag}_tri_rand_inds"], out[f"{tag}_tri_negatives"] = td[0], td[1], td[2]
    out[f"{tag}_tri_next"] = np.array(td[3])
    out[f"{tag}_tri_rand_mask"] = np.asarray(l64["rand_mask"])
    out[f"{tag}_tri_values"] = np.array([float(v.detach()) if torch.is_tensor(v) else float(v) for v in r64])
    out[f"{tag}_tri_values32"] = np.array([float(v.detach()) if torch.is_tensor(v) else float(v) for v in r32], dtype=np.float32)
    g64, g32 = grads(r64[0], a, b), grads(r32[0], a32, b32)
    store_grad(out, f"{tag}_tri_gF0", g64[0])
    store_grad(out, f"{tag}_tri_gF1", g64[1])
    out[f"{tag}_tri_grad32_rel"] = np.array([rel_l2(g32[0], g64[0]), rel_l2(g32[1], g64[1])])
    print(tag, "triplet", out[f"{tag}_tri_values"], "F0 rows", len(out[f"{tag}_tri_gF0_rows"]))

    # ---- hardest triplet ---------------------------------------------------------------------------------------------------
    def hard(a, b):
        ret, loc = call_with_locals(ref["hardest"], stub, a, b, tpairs, num_pos=num_pos, num_hn_samples=num_hn,
                                    num_rand_triplet=num_rand)
        return (ret, loc)
    (r64, l64, a, b, nxt), (r32, l32, a32, b32, _) = legs(hard)
    assert nxt == hd[5]
    for nme, want in zip(("sel0", "sel1", "rand_inds"), (hd[0], hd[1], hd[3])):
        assert np.array_equal(l64[nme], want)
    decisions_agree(l64, l32, ["mask0", "mask1", "rand_mask", "D01ind", "D10ind"])
    m0, m1 = l64["mask0"].numpy(), l64["mask1"].numpy()
    assert (~m0).any() and (~m1).any() and m0.any() and m1.any(), f"{tag}: no mined negative that is a true positive on a side"
    # the top-two gap of every nearest-negative row, outside the planted tie; the tie goes to the lower sub-sample index
    for D, name in ((l64["D01"].detach().numpy(), "D01"), (l64["D10"].detach().numpy(), "D10")):
        two = np.sort(D ** 2, axis=1)[:, :2]
        gap = two[:, 1] - two[:, 0]
        tied = np.zeros(len(D), bool)
        if name == "D01":
            tied = np.isin(D.argmin(1), tie_cols) & (D[:, tie_cols[0]] == D[:, tie_cols[1]])
            assert tied[tie_row] and (D.argmin(1)[tied] == tie_cols[0]).all()
            assert (l64["D01ind"][tied] == hd[1][tie_cols[0]]).all()
        assert (gap > 4 * cfg["c"] * 2.0 ** -24 * two[:, 1])[~tied].all(), f"{tag}: a {name} top-two gap within fp32 rounding"
    pd_, d01, d10 = l64["pos_dist"], l64["D01min"], l64["D10min"]
    hinge = torch.cat([l64["rand_pos_dist"] + 1.4 - l64["rand_neg_dist"], pd_[l64["mask0"]] + 1.4 - d01[l64["mask0"]],
                       pd_[l64["mask1"]] + 1.4 - d10[l64["mask1"]]]).detach().numpy()
    print(tag, "hardest hinge: min abs", np.abs(hinge).min(), "active", int((hinge > 0).sum()), "of", len(hinge))
    assert np.abs(hinge).min() > 1e-5 and 0 < (hinge > 0).sum() < len(hinge), f"{tag}: hardest hinges degenerate"
    for k, v in zip(("sel0", "sel1", "pos_sel", "rand_inds", "negatives"), hd[:5]):
        out[f"{tag}_hard_{k}"] = v
    out[f"{tag}_hard_next"] = np.array(hd[5])
    for k in ("mask0", "mask1", "rand_mask", "D01ind", "D10ind"):
        out[f"{tag}_hard_{k}"] = np.asarray(l64[k].numpy() if torch.is_tensor(l64[k]) else l64[k])
    out[f"{tag}_hard_values"] = np.array([float(v.detach()) if torch.is_tensor(v) else float(v) for v in r64])
    out[f"{tag}_hard_values32"] = np.array([float(v.detach()) if torch.is_tensor(v) else float(v) for v in r32], dtype=np.float32)
    g64, g32 = grads(r64[0], a, b), grads(r32[0], a32, b32)
    store_grad(out, f"{tag}_hard_gF0", g64[0])
    store_grad(out, f"{tag}_hard_gF1", g64[1])
    out[f"{tag}_hard_grad32_rel"] = np.array([rel_l2(g32[0], g64[0]), rel_l2(g32[1], g64[1])])
    print(tag, "hardest", out[f"{tag}_hard_values"], "F0 rows", len(out[f"{tag}_hard_gF0_rows"]),
          "masked", int((~m0).sum()), int((~m1).sum()))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same bytes on every run."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def run_collates(out):
    """collate_pair_fn (lib/data_loaders.py:26-78) and collate_debug_pair_fn (lib/complement_data_loader.py:1282-1333),
    executed unchanged on O.collate_items() with the project's sparse_collate behind the name `ME`."""
    from apr_amd import MinkowskiEngine as ME
    for rel, name in (("lib/data_loaders.py", "collate_pair_fn"), ("lib/complement_data_loader.py", "collate_debug_pair_fn")):
        fn = _defs(rel, [name], {"np": np, "torch": torch, "ME": ME})[name]
        out.update(O.flatten_collated(fn(O.collate_items()), name))


def main():
    ref = reference()
    out = {}
    run_collates(out)
    for tag, cfg in CASES.items():
        run_case(ref, tag, cfg, out)
    path = os.path.join(HERE, "fcgf_losses_ref.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())

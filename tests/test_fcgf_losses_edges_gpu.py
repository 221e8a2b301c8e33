"""The pair-list losses at the edges of their kernels, row by row against the float64 oracle (tests/fcgf_losses_oracle.py).

The HIP path's mined rows are pinned into the oracle after each was checked to be a float64 arg-min up to fp32 rounding;
masks must then be equal, values agree within the value bar of tests/test_fcgf_losses_gpu.py (`_value`), and every gradient row
within its own bound: a row that k pair entries touch sums k contributions of norm <= w / count each (w = 1 for a triplet
pair, whose direction (x - y) / d is at most a unit vector; 2 * max(|x - y|, neg_thresh) for the contrastive terms), and a
contribution carries the rounding of a c-term fp32 sum of squares, a square root, a division and three products: at most
(c + 16) * 2^-24 relative; adding the k contributions one after the other in fp32 rounds each partial sum, itself at most
k * w / count, once more (the recursive-summation bound).  Row bound = k * w / count * (c + 16 + k) * 2^-24; a row in no
active term is exactly zero.

  one      N0 = 5, N1 = 3, c = 4, one triplet: grids and reductions at one element
  run      N0 = N1 = 64, c = 32, row 0 of F0 in 300 positive pairs, 20 rows of either cloud in no term
  tails    c = 128, 1000 contrastive terms; 333 / 333 / 77 for the hardest triplets
  bigkey   N0 = N1 = 50 000, c = 4, partners at j >= 46 341: i + j * hash_seed is above 2^31
  empty    a side whose every mined negative is its true positive; every random triplet filtered; no negative pair
  zeros    inactive hinges, a pair listed twice, two identical rows (d^2 = 0: the gradient stays finite)
  refused  c = 30, CPU tensors, unequal triplet lengths: an exception before any launch
"""
import ctypes as C

import numpy as np
import pytest
import torch

from apr_amd import _lib
from tests import fcgf_losses_oracle as O
from tests.test_fcgf_losses_gpu import BARS
from tests.test_scratch_guard_gpu import _guarded

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _unit(rng, n, c):
    f = rng.standard_normal((n, c))
    return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)


def _leaves(F0, F1, dev):
    return (torch.from_numpy(F0).to(dev).requires_grad_(True), torch.from_numpy(F1).to(dev).requires_grad_(True))


WORST = {"value": 0.0}


def _value(got, want, name, hinge=False):
    """A mean of distances: relative to itself.  A mean of hinges: every term is a difference of neg_thresh (+ a distance)
    and a distance, so its rounding is relative to those operands, not to the possibly small difference: relative to
    |value| + neg_thresh."""
    got = float(got.detach())
    if np.isnan(want):
        assert np.isnan(got), (name, got)
    else:
        scale = abs(want) + (1.4 if hinge else 0.0)
        if scale != 0:
            WORST["value"] = max(WORST["value"], abs(got - want) / scale)
        assert abs(got - want) <= BARS["value"] * scale, (name, got, want)


def _rows(F, ref, touches, w_over_count, name):
    """every row of the gradient within its bound; `touches`: the rows of the gradient-carrying pair entries"""
    g = F.grad.cpu().double().numpy()
    assert np.isfinite(g).all(), name
    c = g.shape[1]
    k = np.bincount(np.asarray(touches, dtype=np.int64), minlength=len(g))
    err = np.linalg.norm(g - ref, axis=1)
    bound = k * w_over_count * (c + 16 + k) * U
    assert not g[k == 0].any(), f"{name}: a row in no active term has a gradient"
    bad = np.flatnonzero(err > bound)
    assert len(bad) == 0, (name, bad[:8], err[bad[:8]], bound[bad[:8]])
    return float((err[k > 0] / bound[k > 0]).max()) if (k > 0).any() else 0.0


def _contrastive(dev, F0, F1, pos, neg, name):
    from apr_amd.fcgf.lib.trainer import ContrastiveLoss
    m = ContrastiveLoss()
    a, b = _leaves(F0, F1, dev)
    out = m.loss(a, b, pos, neg)
    ref = O.contrastive(F0, F1, pos, neg)
    _value(out[0], ref["pos"], name + " pos")
    _value(out[1], ref["neg"], name + " neg", hinge=True)
    (out[0] + out[1]).backward()          # an empty group's NaN mean must leave the other group's gradient alone
    z0, z1 = np.zeros(F0.shape), np.zeros(F1.shape)
    r0 = ref.get("gF0_pos", z0) + ref.get("gF0_neg", z0)
    r1 = ref.get("gF1_pos", z1) + ref.get("gF1_neg", z1)
    pos, neg = np.asarray(pos).reshape(-1, 2), np.asarray(neg).reshape(-1, 2)
    dmax = max(np.linalg.norm(F0[p[:, 0]].astype(np.float64) - F1[p[:, 1]], axis=1).max() if len(p) else 0 for p in (pos, neg))
    w = 2 * max(dmax, 1.4) / max(min(len(pos), len(neg) or len(pos)), 1)
    dn = np.sqrt(((F0[neg[:, 0]].astype(np.float64) - F1[neg[:, 1]]) ** 2).sum(1) + 1e-4)
    act = dn < 1.4 - 1e-5
    worst = [_rows(a, r0, np.concatenate([pos[:, 0], neg[act, 0]]), w, name + " dF0"),
             _rows(b, r1, np.concatenate([pos[:, 1], neg[act, 1]]), w, name + " dF1")]
    print(f"[{name}] values {float(out[0].detach()):.6g} {float(out[1].detach()):.6g}; worst row error / bound {max(worst):.3f}; "
          f"worst value error so far {WORST['value']:.2e}")
    return out, a, b


def _triplets(dev, kind, F0, F1, pairs, draws, name, **kw):
    from apr_amd.fcgf.lib.trainer import HardestTripletLoss, TripletLoss
    m = TripletLoss() if kind == "tri" else HardestTripletLoss()
    a, b = _leaves(F0, F1, dev)
    out = m.triplet_loss(a, b, pairs, draws=draws, **kw)
    out[0].backward()
    got = {k: v.cpu().numpy() for k, v in m.last.mined().items()}
    pairs = np.asarray(pairs, dtype=np.int64)
    c = F0.shape[1]
    if kind == "tri":
        ref = O.triplet(F0, F1, pairs, draws)
        pos_sel, rand_inds, negatives = draws
    else:
        sel0, sel1, pos_sel, rand_inds, negatives = draws
        ref = O.hardest_triplet(F0, F1, pairs, draws, mined=(got["D01ind"], got["D10ind"]))
        # each mined row is an arg-min of the float64 distances up to the fp32 rounding of a c-term sum of squares
        for D, sel, ind in ((ref["D01"], sel1, got["D01ind"]), (ref["D10"], sel0, got["D10ind"])):
            col = {int(r): q for q, r in reversed(list(enumerate(sel)))}
            d2 = D ** 2
            mine = d2[np.arange(len(D)), [col[int(r)] for r in ind]]
            assert (mine <= d2.min(1) + 4 * (c + 4) * U * d2.max(1)).all(), name
        for k in ("mask0", "mask1"):
            assert np.array_equal(got[k].astype(bool), ref[k]), (name, k)
    assert np.array_equal(got["rand_mask"].astype(bool), ref["rand_mask"]), name
    for o, k in zip(out, ("loss", "pos_dist", "neg_dist")):
        _value(o, ref[k], f"{name} {k}", hinge=k == "loss")
    sample = pairs if pos_sel is None else pairs[np.asarray(pos_sel)]
    rp, rm = pairs[np.asarray(rand_inds)], ref["rand_mask"]
    n_rand = int(rm.sum())
    hinge = ref["hinge"]
    assert np.abs(hinge).min() > 1e-5 if len(hinge) else True, f"{name}: a hinge of the test's inputs sits on its corner"
    on = hinge[:n_rand] > 0
    t0 = [rp[rm][on, 0], rp[rm][on, 0]]
    t1 = [rp[rm][on, 1], np.asarray(negatives)[rm][on]]
    if kind == "hard":
        m0, m1 = ref["mask0"], ref["mask1"]
        on0, on1 = hinge[n_rand:n_rand + m0.sum()] > 0, hinge[n_rand + m0.sum():] > 0
        t0 += [sample[m0][on0, 0], sample[m0][on0, 0], sample[m1][on1, 0], got["D10ind"][m1][on1]]
        t1 += [sample[m0][on0, 1], got["D01ind"][m0][on0], sample[m1][on1, 1], sample[m1][on1, 1]]
    w = 1.0 / max(len(hinge), 1)
    worst = [_rows(a, ref["gF0"], np.concatenate(t0), w, name + " dF0"), _rows(b, ref["gF1"], np.concatenate(t1), w, name + " dF1")]
    print(f"[{name}] values {[float(o.detach()) for o in out]}; worst row error / bound {max(worst):.3f}; "
          f"worst value error so far {WORST['value']:.2e}")
    return out, a, b, ref


def test_one_triplet(dev):
    rng = np.random.default_rng(1)
    F0, F1 = _unit(rng, 5, 4), _unit(rng, 3, 4)
    pairs = np.array([[2, 1]])
    _triplets(dev, "tri", F0, F1, pairs, (None, [0], [2]), "one tri", num_rand_triplet=1)
    _triplets(dev, "hard", F0, F1, pairs, ([0, 4], [0, 2], None, [0], [0]), "one hard", num_rand_triplet=1)
    _contrastive(dev, F0, F1, pairs, np.array([[4, 0]]), "one con")


def test_long_run_and_untouched_rows(dev):
    rng = np.random.default_rng(2)
    F0, F1 = _unit(rng, 64, 32), _unit(rng, 64, 32)
    pos = np.stack([np.zeros(300, np.int64), np.arange(300) % 44], 1)
    neg = np.stack([rng.integers(0, 44, 100), rng.integers(0, 44, 100)], 1)
    _, a, b = _contrastive(dev, F0, F1, pos, neg, "run con")
    assert not a.grad[44:].any() and not b.grad[44:].any() and bool(a.grad[0].any())
    # a run of 300 through the triplet kernels: every sampled positive has anchor 0, every negative lies in rows 44..63
    draws = (rng.permutation(44)[:20], 44 + rng.permutation(20), None, np.arange(0, 300, 15), 44 + rng.permutation(20))
    _, a, b, ref = _triplets(dev, "hard", F0, F1, pos, draws, "run hard", num_rand_triplet=20)
    assert ref["mask0"].all() and ref["rand_mask"].all() and not a.grad[44:].any()


def test_tails_at_the_widest_row(dev):
    rng = np.random.default_rng(3)
    F0, F1 = _unit(rng, 300, 128), _unit(rng, 290, 128)
    F1[:200] = (F1[:200] + 3 * F0[:200]) / np.linalg.norm(F1[:200] + 3 * F0[:200], axis=1, keepdims=True)
    pos = np.stack([rng.integers(0, 300, 400), rng.integers(0, 290, 400)], 1)
    neg = np.stack([rng.integers(0, 300, 600), rng.integers(0, 290, 600)], 1)
    _contrastive(dev, F0, F1, pos, neg, "tails con")
    pairs = np.concatenate([np.stack([np.arange(200), np.arange(200)], 1), np.stack([np.arange(133), 200 + np.arange(133) % 90], 1)])
    draws = (rng.permutation(300)[:77], rng.permutation(290)[:77], None, rng.permutation(333)[:290], rng.permutation(290))
    _triplets(dev, "hard", F0, F1, pairs, draws, "tails hard", num_rand_triplet=290)
    _triplets(dev, "tri", F0, F1, pairs, (rng.permutation(333)[:257],) + draws[3:], "tails tri", num_pos=257, num_rand_triplet=290)


def test_keys_above_2_to_31(dev):
    rng = np.random.default_rng(4)
    N = 50000
    F0, F1 = _unit(rng, N, 4), _unit(rng, N, 4)
    i = rng.permutation(N)[:64]
    j = 46341 + rng.permutation(N - 46341)[:64]
    pairs = np.stack([i, j], 1).astype(np.int64)
    assert (pairs[:, 0] + pairs[:, 1] * N > 2 ** 31).all()
    F1[j[:16]] = F0[i[:16]]                       # the nearest row of these anchors is their partner: a true positive
    others = np.setdiff1d(np.arange(N), np.concatenate([i, j]))
    sel1 = np.concatenate([j[:32], rng.permutation(others)[:40]])
    sel0 = np.concatenate([i[32:], rng.permutation(others)[:40]])
    negatives = np.concatenate([j[:8], rng.permutation(others)[:56]])       # 8 random negatives are the anchor's partner
    draws = (sel0, sel1, None, np.arange(64), negatives)
    out, a, b, ref = _triplets(dev, "hard", F0, F1, pairs, draws, "bigkey", num_rand_triplet=64)
    assert not ref["rand_mask"][:8].any() and ref["rand_mask"][8:].all() and not ref["mask0"][:16].any()
    assert int(torch.count_nonzero(a.grad.abs().sum(1))) <= 64 + 64


def test_empty_groups(dev):
    rng = np.random.default_rng(5)
    F0, F1 = _unit(rng, 40, 32), _unit(rng, 36, 32)
    pairs = np.stack([np.arange(12), np.arange(12)], 1)
    F1[:12] = F0[:12]
    draws = (np.arange(20, 30), np.arange(0, 20), None, np.arange(12), 12 + np.arange(12))
    out, a, b, ref = _triplets(dev, "hard", F0, F1, pairs, draws, "empty side", num_rand_triplet=12)
    assert not ref["mask0"].any() and ref["mask1"].all() and np.isfinite(float(out[0]))
    # every random triplet's negative is the anchor's partner: the mean over nothing is NaN, the gradient all zero
    out, a, b, ref = _triplets(dev, "tri", F0, F1, pairs, (None, np.arange(12), np.arange(12)), "empty tri", num_rand_triplet=12)
    assert np.isnan(float(out[0])) and np.isnan(float(out[2])) and np.isfinite(float(out[1]))
    assert not a.grad.any() and not b.grad.any()
    out, a, b = _contrastive(dev, F0, F1, pairs, np.zeros((0, 2), np.int64), "empty con")
    assert np.isnan(float(out[1])) and np.isfinite(float(out[0]))


def test_inactive_duplicate_and_identical_rows(dev):
    rng = np.random.default_rng(6)
    F0, F1 = _unit(rng, 30, 32), _unit(rng, 30, 32)
    pairs = np.stack([np.arange(10), 10 + np.arange(10)], 1)
    pairs = np.concatenate([pairs, pairs[3:4]])                             # the pair (3, 13) listed twice
    F1[:10] = -F0[:10]                  # row i of F1 is at distance 2 of anchor i: hinge = d_pos + 1.4 - 2 < 0
    F1[10:20] = F0[:10] + 0.05 * _unit(rng, 10, 32)
    F1[10] = F0[0]                      # d^2 = 0 on the pair (0, 10)
    near = np.array([0, 2, 3, 5, 6, 8, 9, 3])
    F1[20:28] = F0[near] + 0.3 * _unit(rng, 8, 32)      # rows close to those anchors: their hinge is far above 0
    draws = (None, np.arange(11), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 3]))
    out, a, b, ref = _triplets(dev, "tri", F0, F1, pairs, draws, "zeros tri", num_rand_triplet=11)
    assert (ref["hinge"] < 0).all() and float(out[0]) == 0.0 and not a.grad.any() and not b.grad.any()
    draws = (None, np.arange(11), np.array([20, 1, 21, 22, 4, 23, 24, 7, 25, 26, 27]))
    out, a, b, ref = _triplets(dev, "tri", F0, F1, pairs, draws, "zeros mixed", num_rand_triplet=11)
    assert (ref["hinge"] < 0).sum() == 3 and not a.grad[[1, 4, 7]].any() and bool(a.grad[0].any())
    assert np.linalg.norm(ref["gF0"][3]) > 1e-3 and bool(a.grad[3].any())      # anchor 3: both copies of its pair, summed
    sel = (np.arange(20, 30), np.arange(20, 30))
    _triplets(dev, "hard", F0, F1, pairs, sel + draws, "zeros hard", num_rand_triplet=11)
    out, a, b = _contrastive(dev, F0, F1, pairs, np.stack([np.arange(10), np.arange(10)], 1), "zeros con")
    assert float(out[1]) == 0.0


def test_refused(dev):
    from apr_amd.fcgf.lib.trainer import ContrastiveLoss, HardestTripletLoss, TripletLoss
    rng = np.random.default_rng(7)
    pairs = np.stack([np.arange(30), np.arange(30)], 1)
    for c, where in ((30, dev), (32, "cpu")):
        F0, F1 = torch.from_numpy(_unit(rng, 40, c)).to(where), torch.from_numpy(_unit(rng, 36, c)).to(where)
        with pytest.raises(_lib.AprHipError):
            ContrastiveLoss().loss(F0, F1, pairs, pairs[:4, ::-1].copy())
        for m in (TripletLoss(), HardestTripletLoss()):
            with pytest.raises(_lib.AprHipError):
                m.triplet_loss(F0, F1, pairs, num_rand_triplet=24)
    F0, F1 = torch.from_numpy(_unit(rng, 40, 32)).to(dev), torch.from_numpy(_unit(rng, 36, 32)).to(dev)
    for m in (TripletLoss(), HardestTripletLoss()):
        with pytest.raises(ValueError, match="broadcast"):
            m.triplet_loss(F0, F1, pairs, num_rand_triplet=33)              # min(30, 33) != min(36, 33)
    with pytest.raises(ValueError):
        TripletLoss().triplet_loss(F0, F1, pairs, draws=(None, np.arange(4), np.array([0, 1, 2, 99])), num_rand_triplet=4)


@pytest.mark.parametrize("n_terms,N", [(1, 5), (257, 64), (1000, 300)])
def test_scratch_guard_bands(dev, n_terms, N):
    lib = _lib.load()
    rng = np.random.default_rng(8)
    c = 32
    F0, F1 = torch.from_numpy(_unit(rng, N, c)).to(dev), torch.from_numpy(_unit(rng, N + 3, c)).to(dev)
    n = 2 * n_terms
    r0 = torch.from_numpy(rng.integers(0, N, n).astype(np.int32)).to(dev)
    r1 = torch.from_numpy(rng.integers(0, N + 3, n).astype(np.int32)).to(dev)
    t = np.arange(n_terms)
    terms = torch.from_numpy(np.stack([t, n_terms + t, n_terms + t, np.full(n_terms, 3)], 1).astype(np.int32)).to(dev)
    keys = torch.sort(r0[n_terms::2].long() + r1[n_terms::2].long() * (N + 3))[0]
    d, coef = torch.empty(n, device=dev), torch.empty(n, device=dev)
    grp = torch.empty(n, dtype=torch.int32, device=dev)
    st = _lib.stream()
    p = _lib.ptr
    _lib.check(lib.apr_pair_dist(p(F0), N, p(F1), N + 3, c, p(r0), p(r1), n, 0, 1e-7, p(d), p(coef), p(grp), st))

    def reduce(addr, sb):
        red, mean = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(1, device=dev)
        kept = torch.empty(n_terms, dtype=torch.uint8, device=dev)
        _lib.check(lib.apr_pair_terms_reduce(p(d), p(r0), p(r1), n, p(terms), n_terms, p(keys), keys.shape[0], N + 3, 1.4, 1,
                                             p(red), p(mean), p(coef), p(grp), p(kept), C.c_void_p(addr), sb, st))
        return red, mean, kept, coef.clone(), grp.clone()
    red = _guarded(dev, int(lib.apr_pair_terms_scratch_bytes(n_terms)), reduce)[0]
    red = torch.from_numpy(red).to(dev)
    gout = torch.ones(1, device=dev)

    def grad(addr, sb):
        dF0, dF1 = torch.empty_like(F0), torch.empty_like(F1)
        _lib.check(lib.apr_pair_grad(p(F0), N, p(F1), N + 3, c, p(r0), p(r1), n, p(coef), p(grp), p(red), p(gout), 1, p(dF0),
                                     p(dF1), C.c_void_p(addr), sb, st))
        return dF0, dF1
    _guarded(dev, int(lib.apr_pair_grad_scratch_bytes(n, N, N + 3)), grad)

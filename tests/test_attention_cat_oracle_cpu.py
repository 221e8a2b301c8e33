"""The cross_cat cases hold what they claim, the bounds of tests/attention_cat_oracle.py hold for float32 NumPy evaluations in
two summation orders (two passes; online over 16-key tiles), and one-rule mutants of the oracle are rejected at the bound on
the designated rows -- all on the host, without any kernel.

Worst |float32 restatement - float64 oracle| / bound over all cases, printed by test_print_worst_ratios:
y 0.137,  dq 0.020,  dk 0.040,  dv 0.043.
"""
import numpy as np
import pytest

import attention_cat_cases as K
import attention_cat_oracle as CO
import attention_oracle as O

F32 = np.float32
WORST = {key: 0.0 for key in ("y", "dq", "dk", "dv")}
_REF = {}


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = CO.train(c["q"], c["k"], c["v"], c["c0"], c["c1"], c["dy"], c["H"])
    return _REF[c["name"]]


def _worst(key, got, ref, bound, what):
    r, at = O.compare_rows(got, ref, bound)
    assert r <= 1.0, (what, key, r, at)
    WORST[key] = max(WORST[key], r)


# ------------------------------------------------------------------------------------- float32 restatements
def _probs32(Q, Kk, scale):
    S = (Q @ Kk.T) * F32(scale)
    E = np.exp(S - S.max(1, keepdims=True))
    return E * (F32(1) / E.sum(1, dtype=F32))[:, None]


def _online32(Q, Kk, VC, scale):
    """the weighted sums of the rows VC, keys in 16-key tiles with a running maximum"""
    S = (Q @ Kk.T) * F32(scale)
    n, m = S.shape
    mx, den, num = np.full(n, -np.inf, F32), np.zeros(n, F32), np.zeros((n, VC.shape[1]), F32)
    for t in range(-(-m // 16)):
        sl = slice(16 * t, min(16 * t + 16, m))
        mnew = np.maximum(mx, S[:, sl].max(1))
        f = np.exp(mx - mnew)
        p = np.exp(S[:, sl] - mnew[:, None])
        den = den * f + p.sum(1, dtype=F32)
        num = num * f[:, None] + p @ VC[sl]
        mx = mnew
    return num / den[:, None]


def _rows32(fs, c0):
    """[feat | soft] float32 -> the y rows of one head"""
    dim = fs.shape[1] - 3
    aug1 = fs[:, dim:] - c0
    aug2 = np.sqrt((aug1 * aug1).sum(1, dtype=F32))
    y = np.concatenate([fs, aug1, aug2[:, None]], 1)
    assert y.dtype == F32
    return y


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_orders_are_inside_the_bounds(name):
    c = K.CASES[name]
    H, dim = c["H"], c["dim"]
    ref = reference(c)
    scale = F32(1) / np.sqrt(F32(dim))
    qh, kh, vh, gh = (O.heads_of(c[key], H) for key in ("q", "k", "v", "dy"))
    c0, c1 = c["c0"], c["c1"]
    ys = {"two-pass": [], "online": []}
    grads = {key: [] for key in ("dq", "dk", "dv")}
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for h in range(H):
            Q, Kk, V, G = (np.ascontiguousarray(t[h]) for t in (qh, kh, vh, gh))
            VC = np.concatenate([V, c1], 1)
            P = _probs32(Q, Kk, scale)
            y = _rows32(P @ VC, c0)
            ys["two-pass"].append(y)
            ys["online"].append(_rows32(_online32(Q, Kk, VC, scale), c0))
            aug1, aug2 = y[:, dim + 3:dim + 6], y[:, dim + 6]
            r = np.where(aug2[:, None] != 0, aug1 / np.where(aug2 != 0, aug2, F32(1))[:, None], F32(0))
            gs = (G[:, dim:dim + 3] + G[:, dim + 3:dim + 6]) + G[:, dim + 6:] * r
            dP = G[:, :dim] @ V.T + gs @ c1.T
            D = (P * dP).sum(1, dtype=F32)[:, None]
            dS = P * (dP - D)
            for key, x in (("dq", (dS @ Kk) * scale), ("dk", (dS.T @ Q) * scale), ("dv", P.T @ G[:, :dim])):
                assert x.dtype == F32
                grads[key].append(x)
    for order, rows in ys.items():
        _worst("y", O.interleave(np.stack(rows)), *ref["y"], (name, order))
    for key in grads:
        _worst(key, O.interleave(np.stack(grads[key])), *ref[key], (name, key))


def test_the_forward_statement_is_the_training_statement():
    c = K.CASES["cat-n15-m65"]
    y, bound, P = CO.forward(c["q"], c["k"], c["v"], c["c0"], c["c1"], c["H"])
    ref = reference(c)
    assert np.array_equal(y, ref["y"][0]) and np.array_equal(bound, ref["y"][1]) and np.array_equal(P, ref["P"][0])
    # the feature columns are the plain attention's
    out, ob, _ = O.mha(c["q"], c["k"], c["v"], c["H"])
    cf = c["dim"] * c["H"]
    assert np.allclose(y[:, :cf], out, rtol=1e-13, atol=1e-15) and np.allclose(bound[:, :cf], ob, rtol=1e-9, atol=0)


def test_the_backward_is_the_derivative():
    """central differences of sum(y * dy) in float64 on a small case (the statement itself, not a kernel)"""
    c = K.CASES["cat-d16-n16-m17"]
    ref = reference(c)
    f = lambda q, k, v: float((CO.forward(q, k, v, c["c0"], c["c1"], c["H"])[0] * c["dy"]).sum())
    rng = np.random.default_rng(3)
    base = [c[key].astype(np.float64) for key in ("q", "k", "v")]
    for idx, key in enumerate(("dq", "dk", "dv")):
        for _ in range(6):
            i, j = rng.integers(base[idx].shape[0]), rng.integers(base[idx].shape[1])
            step = 1e-5
            hi, lo = [b.copy() for b in base], [b.copy() for b in base]
            hi[idx][i, j] += step
            lo[idx][i, j] -= step
            num = (f(*hi) - f(*lo)) / (2 * step)
            assert abs(num - ref[key][0][i, j]) <= 1e-6 * max(1.0, abs(num)), (key, i, j, num, ref[key][0][i, j])


# ----------------------------------------------------------------------------------------------- planted facts
def _cols(c, h, e0, e1):
    return [e * c["H"] + h for e in range(e0, e1)]


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_confirms_its_rows(name):
    c = K.CASES[name]
    n, m, H, dim = c["n"], c["m"], c["H"], c["dim"]
    ref = reference(c)
    y, P = ref["y"][0], ref["P"][0]
    c0, c1 = c["c0"].astype(np.float64), c["c1"].astype(np.float64)
    assert np.abs(c["c0"]).max() <= 80 and np.abs(c["c1"]).max() <= 80 and H == 4
    _, soft, aug1, aug2 = CO.split(y, dim, H)
    zero = np.zeros(n, bool)
    zero[c["zero_rows"]] = True
    assert (aug2[:, ~zero] >= K.MIN_AUG2).all(), "aug2 >= 0.5 everywhere outside the planted zero"
    if m == 1:
        assert c["zero_rows"] == [0] and (P == 1.0).all()
        assert all(np.array_equal(soft[h], np.broadcast_to(c1[0], (n, 3))) for h in range(H)), "one key: soft == c1[0] exactly"
        assert not aug1[:, 0].any() and not aug2[:, 0].any(), "c0[0] == c1[0]: aug1 and aug2 are exactly 0"
        for key in ("dq", "dk", "dv"):
            assert np.isfinite(ref[key][0]).all() and np.isfinite(ref[key][1]).all()
        assert not ref["dq"][0].any() and not ref["dk"][0].any(), "one key: dS = 0, whatever the aug2 term is"
        # the aug2 term is zero on the planted row: its gradient does not depend on g[aug2]
        other = dict(c, dy=c["dy"].copy())
        other["dy"][0, _cols(c, 0, dim + 6, dim + 7)] += 5.0
        alt = CO.train(other["q"], other["k"], other["v"], other["c0"], other["c1"], other["dy"], H)
        assert all(np.array_equal(alt[key][0], ref[key][0]) for key in ("dq", "dk", "dv"))
    else:
        assert not c["zero_rows"]
    kinds = [r["kind"] for r in c["rows"]]
    if n * H >= 4 and m > 1:
        assert ("tie2" if c["tie2"] else "dominant") in kinds
    for r in c["rows"]:
        i, h, kind = r["i"], r["h"], r["kind"]
        if kind == "dominant" and m > 1:
            assert P[h, i, m - 1] == 1.0 and np.array_equal(soft[h, i], c1[m - 1]), "soft is not c1 of the dominant key"
            assert np.array_equal(aug1[h, i], c1[m - 1] - c0[i])
        elif kind == "tie2":
            assert P[h, i, m - 1] == 0.5 and P[h, i, m - 2] == 0.5
            assert np.array_equal(soft[h, i], 0.5 * (c1[m - 2] + c1[m - 1])), "soft is not the midpoint of the tied keys"


def test_cases_cover_the_shapes():
    vals = lambda cases, key: {c[key] for c in cases.values()}
    assert vals(K.MFMA, "n") == {1, 15, 16, 17, 33} and vals(K.MFMA, "m") == {1, 15, 16, 17, 63, 64, 65, 130}
    train_only = {name: c for name, c in K.CASES.items() if c["dim"] != 64}
    assert vals(train_only, "dim") == {1, 16} and vals(K.CASES, "H") == {4}
    assert vals(train_only, "n") == {1, 15, 16, 17, 33} and vals(train_only, "m") == {1, 15, 16, 17, 63, 64, 65, 130}
    for fam in (K.MFMA, train_only):
        assert any(c["zero_rows"] for c in fam.values()) and any(c["tie2"] for c in fam.values())
        assert any(r["kind"] == "dominant" for c in fam.values() for r in c["rows"] if c["m"] > 1)


# --------------------------------------------------------------------------------------------------- mutants
def mutant(c, kind):
    """the float64 oracle's (y, dq, dk) with ONE rule changed"""
    H, dim = c["H"], c["dim"]
    qh, kh, vh, gh = (O.heads_of(c[key].astype(np.float64), H) for key in ("q", "k", "v", "dy"))
    c0, c1 = c["c0"].astype(np.float64), c["c1"].astype(np.float64)
    scale = 1.0 / np.sqrt(dim + 3 if kind == "scale_dim_plus_3" else dim)
    ys, dqs, dks = [], [], []
    for h in range(H):
        S = (qh[h] @ kh[h].T) * scale
        E = np.exp(S - S.max(1, keepdims=True))
        P = E / E.sum(1, keepdims=True)
        feat, soft = P @ vh[h], P @ c1
        aug1 = c0 - soft if kind == "aug1_sign" else soft - c0
        four = np.concatenate([soft[:, 2:], aug1], 1)             # the slice [dim + 2, dim + 6) of the row: one column too many
        aug2 = np.sqrt(((four if kind == "aug2_four" else aug1) ** 2).sum(1))
        ys.append(np.concatenate([feat, soft, aug1, aug2[:, None]], 1))
        G = gh[h]
        r = np.where(aug2[:, None] > 0, aug1 / np.where(aug2 > 0, aug2, 1.0)[:, None], 0.0)
        gs = G[:, dim:dim + 3] + G[:, dim + 3:dim + 6] + G[:, dim + 6:] * r
        dP = G[:, :dim] @ vh[h].T + (0.0 if kind == "no_g_soft" else gs @ c1.T)
        dS = P * (dP - (P * dP).sum(1, keepdims=True))
        dqs.append(scale * (dS @ kh[h]))
        dks.append(scale * (dS.T @ qh[h]))
    ys = np.stack(ys)
    y = np.ascontiguousarray(ys.transpose(1, 0, 2)).reshape(c["n"], -1) if kind == "layout_head_major" else O.interleave(ys)
    return y, O.interleave(np.stack(dqs)), O.interleave(np.stack(dks))


# mutant -> (applies to the case, kinds of the designated rows that must see it, quantity, columns e0 .. e1 of the head)
MUTANTS = {
    "scale_dim_plus_3":  (lambda c: c["m"] > 1, ("last", "offset"), "y", lambda dim: (dim, dim + 3)),
    "aug1_sign":         (lambda c: True, ("last", "dominant", "tie2", "tie"), "y", lambda dim: (dim + 3, dim + 6)),
    # seen where soft_z is known to be far from 0: the rows the last key (z = 40) dominates, every row for m = 1
    "aug2_four":         (lambda c: c["m"] == 1 or c["n"] * c["H"] >= 4, ("dominant", "tie2", "last"), "y", lambda dim: (dim + 6, dim + 7)),
    "no_g_soft":         (lambda c: c["m"] > 1, ("last", "offset"), "dq", lambda dim: (0, dim)),
    "layout_head_major": (lambda c: True, ("last", "dominant", "tie2", "tie"), "y", lambda dim: (0, dim + 7)),
}


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_mutant_is_rejected_on_its_designated_rows(name):
    c = K.CASES[name]
    ref = reference(c)
    dim = c["dim"]
    for kind, (applies, row_kinds, key, span) in MUTANTS.items():
        if not applies(c):
            continue
        got = dict(zip(("y", "dq", "dk"), mutant(c, kind)))[key]
        val, bound = ref[key]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.abs(got - val) / bound
        rows = [r for r in c["rows"] if r["kind"] in row_kinds and not (r["i"] in c["zero_rows"] and kind == "aug1_sign")]
        assert rows or (c["n"] == 1 and c["zero_rows"]), (name, kind, "no designated row")      # a lone planted zero has no sign
        for r in rows:
            worst = ratio[r["i"], _cols(c, r["h"], *span(dim))].max()
            assert worst > 1.0, (name, kind, r, float(worst))
    same = dict(zip(("y", "dq", "dk"), mutant(c, "none")))
    for key in same:
        assert np.allclose(same[key], ref[key][0], rtol=1e-12, atol=1e-13), "the mutant generator is not the oracle"


def test_print_worst_ratios():
    print("worst float32 restatement / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())

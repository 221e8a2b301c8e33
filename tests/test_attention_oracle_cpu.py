"""The attention cases hold what they claim, the error bounds of tests/attention_oracle.py hold for float32 evaluations in
three different orders, and one-rule mutants of the oracle are rejected at the bound on the designated rows -- all on the
host, without any kernel.

Worst |float32 restatement - float64 oracle| / bound over all cases, printed by test_print_worst_ratios:
out 0.038 (two passes / online over 16-key tiles / four merged partials),  P 0.052,  dq 0.018,  dk 0.015,  dv 0.020,
group_max 0.493,  d_center 0.497,  score 0.432.
"""
import numpy as np
import pytest

import attention_cases as K
import attention_oracle as O

F32 = np.float32
WORST = {key: 0.0 for key in ("out", "P", "dq", "dk", "dv", "group_max", "d_center", "score")}


def _worst(key, got, ref, bound, what):
    r, at = O.compare_rows(got, ref, bound)
    assert r <= 1.0, (what, key, r, at)
    WORST[key] = max(WORST[key], r)


# ------------------------------------------------------------------------------------- float32 restatements
def _scores32(Q, Kk, scale):
    return (Q @ Kk.T) * F32(scale)


def two_pass32(Q, Kk, V, scale):
    S = _scores32(Q, Kk, scale)
    E = np.exp(S - S.max(1, keepdims=True))
    out = (E @ V) / E.sum(1, dtype=F32)[:, None]
    assert out.dtype == F32
    return out


def _online32(S, V, tiles):
    n, m = S.shape
    mx, den, num = np.full(n, -np.inf, F32), np.zeros(n, F32), np.zeros((n, V.shape[1]), F32)
    for t in tiles:
        sl = slice(16 * t, min(16 * t + 16, m))
        mnew = np.maximum(mx, S[:, sl].max(1))
        f = np.exp(mx - mnew)
        p = np.exp(S[:, sl] - mnew[:, None])
        den = den * f + p.sum(1, dtype=F32)
        num = num * f[:, None] + p @ V[sl]
        mx = mnew
    return mx, den, num


def online32(Q, Kk, V, scale):
    S = _scores32(Q, Kk, scale)
    _, den, num = _online32(S, V, range(-(-S.shape[1] // 16)))
    out = num / den[:, None]
    assert out.dtype == F32
    return out


def partials32(Q, Kk, V, scale, parts=4):
    """tiles dealt to `parts` running triples, merged at the end; a part without a tile carries den = 0"""
    S = _scores32(Q, Kk, scale)
    ntile = -(-S.shape[1] // 16)
    tri = [_online32(S, V, range(p, ntile, parts)) for p in range(parts)]
    M = np.max([t[0] for t in tri], axis=0)
    D, N = np.zeros_like(tri[0][1]), np.zeros_like(tri[0][2])
    for mx, den, num in tri:
        f = np.where(den > 0, np.exp(np.where(den > 0, mx - M, F32(0))), F32(0)).astype(F32)
        D = D + den * f
        N = N + num * f[:, None]
    out = N / D[:, None]
    assert out.dtype == F32
    return out


ORDERS = {"two-pass": two_pass32, "online": online32, "partials": partials32}


def _per_head(fn, c, **kw):
    qh, kh, vh = O.heads_of(c["q"], c["H"]), O.heads_of(c["k"], c["H"]), O.heads_of(c["v"], c["H"])
    return O.interleave(np.stack([fn(np.ascontiguousarray(qh[h]), np.ascontiguousarray(kh[h]), np.ascontiguousarray(vh[h]),
                                     c["scale"], **kw) for h in range(c["H"])]))


_REF = {}


def reference(c):
    """(out, bound, P) of the float64 oracle, computed once per case"""
    if c["name"] not in _REF:
        _REF[c["name"]] = _per_head_oracle(c)
    return _REF[c["name"]]


def _per_head_oracle(c):
    qh, kh, vh = O.heads_of(c["q"], c["H"]), O.heads_of(c["k"], c["H"]), O.heads_of(c["v"], c["H"])
    res = [O.softmax_sum(qh[h], kh[h], vh[h], c["scale"]) for h in range(c["H"])]
    return O.interleave(np.stack([r[0] for r in res])), O.interleave(np.stack([r[1] for r in res])), np.stack([r[2] for r in res])


@pytest.mark.parametrize("name", list(K.SOFTMAX))
def test_float32_orders_are_inside_the_bound(name):
    c = K.SOFTMAX[name]
    ref, bound, _ = reference(c)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for order, fn in ORDERS.items():
            _worst("out", _per_head(fn, c), ref, bound, (name, order))


def test_the_case_oracle_is_the_module_oracle():
    """O.mha (scale from dim) and O.softmax_matvec (scale from the temperature) are what `reference` evaluates"""
    c = K.MHA["mha-n9-m257"]
    out, bound, P = O.mha(c["q"], c["k"], c["v"], c["H"])
    ref = reference(c)
    assert np.allclose(out, ref[0], rtol=1e-12, atol=0) and np.allclose(bound, ref[1], rtol=1e-6) and P.shape == (4, 9, 257)
    c = K.SMV["smv-common"]
    out, bound = O.softmax_matvec(c["q"], c["k"], c["v"][:, 0], K.temperature(c["dim"]))
    assert np.allclose(out, reference(c)[0][:, 0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", list(K.TRAIN))
def test_float32_training_path_is_inside_the_bounds(name):
    c = K.TRAIN[name]
    H, scale = c["H"], F32(c["scale"])
    ref = O.mha_train(c["q"], c["k"], c["v"], c["dout"], H)
    qh, kh, vh, gh = (O.heads_of(c[key], H) for key in ("q", "k", "v", "dout"))
    got = {key: [] for key in ("P", "O", "dq", "dk", "dv")}
    with np.errstate(under="ignore"):
        for h in range(H):
            Q, Kk, V, G = (np.ascontiguousarray(t[h]) for t in (qh, kh, vh, gh))
            S = _scores32(Q, Kk, scale)
            E = np.exp(S - S.max(1, keepdims=True))
            P = E * (F32(1) / E.sum(1, dtype=F32))[:, None]
            dP = G @ V.T
            D = (P * dP).sum(1, dtype=F32)[:, None]
            dS = P * (dP - D)
            for key, x in (("P", P), ("O", P @ V), ("dq", (dS @ Kk) * scale), ("dk", (dS.T @ Q) * scale), ("dv", P.T @ G)):
                assert x.dtype == F32
                got[key].append(x)
    _worst("P", np.stack(got["P"]), *ref["P"], name)
    for key in ("O", "dq", "dk", "dv"):
        _worst("out" if key == "O" else key, O.interleave(np.stack(got[key])), *ref[key], (name, key))


# ----------------------------------------------------------------------------------------------- planted facts
def _row_channels(c, row):
    return slice(row["h"], None, c["H"])


@pytest.mark.parametrize("name", list(K.SOFTMAX))
def test_case_confirms_its_rows(name):
    c = K.SOFTMAX[name]
    n, m, H, dim = c["n"], c["m"], c["H"], c["dim"]
    out, bound, P = reference(c)
    rows = c["rows"]
    assert c["fact"] and len(rows) >= min(2, n * H), "no case may list fewer than two designated rows"
    assert len({(r["i"], r["h"]) for r in rows}) == len(rows)
    vh = O.heads_of(c["v"].astype(np.float64), H)
    qh, kh = O.heads_of(c["q"].astype(np.float64), H), O.heads_of(c["k"].astype(np.float64), H)
    kinds = [r["kind"] for r in rows]
    if n * H >= len(c["first_targets"]) + 1 and m > 1 and not c["same_keys"]:
        # the last key and both keys of the last 16-, 64-, 128- and 256-key boundary that m crosses
        assert "last" in kinds and all(f"key:{t}" in kinds for t in c["first_targets"])
        assert dim < 4 or m < 3 or {t for g in K.GRAN if g < m for t in (g * ((m - 1) // g) - 1, g * ((m - 1) // g))} - {m - 1} \
            == set(c["first_targets"])
    if c["same_keys"]:
        assert np.ptp(kh, axis=1).max() == 0 and np.ptp(P, axis=2).max() == 0
        assert np.allclose(out, np.broadcast_to(c["v"].astype(np.float64).mean(0), out.shape), rtol=1e-13, atol=1e-15)
    for r in rows:
        i, h, kind = r["i"], r["h"], r["kind"]
        p, o, b = P[h, i], out[i, _row_channels(c, r)], bound[i, _row_channels(c, r)]
        S = (qh[h, i] @ kh[h].T) * c["scale"]
        if kind in ("last", "offset") and m > 1:
            assert p[m - 1] >= 0.25
            sep = (np.abs(vh[h, m - 1] - o) / b).max()
            assert sep > 100 or kind == "offset", ("the planted key's value row is not 100 bounds from the output", sep)
            assert (np.diff(S[::16][-256:]) > 0.9).all(), "every tile (of the last 256) must raise the maximum"
            if kind == "offset":
                assert S.min() * np.sqrt(dim) > 4000 or c["family"] == "smv" and S.min() / c["scale"] > 4000
        elif kind.startswith("key:"):
            t = int(kind[4:])
            assert 0.25 <= p[t] <= 0.75, (kind, p[t])
            assert (np.abs(vh[h, t] - o) / b).max() > 100, (kind, (np.abs(vh[h, t] - o) / b).max(), float(np.abs(S).max()))
        elif kind == "dominant" and m > 1:
            assert S[m - 1] - np.delete(S, m - 1).max() > 110
            assert p[m - 1] == 1.0 and np.array_equal(o, vh[h, m - 1]), "the row is not exactly v of the dominant key"
            if m > 16:      # every other tile (so every other wave of either MFMA kernel) is more than 100 below
                assert S[16 * ((m - 1) // 16)] - S[:16 * ((m - 1) // 16)].max() > 100
        elif kind == "tie":
            assert np.ptp(S) == 0.0 and np.ptp(p) == 0.0
            assert np.allclose(o, vh[h].mean(0), rtol=1e-13, atol=1e-15)
            if dim >= 2 and not c["same_keys"]:
                assert S[0] / c["scale"] == K.OFFSET
        elif kind == "first" and m > 16:
            assert S[:16].max() == S.max() and (np.diff(S[::16]) <= 0).all(), "no later tile may raise the maximum"
        elif kind == "firstdom" and m > 16:
            top = K.phi(m) == 0
            assert top[:16].all() and S[top].min() - S[~top].max() > 100 and p[~top].max() < 2.0 ** -149
            assert np.allclose(o, vh[h, top].mean(0), rtol=1e-13, atol=1e-15)


def test_cases_cover_the_edges():
    vals = lambda cases, key: {c[key] for c in cases.values()}
    assert {1, 7, 8, 9} <= vals(K.MHA, "n") and {4, 16, 64, 256} == vals(K.MHA, "dim") and {1, 3, 4} == vals(K.MHA, "H")
    assert {1, 255, 256, 257} <= vals(K.MHA, "m")
    for dim in (4, 16, 64, 256):
        ms = {c["m"] for c in K.MHA.values() if c["dim"] == dim}
        assert {4 * (256 // dim) - 1, 4 * (256 // dim) + 1} <= ms, dim
    assert {(64, 1856), (16, 1904), (256, 1664)} <= {(c["dim"], c["m"]) for c in K.MHA.values()}
    assert all(K.mha_takes(c) for c in K.ATTENTION.values())
    assert vals(K.HEADMAJOR, "n") == {1, 15, 16, 17, 33} and vals(K.HEADMAJOR, "H") == {1, 3, 4}
    assert vals(K.HEADMAJOR, "m") == {1, 5, 15, 16, 17, 63, 64, 65, 129} and vals(K.HEADMAJOR, "dim") == {64}
    route = lambda c: K.expected_route(c["n"], c["m"], c["dim"])
    by = {}
    for c in K.SMV.values():
        by.setdefault(route(c), []).append(c)
        assert c["name"].split("-")[1] in {"mfma": ("c32", "c64", "c128", "c256", "common", "samekeys"), "transposed": ("t",),
                                            "first": ("1",)}[route(c)]
    assert {c["dim"] for c in by["mfma"]} == {32, 64, 128, 256} and {1, 15, 16, 17} <= {c["n"] for c in by["mfma"]}
    assert {1, 15, 16, 17, 127, 128, 129, 257} <= {c["m"] for c in by["mfma"]}
    assert {c["dim"] for c in by["transposed"]} == {20, 33, 96} and {c["n"] for c in by["transposed"]} == {1, 3, 4, 5}
    assert all(c["m"] + c["dim"] == 3840 for c in by["transposed"])
    assert sorted(c["m"] + c["dim"] for c in by["first"]) == [3841, 15360] and all(c["n"] == 5 for c in by["first"])
    assert {1, 255, 256, 257} <= vals(K.TRAIN, "m") and {1, 64, 300, 1024} == vals(K.TRAIN, "dim")
    assert any(c["vdim"] == 1 and c["H"] == 1 for c in K.TRAIN.values())
    assert K.TRAIN["tr-sweep-row"]["n"] * 256 > 16384 * 256 < K.TRAIN["tr-sweep-col"]["m"] * 256
    # every kind of row on every family; every mutant has a case it applies to in every family it can touch
    for fam in (K.MHA, K.HEADMAJOR, K.SMV, K.TRAIN):
        kinds = {r["kind"].split(":")[0] for c in fam.values() for r in c["rows"]}
        assert {"last", "key", "dominant", "tie", "first", "offset", "firstdom"} <= kinds
    e = K.EDGE.values()
    assert {1, 3, 64, 256} == {c["c"] for c in e} and {1, 6, 15} == {c["k"] for c in e}
    assert K.EDGE["e-sweep"]["n"] * 15 * 256 > 16384 * 256 < K.EDGE_BWD_SWEEP["n"] * 256
    assert {"row0+self", "lastrow", "self", "repeat"} <= {p for c in e for p in c["plants"].values()}
    g = K.GROUP.values()
    assert {1, 3, 64, 256} == {c["c"] for c in g} and {1, 2, 6, 15} == {c["k"] for c in g}
    assert {(c["scale"] is None, c["slope"]) for c in g} >= {(True, 0.0), (True, 0.2), (False, 0.0), (False, 0.2)}
    assert any(c["ldy_extra"] and c["ldo_extra"] for c in g)


# --------------------------------------------------------------------------------------------------- mutants
def round_bits(x, keep):
    """float32 rounded to `keep` stored mantissa bits, to nearest even (7: bfloat16, 16 bits; 10: the 19-bit format)"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    drop = 23 - keep
    b = ((b + (1 << (drop - 1)) - 1 + ((b >> drop) & 1)) >> drop) << drop
    return b.astype(np.uint32).view(F32).astype(np.float64)


def mutant(c, kind):
    """the float64 oracle's out [n, vdim * H] with ONE rule changed"""
    n, m, H, dim, scale = c["n"], c["m"], c["H"], c["dim"], c["scale"]
    q, k, v = (c[key].astype(np.float64) for key in ("q", "k", "v"))
    if kind == "bf16":
        q, k, v = (round_bits(c[key], 7) for key in ("q", "k", "v"))
    elif kind == "bits19":
        q, k, v = (round_bits(c[key], 10) for key in ("q", "k", "v"))
    if kind == "headmajor_as_interleaved":
        hm = lambda x: np.ascontiguousarray(x.reshape(len(x), H, -1).transpose(1, 0, 2))
        qh, kh, vh = hm(q), hm(k), hm(v)
    else:
        qh, kh, vh = O.heads_of(q, H), O.heads_of(k, H), O.heads_of(v, H)
    outs = []
    for h in range(H):
        Q, Kk, V = qh[h], kh[h], vh[h]
        keep = np.ones(m, bool)
        if kind == "neighbour_head":
            Kk, V = kh[(h + 1) % H], vh[(h + 1) % H]
        elif kind == "drop_last":
            keep[m - 1] = False
        elif kind == "drop_tile_first":
            keep[16 * ((m - 1) // 16)] = False
        elif kind == "merge_skip":
            keep[(np.arange(m) // 16) % 4 == ((m - 1) // 16) % 4] = False
        elif kind == "drop_channel":
            Q = Q.copy()
            Q[:, 0] = 0
        elif kind == "v_shift":
            V = np.roll(V, 1, axis=0)
        Kk, V = Kk[keep], V[keep]
        if kind == "dup_last":
            Kk, V = np.concatenate([Kk, Kk[-1:]]), np.concatenate([V, V[-1:]])
        if len(Kk) == 0:
            outs.append(np.full((n, V.shape[1]), np.nan))
            continue
        S = (Q @ Kk.T) * (1.0 / dim if kind == "scale_1_over_dim" else scale)
        E = np.exp(S - S.max(1, keepdims=True))
        outs.append((E / E.sum(1, keepdims=True)) @ V)
    out = O.interleave(np.stack(outs))
    if kind == "guard_row":
        out[n - 1] = np.nan                      # the row went to the guard row behind it
    return out


def _tile_first_rows(c):
    b = 16 * ((c["m"] - 1) // 16)
    return ("last", "offset") if b == c["m"] - 1 else (f"key:{b}",) if b in c["targets"] else ("tie",)


# mutant -> (applies to the case, kinds of the designated rows that must see it)
MUTANTS = {
    "drop_last":       (lambda c: True, lambda c: ("last", "offset")),
    "dup_last":        (lambda c: c["m"] > 1, lambda c: ("last", "offset")),      # one key twice is still that key
    "drop_tile_first": (lambda c: True, _tile_first_rows),
    "neighbour_head":  (lambda c: c["H"] > 1, lambda c: ("last", "dominant", "tie")),
    "headmajor_as_interleaved": (lambda c: c["H"] > 1 and c["vdim"] > 1, lambda c: ("last", "dominant", "tie")),
    # the cross-saliency and softmax-matvec forms state their scale through the temperature
    "scale_1_over_dim": (lambda c: c["dim"] > 1 and c["m"] > 1 and c["family"] != "smv", lambda c: ("last", "offset")),
    "v_shift":         (lambda c: c["m"] > 1, lambda c: ("last", "offset", "dominant")),
    "guard_row":       (lambda c: True, None),
    # a row that is one value row (`dominant`, or any row for m = 1) has the bound 2 S u |v|: a format of unit roundoff r is
    # sure to be seen on some channel when r / 4 is above that, i.e. S < 2^(20 - stored bits)
    "bf16":            (lambda c: O.s_count(c["m"]) < 2 ** 13 and c["vdim"] >= 16, lambda c: ("dominant",) if c["m"] > 1 else ("last",)),
    "bits19":          (lambda c: O.s_count(c["m"]) < 2 ** 10 and c["vdim"] >= 16, lambda c: ("dominant",) if c["m"] > 1 else ("last",)),
    "drop_channel":    (lambda c: c["m"] > 1, lambda c: ("last", "offset")),
    "merge_skip":      (lambda c: True, lambda c: ("last", "offset")),
}


@pytest.mark.parametrize("name", list(K.SOFTMAX))
def test_every_mutant_is_rejected_on_its_designated_rows(name):
    c = K.SOFTMAX[name]
    ref, bound, _ = reference(c)
    assert O.compare_rows(ref, ref, bound) == (0.0, None) and O.compare_rows(ref.astype(F32), ref, bound)[0] <= 1.0
    for kind, (applies, row_kinds) in MUTANTS.items():
        if not applies(c):
            continue
        got = mutant(c, kind)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)
        if row_kinds is None:
            assert np.isinf(ratio[c["n"] - 1]).all() and O.compare_rows(got, ref, bound)[0] > 1
            continue
        rows = K.rows_of(c, *row_kinds(c))
        if c["same_keys"]:              # no planted key: these cases are held to the rows every case has (guard row, v shift)
            rows = [r for r in rows if kind in ("v_shift", "neighbour_head", "headmajor_as_interleaved")]
        assert rows or c["same_keys"] or c["n"] * c["H"] < len(c["rows"]) + 1, (name, kind, "no designated row")
        for r in rows:
            assert ratio[r["i"], _row_channels(c, r)].max() > 1.0, (name, kind, r, float(ratio[r["i"], _row_channels(c, r)].max()))


@pytest.mark.parametrize("name", [n for n, c in K.SOFTMAX.items() if c["targets"]])
def test_every_planted_key_is_missed_when_dropped_or_doubled(name):
    """each key:<t> row rejects the sum without key t and the sum with key t twice (the first or last key of a tile)"""
    c = K.SOFTMAX[name]
    ref, bound, _ = reference(c)
    H = c["H"]
    qh, kh, vh = (O.heads_of(c[key].astype(np.float64), H) for key in ("q", "k", "v"))
    for r in K.rows_of(c, "key"):
        i, h, t = r["i"], r["h"], int(r["kind"][4:])
        for sel in (np.delete(np.arange(c["m"]), t), np.append(np.arange(c["m"]), t)):
            S = (qh[h, i] @ kh[h, sel].T) * c["scale"]
            E = np.exp(S - S.max())
            got = (E / E.sum()) @ vh[h, sel]
            ratio = np.abs(got - ref[i, _row_channels(c, r)]) / bound[i, _row_channels(c, r)]
            assert ratio.max() > 1.0, (name, r, len(sel), float(ratio.max()))


def test_every_mutant_applies_in_every_family():
    for fam_name, fam in (("mha", K.MHA), ("headmajor", K.HEADMAJOR), ("smv", K.SMV), ("train", K.TRAIN)):
        for kind, (applies, row_kinds) in MUTANTS.items():
            if fam_name == "smv" and kind in ("neighbour_head", "headmajor_as_interleaved", "scale_1_over_dim", "bf16", "bits19"):
                continue                                     # one head, one value column, a temperature
            hit = [c for c in fam.values() if applies(c) and (row_kinds is None or K.rows_of(c, *row_kinds(c)))]
            assert hit, (fam_name, kind)


# -------------------------------------------------------------------------------------------------- edge kernels
@pytest.mark.parametrize("name", list(K.EDGE))
def test_edge_features_oracle_and_mutants(name):
    c = K.EDGE[name]
    n, k, ch, knn = c["n"], c["k"], c["c"], c["knn"]
    e = O.edge_features(c["f"], knn)
    e32 = O.edge_features_f32(c["f"], knn)
    assert e.shape == (n * k, 2 * ch) and np.array_equal(e[:, :ch], e32[:, :ch])
    assert np.abs(e32[:, ch:] - e[:, ch:]).max() <= O.U * np.abs(e[:, ch:]).max()
    for row, plant in c["plants"].items():
        if plant == "row0+self":
            assert knn[0, 0] == 0 and not e[0, ch:].any()
        elif plant == "lastrow":
            assert knn[1, 0] == n - 1
        elif plant == "self":
            assert knn[2, k - 1] == 2 and not e[2 * k + k - 1, ch:].any()
        elif plant == "repeat":
            assert knn[3, 0] == knn[3, k - 1] and np.array_equal(e[3 * k], e[3 * k + k - 1])
    wrong = np.concatenate([e[:, :ch], -e[:, ch:]], 1)                      # mutant: f_i - f_j
    assert not np.array_equal(wrong.astype(F32), e32)
    if n * k * ch > 16384 * 256:
        return
    dc, contrib, bound = O.edge_features_backward(c["de"], n, k)
    de = c["de"]
    acc = np.zeros((n, ch), F32)
    for j in range(k):
        acc = acc + (de[j::k, :ch] - de[j::k, ch:])
    _worst("d_center", acc, dc, bound, name)
    assert np.array_equal(contrib, de[:, ch:].astype(np.float64))
    plus = (de[:, :ch].astype(np.float64) + de[:, ch:]).reshape(n, k, ch).sum(1)           # mutant: + for -
    assert O.compare_rows(plus, dc, bound)[0] > 1.0


@pytest.mark.parametrize("name", list(K.GROUP))
def test_group_max_oracle_and_mutants(name):
    c = K.GROUP[name]
    n, k, ch, slope = c["n"], c["k"], c["c"], c["slope"]
    out, bound = O.group_max(c["y"], n, k, c["scale"], c["shift"], slope)
    sc = F32(1) if c["scale"] is None else c["scale"]
    sh = F32(0) if c["shift"] is None else c["shift"]
    z = c["y"] * sc + sh
    a = np.where(z > 0, z, z * F32(slope))
    assert a.dtype == F32
    _worst("group_max", a.reshape(n, k, ch).max(1), out, bound, name)
    assert (out[0] <= 0).all() and (slope != 0.0 or not out[0].any()), "group 0 is all negative"
    z64 = c["y"].astype(np.float64) * (1.0 if c["scale"] is None else c["scale"]) + (0.0 if c["shift"] is None else c["shift"])
    if n >= 2:
        assert (z64.reshape(n, k, ch)[1].argmax(0) == k - 1).all(), "group 1's maximum is its last row"
        last_dropped = O.leaky(z64, slope).reshape(n, k, ch)[:, :max(k - 1, 1)].max(1)     # mutant: the last row of a group left out
        assert k == 1 or O.compare_rows(last_dropped, out, bound)[0] > 1.0
    no_act = z64.reshape(n, k, ch).max(1)                                    # mutant: no activation
    r, at = O.compare_rows(no_act, out, bound)
    assert r > 1.0 and at[0] == 0, "the all-negative group must see a missing activation"


def test_score_head_oracle():
    x = K.score_case(257)
    y, bound = O.score_head(x)
    y32 = y.astype(F32)
    for i, val in K.SCORE_SPECIALS.items():
        assert x[i] == val or np.isnan(val)
    assert y32[0] == 0 and y32[1] == 1 and y32[2] == 0 and y32[3] == 0 and y32[4] == 1 and y[5] == 0.5 and y[6] == 0.5
    assert not bound[:3].any() and (y >= 0).all() and (y <= 1).all()
    with np.errstate(over="ignore"):
        got = F32(1) / (F32(1) + np.exp(-x))
    got = np.where(np.isnan(got), F32(0), np.clip(got, 0, 1))
    fin = np.isfinite(x)
    _worst("score", got[fin], y[fin], bound[fin], "score")
    assert np.array_equal(got[~fin], y32[~fin])
    with np.errstate(over="ignore"):
        assert O.compare_rows(1.0 / (1.0 + np.exp(-0.5 * x[fin])), y[fin], bound[fin])[0] > 1.0     # mutant: x / 2


def test_print_worst_ratios():
    print("worst float32 restatement / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())

"""The KPConv cases hold what they claim, the error bounds hold for a plain float32 evaluation, and one-rule mutants of
the oracle are rejected at the bound -- all on the host, without any kernel.

Worst |float32 restatement - float64 oracle| / bound over all cases (ascending h, and 4-wide blocks of h), printed by
test_print_worst_ratios:  wf 0.516,  contrib 0.274,  d_x 0.274.
"""
import numpy as np
import pytest

import kpconv_cases as K
import kpconv_oracle as O

F32 = np.float32
WORST = {"wf": 0.0, "contrib": 0.0, "d_x": 0.0}


def _args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


# ------------------------------------------------------------------------------------- float32 restatements
def _w32(c):
    q, s, nbr, x, kp, extent = _args(c)
    real = O.real_mask(nbr, c["ns"])
    idx = np.where(real, nbr, 0)
    diff = s[idx] - q[:, None, :]
    e = diff[:, None, :, :] - kp[None, :, None, :]
    d2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]
    inv = F32(1) / F32(extent)
    w = np.maximum(F32(1) - np.sqrt(d2) * inv, F32(0)) * real[:, None, :].astype(F32)
    cnt = (real & (x.sum(1, dtype=F32)[idx] > 0)).sum(1)
    inv_num = (F32(1) / np.maximum(cnt, 1).astype(F32)).astype(F32)
    assert w.dtype == F32 and inv_num.dtype == F32
    return w, real, idx, inv_num


def _sum32(terms, blocked):
    """terms(h) -> float32 array; summed over h ascending, or in 4-wide blocks ((t0 + t1) + (t2 + t3)) added in turn"""
    n, acc = terms.n, None
    if not blocked:
        for h in range(n):
            t = terms(h)
            acc = t if acc is None else acc + t
    else:
        for h0 in range(0, n, 4):
            t = [terms(h) for h in range(h0, min(h0 + 4, n))]
            while len(t) < 4:
                t.append(np.zeros_like(t[0]))
            part = (t[0] + t[1]) + (t[2] + t[3])
            acc = part if acc is None else acc + part
    assert acc.dtype == F32
    return acc


class _Terms:
    def __init__(self, n, fn):
        self.n, self.fn = n, fn

    def __call__(self, h):
        return self.fn(h)


def weighted32(c, blocked):
    w, real, idx, inv_num = _w32(c)
    xg = c["x"][idx] * real[:, :, None].astype(F32)
    acc = _sum32(_Terms(c["H"], lambda h: w[:, :, h, None] * xg[:, None, h, :]), blocked)
    return (acc * inv_num[:, None, None]).reshape(c["nq"], -1)


def contrib32(c, blocked):
    w, real, idx, inv_num = _w32(c)
    g = c["dwf"].reshape(c["nq"], 15, -1) * inv_num[:, None, None]
    acc = _sum32(_Terms(15, lambda k: w[:, k, :, None] * g[:, k, None, :]), blocked)
    return acc.reshape(c["nq"] * c["H"], -1)


def dx32(c, rows, blocked):
    rev_t, start = O.reverse_table(c["nbr"], c["ns"])
    out = np.zeros((c["ns"], c["cin"]), F32)
    for r in range(c["ns"]):
        run = rev_t[start[r]:start[r + 1]]
        if len(run):
            out[r] = _sum32(_Terms(len(run), lambda i: rows[run[i]]), blocked)
    return out


@pytest.mark.parametrize("name", list(K.ALL))
def test_float32_restatement_is_inside_the_bounds(name):
    c = K.ALL[name]
    wf, _, _ = O.weighted(*_args(c))
    bw = O.bound_weighted(*_args(c))
    ct, bc = O.contrib(*_args(c), c["dwf"]), O.bound_contrib(*_args(c), c["dwf"])
    dx, bd = O.d_x_from_dwf(*_args(c), c["dwf"]), O.bound_dx(*_args(c), c["dwf"])
    for blocked in (False, True):
        r, at = O.compare_rows(weighted32(c, blocked), wf, bw)
        assert r <= 1.0, ("wf", blocked, r, at)
        WORST["wf"] = max(WORST["wf"], r)
        rows = contrib32(c, blocked)
        r, at = O.compare_rows(rows, ct, bc)
        assert r <= 1.0, ("contrib", blocked, r, at)
        WORST["contrib"] = max(WORST["contrib"], r)
        r, at = O.compare_rows(dx32(c, rows, blocked), dx, bd)
        assert r <= 1.0, ("d_x", blocked, r, at)
        WORST["d_x"] = max(WORST["d_x"], r)


def test_print_worst_ratios():
    print("worst float32 restatement / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# ----------------------------------------------------------------------------------------------- stated facts
@pytest.mark.parametrize("name", list(K.ALL))
def test_case_confirms_its_fact(name):
    c = K.ALL[name]
    nq, ns, H, cin, nbr = c["nq"], c["ns"], c["H"], c["cin"], c["nbr"]
    assert nq <= 67 and ns <= 200 and cin <= 512 and c["fact"]
    wf, num, w = O.weighted(*_args(c))
    _, raw = O.neighbour_count(nbr, c["x"])
    real = O.real_mask(nbr, ns)
    bw = O.bound_weighted(*_args(c))
    wf3 = wf.reshape(nq, 15, cin)
    # the route the name claims
    route = K.expected_route(cin, H, c["layout"])
    if name in K.FORWARD:
        assert route == {"g": "generic", "m1": "mfma1", "m2": "mfma2", "m4": "mfma4"}[name.split("-")[0]]
    else:
        assert ("atomic" in c["fact"]) == (cin % 4 != 0) and H <= 128 and cin <= 512
        if "CPL" in c["fact"]:
            assert f"CPL {K.expected_cpl(cin)}" in c["fact"]
    if "blocks" in c["fact"]:
        assert f"{K.blocks(nq)} blocks" in c["fact"]
    if "nobody points at" in c["fact"]:
        pointed = np.zeros(ns, bool)
        pointed[nbr[real]] = True
        assert not pointed.all() and O.d_x_from_dwf(*_args(c), c["dwf"])[~pointed].any() == False    # noqa: E712
    if "nq > ns" in c["fact"]:
        assert nq > ns
    if cin > 256:
        assert np.abs(wf3[:, :, 256:]).max() > 0, "channel groups >= 4 are all zero"
    if cin % 64 and cin > 64:
        assert np.abs(O.contrib(*_args(c), c["dwf"])[:, 64 * (cin // 64):]).max() > 0
    # planted rows
    assert len(c["plants"]) >= min(nq, 3) - (0 if ns >= 4 else 2)
    for row, kind in c["plants"].items():
        if kind == "allpad":
            assert not real[row].any() and num[row] == 1 and not wf[row].any() and not bw[row].any()
        elif kind == "padkinds":
            n = min(H, 4)
            assert not real[row, :n].any()
            if H >= 4:
                assert set(int(v) for v in nbr[row, :4]) == {ns, -1, -7, ns + 5}
        elif kind == "dup":
            assert real[row].all() and len(set(nbr[row])) == 1 and raw[row] == H == num[row] and wf[row].any()
        elif kind == "floor":
            assert raw[row] == 0 and num[row] == 1 and real[row].sum() == min(H, 2)
            assert all(w[row, :, h].max() > 0 for h in np.flatnonzero(real[row])) and wf[row].any()
            assert float(c["x"][1].astype(np.float64).sum()) < 0 and float(c["x"][0].astype(np.float64).sum()) == 0
        elif kind == "far":
            assert raw[row] == 2 == num[row] and w[row, :, 0].max() == 0 and w[row, :, H - 1].max() > 0
            assert real[row].sum() == (3 if H >= 3 else 2)
        elif kind == "self":
            assert w[row, 0, 0] == 1.0 and (H < 3 or nbr[row, 0] == nbr[row, H - 1])
        elif kind == "lastonly":
            assert real[row].sum() == 1 and real[row, H - 1] and wf[row].any()      # h = H - 1 carries all of the row
        else:
            raise AssertionError(kind)


def test_cases_cover_the_routes_and_edges():
    f, b = K.FORWARD, K.BACKWARD
    assert len(f) <= 42 and len(b) <= 27
    by_route = {}
    for c in f.values():
        by_route.setdefault(K.expected_route(c["cin"], c["H"], c["layout"]), []).append(c)
    cins = lambda r: {c["cin"] for c in by_route[r]}
    assert {1, 3, 8, 9, 63, 64} <= cins("generic") and cins("mfma1") == {64, 192} and cins("mfma2") == {128}
    assert cins("mfma4") == {256, 320, 384, 512}
    assert {c["layout"] for c in by_route["generic"] if c["cin"] == 64 and c["H"] <= 128} == {"slice1", "ldodd"}
    assert {1, 2, 3, 4, 5, 63, 64, 65, 127, 128} <= {c["H"] for c in by_route["mfma1"]}
    assert {129, 130} <= {c["H"] for c in by_route["generic"]}
    for r in ("mfma2", "mfma4"):
        hs = {c["H"] for c in by_route[r]}
        assert {3, 5, 128} <= hs and hs & {64, 65} and hs & {127, 128}, r
    mf = [c for r in ("mfma1", "mfma2", "mfma4") for c in by_route[r]]
    assert {1, 3, 4, 5, 29, 33, 61, 67} <= {c["nq"] for c in mf}
    assert {1, 2, 8, 9, 16, 17} <= {K.blocks(c["nq"]) for c in mf}
    assert {9, 17} <= {K.blocks(c["nq"]) for c in by_route["mfma4"]}
    assert any(c["ns"] == 1 for c in mf) and any(c["ns"] == 1 for c in by_route["generic"])
    assert any(c["nq"] < c["ns"] for c in mf) and any(c["nq"] > c["ns"] for c in mf)
    for kind in K.PLANTS:            # every planted row on the MFMA route, the generic route and in the backward
        for group in (mf, by_route["generic"], list(b.values())):
            assert any(kind in c["plants"].values() for c in group), kind
    assert any(c["H"] >= 4 and "padkinds" in c["plants"].values() for c in mf)
    assert {1, 3, 130} <= {c["cin"] for c in b.values()} and {4, 60, 64, 68, 128, 132, 256, 260, 512} <= {c["cin"] for c in b.values()}
    assert {1, 2, 3, 4, 5, 63, 64, 65, 127, 128} <= {c["H"] for c in b.values()}
    assert {K.expected_cpl(c["cin"]) for c in b.values()} == {1, 2, 4, 8}
    for name, cout in K.END_TO_END:
        assert name in K.ALL
    assert [(K.ALL[n]["cin"], co) for n, co in K.END_TO_END] == [(1, 128), (3, 34), (64, 34), (68, 129), (192, 64), (320, 64),
                                                                 (384, 128), (512, 64)]
    rv = K.REVERSE.values()
    assert {1, 2, 255, 256, 257} <= {c["ns"] for c in rv} and {1, 255, 256, 257} <= {c["nq"] * c["H"] for c in rv}
    assert {"allpad", "nopad", "negatives"} <= {c["kind"] for c in rv}
    pv = K.POOLS.values()
    assert {1, 3, 4, 5, 8} <= {c["c"] for c in pv} and {1, 7, 8, 9, 255} <= {c["H"] for c in pv}
    assert any(c["layout"] == "slice1" for c in pv)
    planted = {p for c in pv for p in c["plants"].values()}
    assert ("tie", 0, 3) in planted and ("tie", 7, 8) in planted and ("allshadow",) in planted
    assert any(p[0] == "shadowmax" for p in planted)


# --------------------------------------------------------------------------------------------------- mutants
def _swizzle(blk, nb):
    xcd, loc = blk & 7, blk >> 3
    return xcd * (nb >> 3) + min(xcd, nb & 7) + loc


def mutant_weighted(c, kind):
    """wf of the float64 oracle with ONE rule changed"""
    q, s, nbr, x, kp, extent = _args(c)
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    nbr = nbr.astype(np.int64).copy()
    real = O.real_mask(nbr, ns)
    if kind == "pad_as_last_row":
        nbr[~real] = ns - 1
    elif kind == "negative_from_end":
        neg = (nbr < 0) & (nbr + ns >= 0)
        nbr[neg] += ns
    elif kind == "dup_listed_once":
        for r in range(nq):
            seen = set()
            for h in range(H):
                v = int(nbr[r, h])
                if 0 <= v < ns:
                    if v in seen:
                        nbr[r, h] = ns
                    seen.add(v)
    elif kind == "drop_last":
        nbr[:, H - 1] = ns
    elif kind == "drop_h64":
        nbr[:, 64:] = ns
    elif kind == "drop_tail4":
        nbr[:, 4 * (H // 4):] = ns
    w, d, real, idx, _ = O.geometry(q, s, nbr, kp, extent)
    if kind == "squared_distance":
        w = np.maximum(0.0, 1.0 - d * d / extent) * real[:, None, :]
    x64 = x.astype(np.float64)
    rs = x64.sum(1)[idx]
    if kind in ("drop_last", "drop_h64", "drop_tail4"):      # the dropped neighbours are still counted: only the sum misses them
        num, _ = O.neighbour_count(c["nbr"], x)
    else:
        counted = real & ((rs >= 0) if kind == "count_ge0" else (rs > 0))
        if kind == "dup_counted_once":
            for r in range(nq):
                _, first = np.unique(np.where(real[r], nbr[r], -1 - np.arange(H)), return_index=True)
                keep = np.zeros(H, bool)
                keep[first] = True
                counted[r] &= keep
        if kind == "count_w_positive":
            counted &= w.max(1) > 0
        raw = counted.sum(1).astype(np.float64)
        num = raw if kind == "no_floor" else np.maximum(raw, 1.0)
    if kind == "divide_by_H":
        num = np.full(nq, float(H))
    with np.errstate(divide="ignore", invalid="ignore"):
        wf = np.einsum("qkh,qhc->qkc", w, x64[idx] * real[:, :, None]) / num[:, None, None]
    if kind == "drop_k14":
        wf[:, 14] = 0
    elif kind == "channel_permutation":
        r, cb = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
        perm = np.arange(64)
        perm[(4 * r + cb).ravel()] = (16 * cb + r).ravel()
        wf = wf.reshape(nq, 15, cin // 64, 64)[..., perm].reshape(nq, 15, cin)
    elif kind == "groups_ge4_zero":
        wf[:, :, 256:] = 0
    elif kind == "unswizzled_rows":
        nb = K.blocks(nq)
        out = np.zeros_like(wf)
        for row in range(nq):
            src = _swizzle(row // 4, nb) * 4 + row % 4
            if src < nq:
                out[row] = wf[src]
        wf = out
    return wf.reshape(nq, -1)


def mutant_contrib(c, kind):
    rows = O.contrib(*_args(c), c["dwf"])
    if kind == "bwd_no_inv_num":
        num, _ = O.neighbour_count(c["nbr"], c["x"])
        rows = rows * np.repeat(num, c["H"])[:, None]
    elif kind == "bwd_channel_tail_dropped":
        rows = rows.copy()
        rows[:, 64 * (c["cin"] // 64):] = 0
    return rows


# mutant -> the named cases that must reject it (and why that case)
FORWARD_MUTANTS = {
    "count_ge0": ["m1-c64", "g-c1"],                    # the `far` row lists the zero-sum support: 3 instead of 2
    "count_w_positive": ["m1-c64", "g-c63"],            # the `far` row: the far support counts without any influence
    "divide_by_H": ["m1-c64", "g-c1"],
    "no_floor": ["m1-c64", "g-c63"],                    # `allpad` / `floor` rows: 0 / 0
    "drop_k14": ["m1-c64", "g-c9-H129", "m4-c512"],
    "drop_last": ["m1-H4-nq5", "m1-H128", "g-c64-H130"],      # the `lastonly` row
    "drop_h64": ["m1-H65-nq67", "m2-H65", "m4-c320-H65", "g-c8-H65"],
    "drop_tail4": ["m1-H127", "m1-H65-nq67", "m1-H2-nq3", "m4-c384-H127"],
    "squared_distance": ["m1-c64", "g-c1"],
    "pad_as_last_row": ["m1-c64", "m1-ns1", "g-c3-ns1"],
    "negative_from_end": ["m1-c64", "g-c63", "m4-c256"],       # the `padkinds` row
    "dup_counted_once": ["m1-c64", "g-c63", "m1-ns1", "m2-H3"],      # the `dup` row: num = 1, not H
    "dup_listed_once": ["m1-c64", "g-c63", "m2-H128"],        # the `self` row lists its first support again at h = H - 1
    "channel_permutation": ["m1-c64", "m2-c128", "m4-c320", "m1-c192"],
    "groups_ge4_zero": ["m4-c320", "m4-c384", "m4-c512"],
    "unswizzled_rows": ["m1-H63-nq33", "m1-H65-nq67", "m4-c320", "m4-c512"],      # 9, 17, 9 and 17 blocks
}
BACKWARD_MUTANTS = {
    "bwd_no_inv_num": ["b-c1", "b-c64-H65", "b-c512"],
    "bwd_channel_tail_dropped": ["b-c68", "b-c130", "b-c132", "b-c260-H3", "b-c60-H2"],
}


@pytest.mark.parametrize("kind", list(FORWARD_MUTANTS))
def test_forward_mutant_is_rejected(kind):
    for name in FORWARD_MUTANTS[kind]:
        c = K.ALL[name]
        wf, _, _ = O.weighted(*_args(c))
        r, at = O.compare_rows(mutant_weighted(c, kind), wf, O.bound_weighted(*_args(c)))
        assert r > 1.0 and at is not None, (kind, name, r)


@pytest.mark.parametrize("kind", list(BACKWARD_MUTANTS))
def test_backward_mutant_is_rejected(kind):
    for name in BACKWARD_MUTANTS[kind]:
        c = K.ALL[name]
        rows = mutant_contrib(c, kind)
        r, at = O.compare_rows(rows, O.contrib(*_args(c), c["dwf"]), O.bound_contrib(*_args(c), c["dwf"]))
        assert r > 1.0 and at is not None, (kind, name, r)
        r, _ = O.compare_rows(O.scatter_rows(rows, c["nbr"], c["ns"]), O.d_x_from_dwf(*_args(c), c["dwf"]),
                              O.bound_dx(*_args(c), c["dwf"]))
        assert r > 1.0, (kind, name, "d_x", r)


def test_identity_is_not_rejected():
    """the comparison accepts the oracle itself, and the oracle rounded to float32 (the final rounding is in the bound)"""
    for name in ("m1-c64", "g-c1", "m4-c512"):
        c = K.ALL[name]
        wf, _, _ = O.weighted(*_args(c))
        assert O.compare_rows(wf, wf, O.bound_weighted(*_args(c))) == (0.0, None)
        assert O.compare_rows(wf.astype(F32), wf, O.bound_weighted(*_args(c)))[0] <= 1.0
    bad = np.zeros((2, 2))
    bad[1, 0] = np.nan
    assert O.compare_rows(bad, np.zeros((2, 2)), np.ones((2, 2))) == (np.inf, (1, 0))
    assert O.compare_rows(np.ones((1, 1)), np.zeros((1, 1)), np.zeros((1, 1))) == (np.inf, (0, 0))


# ------------------------------------------------------------------------------------------- reverse table, pools
@pytest.mark.parametrize("name", list(K.REVERSE))
def test_reverse_table_oracle(name):
    c = K.REVERSE[name]
    nbr, ns = c["nbr"], c["ns"]
    rev_t, start = O.reverse_table(nbr, ns)
    flat = nbr.reshape(-1)
    real = (flat >= 0) & (flat < ns)
    assert sorted(rev_t) == list(range(len(flat))) and start[0] == 0 and start[ns] == real.sum()
    for r in range(ns):
        run = rev_t[start[r]:start[r + 1]]
        assert (flat[run] == r).all() and (np.diff(run) > 0).all()
    assert not real[rev_t[start[ns]:]].any()
    if c["kind"] == "allpad":
        assert start[ns] == 0
    if c["kind"] == "nopad":
        assert start[ns] == len(flat)
    if c["kind"] == "negatives":
        assert (flat < 0).any() and (flat > ns).any()


@pytest.mark.parametrize("name", list(K.POOLS))
def test_pool_oracle_and_mutants(name):
    c = K.POOLS[name]
    x, inds, dout, ns = c["x"], c["inds"], c["dout"], c["ns"]
    out, amax = O.max_pool(x, inds)
    dx = O.max_pool_grad(x, inds, dout)
    assert np.array_equal(out.astype(F32), out) and np.array_equal(dx.astype(F32), dx), "not float32-exact"
    g, real = O._padded(x, inds)
    for row, plant in c["plants"].items():
        if plant[0] == "tie":
            h0, h1 = plant[1:]
            assert inds[row, h0] != inds[row, h1] and np.array_equal(g[row, h0], g[row, h1])
            assert (amax[row] == h0).all() and (out[row] == g[row, h0]).all()
            # mutant: the last maximum -- moves the gradient from one support row to the other
            last = g.shape[1] - 1 - g[:, ::-1].argmax(1)
            assert (last[row] == h1).all()
            assert dout[row].any() and dx[inds[row, h0]].any()
        elif plant[0] == "shadowmax":
            h = plant[1]
            assert not real[row, h] and out[row, 0] == 0 and amax[row, 0] == h and (g[row, real[row], 0] < 0).all()
            # mutant: the shadow entry as -inf -- the maximum becomes a negative feature
            gm = np.where(real[:, :, None], g, -np.inf)
            assert gm.max(1)[row, 0] < 0
        elif plant[0] == "allshadow":
            assert not real[row].any() and not out[row].any() and not amax[row].any()
    # gradients: every dout lands on its arg-max row or, for a shadow arg-max, nowhere
    tgt = np.take_along_axis(inds.astype(np.int64), amax, 1)
    lost = ~((tgt >= 0) & (tgt < ns))
    assert np.isclose(dx.sum(), dout.astype(np.float64)[~lost].sum())
    cp = O.closest_pool(x, inds)
    assert np.array_equal(cp, g[:, 0])
    assert np.isclose(O.closest_pool_grad(x, inds, dout).sum(), dout.astype(np.float64)[real[:, 0]].sum())

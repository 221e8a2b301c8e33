"""The sparse-conv oracle, its cases and the library's host-side kernel choice, without a GPU.

* tests/spconv_oracle.py against a triple Python loop on tiny shapes, and against oracle/me_oracle.py::conv_forward (values
  and, through autograd in float64, both gradients) on a real coordinate set, same-level, strided and transposed.
* every exact / piece-crossing case proves its own exactness from its actual values (spconv_cases.prove_exact).
* apr_spconv_route, apr_spconv_tile_variant, apr_dense_gemm_bf3_variant and apr_spconv_wgrad_plan are walked over every
  case with stand-in pointers of the case's alignment: the answers must be the literals the cases carry.
* the cases have teeth: numpy restatements of the kernels' STRUCTURE (tiles, 16-pair groups, per-offset lists, units of 64 G
  pairs, triples, 512-row blocks and splits) reproduce the oracle bit for bit on every exact case, and each of them with
  one planted fault fails at least one named case.  No mutated kernel is built or run on a GPU.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import spconv_cases as K
import spconv_oracle as O
from apr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------- the oracle against loops
def _loop_forward(x, nbr, W, scale, shift, res, relu):
    n_out, K_ = nbr.shape
    out = np.zeros((n_out, W.shape[2]))
    for j in range(n_out):
        for c in range(W.shape[2]):
            s = 0.0
            for k in range(K_):
                if nbr[j, k] >= 0:
                    for ci in range(W.shape[1]):
                        s += float(x[nbr[j, k], ci]) * float(W[k, ci, c])
            s = s * float(scale[c]) + float(shift[c]) + float(res[j, c])
            out[j, c] = max(s, 0.0) if relu else s
    return out


@pytest.mark.parametrize("relu", [False, True])
def test_oracle_equals_a_triple_loop(relu):
    rng = np.random.default_rng(1)
    n_in, n_out, K_, cin, cout = 7, 6, 5, 3, 4
    x, W = rng.integers(-7, 8, (n_in, cin)).astype(F32), rng.integers(-3, 4, (K_, cin, cout)).astype(F32)
    nbr = K.random_map(rng, n_out, K_, n_in, 0.5)
    scale, shift = rng.choice([0.5, 2.0], cout).astype(F32), rng.integers(-5, 6, cout).astype(F32)
    res, dy = rng.integers(-9, 10, (n_out, cout)).astype(F32), rng.integers(-7, 8, (n_out, cout)).astype(F32)
    assert np.array_equal(O.conv_forward(x, nbr, W, scale, shift, res, relu), _loop_forward(x, nbr, W, scale, shift, res, relu))
    dw, dx = np.zeros((K_, cin, cout)), np.zeros((n_in, cin))
    for j in range(n_out):
        for k in range(K_):
            i = nbr[j, k]
            if i >= 0:
                for ci in range(cin):
                    for c in range(cout):
                        dw[k, ci, c] += float(x[i, ci]) * float(dy[j, c])
                        dx[i, ci] += float(dy[j, c]) * float(W[k, ci, c])
    assert np.array_equal(O.conv_wgrad(x, nbr, dy), dw)
    assert np.array_equal(O.conv_dx(dy, nbr, W, n_in), dx)
    v = O.conv_forward(x, nbr, W, l2norm=True)
    plain = O.conv_forward(x, nbr, W)
    nz = np.abs(plain).sum(1) > 0
    assert np.allclose((v[nz] ** 2).sum(1), 1.0, rtol=0, atol=1e-14) and np.isnan(v[~nz]).all()
    ident = O.conv_forward(x, None, W[:1])
    assert np.array_equal(ident, x.astype(np.float64) @ W[0].astype(np.float64))


@pytest.mark.parametrize("kind", ["same", "strided", "transposed"])
def test_oracle_equals_me_oracle_on_real_coordinates(kind):
    from oracle import me_oracle as OME
    rng = np.random.default_rng(2)
    clouds = [OME.sparse_quantize(rng.uniform(-2, 2, (300, 3)).astype(F32) / F32(0.5), return_index=True)[0] for _ in range(2)]
    Cc = OME.batched_coordinates(clouds)
    cin, cout = 5, 7
    W = torch.from_numpy(rng.standard_normal((27, cin, cout))).requires_grad_(True)
    cm = OME.SparseTensor(torch.zeros(len(Cc), 1, dtype=torch.float64), coordinates=Cc)
    if kind == "transposed":
        coarse = OME.conv_forward(cm, torch.zeros(27, 1, 1, dtype=torch.float64), 3, 2)
        n_in = coarse.F.shape[0]
        F = torch.from_numpy(rng.standard_normal((n_in, cin))).requires_grad_(True)
        y = OME.conv_forward(coarse._like(F), W, 3, 2, transpose=True)
        nbr = OME.transpose_map(cm.coordinate_manager.get_map(1, 2, 3), len(Cc))
    else:
        n_in = len(Cc)
        F = torch.from_numpy(rng.standard_normal((n_in, cin))).requires_grad_(True)
        y = OME.conv_forward(cm._like(F), W, 3, 1 if kind == "same" else 2)
        nbr = cm.coordinate_manager.get_map(1, 1 if kind == "same" else 2, 3)
    assert (nbr >= 0).sum() > 2 * nbr.shape[0] or kind != "same"
    dy = rng.standard_normal(tuple(y.F.shape))
    (y.F * torch.from_numpy(dy)).sum().backward()
    x, Wn = F.detach().numpy(), W.detach().numpy()
    assert np.allclose(O.conv_forward(x, nbr, Wn), y.F.detach().numpy(), rtol=0, atol=1e-12)
    assert np.allclose(O.conv_wgrad(x, nbr, dy), W.grad.numpy(), rtol=0, atol=1e-11)
    assert np.allclose(O.conv_dx(dy, nbr, Wn, n_in), F.grad.numpy(), rtol=0, atol=1e-12)


def test_split3_is_exact_and_truncating():
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(4000) * np.exp(rng.uniform(-20, 20, 4000))).astype(F32)
    h, m, l = O.split3(a)
    assert np.array_equal(h + m + l, a.astype(np.float64))
    for p in (h, m, l):      # each piece is a bf16: 8 significant bits
        assert np.array_equal(p.astype(F32).view(np.uint32) & 0xFFFF, np.zeros(len(a), np.uint32))
    nz = a != 0
    assert np.all(np.abs(m[nz]) < np.abs(a[nz]) * 2.0 ** -7) and np.all(np.abs(l[nz]) < np.abs(a[nz]) * 2.0 ** -14)
    assert np.all(np.abs(h) <= np.abs(a))


def test_bounds_hold_for_float32_restatements_in_the_kernels_orders():
    """a float32 chain (one rounding per product-add) and the six-term split product in float32 stay inside the bounds,
    and the bound is not vacuous: a result computed with bf16-rounded x does not"""
    c = K.get("ws_bf3_c128_o64/bound")
    x, W, nbr = c["x"], c["W"], c["nbr"]
    ref = O.contract(x, nbr, W)
    chain = np.zeros(ref.shape, F32)
    split = np.zeros(ref.shape, F32)
    xh, xm, xl = (p.astype(F32) for p in O.split3(x))
    wh, wm, wl = (p.astype(F32) for p in O.split3(W))
    for k in range(27):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        i = nbr[j, k]
        for ci in range(c["cin"]):
            chain[j] = chain[j] + x[i, ci:ci + 1] * W[k, ci:ci + 1]          # float32 product and add: two roundings per term
        for a, b in ((xl, wh), (xh, wl), (xm, wm), (xm, wh), (xh, wm), (xh, wh)):
            split[j] = split[j] + (a[i].astype(np.float64) @ b[k].astype(np.float64)).astype(F32)
    b32 = O.forward_bound("ws", x, nbr, W)
    b3 = O.forward_bound("ws_bf3", x, nbr, W)
    assert O.worst_ratio(chain, ref, 2 * b32) <= 1.0      # the chain above rounds twice per term, the MFMA / fma chain once
    assert O.worst_ratio(split, ref, b3) <= 1.0
    dropped_m = O.contract(xh.astype(np.float64) + xl, nbr, W)
    print("middle piece dropped: worst ratio", O.worst_ratio(dropped_m, ref, b3))
    assert O.worst_ratio(dropped_m, ref, b3) > 1.0


# ------------------------------------------------------------------------------------------------------ the cases
EXACT = [n for n in K.REGISTRY if K.REGISTRY[n].meta["kind"] in ("exact", "cross")]


def test_every_exact_case_proves_its_exactness():
    assert len(EXACT) > 100
    for name in EXACT:
        c = K.get(name)
        K.prove_exact(c)
        ref = O.conv_forward(c["x"], c["nbr"], c["W"], c["scale"], c["shift"], c["res"], c["relu"], n_out=c["n_out"])
        assert np.array_equal(ref.astype(F32).astype(np.float64), ref), name
    for name, build in K.WGRAD.items():
        c = build()
        if c["kind"] == "exact":
            n_pairs = c["n_out"] if c["nbr"] is None else int((c["nbr"] >= 0).sum(0).max())
            assert np.abs(c["x"]).max() <= 7 and np.abs(c["dy"]).max() <= 7 and 49 * n_pairs < 2 ** 24, name


def test_cases_reach_the_edges_they_name():
    c = K.get("pairs_counts_tm32/exact")
    assert sorted((c["nbr"][:32] >= 0).sum(0)[[3, 4, 5, 9]]) == [15, 16, 17, 32] and (c["nbr"][:32] >= 0).sum() == 80
    c = K.get("pairs_tm64_cout256/exact")
    assert list((c["nbr"][:64] >= 0).sum(0)[[3, 4, 5, 9]]) == [15, 16, 17, 64]
    assert (K.get("pairs_full27/exact")["nbr"] >= 0).all()
    for a in (1, 2, 3, 5):
        assert ((K.get(f"pairs_items{a}/exact")["nbr"] >= 0).sum(0) > 0).sum() == a
    assert (K.get("pairs_empty_tile/exact")["nbr"][32:64] == -1).all()
    c = K.get("pairs_same_row/exact")
    assert set(np.unique(c["nbr"])) == {-1, c["n_in"] - 1}
    c = K.get("ws_bf3_counts_n513/exact")
    assert list((c["nbr"] >= 0).sum(0)[:5]) == [0, 1, 63, 64, 65]
    c = K.get("ws3_mixed_n257/exact")
    pat = ((c["nbr"].reshape(-1, 9, 3) >= 0) * np.array([1, 2, 4])).sum(2)
    assert set(np.unique(pat)) == set(range(8))
    pat = ((K.get("ws3_alone/exact")["nbr"].reshape(-1, 9, 3) >= 0) * np.array([1, 2, 4])).sum(2)
    assert set(np.unique(pat)) == set(range(8)) and ((pat > 0).sum(1) <= 1).all()
    c = K.get("os_r64_n129/exact")
    assert list((c["nbr"][:64] >= 0).sum(0)[[0, 13, 26]]) == [1, 16, 17] and (c["nbr"][64:128] == -1).all()
    assert ((K.get("os_groups/exact")["nbr"][:160] >= 0).sum(0) == 160).all()      # 10 groups per (tile, offset)
    for kind in ("bound",):
        c = K.get("pairs_c64_64_n65/" + kind)
        ref = O.contract(c["x"], c["nbr"], c["W"])
        mag = O.contract(np.abs(c["x"]), c["nbr"], np.abs(c["W"]))
        cancelled = np.arange(3, 65, 7)
        assert (np.abs(ref[cancelled]) <= 1e-12 * mag[cancelled]).all() and (mag[cancelled] > 0).all()      # rows that cancel to zero
        rows = np.abs(c["x"]).max(1)
        assert rows.max() / rows.min() > 1e4
    for name in K.names(kind="poison"):
        c = K.get(name)
        tbl = O._table(c["nbr"], c["n_out"])
        ref = np.bincount(tbl[tbl >= 0], minlength=c["n_in"])
        assert np.isnan(c["x"][ref == 0]).all() and np.isnan(c["x"][c["poison"]]).all()
        assert np.isfinite(np.delete(c["x"], np.r_[np.nonzero(ref == 0)[0], c["poison"]], axis=0)).all()
        hit = (tbl == c["poison"]).any(1)
        assert 0 < hit.sum() < c["n_out"], name
        assert not c["relu"]
    assert (K.WGRAD["wgrad_same_n1025/exact"]()["nbr"][:, 13] >= 0).all()
    assert not (K.WGRAD["wgrad_same_sparse_centre/exact"]()["nbr"][:, 13] >= 0).all()
    assert (K.WGRAD["wgrad_c64_o64_n511/exact"]()["nbr"][:, 4] == -1).all()


# ------------------------------------------------------------------------------------------- the host's kernel choice
BASE = 0x10000


def _standin(i, off=0):
    return BASE + 0x1000 * i + 4 * off


def _desc_of(m):
    """apr_spconv_desc with stand-in pointers of the case's alignment; nothing dereferences them"""
    d = _lib.SpconvDesc()
    lay = m["lay"]
    d.inp, d.ldi = _standin(1, lay["x"][1]), m["cin"] + lay["x"][0]
    d.out, d.ldo = _standin(2, lay["out"][1]), m["cout"] + lay["out"][0]
    d.residual, d.ldr = _standin(3, lay["res"][1]), m["cout"] + lay["res"][0]
    d.nbr = None if m["identity"] else _standin(4)
    d.n_out, d.K, d.cin, d.cout = m["n_out"], m["K"], m["cin"], m["cout"]
    d.scale, d.shift, d.w_packed = _standin(5), _standin(6), _standin(7)
    d.l2norm = int(m["l2norm"])
    if m["bf3"]:
        d.w_bf3 = _standin(8)
    if m["aux"] in ("pairs", "triples"):
        d.plist, d.counters, d.ws3 = _standin(9), _standin(10), int(m["aux"] == "triples")
    if m["aux"] == "os":
        d.os_pairs, d.os_rows = _standin(11), 64
    return d


def test_ids_of_the_binding_are_the_headers():
    header = open(os.path.join(ROOT, "include", "apr_hip.h")).read()
    enum = re.search(r"enum \{ (APR_TILE_NONE = 0,[^}]*)\};", header).group(1)
    names = [n.strip().split(" ")[0] for n in enum.replace("\n", " ").split(",")]
    assert names == ["APR_TILE_NONE", "APR_TILE_PAIRS", "APR_TILE_MFMA", "APR_TILE_DENSE", "APR_TILE_BIGK", "APR_TILE_SMALLCIN",
                     "APR_TILE_GENERIC", "APR_TILE_DENSE_BF3"]
    assert [_lib.TILE_NONE, _lib.TILE_PAIRS, _lib.TILE_MFMA, _lib.TILE_DENSE, _lib.TILE_BIGK, _lib.TILE_SMALLCIN, _lib.TILE_GENERIC,
            _lib.TILE_DENSE_BF3] == list(range(8))
    assert "#define APR_TILE_ID(kernel, tm, cn, ck) (((kernel) << 24) | ((tm) << 14) | ((cn) << 7) | (ck))" in header
    assert "#define APR_TILE_FLAG (1 << 22)" in header and "#define APR_TILE_NW8 (1 << 23)" in header
    assert "enum { APR_WGRAD_BF3 = 1, APR_WGRAD_PARTIAL = 2 };" in header
    assert _lib.tile_id(_lib.TILE_PAIRS, 64, 32, 64, flag=True) == (1 << 24) | (64 << 14) | (32 << 7) | 64 | (1 << 22)
    assert (_lib.WGRAD_BF3, _lib.WGRAD_PARTIAL) == (1, 2)


def test_every_forward_case_takes_the_route_and_variant_it_names(lib):
    seen = set()
    for name, build in K.REGISTRY.items():
        m = build.meta
        d = _desc_of(m)
        if m["aux"] == "rows":
            assert lib.apr_dense_rows_bf3_ok(m["cin"], m["cout"]) == 1 and m["route"] == K.DENSE_ROWS, name
            continue
        assert lib.apr_spconv_route(C.byref(d)) == m["route"], name
        if m["route"] == K.TILE:
            got = lib.apr_spconv_tile_variant(C.byref(d))
            assert got == m["variant"], f"{name}: {got:#x} != {m['variant']:#x}"
        elif m["route"] == K.DENSE_GEMM:
            assert lib.apr_dense_gemm_bf3_variant(m["n_out"], m["cin"], m["cout"]) == m["variant"], name
        else:
            assert m["variant"] is None
        seen.add((m["route"], m["variant"]))
    T, P, M = K.TILE, _lib.TILE_PAIRS, _lib.TILE_MFMA
    tid = _lib.tile_id
    # all eight 32- / 64-row instances of k_spconv_pairs that shapes can reach without a switch ... (TM 64 needs >= 400 workgroups)
    for v in (tid(P, 32, 32, 32), tid(P, 32, 32, 64), tid(P, 32, 64, 32), tid(P, 32, 64, 64), tid(P, 64, 64, 32), tid(P, 64, 32, 64),
              tid(P, 32, 64, 64, flag=True), tid(P, 32, 32, 64, flag=True),
              tid(M, 32, 64, 64), tid(M, 32, 64, 32), tid(M, 32, 32, 64), tid(M, 32, 32, 32), tid(M, 64, 32, 32), tid(M, 64, 64, 64),
              tid(_lib.TILE_DENSE, 64, 64, 64), tid(_lib.TILE_DENSE, 128, 64, 64), tid(_lib.TILE_BIGK), tid(_lib.TILE_SMALLCIN, 64, 0, 1),
              tid(_lib.TILE_SMALLCIN, 64, 0, 3), tid(_lib.TILE_GENERIC)):
        assert (T, v) in seen, hex(v)
    for v in (tid(_lib.TILE_DENSE_BF3, 64, 64, 64), tid(_lib.TILE_DENSE_BF3, 64, 64, 64, flag=True),
              tid(_lib.TILE_DENSE_BF3, 128, 64, 64), tid(_lib.TILE_DENSE_BF3, 128, 64, 64, flag=True)):
        assert (K.DENSE_GEMM, v) in seen, hex(v)
    assert {r for r, _ in seen} == {K.TILE, K.WS, K.WS_BF3, K.WS3, K.OS, K.DENSE_ROWS, K.DENSE_GEMM}


def _plain(K_, cin, cout, n_out, nbr=True, **kw):
    m = dict(lay=K.ALIGNED, cin=cin, cout=cout, K=K_, n_out=n_out, identity=not nbr, l2norm=False, bf3=False, aux=None)
    d = _desc_of(m)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_tile_variant_thresholds_read_off_the_rule(lib):
    """literals from spconv_fwd_plain's rule: TM 64 from 400 workgroups of 64 rows x CN columns; k_spconv_mfma for K 28..32
    and for unaligned out / residual rows, TM 64 from 32 768 rows; k_dense_gemm from 144 workgroups, G = 2 from 512"""
    tid, P, M, D = _lib.tile_id, _lib.TILE_PAIRS, _lib.TILE_MFMA, _lib.TILE_DENSE
    v = lambda d: lib.apr_spconv_tile_variant(C.byref(d))
    assert v(_plain(27, 64, 64, 25536)) == tid(P, 32, 64, 64) and v(_plain(27, 64, 64, 25537)) == tid(P, 64, 64, 64)      # 399 / 400
    assert v(_plain(27, 64, 32, 25537)) == tid(P, 64, 32, 64) and v(_plain(27, 32, 32, 25536)) == tid(P, 32, 32, 32)
    assert v(_plain(27, 96, 128, 12737)) == tid(P, 64, 64, 32) and v(_plain(27, 96, 128, 12736)) == tid(P, 32, 64, 32)    # 2 x 200
    assert v(_plain(27, 64, 64, 100, l2norm=1)) == tid(P, 32, 64, 64, flag=True)
    assert v(_plain(27, 64, 128, 100, l2norm=1)) == tid(P, 32, 64, 64)                  # the row spans two tiles: not fused
    assert v(_plain(27, 64, 64, 0)) == _lib.TILE_NONE
    for K_ in (28, 32):
        assert v(_plain(K_, 64, 64, 1000)) == tid(M, 32, 64, 64)
    assert v(_plain(33, 64, 64, 1000)) == tid(_lib.TILE_BIGK) and v(_plain(126, 64, 64, 1000)) == tid(_lib.TILE_GENERIC)
    assert v(_plain(27, 64, 64, 32767, ldo=65)) == tid(M, 32, 64, 64) and v(_plain(27, 64, 64, 32768, ldo=65)) == tid(M, 64, 64, 64)
    assert v(_plain(27, 64, 64, 1000, residual=BASE + 0x3000 + 4)) == tid(M, 32, 64, 64)
    assert v(_plain(27, 64, 64, 1000, inp=BASE + 0x1000 + 4)) < 0 and b"16-B aligned input rows" in lib.apr_last_error()
    assert v(_plain(27, 64, 64, 1000, ldi=65)) < 0
    assert v(_plain(27, 3, 64, 1000, ldi=3)) == tid(_lib.TILE_SMALLCIN, 64, 0, 3)
    assert v(_plain(343, 1, 32, 1000, ldi=1)) == tid(_lib.TILE_GENERIC) and v(_plain(256, 1, 32, 1000, ldi=1)) == tid(_lib.TILE_SMALLCIN, 64, 0, 1)
    assert v(_plain(1, 64, 512, 1088, nbr=False)) == tid(P, 32, 64, 64) and v(_plain(1, 64, 512, 1089, nbr=False)) == tid(D, 64, 64, 64)
    assert v(_plain(1, 64, 512, 8064, nbr=False)) == tid(D, 64, 64, 64) and v(_plain(1, 64, 512, 8065, nbr=False)) == tid(D, 128, 64, 64)
    assert v(_plain(1, 64, 512, 8065, nbr=False, scale=BASE + 0x5000 + 4)) == tid(P, 64, 64, 64)     # scale off 16 bytes: tile kernel
    assert lib.apr_spconv_tile_variant(None) < 0
    B = _lib.TILE_DENSE_BF3
    assert lib.apr_dense_gemm_bf3_variant(8064, 64, 512) == tid(B, 64, 64, 64)
    assert lib.apr_dense_gemm_bf3_variant(8065, 64, 512) == tid(B, 128, 64, 64)
    assert lib.apr_dense_gemm_bf3_variant(100, 128, 64) == tid(B, 64, 64, 64, flag=True)
    assert [lib.apr_spconv_os_tile_rows(20000, ci, co) for (ci, co) in K.OS_R] == list(K.OS_R.values())


def test_every_wgrad_case_gets_the_plan_it_names(lib):
    plan = (C.c_int32 * 6)()
    for name, build in K.WGRAD.items():
        m = build.meta
        ldx = m["cin"] + 4 + (-m["x_off"]) % 4
        assert lib.apr_spconv_wgrad_plan(_standin(1, m["x_off"]), ldx, _standin(2, 4), m["cout"] + 4, m["n_out"], m["K"], m["cin"],
                                         m["cout"], int(m["same_level"]), plan) == 0
        assert tuple(plan) == tuple(m["plan"]), f"{name}: {tuple(plan)}"
    kinds = {(b.meta["plan"][1], b.meta["plan"][2]) for b in K.WGRAD.values() if b.meta["plan"][0] == _lib.WGRAD_BF3}
    assert kinds == {(32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (64, 128)}            # all six instances
    arms = {(p[4] == 4 * p[3]) for p in (b.meta["plan"] for b in K.WGRAD.values()) if p[5] >= 0}
    assert arms == {True, False}                                                             # S_c = 4 S and S_c = nrb
    assert lib.apr_spconv_wgrad_plan(_standin(1), 64, _standin(2), 64, 0, 27, 64, 64, 0, plan) < 0


# ------------------------------------------------------------------------ restatements of the kernels' structure, mutants
GUARD = 40          # columns behind the slice in the restatements' output buffer
SENT = -777.25


DT = {0: np.float64}      # the restatements' arithmetic: float64 (exact on the exact cases) or float32 (held to the bounds)


def _mul(a, w, bf3=False, drop_m=False):
    """[rows, ck] @ [ck, cout] in DT: exact in float64 on the exact cases, a float32 sum in BLAS's order otherwise; bf3: the
    six kept terms of the split, small first, each a sum of exact products"""
    dt = DT[0]
    if not bf3:
        return a.astype(dt) @ w.astype(dt)
    ah, am, al = (p.astype(dt) for p in O.split3(a))
    wh, wm, wl = (p.astype(dt) for p in O.split3(w))
    if drop_m:
        am = np.zeros_like(am)
    return al @ wh + ah @ wl + am @ wm + am @ wh + ah @ wm + ah @ wh


def _finish(c, acc, buf, row0, rows, fault):
    v = acc[:rows]
    if c["scale"] is not None:
        v = v * c["scale"].astype(v.dtype)
    if c["shift"] is not None:
        v = v + c["shift"].astype(v.dtype)
    if c["res"] is not None:
        v = v + c["res"][row0:row0 + rows].astype(v.dtype)
    buf[row0:row0 + rows, :c["cout"]] = np.maximum(v, 0) + 0 * v if c["relu"] else v
    if fault == "guard_epilogue":      # the epilogue walks whole 64-column blocks
        wide = -(-c["cout"] // 64) * 64
        buf[row0:row0 + rows, c["cout"]:wide] = 0.0


def restate_tiles(c, TM, CK, fault=None, bf3=False):
    """k_spconv_pairs / k_spconv_bigk / k_os_conv: tiles of TM rows, per-offset compacted lists, chunks of CK channels,
    groups of 16 pairs (padded lanes gather pair 0 and are not written back), an accumulator tile, the epilogue"""
    n_out, K_, cin, cout = c["n_out"], c["K"], c["cin"], c["cout"]
    nbr = O._table(c["nbr"], n_out)
    x, W = c["x"], c["W"]
    buf = np.full((n_out, cout + GUARD), SENT)
    for row0 in range(0, n_out, TM):
        rows = min(TM, n_out - row0)
        if fault == "tail_tile" and rows < TM:
            continue
        acc = np.zeros((TM, cout), DT[0])
        for k in range(K_):
            r = np.nonzero(nbr[row0:row0 + rows, k] >= 0)[0]
            cnt = len(r)
            if not cnt:
                continue
            idx = nbr[row0 + r, k]
            ngroups = -(-cnt // 16)
            if fault == "last_group" and ngroups > 1:
                ngroups -= 1
            for ch in range(cin // CK if cin >= CK else 1):
                lo, hi = ch * CK, min((ch + 1) * CK, cin)
                wk = W[k, lo:hi]
                if fault == "chunk_weights" and ch == 1:
                    wk = W[k, 0:CK]
                for g in range(ngroups):
                    p = 16 * g + np.arange(16)
                    valid = p < cnt
                    pc = np.where(valid, p, 0)
                    prod = _mul(x[idx[pc], lo:hi], wk, bf3, fault == "middle_piece")
                    keep = np.ones(16, bool) if fault == "padded_writeback" else valid
                    np.add.at(acc, r[pc][keep], prod[keep])
        _finish(c, acc, buf, row0, rows, fault)
    return buf


def restate_lists(c, fault=None, bf3=False, target=768):
    """k_pairs_build + k_ws_gemm[_bf3] + k_ws_reduce: one list per offset over the whole table, units of 64 G pairs, groups
    of 16, a product row per pair, the reduce over the row's K pair ids in ascending offset order"""
    n_out, K_, cin, cout = c["n_out"], c["K"], c["cin"], c["cout"]
    nbr, x, W = c["nbr"], c["x"], c["W"]
    prod = np.zeros((K_ * n_out, cout), DT[0])
    pid = np.full((n_out, K_), -1, np.int64)
    P = int((nbr >= 0).sum(0).max())
    G = min(max(-(-(-(-P // 64) * (cout // 64)) // target), 1), 64)
    for k in range(K_):
        j = np.nonzero(nbr[:, k] >= 0)[0]
        pid[j, k] = k * n_out + np.arange(len(j))
        for u0 in range(0, len(j), 64 * G):
            unit = j[u0:u0 + 64 * G]
            ngroups = -(-len(unit) // 16)
            if fault == "last_group" and ngroups > 1 and u0 + 64 * G >= len(j):
                ngroups -= 1
            for g in range(ngroups):
                rows = unit[16 * g:16 * g + 16]
                acc = np.zeros((len(rows), cout), DT[0])
                for ch in range(cin // 64):
                    wk = W[k, 64 * ch:64 * ch + 64] if not (fault == "chunk_weights" and ch == 1) else W[k, 0:64]
                    acc += _mul(x[nbr[rows, k], 64 * ch:64 * ch + 64], wk, bf3, fault == "middle_piece")
                prod[k * n_out + u0 + 16 * g:k * n_out + u0 + 16 * g + len(rows)] = acc
    buf = np.full((n_out, cout + GUARD), SENT)
    acc = np.zeros((n_out, cout), DT[0])
    for k in range(K_ - 1 if fault == "reduce_k_minus_1" else K_):
        j = np.nonzero(pid[:, k] >= 0)[0]
        acc[j] += prod[pid[j, k]]
    _finish(c, acc, buf, 0, n_out, fault)
    return buf


def restate_triples(c, fault=None):
    """k_pairs3_build + k_ws3_gemm_bf3 + k_ws_reduce: an entry of triple t is a row with any of offsets 3 t .. 3 t + 2; an
    absent slot gathers a zero row; one product row per entry; the reduce over 9 ids"""
    n_out, cout = c["n_out"], c["cout"]
    nbr, x, W = c["nbr"], c["x"], c["W"]
    acc = np.zeros((n_out, cout), DT[0])
    zero = np.zeros((1, c["cin"]), F32)
    for t in range(8 if fault == "reduce_k_minus_1" else 9):
        rows = np.nonzero((nbr[:, 3 * t:3 * t + 3] >= 0).any(1))[0]
        for b in range(3):
            i = nbr[rows, 3 * t + b]
            absent = x[np.zeros(len(rows), int)] if fault == "absent_row0" else np.repeat(zero, len(rows), 0)
            a = np.where((i >= 0)[:, None], x[np.maximum(i, 0)], absent)
            acc[rows] += _mul(a, W[3 * t + b], True, fault == "middle_piece")
    buf = np.full((n_out, cout + GUARD), SENT)
    _finish(c, acc, buf, 0, n_out, fault)
    return buf


def restate_dense(c, TM, fault=None, bf3=False):
    """k_dense_gemm[_bf3] / k_dense_rows_bf3: tiles of TM rows, chunks of 64 (rows kernel: 32) channels through two buffers"""
    n_out, cin, cout = c["n_out"], c["cin"], c["cout"]
    x, W = c["x"], c["W"][0]
    step = 64 if cin % 64 == 0 else 32
    buf = np.full((n_out, cout + GUARD), SENT)
    for row0 in range(0, n_out, TM):
        rows = min(TM, n_out - row0)
        if fault == "tail_tile" and rows < TM:
            continue
        acc = np.zeros((rows, cout), DT[0])
        for ch in range(cin // step):
            wk = W[step * ch:step * ch + step] if not (fault == "chunk_weights" and ch == 1) else W[0:step]
            acc += _mul(x[row0:row0 + rows, step * ch:step * ch + step], wk, bf3, fault == "middle_piece")
        _finish(c, acc, buf, row0, rows, fault)
    return buf


def restate_wgrad(c, fault=None):
    """k_wgrad_bf3 + k_wgrad_reduce_work (k_wgrad_partial + k_wgrad_reduce: S = the chunk count): split s of offset k sums
    the 512-row blocks s, s + S, ...; the reduce adds the offset's S partials"""
    kid, _ci, _co, s_all, s_c, k_c = c["plan"]
    n_out, K_ = c["n_out"], c["K"]
    nbr = O._table(c["nbr"], n_out)
    nrb = -(-n_out // 512)
    dw = np.zeros((K_, c["cin"], c["cout"]))
    for k in range(K_):
        S = s_c if k == k_c else s_all
        parts = []
        for s in range(S):
            part = np.zeros((c["cin"], c["cout"]))
            last = nrb - 1 if fault == "last_block" and nrb > 1 else nrb
            for rb in range(s, last, S):
                j = np.arange(512 * rb, min(512 * rb + 512, n_out))
                j = j[nbr[j, k] >= 0]
                part += c["x"][nbr[j, k]].astype(np.float64).T @ c["dy"][j].astype(np.float64)
            parts.append(part)
        n = s_all if (fault == "centre_s_all" or k != k_c) else s_c
        dw[k] = sum(parts[:n])
    return dw


def _tile_shape(c):
    v = c["variant"]
    return (v >> 14) & 255, v & 127


FAMILIES = {
    # restatement family: (case names, runner(case, fault))
    "tiles": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] == "pairs"],
              lambda c, f: restate_tiles(c, *_tile_shape(c), fault=f)),
    "bigk": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] == "bigk"], lambda c, f: restate_tiles(c, 64, 32, fault=f)),
    "os": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] == "os"], lambda c, f: restate_tiles(c, c["os_R"], 64, fault=f, bf3=True)),
    "lists": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] in ("ws", "ws_bf3")],
              lambda c, f: restate_lists(c, fault=f, bf3=c["kernel"] == "ws_bf3")),
    "triples": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] == "ws3"], lambda c, f: restate_triples(c, fault=f)),
    "dense": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] in ("dense", "dense_bf3")],
              lambda c, f: restate_dense(c, (c["variant"] >> 14) & 255, fault=f, bf3=c["kernel"] == "dense_bf3")),
    "rows": ([n for n in EXACT if K.REGISTRY[n].meta["kernel"] == "dense_rows"], lambda c, f: restate_dense(c, 256, fault=f, bf3=True)),
}
MUTANTS = [("tiles", "last_group"), ("tiles", "tail_tile"), ("tiles", "chunk_weights"), ("tiles", "padded_writeback"),
           ("tiles", "guard_epilogue"), ("bigk", "last_group"), ("bigk", "chunk_weights"),
           ("os", "last_group"), ("os", "tail_tile"), ("os", "padded_writeback"), ("os", "middle_piece"),
           ("lists", "last_group"), ("lists", "chunk_weights"), ("lists", "reduce_k_minus_1"), ("lists", "middle_piece"),
           ("triples", "absent_row0"), ("triples", "reduce_k_minus_1"), ("triples", "middle_piece"),
           ("dense", "tail_tile"), ("dense", "chunk_weights"), ("dense", "middle_piece"),
           ("rows", "tail_tile"), ("rows", "chunk_weights"), ("rows", "middle_piece"), ("rows", "guard_epilogue")]
SMALL = 2100        # the mutants run on the cases up to this many rows; the unmutated restatements on every case


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = K.get(name)
    return O.conv_forward(c["x"], c["nbr"], c["W"], c["scale"], c["shift"], c["res"], c["relu"], n_out=c["n_out"])


def _fails(c, buf):
    ref = _ref(c["name"])
    return not (np.array_equal(buf[:, :c["cout"]], ref) and (buf[:, c["cout"]:] == SENT).all())


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_restatement_reproduces_the_oracle_on_every_exact_case(family):
    names, run = FAMILIES[family]
    assert len(names) >= 4
    for n in names:
        c = K.get(n)
        assert not _fails(c, run(c, None)), n


@pytest.mark.parametrize("family, fault", MUTANTS)
def test_each_planted_fault_fails_a_named_case(family, fault):
    names, run = FAMILIES[family]
    killers = [n for n in names if K.REGISTRY[n].meta["n_out"] <= SMALL and _fails(K.get(n), run(K.get(n), fault))]
    print(f"{family:8s} {fault:18s} killed by {len(killers)} cases, e.g. {killers[:3]}")
    assert killers, f"no case rejects the {family} restatement with the fault '{fault}'"
    if fault == "middle_piece":
        assert all(n.endswith("/cross") for n in killers)      # integers of 8 bits have no middle piece


HOST_WORST = {}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_float32_restatement_stays_inside_the_bounds(family, monkeypatch):
    """the same restatements in float32 arithmetic on the bound cases: the derived bounds hold for a float32 evaluation in
    the kernels' structure (the worst ratios are DESIGN 33's host column)"""
    kernels = {K.REGISTRY[n].meta["kernel"] for n in FAMILIES[family][0]}
    names = [n for n, b in K.REGISTRY.items() if b.meta["kernel"] in kernels and b.meta["kind"] == "bound" and not b.meta["l2norm"]]
    assert names
    monkeypatch.setitem(DT, 0, np.float32)
    for n in names:
        c = K.get(n)
        got = FAMILIES[family][1](c, None)[:, :c["cout"]]
        args = (c["x"], c["nbr"], c["W"], c["scale"], c["shift"], c["res"], c["relu"], False, c["n_out"])
        r = O.worst_ratio(got, O.conv_forward(*args), O.forward_bound(c["kernel"], *args))
        HOST_WORST[c["kernel"]] = max(HOST_WORST.get(c["kernel"], 0.0), r)
        assert r <= 1.0, n
        bare = dict(c, scale=None, shift=None, res=None, relu=False)      # the sums alone, without the epilogue's own roundings
        r0 = O.worst_ratio(FAMILIES[family][1](bare, None)[:, :c["cout"]], O.contract(c["x"], c["nbr"], c["W"], c["n_out"]),
                           O.forward_bound(c["kernel"], c["x"], c["nbr"], c["W"], n_out=c["n_out"]))
        HOST_WORST[c["kernel"] + " bare"] = max(HOST_WORST.get(c["kernel"] + " bare", 0.0), r0)
        assert r0 <= 1.0, n
    print({k: round(v, 3) for k, v in HOST_WORST.items()})


def test_wgrad_restatement_and_its_mutants():
    exact = [n for n in K.WGRAD if n.endswith("/exact")]
    killed = {"centre_s_all": [], "last_block": []}
    for n in exact:
        c = K.WGRAD[n]()
        ref = O.conv_wgrad(c["x"], c["nbr"], c["dy"])
        assert np.array_equal(restate_wgrad(c), ref), n
        for fault in killed:
            if not np.array_equal(restate_wgrad(c, fault), ref):
                killed[fault].append(n)
    print(killed)
    assert "wgrad_same_n2049_s1/exact" in killed["centre_s_all"] and "wgrad_same_n6657/exact" in killed["centre_s_all"]
    assert "wgrad_n513/exact" in killed["last_block"] and "wgrad_partial_misaligned_n513/exact" in killed["last_block"]

"""Every conv route and every inner kernel variant on the GPU, element by element against the float64 oracle
(tests/spconv_oracle.py) on the named cases of tests/spconv_cases.py: k_spconv_pairs, k_spconv_mfma, k_spconv_smallcin,
k_spconv_generic, k_spconv_bigk, k_dense_gemm, k_dense_gemm_bf3, k_dense_rows_bf3, the weight-stationary pair and triple
lists, the output-stationary conv, both weight-gradient kernels and the input gradient through ops.SparseConvFunction.

Before a case launches, the route (apr_spconv_route) and the inner variant (apr_spconv_tile_variant,
apr_dense_gemm_bf3_variant, apr_spconv_wgrad_plan) that the library reports for the very descriptor are compared with the
literals the case was written for; the rule itself is not restated here.  Then: exact and piece-crossing cases must equal
the oracle rounded to float32 bit for bit; bound cases stay inside the derived per-element bound (ratio <= 1, no element
excluded, no whole-tensor norm); poison cases have the oracle's NaN pattern -- exactly the rows that reference the poisoned
input row -- with every finite element inside the bound; x / out / residual are column slices of wider and taller buffers
and every float outside out's slice keeps its sentinel; a second run gives the same bytes.

Worst |kernel - oracle| / bound per kernel is printed by test_zz_print_worst_ratios (records, not thresholds; DESIGN 33 has
the table).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import spconv_cases as K
import spconv_oracle as O
from apr_amd import _lib, ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = -777.25
ROWS_ABOVE, ROWS_BELOW = 2, 3      # guard rows of every buffer
WORST = {}


class Buf:
    """[n, c] values as a column slice (extra columns, `off` floats in) and row slice of a filled buffer"""

    def __init__(self, dev, n, c, layout, values=None, fill=NAN):
        extra, off = layout
        self.ld = c + extra
        rows = ROWS_ABOVE + n + ROWS_BELOW
        self.flat = torch.full((rows * self.ld,), fill, dtype=torch.float32, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.flat, (n, c), (self.ld, 1), ROWS_ABOVE * self.ld + off)
        inside = torch.zeros_like(self.flat, dtype=torch.bool)
        torch.as_strided(inside, (n, c), (self.ld, 1), ROWS_ABOVE * self.ld + off).fill_(True)
        self.outside = ~inside
        if values is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)).to(dev))
        self.before = self.flat.clone()

    def get(self):
        """the slice as numpy, after checking that no float outside it changed"""
        same = self.flat.view(torch.int32)[self.outside] == self.before.view(torch.int32)[self.outside]
        assert bool(same.all()), "a float outside the slice was written"
        return self.view.cpu().numpy()


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _record(kernel, what, ratio):
    WORST[(kernel, what)] = max(WORST.get((kernel, what), 0.0), ratio)


def _equal_bits(got, ref64):
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64, equal_nan=True), "the oracle's value is not a float32: not an exact case"
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    assert not len(bad[0]), f"{len(bad[0])} elements differ from the oracle, first at {tuple(int(b[0]) for b in bad)}: " \
                            f"{got[tuple(b[0] for b in bad)]} vs {ref[tuple(b[0] for b in bad)]}"


# ------------------------------------------------------------------------------------------------------------ forward
def _launch_forward(dev, c, lib):
    n_out, K_, cin, cout = c["n_out"], c["K"], c["cin"], c["cout"]
    x = Buf(dev, c["n_in"], cin, c["lay"]["x"], c["x"])
    out = Buf(dev, n_out, cout, c["lay"]["out"], fill=SENTINEL)
    res = None if c["res"] is None else Buf(dev, n_out, cout, c["lay"]["res"], c["res"])
    W = _t(c["W"], dev)
    nbr = _t(c["nbr"], dev)
    scale, shift = _t(c["scale"], dev), _t(c["shift"], dev)
    w3 = ops.pack_weights_bf3(W) if c["bf3"] else None
    assert (w3 is not None) == c["bf3"]
    if c["aux"] == "rows":      # apr_dense_rows_bf3 by name: below the router's row threshold
        assert lib.apr_dense_rows_bf3_ok(cin, cout) == 1
        ops.dense_rows_bf3(x.view, w3, cin, cout, scale=scale, shift=shift, residual=None if res is None else res.view,
                           relu=c["relu"], l2norm=c["l2norm"], out=out.view)
        torch.cuda.synchronize()
        return out.get()
    plist = os_pairs = None
    if c["aux"] == "pairs":
        plist = ops.build_pairlist(nbr)
    elif c["aux"] == "triples":
        plist = ops.build_pairlist3(nbr)
    elif c["aux"] == "os":
        os_pairs = ops.build_os_pairs(nbr, c["n_in"], c["os_R"])
    batch = ops.SpconvBatch()
    batch.add(x.view, nbr, K_, cin, cout, lambda: ops.pack_weights(W), scale=scale, shift=shift,
              residual=None if res is None else res.view, relu=c["relu"], out=out.view, n_out=n_out, plist=plist, w_bf3=w3,
              os_pairs=os_pairs, l2norm=c["l2norm"])
    d = batch.descs[-1]
    # the kernel this case was written for, asked of the library for this very descriptor
    assert lib.apr_spconv_route(C.byref(d)) == c["route"], "the case does not take the route it was written for"
    if c["route"] == K.TILE:
        assert lib.apr_spconv_tile_variant(C.byref(d)) == c["variant"], \
            f"tile variant {lib.apr_spconv_tile_variant(C.byref(d)):#x}, the case was written for {c['variant']:#x}"
    elif c["route"] == K.DENSE_GEMM:
        assert lib.apr_dense_gemm_bf3_variant(n_out, cin, cout) == c["variant"]
    else:
        assert c["variant"] is None
    batch.launch()
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize("name", sorted(K.REGISTRY))
def test_forward_case(dev, lib, name):
    c = K.get(name)
    got = _launch_forward(dev, c, lib)
    args = (c["x"], c["nbr"], c["W"], c["scale"], c["shift"], c["res"], c["relu"], c["l2norm"], c["n_out"])
    ref = O.conv_forward(*args)
    if c["kind"] in ("exact", "cross"):
        assert not c["l2norm"]
        _equal_bits(got, ref)
    else:
        bound = O.forward_bound(c["kernel"], *args)
        ratio = O.worst_ratio(got, ref, bound)      # asserts the NaN pattern too
        print(f"{name}: worst |kernel - oracle| / bound = {ratio:.3f}")
        _record(c["kernel"], c["kind"] + (" l2" if c["l2norm"] else ""), ratio)
        assert ratio <= 1.0
        if c["kind"] == "bound" and c["scale"] is not None:
            # the bare contraction: no epilogue whose own roundings (u |out| each, reached by construction) hide the sums'
            # (a zero residual keeps the descriptor's alignment facts and with them the kernel; adding 0 is exact)
            bare = dict(c, scale=None, shift=None, res=np.zeros_like(c["res"]), relu=False)
            r0 = O.worst_ratio(_launch_forward(dev, bare, lib), O.contract(c["x"], c["nbr"], c["W"], c["n_out"]),
                               O.forward_bound(c["kernel"], c["x"], c["nbr"], c["W"], n_out=c["n_out"]))
            print(f"{name}: bare contraction, worst ratio = {r0:.3f}")
            _record(c["kernel"], "bare sums", r0)
            assert r0 <= 1.0
    if c["kind"] == "poison":
        tbl = O._table(c["nbr"], c["n_out"])
        want = (tbl == c["poison"]).any(axis=1)
        assert want.any() and not want.all()
        assert np.array_equal(np.isnan(got).any(axis=1), want) and np.array_equal(np.isnan(got).all(axis=1), want), \
            "NaN rows are not exactly the rows that reference the poisoned input row"
    if c["l2norm"]:
        assert np.isnan(got[5]).all(), "the all-zero row must come out as 0 / 0"
    again = _launch_forward(dev, c, lib)
    assert got.tobytes() == again.tobytes(), "a second run gives other bits"


def test_misaligned_input_rows_of_an_mfma_shaped_layer_are_refused(dev, lib):
    c = K.get("mfma_c64_64_n1/exact")
    x = Buf(dev, c["n_in"], 64, (7, 1), c["x"])
    out = Buf(dev, 1, 64, (12, 8), fill=SENTINEL)
    with pytest.raises(_lib.AprHipError, match="16-B aligned input rows"):
        ops.spconv(x.view, _t(c["nbr"], dev), 27, 64, 64, ops.pack_weights(_t(c["W"], dev)), out=out.view)
    torch.cuda.synchronize()
    assert bool((out.flat == SENTINEL).all()), "a refused launch wrote something"


def test_os_pairs_refuse_2_pow_23_input_rows(dev):
    nbr = torch.full((64, 27), -1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AprHipError, match="n_in < 2\\^23"):
        ops.build_os_pairs(nbr, 1 << 23, 64)
    ops.build_os_pairs(nbr, (1 << 23) - 1, 64)


# ---------------------------------------------------------------------------------------------------- kernel gradient
def _launch_wgrad(dev, c, lib, monkeypatch):
    n, K_, cin, cout = c["n_out"], c["K"], c["cin"], c["cout"]
    x = Buf(dev, n, cin, (4 + (-c["x_off"]) % 4, c["x_off"]), c["x"])
    dy = Buf(dev, n, cout, (4, 4), c["dy"])
    nbr = _t(c["nbr"], dev)
    plan = (C.c_int32 * 6)()
    ld = lambda b: b.view.stride(0) if n > 1 else max(b.view.stride(0), b.view.shape[1])
    _lib.check(lib.apr_spconv_wgrad_plan(_lib.ptr(x.view), ld(x), _lib.ptr(dy.view), ld(dy), n, K_, cin, cout, int(c["same_level"]), plan))
    assert tuple(plan) == tuple(c["plan"]), f"wgrad plan {tuple(plan)}, the case was written for {c['plan']}"
    if not c["pad"]:
        monkeypatch.setattr(ops, "WGRAD_PAD", False)
    dw = ops.spconv_wgrad(x.view, dy.view, nbr, K_, cin, cout, same_level=c["same_level"])
    torch.cuda.synchronize()
    x.get(), dy.get()
    return dw.cpu().numpy()


@pytest.mark.parametrize("name", sorted(K.WGRAD))
def test_wgrad_case(dev, lib, name, monkeypatch):
    c = K.WGRAD[name]()
    got = _launch_wgrad(dev, c, lib, monkeypatch)
    ref = O.conv_wgrad(c["x"], c["nbr"], c["dy"])
    kid, _ci, _co, s_all, s_c, k_c = c["plan"]
    if c["kind"] == "exact":
        _equal_bits(got, ref)
    else:
        splits = [s_c if k == k_c else s_all for k in range(c["K"])]
        ratio = O.worst_ratio(got, ref, O.wgrad_bound(c["kernel"], c["x"], c["nbr"], c["dy"], splits))
        print(f"{name}: worst |kernel - oracle| / bound = {ratio:.3f}")
        _record(c["kernel"], "dW", ratio)
        assert ratio <= 1.0
    if c["nbr"] is not None:
        for k in np.nonzero((c["nbr"] >= 0).sum(axis=0) == 0)[0]:
            assert not got[k].any(), f"dW[{k}] of an empty offset is not exactly zero"
    assert got.tobytes() == _launch_wgrad(dev, c, lib, monkeypatch).tobytes(), "a second run gives other bits"


# ----------------------------------------------------------------------------------------------------- input gradient
@pytest.fixture(scope="module")
def real_maps(dev):
    """forward table, reverse table and flip of a same-level, a stride-2 and a transposed 3^3 conv over two small clouds,
    as the conv modules hand them to ops.SparseConvFunction"""
    from apr_amd import MinkowskiEngine as ME
    from oracle import me_oracle as OME
    rng = np.random.default_rng(33)
    clouds = [OME.sparse_quantize(rng.uniform(-2, 2, (400, 3)).astype(np.float32) / np.float32(0.45), return_index=True)[0]
              for _ in range(2)]
    Cc = OME.batched_coordinates(clouds)
    hx = ME.SparseTensor(torch.ones(len(Cc), 1, device=dev), coordinates=torch.from_numpy(Cc).to(dev))
    same = ME.MinkowskiConvolution(1, 1, kernel_size=3, stride=1, dimension=3).to(dev)
    down = ME.MinkowskiConvolution(1, 1, kernel_size=3, stride=2, dimension=3).to(dev)
    up = ME.MinkowskiConvolutionTranspose(1, 1, kernel_size=3, stride=2, dimension=3).to(dev)
    maps = {}
    with torch.no_grad():
        hx2 = down(hx)
    for kind, mod, t in (("same", same, hx), ("strided", down, hx), ("transposed", up, hx2)):
        nbr, ts_out = mod._maps(t)
        nbr_bwd, flip = mod._reverse_map(t, nbr, ts_out)
        maps[kind] = (nbr, nbr_bwd, flip, int(t.F.shape[0]))
    assert 200 < len(Cc) < 800
    return maps


@pytest.mark.parametrize("cin, cout", [(32, 64), (64, 128)])
@pytest.mark.parametrize("data", ["exact", "bound"])
@pytest.mark.parametrize("kind", ["same", "strided", "transposed"])
def test_input_and_kernel_gradient_on_real_maps(dev, lib, real_maps, kind, data, cin, cout):
    """ops.SparseConvFunction's dx against the oracle stated over the FORWARD table (no reverse map, flip or transpose on
    the oracle's side), and its dW, per element"""
    nbr, nbr_bwd, flip, n_in = real_maps[kind]
    tbl = nbr.cpu().numpy()
    n_out = tbl.shape[0]
    assert tbl.max() < n_in
    rng = np.random.default_rng(K._seed(f"{kind}{data}{cin}"))
    if data == "exact":
        x = rng.integers(-7, 8, size=(n_in, cin)).astype(np.float32)
        dy = rng.integers(-7, 8, size=(n_out, cout)).astype(np.float32)
        W = rng.integers(-3, 4, size=(27, cin, cout)).astype(np.float32)
    else:
        x = (rng.standard_normal((n_in, cin)) * np.exp(rng.uniform(-9.2, 9.2, (n_in, 1)))).astype(np.float32)
        dy = (rng.standard_normal((n_out, cout)) * np.exp(rng.uniform(-4.6, 4.6, (n_out, 1)))).astype(np.float32)
        W = (rng.standard_normal((27, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32)
    xd, Wd = _t(x, dev).requires_grad_(True), _t(W, dev).requires_grad_(True)
    # the tile variants of the function's two launches, asked through descriptors that are never launched: 32-row tiles
    # at a few hundred rows, CN / CK by the channel counts
    ask = ops.SpconvBatch()
    ask.add(xd.detach(), nbr, 27, cin, cout, lambda: ops.pack_weights(Wd.detach()))
    ask.add(_t(dy, dev), nbr_bwd, 27, cout, cin, lambda: ops.pack_weights(Wd.detach().transpose(1, 2).contiguous()))
    want = [_lib.tile_id(_lib.TILE_PAIRS, 32, 64, 32 if cin == 32 else 64), _lib.tile_id(_lib.TILE_PAIRS, 32, 32 if cin == 32 else 64, 64)]
    assert [lib.apr_spconv_tile_variant(C.byref(d)) for d in ask.descs] == want
    out = ops.SparseConvFunction.apply(xd, Wd, nbr, nbr_bwd, flip)
    out.backward(_t(dy, dev))
    torch.cuda.synchronize()
    dx, dw = xd.grad.cpu().numpy(), Wd.grad.cpu().numpy()
    ref_dx, ref_dw = O.conv_dx(dy, tbl, W, n_in), O.conv_wgrad(x, tbl, dy)
    plan = (C.c_int32 * 6)()
    _lib.check(lib.apr_spconv_wgrad_plan(_lib.ptr(xd), cin, _lib.ptr(out), cout, n_out, 27, cin, cout, 0, plan))
    assert plan[0] == _lib.WGRAD_BF3
    if data == "exact":
        _equal_bits(out.detach().cpu().numpy(), O.conv_forward(x, tbl, W))
        _equal_bits(dx, ref_dx)
        _equal_bits(dw, ref_dw)
    else:
        r_dx = O.worst_ratio(dx, ref_dx, O.dx_bound("pairs", dy, tbl, W, n_in))
        r_dw = O.worst_ratio(dw, ref_dw, O.wgrad_bound("wgrad_bf3", x, tbl, dy, [plan[3]] * 27))
        print(f"{kind} {cin}->{cout}: worst ratio dx {r_dx:.3f}, dW {r_dw:.3f}")
        _record("pairs", "dx", r_dx)
        _record("wgrad_bf3", "dW (module)", r_dw)
        assert r_dx <= 1.0 and r_dw <= 1.0


def test_zz_print_worst_ratios():
    for (kernel, what), r in sorted(WORST.items()):
        print(f"worst ratio  {kernel:14s} {what:12s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())

"""One smallest layer per conv route (apr_spconv_route): the route id that the shared descriptor filler gets, the eager launch
(ops.spconv) against a SpconvBatch of one and against the family's direct wrapper where there is one -- all bitwise, the same
kernel runs in each -- and the lazy tile pack: a callable `wp` is called once on the routes whose kernels read the pack and
not at all on the others."""
import numpy as np
import pytest
import torch

from apr_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROWS = 70      # crosses the 16 / 32 / 64-row tiles and a 64-pair unit, a multiple of none


class LazyPack:
    """A callable tile pack that counts its calls; `allowed` False: the routed kernel does not read the pack."""

    def __init__(self, W, allowed):
        self.W, self.allowed, self.calls = W, allowed, 0

    def __call__(self):
        self.calls += 1
        assert self.allowed, "the tile pack was asked for on a route that does not read it"
        return ops.pack_weights(self.W)


def _layer(dev, K, cin, cout, n_out, seed, wide=False):
    """Operands of one layer with a full epilogue; K = 27: a random map with about 40 % of its entries -1."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    n_in = n_out if K == 1 else 53
    xw = f32(rng.standard_normal((n_in, cin + 4)))
    x = xw[:, 1:1 + cin] if wide else xw[:, 4:]      # `wide`: rows that are not 16-byte aligned
    W = f32(rng.standard_normal((K, cin, cout)) / np.sqrt(cin * 8))
    nbr = None
    if K > 1:
        m = rng.integers(0, n_in, size=(n_out, K)).astype(np.int32)
        m[rng.random((n_out, K)) < 0.4] = -1
        nbr = torch.from_numpy(m).to(dev)
    epi = dict(scale=f32(rng.uniform(0.5, 1.5, cout)), shift=f32(rng.standard_normal(cout)),
               residual=f32(rng.standard_normal((n_out, cout + 4)))[:, 4:], relu=True)
    return x, nbr, W, epi


def _pack_bf3(W):
    """The split image of W; for a width ops.pack_weights_bf3 leaves out (no kernel reads it there) straight from the library,
    so that a route can be asked with the image PRESENT."""
    w3 = ops.pack_weights_bf3(W)
    if w3 is None:
        lib, (K, cin, cout) = ops._lib_(), W.shape
        w3 = torch.empty(int(lib.apr_spconv_packed_bf3_bytes(K, cin, cout)), dtype=torch.uint8, device=W.device)
        ops.check(lib.apr_spconv_pack_weights_bf3(ops.ptr(W.contiguous()), K, cin, cout, ops.ptr(w3), ops.stream()))
    return w3


def _check(dev, want, K, cin, cout, n_out, lists=None, bf3=True, direct=None):
    """`lists`: nbr -> the keyword (plist / os_pairs) of a fresh, unbuilt list of the map, one per launch."""
    x, nbr, W, epi = _layer(dev, K, cin, cout, n_out, seed=K * 1000 + cin + cout + n_out)
    w3 = _pack_bf3(W) if bf3 else None
    reads_pack = want in (_lib.ROUTE_TILE, _lib.ROUTE_WS)
    mk = (lambda: lists(nbr)) if lists else dict
    lazy = LazyPack(W, reads_pack)
    route = ops._spconv_desc(x, nbr, K, cin, cout, lazy, None, None, None, False, None, n_out, mk().get("plist"), w3,
                             mk().get("os_pairs"), {})[1]
    assert route == want
    assert lazy.calls == int(reads_pack)
    lazy = LazyPack(W, reads_pack)
    eager = ops.spconv(x, nbr, K, cin, cout, lazy, n_out=n_out, w_bf3=w3, **epi, **mk())
    assert lazy.calls == int(reads_pack)
    batch = ops.SpconvBatch()
    batched = batch.add(x, nbr, K, cin, cout, ops.pack_weights(W), n_out=n_out, w_bf3=w3, **epi, **mk())
    batch.launch()
    assert torch.equal(eager, batched)
    assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 0
    if direct is not None:
        assert torch.equal(eager, direct(x, nbr, w3, epi))
    return x, nbr, W, epi, eager


def _plist(nbr):
    return {"plist": ops.build_pairlist(nbr, lazy=True)}


def _plist3(nbr):
    return {"plist": ops.build_pairlist3(nbr, lazy=True)}


def test_tile(dev):
    _check(dev, _lib.ROUTE_TILE, 27, 64, 64, ROWS, bf3=False)
    _check(dev, _lib.ROUTE_TILE, 27, 96, 64, ROWS, lists=_plist, bf3=False)      # a list on a shape the lists do not cover


@pytest.mark.parametrize("cin, bf3", [(64, False), (320, True)])
def test_ws_fp32(dev, cin, bf3):
    """No split weights, or a width that k_ws_gemm_bf3 is not instantiated for: the fp32 kernel, which reads the tile pack."""
    _check(dev, _lib.ROUTE_WS, 27, cin, 64, ROWS, lists=_plist, bf3=bf3)


def test_ws_bf3(dev):
    _check(dev, _lib.ROUTE_WS_BF3, 27, 64, 64, ROWS, lists=_plist)


def test_ws3(dev):
    _check(dev, _lib.ROUTE_WS3, 27, 64, 64, ROWS, lists=_plist3)


def test_os(dev):
    first = next(n for n in range(1, 4096) if ops.os_tile_rows(n, 64, 64) > 0)
    for n_out in (first + 1, ROWS):
        R = ops.os_tile_rows(n_out, 64, 64)
        n_in = 53
        _check(dev, _lib.ROUTE_OS, 27, 64, 64, n_out, lists=lambda nbr: {"os_pairs": ops.build_os_pairs(nbr, n_in, R, lazy=True)},
               direct=lambda x, nbr, w3, epi: ops.spconv_os(x, ops.build_os_pairs(nbr, n_in, R), 64, 64, w3, **epi))


def test_dense_rows(dev):
    route = lambda n: bool(ops._lib_().apr_dense_rows_bf3_route(n, 96, 32))
    n = ROWS
    if not route(n):      # the smallest row count the row stream takes (the rule is a threshold on the rows)
        lo, n = ROWS, next(1 << s for s in range(7, 24) if route(1 << s))
        while n - lo > 1:
            mid = (lo + n) // 2
            lo, n = (lo, mid) if route(mid) else (mid, n)
    assert route(n) and (n == ROWS or not route(n - 1))
    _check(dev, _lib.ROUTE_DENSE_ROWS, 1, 96, 32, n,
           direct=lambda x, nbr, w3, epi: ops.dense_rows_bf3(x, w3, 96, 32, **epi))


def test_dense_gemm(dev):
    assert not ops._lib_().apr_dense_rows_bf3_route(ROWS, 64, 64)
    _check(dev, _lib.ROUTE_DENSE_GEMM, 1, 64, 64, ROWS,
           direct=lambda x, nbr, w3, epi: ops.dense_gemm_bf3(x, w3, 64, 64, **epi))


def test_tile_by_misalignment(dev):
    """A K = 1, 64 -> 64 layer with the split weights given and rows that start 4 bytes off a 16-byte boundary: the route is
    the tile family's, and the launch does exactly what it does without the split weights.  For misaligned OUTPUT rows that
    is k_spconv_mfma's result; misaligned INPUT rows of an MFMA-shaped layer the tile family refuses, with or without them."""
    x, nbr, W, epi = _layer(dev, 1, 64, 64, ROWS, seed=5)
    w3, wp = ops.pack_weights_bf3(W), ops.pack_weights(W)
    route = lambda x, out: ops._spconv_desc(x, None, 1, 64, 64, wp, None, None, None, False, out, ROWS, None, w3, None, {})[1]
    assert route(x, None) == _lib.ROUTE_DENSE_GEMM
    outs = []
    for bf3 in (w3, None):
        wide = torch.zeros(ROWS, 68, device=dev)
        assert wide[:, 1:65].data_ptr() % 16 == 4 and route(x, wide[:, 1:65]) == _lib.ROUTE_TILE
        lazy = LazyPack(W, True)
        batch = ops.SpconvBatch()
        batch.add(x, None, 1, 64, 64, wp, out=wide[:, 1:65], n_out=ROWS, w_bf3=bf3, **epi)
        batch.launch()
        outs += [ops.spconv(x, None, 1, 64, 64, lazy, out=torch.zeros_like(wide)[:, 1:65], n_out=ROWS, w_bf3=bf3, **epi),
                 wide[:, 1:65]]
        assert lazy.calls == 1 and float(wide[:, 0].abs().max()) == 0 and float(wide[:, 65:].abs().max()) == 0
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and float(outs[0].abs().max()) > 0
    xs = _layer(dev, 1, 64, 64, ROWS, seed=5, wide=True)[0]
    assert xs.data_ptr() % 16 == 4 and route(xs, None) == _lib.ROUTE_TILE
    for bf3 in (w3, None):
        with pytest.raises(_lib.AprHipError, match="16-B aligned input rows"):
            ops.spconv(xs, None, 1, 64, 64, wp, n_out=ROWS, w_bf3=bf3, **epi)

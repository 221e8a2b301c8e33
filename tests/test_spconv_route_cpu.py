"""apr_spconv_route on the host: the kernel family of a conv descriptor, row by row of the rule table ("How a conv
layer is routed").  No GPU and no launch: the pointers are small non-NULL stand-ins that nothing dereferences.  The expected
routes are literals read off the rule, not computed from the code under test; every row is asked twice, with w_packed NULL
and non-NULL, since the route must not depend on the tile pack."""
import ctypes as C
import os
import re

import pytest

from apr_amd import _lib

TILE, WS, WS_BF3, WS3, OS, DENSE_ROWS, DENSE_GEMM = range(7)
A = 0x1000          # stand-in pointers, 16-byte aligned and 256 bytes apart
NBR, IN, OUT, RES, SCALE, SHIFT, W3, PLIST, CNT, OSP, WP = (A + 256 * i for i in range(11))


def desc(K, cin, cout, n_out=1000, nbr=True, **kw):
    d = _lib.SpconvDesc()
    d.inp, d.ldi, d.nbr, d.n_out = IN, cin, (NBR if nbr else None), n_out
    d.K, d.cin, d.cout, d.out, d.ldo = K, cin, cout, OUT, cout
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def route(lib, d):
    got = []
    for wp in (None, WP):
        d.w_packed = wp
        got.append(lib.apr_spconv_route(C.byref(d)))
    assert got[0] == got[1], "the route depends on w_packed"
    return got[0]


def test_ids_of_the_binding_are_the_headers():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "apr_hip.h")).read()
    names = ["TILE", "WS", "WS_BF3", "WS3", "OS", "DENSE_ROWS", "DENSE_GEMM"]
    assert re.findall(r"^  APR_ROUTE_([A-Z0-9_]+)( = 0)?,? +/\*", header, flags=re.M) == [(n, " = 0" if n == "TILE" else "")
                                                                                          for n in names]
    assert [getattr(_lib, "ROUTE_" + n) for n in names] == [TILE, WS, WS_BF3, WS3, OS, DENSE_ROWS, DENSE_GEMM]


def test_ws_supported(lib):
    yes = [(27, 64, 64), (27, 128, 64), (8, 512, 128), (27, 320, 64), (1, 64, 64)]
    no = [(27, 96, 64), (27, 576, 64), (27, 64, 96), (28, 64, 64), (125, 64, 64), (27, 32, 64)]
    assert [lib.apr_spconv_ws_supported(*s) for s in yes] == [1] * len(yes)
    assert [lib.apr_spconv_ws_supported(*s) for s in no] == [0] * len(no)


@pytest.mark.parametrize("cin, w_bf3, want", [
    (64, W3, WS_BF3), (64, None, WS), (128, W3, WS_BF3), (192, W3, WS_BF3), (256, W3, WS_BF3), (384, W3, WS_BF3),
    (320, W3, WS),          # a weight-stationary width without a bf16 instantiation: the fp32 kernel, which reads w_packed
    (512, W3, WS), (96, W3, TILE), (96, None, TILE), (576, W3, TILE)])
def test_weight_stationary_shapes(lib, cin, w_bf3, want):
    assert route(lib, desc(27, cin, 64, plist=PLIST, counters=CNT, w_bf3=w_bf3)) == want


def test_weight_stationary_needs_the_map_and_a_covered_cout(lib):
    assert route(lib, desc(27, 64, 96, plist=PLIST, counters=CNT, w_bf3=W3)) == TILE
    assert route(lib, desc(27, 64, 64, w_bf3=W3)) == TILE                      # no list given
    assert route(lib, desc(1, 64, 48, nbr=False, plist=PLIST, counters=CNT)) == TILE


def test_triple_lists(lib):
    assert route(lib, desc(27, 64, 64, plist=PLIST, counters=CNT, w_bf3=W3, ws3=1)) == WS3
    assert route(lib, desc(27, 128, 64, plist=PLIST, counters=CNT, w_bf3=W3, ws3=1)) == WS3
    for bad in (desc(27, 192, 64, plist=PLIST, counters=CNT, w_bf3=W3, ws3=1),      # weight-stationary, not triple-list
                desc(27, 64, 64, plist=PLIST, counters=CNT, ws3=1),                 # no split weights
                desc(8, 64, 64, plist=PLIST, counters=CNT, w_bf3=W3, ws3=1)):       # not a 27-offset map
        assert route(lib, bad) < 0
        assert len(lib.apr_last_error()) > 0 and b"triple" in lib.apr_last_error()
    # a shape outside the weight-stationary families ignores the list altogether, triple or not
    assert route(lib, desc(27, 96, 64, plist=PLIST, counters=CNT, w_bf3=W3, ws3=1)) == TILE


def test_output_stationary(lib):
    assert route(lib, desc(27, 64, 64, os_pairs=OSP, os_rows=48, w_bf3=W3)) == OS
    assert route(lib, desc(27, 64, 64, os_pairs=OSP, os_rows=48, w_bf3=W3, plist=PLIST, counters=CNT)) == OS      # before the lists
    # without the split weights: whatever the pair list / the tile family gives
    assert route(lib, desc(27, 64, 64, os_pairs=OSP, os_rows=48)) == TILE
    assert route(lib, desc(27, 64, 64, os_pairs=OSP, os_rows=48, plist=PLIST, counters=CNT)) == WS
    assert route(lib, desc(27, 96, 64, os_pairs=OSP, os_rows=48, plist=PLIST, counters=CNT)) == TILE
    # without a kernel map there is nothing to tile
    assert route(lib, desc(1, 64, 64, nbr=False, os_pairs=OSP, os_rows=48, w_bf3=W3)) in (DENSE_GEMM, DENSE_ROWS)


def rows_or(lib, n, cin, cout, other):
    """DENSE_ROWS where the library's row threshold (apr_dense_rows_bf3_route; 32768 rows unless APR_DENSE_ROWS_MIN says
    otherwise) takes the layer, else `other`."""
    return DENSE_ROWS if lib.apr_dense_rows_bf3_route(n, cin, cout) else other


def test_k1_dense_aligned(lib):
    k1 = dict(nbr=False, w_bf3=W3)
    # 96 -> 32: the row stream above its row threshold, the tile family below (cin is no multiple of 64: no dense GEMM)
    assert route(lib, desc(1, 96, 32, n_out=1000, **k1)) == rows_or(lib, 1000, 96, 32, TILE)
    assert route(lib, desc(1, 96, 32, n_out=200000, **k1)) == rows_or(lib, 200000, 96, 32, TILE)
    if "APR_DENSE_ROWS_MIN" not in os.environ:
        assert route(lib, desc(1, 96, 32, n_out=1000, **k1)) == TILE
        assert route(lib, desc(1, 96, 32, n_out=32768, **k1)) == DENSE_ROWS
        assert route(lib, desc(1, 96, 32, n_out=32767, **k1)) == TILE
        assert route(lib, desc(1, 64, 64, n_out=1000, **k1)) == DENSE_GEMM
        assert route(lib, desc(1, 64, 64, n_out=200000, **k1)) == DENSE_ROWS
    assert route(lib, desc(1, 64, 64, n_out=1000, **k1)) == rows_or(lib, 1000, 64, 64, DENSE_GEMM)
    assert route(lib, desc(1, 64, 64, n_out=200000, **k1)) == rows_or(lib, 200000, 64, 64, DENSE_GEMM)
    assert route(lib, desc(1, 256, 128, n_out=200000, **k1)) == DENSE_GEMM      # wider than the row stream's images
    assert route(lib, desc(1, 64, 48, **k1)) == TILE
    assert route(lib, desc(1, 64, 64, nbr=False)) == TILE                        # no split weights
    assert route(lib, desc(1, 64, 64, w_bf3=W3)) == TILE                         # a K = 1 kernel MAP is not the identity
    full = desc(1, 64, 64, residual=RES, ldr=64, scale=SCALE, shift=SHIFT, **k1)
    assert route(lib, full) == rows_or(lib, 1000, 64, 64, DENSE_GEMM)


MISALIGN = {
    "in + 4 bytes": dict(inp=IN + 4), "out + 4 bytes": dict(out=OUT + 4), "ldi = cin + 1": dict(ldi=65), "ldo odd": dict(ldo=65),
    "residual + 4 bytes": dict(residual=RES + 4), "ldr odd": dict(ldr=65), "scale + 4 bytes": dict(scale=SCALE + 4),
    "shift + 4 bytes": dict(shift=SHIFT + 4), "ldi = cin + 2": dict(ldi=66), "in + 8 bytes": dict(inp=IN + 8)}


@pytest.mark.parametrize("what", sorted(MISALIGN))
@pytest.mark.parametrize("n_out", [1000, 200000])
def test_k1_dense_misaligned_takes_the_tile_family(lib, what, n_out):
    base = dict(n_out=n_out, nbr=False, w_bf3=W3, residual=RES, ldr=64, scale=SCALE, shift=SHIFT)
    assert route(lib, desc(1, 64, 64, **base)) in (DENSE_GEMM, DENSE_ROWS)
    base.update(MISALIGN[what])
    assert route(lib, desc(1, 64, 64, **base)) == TILE


def test_misaligned_residual_stride_counts_only_with_a_residual(lib):
    assert route(lib, desc(1, 64, 64, nbr=False, w_bf3=W3, ldr=65)) == DENSE_GEMM or "APR_DENSE_ROWS_MIN" in os.environ


def test_no_rows(lib):
    assert route(lib, desc(1, 64, 64, n_out=0, nbr=False, w_bf3=W3)) == TILE
    assert route(lib, desc(1, 96, 32, n_out=0, nbr=False, w_bf3=W3)) == TILE
    assert route(lib, desc(27, 64, 64, n_out=0)) == TILE
    assert lib.apr_spconv_route(None) < 0 and b"null descriptor" in lib.apr_last_error()

"""Named inputs for the sparse-convolution family (tests/spconv_oracle.py has the operations and the bounds).  numpy only
on top of the binding's id constants.  A case is a dict built on first use and cached (`get(name)`); tests treat it as
read-only.  Every case names the kernel it was written for: `route` (apr_spconv_route), `variant` (apr_spconv_tile_variant /
apr_dense_gemm_bf3_variant, None where the route has no inner choice) and `kernel` (the oracle's bound key).  The GPU test
asserts route and variant before it launches, the host test walks the same literals through the host functions.

Three kinds of data
  exact   x, dy integers in [-7, 7], W integers in [-3, 3], scale a power of two, shift and residual integers: every operand
          fits one bf16 piece, every partial sum is an integer below 2^24 in any order -- every kernel must return the
          oracle's bits.  `cross` (the split kernels): two x per input row have 16 significant bits, so the middle piece is non-zero,
          W in {-1, 0, 1}; still exact (prove_exact shows it from the actual pieces).
  bound   floats whose row magnitudes span 8 decades, plus (on random maps) rows that cancel to zero through two offsets with
          equal weights: compared per element against the derived bound.
  poison  every input row that the map does not reference is NaN, and so is ONE referenced row: pair 0 of an offset list whose
          length is no multiple of 16 -- the row that padded lanes gather again.  The output's NaN pattern is the oracle's.
          Poison cases run without the ReLU: the kernels' ReLU is fmaxf(v, 0), which turns a NaN into 0.
`lay` gives (extra columns, column offset) of x / out / res inside wider, taller, sentinel-filled buffers.
"""
import functools

import numpy as np

from apr_amd import _lib as L

TILE, WS, WS_BF3, WS3, OS, DENSE_ROWS, DENSE_GEMM = range(7)
PAIRS, MFMA, DENSE, BIGK, SMALLCIN, GENERIC, DENSE_BF3 = (L.TILE_PAIRS, L.TILE_MFMA, L.TILE_DENSE, L.TILE_BIGK, L.TILE_SMALLCIN,
                                                          L.TILE_GENERIC, L.TILE_DENSE_BF3)
tid = L.tile_id
ALIGNED = {"x": (8, 4), "out": (12, 8), "res": (4, 4)}          # column slices of wider buffers, rows 16-byte aligned
REGISTRY = {}


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


# ------------------------------------------------------------------------------------------------------------------ maps
def random_map(rng, n_out, K, n_in, density=0.3):
    nbr = rng.integers(0, n_in, size=(n_out, K)).astype(np.int32)
    nbr[rng.random((n_out, K)) > density] = -1
    return nbr


def planted_map(rng, n_out, K, n_in, plan, base=None):
    """plan: (first row, offset, count): `count` consecutive rows from `first row` get a neighbour under `offset`;
    everything else of `base` (default: nothing) is kept"""
    nbr = np.full((n_out, K), -1, np.int32) if base is None else base.copy()
    for row0, k, count in plan:
        nbr[row0:row0 + count, k] = rng.integers(0, n_in, size=count)
    return nbr


def same_level_map(rng, n, K, n_in=None):
    """a stride-1 map's shape: the centre column holds every row, mirrored offsets hold mirrored pairs"""
    nbr = np.full((n, K), -1, np.int32)
    nbr[:, K // 2] = np.arange(n)
    for k in range(K // 2):
        j = np.nonzero(rng.random(n) < 0.25)[0]
        i = rng.permutation(n)[:len(j)]
        nbr[j, k] = i
        nbr[i, K - 1 - k] = j
    return nbr


# ------------------------------------------------------------------------------------------------------------------ data
def _exact_data(rng, n_in, K, cin, cout, n_out, cross=False):
    x = rng.integers(-7, 8, size=(n_in, cin)).astype(np.float32)
    W = rng.integers(-3, 4, size=(K, cin, cout)).astype(np.float32)
    if cross:      # two values per input row with 16 significant bits (h = 128..255, m = 1..255), W in {-1, 0, 1}
        W = rng.integers(-1, 2, size=(K, cin, cout)).astype(np.float32)
        cols = rng.integers(0, cin, size=(n_in, 2))
        val = (rng.integers(128, 256, size=(n_in, 2)) * 256 + rng.integers(1, 256, size=(n_in, 2))) * rng.choice([-1, 1], size=(n_in, 2))
        x[np.arange(n_in)[:, None], cols] = val
    scale = rng.choice([0.5, 1.0, 2.0] if cross else [0.5, 1.0, 2.0, 4.0], size=cout).astype(np.float32)
    shift = rng.integers(-5, 6, size=cout).astype(np.float32)
    res = rng.integers(-9, 10, size=(n_out, cout)).astype(np.float32)
    return x, W, scale, shift, res


def _bound_data(rng, n_in, K, cin, cout, n_out):
    x = (rng.standard_normal((n_in, cin)) * np.exp(rng.uniform(-9.2, 9.2, (n_in, 1)))).astype(np.float32)
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(cin * 8)).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1, 1], size=cout)).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n_out, cout)).astype(np.float32)
    return x, W, scale, shift, res


def _plant_cancelling_rows(rng, x, W, nbr):
    """every 7th output row reads x[a] under offset 0 and x[b] = -x[a] under offset 1, and W[1] = W[0]: its exact sum is 0"""
    n_in = len(x)
    rows = np.arange(3, nbr.shape[0], 7)
    if nbr.shape[1] < 2 or n_in < 2 or not len(rows):
        return
    W[1] = W[0]
    a = rng.integers(0, n_in // 2, size=len(rows))
    b = n_in // 2 + (np.arange(len(rows)) % (n_in - n_in // 2))
    x[b] = -x[a]
    nbr[rows] = -1
    nbr[rows, 0], nbr[rows, 1] = a, b
    x[b] = -x[nbr[rows, 0]]


def poison_rows(nbr, n_in, tile=None):
    """-> (referenced row to poison, mask of unreferenced rows): the row is pair 0 (first in row order) of an offset list --
    of the first `tile` rows where the kernel lists per tile, of the whole table otherwise -- whose length is no multiple of
    16; among those the one that the fewest other entries reference"""
    nbr = np.asarray(nbr)
    ref = np.bincount(nbr[nbr >= 0].ravel(), minlength=n_in)
    best = None
    for k in range(nbr.shape[1]):
        j = np.nonzero(nbr[:tile, k] >= 0)[0]
        if len(j) % 16 and len(j):
            cand = int(nbr[j[0], k])
            if best is None or ref[cand] < ref[best]:
                best = cand
    assert best is not None, "no offset list with a padded group"
    return best, ref == 0


def case(name, doc, kernel, route, variant, kind, K, cin, cout, n_out, n_in=None, nbr="random", density=0.3, lay=ALIGNED,
         epi=True, relu=True, l2norm=False, aux=None, os_R=0, bf3=False, cancel=False, cross=False, zero_rows=(), ptile=None):
    """register a forward case; nbr: 'random', None (identity) or a callable (rng, n_out, K, n_in) -> table"""
    assert name not in REGISTRY, name
    cross = cross or kind == "cross"

    @functools.lru_cache(maxsize=None)
    def build():
        rng = np.random.default_rng(_seed(name))
        nin = n_out if n_in is None else n_in
        if nbr is None:
            tbl = None
        elif nbr == "random":
            tbl = random_map(rng, n_out, K, nin, density)
        else:
            tbl = np.ascontiguousarray(nbr(rng, n_out, K, nin), np.int32)
        make = _bound_data if kind == "bound" else _exact_data
        kw = {"cross": True} if cross else {}
        x, W, scale, shift, res = make(rng, nin, K, cin, cout, n_out, **kw)
        if kind == "bound" and cancel and tbl is not None:
            _plant_cancelling_rows(rng, x, W, tbl)
        for r in zero_rows:          # an output row whose value is exactly zero: no neighbour, and no shift / residual below
            if tbl is None:
                x[r] = 0
            else:
                tbl[r] = -1
        c = dict(name=name, doc=doc, kernel=kernel, route=route, variant=variant, kind=kind, K=K, cin=cin, cout=cout, n_out=n_out,
                 n_in=nin, nbr=tbl, x=x, W=W, scale=scale if epi else None, shift=shift if epi else None,
                 res=res if epi else None, relu=bool(relu and epi and kind != "poison"), l2norm=l2norm, lay=lay, aux=aux, os_R=os_R, bf3=bf3,
                 cross=cross, poison=None)
        if kind == "poison":
            row, unref = poison_rows(tbl, nin, ptile)
            x[unref] = np.nan
            x[row] = np.nan
            c["poison"] = row
        return c
    REGISTRY[name] = build
    build.meta = dict(name=name, kernel=kernel, route=route, variant=variant, kind=kind, K=K, cin=cin, cout=cout, n_out=n_out,
                      lay=lay, bf3=bf3, aux=aux, l2norm=l2norm, identity=nbr is None, doc=doc)


def get(name):
    return REGISTRY[name]()


def names(kernel=None, kind=None):
    return [n for n, b in REGISTRY.items() if (kernel is None or b.meta["kernel"] == kernel) and (kind is None or b.meta["kind"] == kind)]


def prove_exact(c):
    """an exact case's claim, from its actual values: operands of at most 8 significant bits (cross: x of at most 16, W of 8,
    so only kept cross terms are non-zero), and max sum |x| |W| (times |scale|, plus |shift| + |res|) below 2^24 in integers"""
    import spconv_oracle as O
    xh, xm, xl = O.split3(c["x"])
    wh, wm, wl = O.split3(c["W"])
    assert not wm.any() and not wl.any() and not xl.any()
    assert bool(xm.any()) == bool(c["cross"])
    for a in (c["x"], c["W"], c["shift"], c["res"]):
        assert a is None or np.array_equal(a, np.round(a))
    mag = O.contract(np.abs(xh) + np.abs(xm), c["nbr"], np.abs(wh), c["n_out"])
    if c["scale"] is not None:
        assert np.all(np.log2(c["scale"]) == np.round(np.log2(c["scale"])))
        mag = mag * c["scale"] + np.abs(c["shift"]) + np.abs(c["res"])
    assert float(mag.max(initial=0.0)) < 2.0 ** 23           # half-integers after scale 0.5 need one more bit
    return float(mag.max(initial=0.0))


# ============================================================================================== k_spconv_pairs (route TILE)
def _each_kind(name, doc, *a, kinds=("exact", "bound"), **kw):
    for kind in kinds:
        case(f"{name}/{kind}", doc, *a[:3], kind, *a[3:], **kw)


_ROWS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
for _i, (_ci, _co) in enumerate([(a, b) for a in (32, 64, 96) for b in (32, 64, 96)] + [(64, 64)]):
    _each_kind(f"pairs_c{_ci}_{_co}_n{_ROWS[_i]}",
               f"cin {_ci} -> cout {_co}: CK = {64 if _ci % 64 == 0 else 32}, CN = {64 if _co % 64 == 0 else 32}; {_ROWS[_i]} rows: "
               "a ragged or single tile, fewer than 8 workgroups for the XCD tile map",
               "pairs", TILE, tid(PAIRS, 32, 64 if _co % 64 == 0 else 32, 64 if _ci % 64 == 0 else 32), 27, _ci, _co, _ROWS[_i],
               n_in=40, cancel=True)


def _planted_counts(TM):
    def f(rng, n_out, K, n_in):
        base = random_map(rng, n_out, K, n_in, 0.3)
        base[:TM] = -1
        return planted_map(rng, n_out, K, n_in, [(0, 3, 15), (0, 4, 16), (0, 5, 17), (0, 9, TM)], base)
    return f


_each_kind("pairs_tm64_cout256", "cdiv(6337, 64) * (256 / 64) = 400 workgroups: the smallest row count with 64-row tiles at cout "
           "256 (CN 64, CK 32); tile 0 holds offsets with exactly 15, 16, 17 and 64 pairs",
           "pairs", TILE, tid(PAIRS, 64, 64, 32), 27, 32, 256, 6337, nbr=_planted_counts(64), kinds=("exact", "bound", "poison"), ptile=64)
_each_kind("pairs_tm32_cout256", "one row fewer: 396 workgroups, 32-row tiles", "pairs", TILE, tid(PAIRS, 32, 64, 32), 27, 32, 256,
           6336, nbr=_planted_counts(32), kinds=("exact",))
_each_kind("pairs_tm64_cout96", "cout 96 gives CN = 32: cdiv(8513, 64) * 3 = 402 >= 400 -> TM 64, CN 32, CK 64",
           "pairs", TILE, tid(PAIRS, 64, 32, 64), 27, 64, 96, 8513, nbr=_planted_counts(64))
_each_kind("pairs_tm32_cout96", "8512 rows: 399 workgroups, 32-row tiles", "pairs", TILE, tid(PAIRS, 32, 32, 64), 27, 64, 96, 8512,
           nbr=_planted_counts(32), kinds=("exact",))
_each_kind("pairs_counts_tm32", "tile 0 holds offsets with exactly 15, 16, 17 and 32 (= TM) pairs; 3 tiles, 75 rows",
           "pairs", TILE, tid(PAIRS, 32, 64, 64), 27, 64, 64, 75, nbr=_planted_counts(32), kinds=("exact", "bound", "poison"), ptile=32)
_each_kind("pairs_full27", "all 27 offsets of every row present: every list has TM pairs, 27 items over 4 waves",
           "pairs", TILE, tid(PAIRS, 32, 64, 64), 27, 64, 64, 50, n_in=64, density=1.1)
for _a in (1, 2, 3, 5):
    _each_kind(f"pairs_items{_a}", f"{_a} active offset(s) and one chunk: {_a} work item(s) for 4 waves" +
               (" -- waves 1 to 3 have none" if _a == 1 else ""), "pairs", TILE, tid(PAIRS, 32, 64, 64), 27, 64, 64, 40,
               nbr=(lambda a: lambda rng, n, K, nin: planted_map(rng, n, K, nin, [(0, 2 * i + 1, n - i) for i in range(a)]))(_a),
               kinds=("exact",))
_each_kind("pairs_items3_chunks", "one active offset, cin 96 = three 32-channel chunks: 3 items of the same offset",
           "pairs", TILE, tid(PAIRS, 32, 32, 32), 27, 96, 96, 40,
           nbr=lambda rng, n, K, nin: planted_map(rng, n, K, nin, [(0, 13, n)]), kinds=("exact",))
_each_kind("pairs_empty_tile", "rows 32..63 (tile 1) have no neighbour at all: the epilogue still writes shift + residual",
           "pairs", TILE, tid(PAIRS, 32, 64, 64), 27, 64, 64, 96,
           nbr=lambda rng, n, K, nin: np.concatenate([random_map(rng, 32, K, nin), np.full((32, K), -1), random_map(rng, n - 64, K, nin)]))
_each_kind("pairs_same_row", "every pair of the map reads input row n_in - 1", "pairs", TILE, tid(PAIRS, 32, 64, 32), 27, 32, 64, 45,
           n_in=77, nbr=lambda rng, n, K, nin: np.where(random_map(rng, n, K, nin, 0.4) >= 0, nin - 1, -1))
_each_kind("pairs_k1_identity", "identity map (nbr NULL, K = 1) below the dense kernel's 144 workgroups", "pairs", TILE,
           tid(PAIRS, 32, 64, 64), 1, 64, 64, 100, nbr=None)
_each_kind("pairs_k1_dense_neighbour", "cout 512 at 1088 rows: 17 * 8 = 136 < 144 workgroups, the identity map stays on the tile kernel",
           "pairs", TILE, tid(PAIRS, 32, 64, 64), 1, 64, 512, 1088, nbr=None, kinds=("exact",))
for _K in (2, 8):
    _each_kind(f"pairs_k{_K}", f"a {_K}-offset map", "pairs", TILE, tid(PAIRS, 32, 64, 64), _K, 64, 64, 70, density=0.6, cancel=True)
for _co, _fused in ((32, True), (64, True), (96, False), (128, False)):
    case(f"pairs_l2_cout{_co}/bound", f"row normalisation behind the layer, cout {_co}: " +
         ("fused into the epilogue" if _fused else "a second launch") + "; row 5 is all zero (0 / 0)", "pairs", TILE,
         tid(PAIRS, 32, 64 if _co % 64 == 0 else 32, 64, flag=_fused), "bound", 27, 64, _co, 70, epi=False, l2norm=True, zero_rows=(5,))

# ================================================================================================ k_spconv_mfma (route TILE)
OUT_OFF1 = {"x": (8, 4), "out": (11, 1), "res": (4, 4)}         # out rows start 1 float off a 16-byte boundary
RES_OFF1 = {"x": (8, 4), "out": (12, 8), "res": (3, 1)}         # residual rows likewise
for _ci, _co, _n in ((64, 64, 1), (32, 64, 17), (64, 32, 33), (32, 32, 49)):
    _each_kind(f"mfma_c{_ci}_{_co}_n{_n}", f"out at a column offset of 1 float -> k_spconv_mfma<32, {64 if _co == 64 else 32}, .., "
               f"{64 if _ci == 64 else 32}>; row tail {_n % 32}", "mfma", TILE,
               tid(MFMA, 32, 64 if _co == 64 else 32, 64 if _ci == 64 else 32), 27, _ci, _co, _n, n_in=50, lay=OUT_OFF1,
               kinds=("exact", "bound", "poison") if _n == 49 else ("exact", "bound"), cancel=True)
_each_kind("mfma_res_misaligned", "only the residual's rows are misaligned", "mfma", TILE, tid(MFMA, 32, 64, 64), 27, 64, 64, 70,
           lay=RES_OFF1)
for _K in (28, 32):
    _each_kind(f"mfma_k{_K}", f"K = {_K} > 27: aligned rows, still k_spconv_mfma; offset {_K - 1} is bit {_K - 1} of its offset mask "
               "and is the only offset of rows 0..19", "mfma", TILE, tid(MFMA, 32, 64, 32), _K, 32, 64, 70,
               nbr=(lambda K_: lambda rng, n, K, nin: planted_map(rng, n, K, nin, [(0, K_ - 1, 20)],
                                                                    np.concatenate([np.full((20, K), -1), random_map(rng, n - 20, K, nin)])))(_K))
_each_kind("mfma_n32767", "32767 rows: the last row count with 32-row tiles", "mfma", TILE, tid(MFMA, 32, 32, 32), 2, 32, 32, 32767,
           lay=OUT_OFF1, density=0.6, kinds=("exact",))
_each_kind("mfma_n32768", "32768 rows: 64-row tiles", "mfma", TILE, tid(MFMA, 64, 32, 32), 2, 32, 32, 32768, lay=OUT_OFF1,
           density=0.6, kinds=("exact",))
_each_kind("mfma_tm64_tail33", "64-row tiles with a row tail of 33", "mfma", TILE, tid(MFMA, 64, 64, 64), 2, 64, 64, 32768 + 33,
           lay=OUT_OFF1, density=0.6)

# ======================================================================== k_spconv_smallcin / k_spconv_generic (route TILE)
for _ci, _K, _co, _n in ((1, 27, 32, 1), (1, 125, 64, 63), (3, 27, 96, 64), (3, 125, 32, 65), (1, 27, 96, 65), (3, 27, 64, 63)):
    _each_kind(f"smallcin_c{_ci}_k{_K}_o{_co}_n{_n}", f"cin {_ci}, K {_K}, cout {_co}, {_n} rows (64 rows per workgroup)", "smallcin",
               TILE, tid(SMALLCIN, 64, 0, _ci), _K, _ci, _co, _n, n_in=90, kinds=("exact", "bound", "poison") if _n == 65 else ("exact", "bound"))
_each_kind("generic_c5_o7", "odd widths", "generic", TILE, tid(GENERIC), 27, 5, 7, 333, lay={"x": (3, 1), "out": (2, 1), "res": (1, 1)},
           kinds=("exact", "bound", "poison"))
_each_kind("generic_c1_o8", "cin 1 with a cout that the small-cin kernel does not take", "generic", TILE, tid(GENERIC), 27, 1, 8, 130)
_each_kind("generic_k343", "K = 343 with cin 1: 64 rows of the table are 87 808 B, past the small-cin kernel's 64 KB of LDS",
           "generic", TILE, tid(GENERIC), 343, 1, 32, 70, density=0.1)

# ================================================================================================ k_spconv_bigk (route TILE)
for _K, _ci, _co in ((33, 32, 32), (64, 64, 32), (124, 32, 64), (125, 128, 32)):
    _each_kind(f"bigk_k{_K}", f"K = {_K}, {_ci} -> {_co}", "bigk", TILE, tid(BIGK), _K, _ci, _co, 130, density=0.15)

# ======================================================================================= k_dense_gemm<1|2> (route TILE, K = 1)
for _ci, _co, _M, _G in ((64, 9216, 1, 1), (128, 9216, 63, 1), (192, 9216, 64, 1), (64, 4608, 65, 1), (128, 4608, 127, 1),
                         (64, 4608, 128, 1), (192, 3072, 129, 1), (64, 512, 1089, 1), (128, 512, 8064, 1), (64, 512, 8065, 2)):
    _each_kind(f"dense_c{_ci}_o{_co}_m{_M}", f"{_M} rows x {_ci} -> {_co}: {_ci // 64} input chunk(s), {64 * _G}-row tiles; "
               "cdiv(M, 64) * cout / 64 >= 144 workgroups", "dense", TILE, tid(DENSE, 64 * _G, 64, 64), 1, _ci, _co, _M, nbr=None,
               kinds=("exact", "bound") if _M in (65, 1089, 8065) else ("exact",))

# =========================================================================== k_dense_gemm_bf3 (route DENSE_GEMM), split weights
for _ci, _co, _M, _G in ((64, 64, 1, 1), (128, 64, 63, 1), (192, 64, 64, 1), (64, 128, 65, 1), (128, 64, 127, 1), (64, 64, 128, 1),
                         (256, 64, 129, 1), (128, 512, 8064, 1), (128, 512, 8065, 2), (64, 512, 8065, 2)):
    _each_kind(f"densebf3_c{_ci}_o{_co}_m{_M}", f"{_M} rows x {_ci} -> {_co}: {_ci // 64} chunk(s), rows " +
               ("staged through LDS" if _ci >= 128 else "loaded as fragments") + f", {64 * _G}-row tiles", "dense_bf3", DENSE_GEMM,
               tid(DENSE_BF3, 64 * _G, 64, 64, flag=_ci >= 128), 1, _ci, _co, _M, nbr=None, bf3=True,
               kinds=("exact", "cross", "bound") if _M in (65, 129, 8065) else ("exact", "cross"))

# ================================================================================== k_dense_rows_bf3 (route DENSE_ROWS, K = 1)
# aux "rows": called by name (apr_dense_rows_bf3); the router sends a layer there from 32 768 rows on, as in dense_rows_m65537
_MS = [1, 31, 32, 33, 255, 256, 257]
for _i, (_ci, _co) in enumerate([(a, b) for a in (64, 96, 128, 160, 192) for b in (32, 64, 128)]):
    _M = _MS[_i % 7]
    _each_kind(f"dense_rows_c{_ci}_o{_co}_m{_M}", f"{_M} rows x {_ci} -> {_co} (32 rows per wave, 256 per tile)", "dense_rows", DENSE_ROWS,
               None, 1, _ci, _co, _M, nbr=None, bf3=True, aux="rows", kinds=("exact", "cross", "bound") if _i % 3 == 0 else ("exact", "cross"))
_each_kind("dense_rows_m65537", "65 537 rows: 257 tiles for at most 256 workgroups, the grid-stride loop's second trip; routed", "dense_rows",
           DENSE_ROWS, None, 1, 64, 32, 65537, nbr=None, bf3=True, kinds=("exact", "cross"))
for _co in (32, 128):
    case(f"dense_rows_l2_o{_co}/bound", "row normalisation in the row stream's epilogue; row 5 is all zero (0 / 0)", "dense_rows",
         DENSE_ROWS, None, "bound", 1, 96, _co, 300, nbr=None, bf3=True, aux="rows", epi=False, l2norm=True, zero_rows=(5,))

# =================================================================== k_pairs_build + k_ws_gemm[_bf3] + k_ws_reduce (WS / WS_BF3)
def _ws_counts(rng, n_out, K, n_in):
    """offsets with 0, 1, 63, 64 and 65 pairs, the rest random"""
    base = random_map(rng, n_out, K, n_in, 0.3)
    base[:, :5] = -1
    return planted_map(rng, n_out, K, n_in, [(7, 1, 1), (100, 2, 63), (200, 3, 64), (300, 4, 65)], base)


for _n in (511, 512, 513):
    for _kern, _route, _bf3 in (("ws", WS, False), ("ws_bf3", WS_BF3, True)):
        _each_kind(f"{_kern}_counts_n{_n}", f"{_n} rows (512 per build block); offsets with 0, 1, 63, 64, 65 pairs", _kern, _route, None,
                   27, 64, 64, _n, nbr=_ws_counts, aux="pairs", bf3=_bf3,
                   kinds=(("exact", "cross", "bound", "poison") if _bf3 else ("exact", "bound", "poison")) if _n == 513 else ("exact",))
for _K in (1, 8, 9):
    _each_kind(f"ws_bf3_k{_K}", f"a {_K}-offset map" + (": k_ws_reduce<8>" if _K == 8 else ""), "ws_bf3", WS_BF3, None, _K, 64, 64, 300,
               density=0.7, aux="pairs", bf3=True)
    _each_kind(f"ws_k{_K}", f"a {_K}-offset map on the fp32 kernel", "ws", WS, None, _K, 64, 64, 300, density=0.7, aux="pairs", kinds=("exact",))
for _ci, _co in ((128, 64), (192, 192), (256, 64), (384, 64)):
    _each_kind(f"ws_bf3_c{_ci}_o{_co}", f"cin {_ci}: {_ci // 64} chunks per group; cout {_co}", "ws_bf3", WS_BF3, None, 27, _ci, _co, 200,
               n_in=150, aux="pairs", bf3=True, kinds=("exact", "cross", "bound"), cancel=True)
for _ci, _co in ((320, 64), (512, 192)):
    _each_kind(f"ws_c{_ci}_o{_co}", f"cin {_ci}: a weight-stationary width without a bf16 instance: the fp32 kernel",
               "ws", WS, None, 27, _ci, _co, 200, n_in=150, aux="pairs", cancel=True)
for _kern, _route, _bf3 in (("ws", WS, False), ("ws_bf3", WS_BF3, True)):
    _each_kind(f"{_kern}_g3", "4 000 rows of a full 27-offset map: 108 000 pairs, 1 688 64-pair blocks > 768 units, so the "
               "device-side G is 3", _kern, _route, None, 27, 64, 64, 4000, density=1.1, aux="pairs", bf3=_bf3, kinds=("exact",))

# ============================================================================ k_pairs3_build + k_ws3_gemm_bf3 + k_ws_reduce (WS3)
def _ws3_patterns(mixed):
    def f(rng, n_out, K, n_in):
        nbr = np.full((n_out, 27), -1, np.int32)
        for j in range(n_out):
            for t in range(9):
                p = ((j + t) % 8) if mixed else ((j // 8) % 8 if t == j % 9 else 0)      # presence pattern of the triple, 0 = no entry
                for b in range(3):
                    if p >> b & 1:
                        nbr[j, 3 * t + b] = rng.integers(0, n_in)
        return nbr
    return f


for _n in (255, 256, 257):
    _each_kind(f"ws3_mixed_n{_n}", f"{_n} rows (256 per build block); every row mixes the seven presence patterns of a triple "
               "and one triple with no entry", "ws3", WS3, None, 27, 64, 64, _n, nbr=_ws3_patterns(True), aux="triples", bf3=True,
               kinds=("exact", "cross", "bound", "poison") if _n == 257 else ("exact",))
_each_kind("ws3_alone", "each row has at most ONE triple with entries, its pattern walking through the seven (and none)", "ws3", WS3, None,
           27, 64, 64, 300, nbr=_ws3_patterns(False), aux="triples", bf3=True, kinds=("exact", "cross"))
_each_kind("ws3_c128", "cin 128: the 8-wave form", "ws3", WS3, None, 27, 128, 128, 300, aux="triples", bf3=True,
           kinds=("exact", "cross", "bound"), cancel=True)

# ========================================================================================== k_os_build + k_os_conv (route OS)
def _os_map(R):
    def f(rng, n_out, K, n_in):
        base = random_map(rng, n_out, K, n_in, 0.3)
        base[:min(R, n_out)] = -1                      # tile 0: offsets with 1, 16 and 17 pairs, nothing else
        nbr = planted_map(rng, n_out, K, n_in, [(0, 0, 1), (0, 13, min(16, n_out)), (0, 26, min(17, n_out))], base)
        if n_out > 2 * R:
            nbr[R:2 * R] = -1                          # tile 1: empty
        return nbr
    return f


for _n in (63, 64, 65, 129):
    _each_kind(f"os_r64_n{_n}", f"{_n} rows in tiles of 64; tile 0: offsets with 1, 16 and 17 pairs (3 items: an odd count)" +
               ("; tile 1 empty" if _n == 129 else ""), "os", OS, None, 27, 64, 64, _n, n_in=100, nbr=_os_map(64), aux="os", os_R=64, bf3=True, ptile=64,
               kinds=("exact", "cross", "bound", "poison") if _n == 129 else ("exact",))
_each_kind("os_groups", "all 27 offsets of 160 rows full: 10 groups per (tile, offset), more than the 8 waves deal in one slot",
           "os", OS, None, 27, 64, 64, 160 + 5, n_in=200, density=1.1, aux="os", os_R=160, bf3=True, kinds=("exact", "cross"))
OS_R = {(64, 64): 80, (128, 64): 80, (64, 128): 160, (128, 128): 160}      # apr_spconv_os_tile_rows(20 000 rows, cin, cout)
for (_ci, _co), _R in OS_R.items():
    for _n in (_R - 1, _R, _R + 1, 2 * _R + 1):
        _each_kind(f"os_c{_ci}_o{_co}_n{_n}", f"{_ci} -> {_co} in tiles of R = {_R} rows, the height the library picks for 20 000 rows "
                   f"of this shape: {_n} rows", "os", OS, None, 27, _ci, _co, _n, n_in=300, nbr=_os_map(_R), aux="os", os_R=_R, bf3=True,
                   kinds=("exact", "cross", "bound") if _n == 2 * _R + 1 else ("exact",))


# ==================================================================================================== gradients (spconv_bwd.hip)
WGRAD = {}


def wgrad_case(name, doc, kernel, plan, K, cin, cout, n_out, nbr, same_level=False, x_off=0, kinds=("exact", "bound"), pad=True):
    """plan: the literal (kernel id, CI, CO, S_all, S_c, k_c) that apr_spconv_wgrad_plan must report; x_off: column offset of
    x inside a wider buffer (1: rows not 16-byte aligned); pad False: ops.WGRAD_PAD off (odd widths on the fp32 kernel)"""
    for kind in kinds:
        full = f"{name}/{kind}"
        assert full not in WGRAD

        @functools.lru_cache(maxsize=None)
        def build(kind=kind, full=full):
            rng = np.random.default_rng(_seed(full))
            tbl = None if nbr is None else np.ascontiguousarray(nbr(rng, n_out, K, n_out), np.int32)
            if kind == "exact":
                x = rng.integers(-7, 8, size=(n_out, cin)).astype(np.float32)
                dy = rng.integers(-7, 8, size=(n_out, cout)).astype(np.float32)
            else:
                x = (rng.standard_normal((n_out, cin)) * np.exp(rng.uniform(-9.2, 9.2, (n_out, 1)))).astype(np.float32)
                dy = (rng.standard_normal((n_out, cout)) * np.exp(rng.uniform(-4.6, 4.6, (n_out, 1)))).astype(np.float32)
            return dict(name=full, doc=doc, kernel=kernel, plan=plan, K=K, cin=cin, cout=cout, n_out=n_out, nbr=tbl, x=x, dy=dy,
                        same_level=same_level, x_off=x_off, kind=kind, pad=pad)
        build.meta = dict(kernel=kernel, plan=plan, K=K, cin=cin, cout=cout, n_out=n_out, same_level=same_level, x_off=x_off, pad=pad)
        WGRAD[full] = build


def _rand(density):
    return lambda rng, n, K, nin: random_map(rng, n, K, nin, density)


def _with_empty_offset(rng, n, K, nin):
    nbr = random_map(rng, n, K, nin, 0.3)
    nbr[:, 4] = -1
    return nbr


B3, PT = L.WGRAD_BF3, L.WGRAD_PARTIAL
# S = min(cdiv(512, K * tiles), nrb); same level, odd K > 1: k_c = K / 2, S_c = min(4 S, nrb)
for _ci, _co, _CI, _CO, _n in ((32, 32, 32, 32, 1), (32, 64, 32, 64, 31), (32, 128, 32, 128, 32), (64, 32, 64, 32, 33),
                               (64, 64, 64, 64, 511), (64, 128, 64, 128, 512)):
    wgrad_case(f"wgrad_c{_ci}_o{_co}_n{_n}", f"k_wgrad_bf3<{_CI}, {_CO}>, {_n} rows: one 512-row block, one split; offset 4 is empty",
               "wgrad_bf3", (B3, _CI, _CO, 1, 1, -1), 27, _ci, _co, _n, _with_empty_offset)
wgrad_case("wgrad_n513", "513 rows: two row blocks, S_all = min(19, 2) = 2", "wgrad_bf3", (B3, 32, 32, 2, 2, -1), 27, 32, 32, 513, _rand(0.3))
wgrad_case("wgrad_same_n1025", "same-level map, 1 025 rows (3 blocks): S_all = 3 and S_c = min(12, 3) = 3, the nrb arm; the centre "
           "column is full", "wgrad_bf3", (B3, 64, 64, 3, 3, 13), 27, 64, 64, 1025, same_level_map, same_level=True)
wgrad_case("wgrad_same_n2049_wide", "same-level map, 2 049 rows (5 blocks) at 128 -> 128: 2 tiles, S_all = cdiv(512, 54) = 10 -> 5; "
           "S_c = 5", "wgrad_bf3", (B3, 64, 128, 5, 5, 13), 27, 128, 128, 2049, same_level_map, same_level=True, kinds=("exact",))
wgrad_case("wgrad_same_n2049_s1", "same-level map, 2 049 rows at 256 -> 256: 8 tiles, S_all = cdiv(512, 216) = 3 of 5 blocks, and "
           "S_c = min(12, 5) = 5: both arms differ", "wgrad_bf3", (B3, 64, 128, 3, 5, 13), 27, 256, 256, 2049, same_level_map,
           same_level=True, kinds=("exact",))
wgrad_case("wgrad_same_n6657", "same-level map, 6 657 rows (14 blocks) at 256 -> 256: S_all = 3, S_c = min(12, 14) = 12, the 4 S arm",
           "wgrad_bf3", (B3, 64, 128, 3, 12, 13), 27, 256, 256, 6657, same_level_map, same_level=True, kinds=("exact",))
wgrad_case("wgrad_same_sparse_centre", "the same-level entry point on a map whose centre column is NOT full", "wgrad_bf3",
           (B3, 64, 64, 3, 3, 13), 27, 64, 64, 1025, _rand(0.3), same_level=True)
wgrad_case("wgrad_k1_identity", "identity map, K = 1: no centre offset even through the same-level entry", "wgrad_bf3",
           (B3, 64, 64, 2, 2, -1), 1, 64, 64, 513, None, same_level=True)
for _n in (511, 512, 513):
    wgrad_case(f"wgrad_partial_misaligned_n{_n}", f"x rows 1 float off a 16-byte boundary -> k_wgrad_partial; {_n} rows: "
               f"{-(-_n // 512)} chunk(s)", "wgrad_partial", (PT, 64, 64, -(-_n // 512), -(-_n // 512), -1), 27, 32, 64, _n, _rand(0.3), x_off=1)
wgrad_case("wgrad_partial_c3_o5", "odd widths with the zero padding switched off", "wgrad_partial", (PT, 64, 64, 2, 2, -1), 27, 3, 5, 513,
           _rand(0.3), pad=False)
wgrad_case("wgrad_partial_c1_o32", "cin 1 with the zero padding switched off", "wgrad_partial", (PT, 64, 64, 1, 1, -1), 8, 1, 32, 300,
           _rand(0.6), pad=False)

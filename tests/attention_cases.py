"""Named inputs for the kernels of the overlap-attention module, each with the edge it exists for
(tests/test_attention_oracle_cpu.py confirms the planted facts from the oracle's own float64 values).  numpy only; everything
is built on the host from small integer seeds.

Kernel constants the cases are built around (apr_amd/csrc/attention.hip):
* k_mha: 8 queries per workgroup, 256 threads over the keys, scores [8][max(m, 256)] + queries [8][dim] in 60 KB of LDS
  (m <= 1920 - dim), dim divides 256; the value pass has ngrp = 256 / dim key groups stepping 4 * ngrp keys.
* k_mha_mfma: dim 64, 16 queries per workgroup, 4 waves over the 16-key tiles (wave = tile % 4), online softmax, merge of 4.
* k_softmax_matvec_mfma: c in {32, 64, 128, 256}, 16 queries per workgroup, 8 waves (wave = tile % 8), 32 partial triples.
* k_softmax_matvec_t: 4 queries per workgroup, 4 (m + c) floats of LDS (m + c <= 3840); k_softmax_matvec: one query per
  workgroup, m + c <= 15360.
* training path: one workgroup per (query, head) with the head vector in LDS (dim <= 1024, strided by 256 threads);
  k_mha_rowmat / k_mha_colmat and the edge kernels are grid-stride loops of at most 16384 x 256 threads.

Softmax cases.  Channels are interleaved (d * H + h).  In every head, channel d = 0 of the keys holds
phi_j = j // 16 + 3 [j == m - 1] (the tile index, counted over the last 256 tiles and 0 before them, so that no score
leaves the range in which a first-order bound is meaningful; small integers, exact in every format) and channel d = 1
(dim >= 2) holds 1; the other channels, the values and the remaining queries are standard normal.  A DESIGNATED row is a
(query, head) pair whose query vector is zero outside what its kind names, so its scores are known in closed form:
  last       q_0 = 1 / scale: s_j = phi_j.  Tiles ascend by 1, so every step of an online softmax rescales; the last key
             carries e^3 / (e^3 + 15 + 16 / (e - 1)) > 0.44 of the weight: dropping or doubling it, shifting v, or leaving out
             the partial that holds it is visible here.
  dominant   q_0 = 112 / scale: the last key is 336 above its tile-mates and every tile 112 above the one before: all other
             weights underflow, the row is v[m - 1]; every other wave's merge factor is exp(< -110) = 0.
  tie        q_1 = 4096 (dim >= 2; q = 0 for dim = 1): every key has the same products, so the scores tie exactly on a
             common offset of 4096 before scaling and the row is the mean of v.  (Identical scores through the channels the
             query reads; the other key channels stay random so that the other rows keep their own scores.)
  first      q_0 = -1 / scale: the first tile holds the maximum (with the tiles of phi = 0 behind it): no step rescales.
  offset     q_0 = 1 / scale, q_1 = 4096: `last` on a common offset of 4096 before scaling (Inf / NaN without the max).
  firstdom   q_0 = -112 / scale: the keys of phi = 0 (the first tile for m <= 4096) are 112 above every other key, the row
             is the mean of their values.
  key:<t>    (dim >= 4) the query points along the random channels of key t, whose random part was stretched to 1.5 times
             the longest other key (below 18 channels the planted keys' random parts are spread on a circle instead), with
             the length L that solves e^L = sum_{j != t} e^{s_j}: key t carries half of the weight.  Planted for the keys
             b - 1 and b (the last and the first key of a tile) of the LAST boundary b = g * ((m - 1) // g) > 0 of each g in
             16, 64, 128, 256, and, in the rows left over after every other kind, of every other boundary b = g, 2 g, ...
             from the last backwards (at most 40 keys); m - 1 itself is the `last` row.  The first value channel of a
             planted key (and of the last key) is +-(3 + h / 4), clear of the standard normal others.
Kinds are handed to the rows (i, h) = (r % n, r // n % H), r = 0, 1, ... in the order last, key:* (last boundaries),
dominant, tie, first, offset, firstdom, key:* (the other boundaries) until the n * H rows are used up; every case with
n * H >= 2 has at least two designated rows (a case with one query and one head has one row, which is designated).
The `*-samekeys` cases state the tie the other way: every key row is the same row, so EVERY query, random as it is, ties
exactly and every output row is the mean of v.
"""
import numpy as np

F32 = np.float32
GRAN = (16, 64, 128, 256)
BONUS = 3.0
OFFSET = 4096.0
GAP = 112.0


def phi(m):
    tile = np.arange(m) // 16
    p = np.maximum(tile - max(0, tile[-1] - 255), 0).astype(np.float64)
    p[m - 1] += BONUS
    return p


def target_keys(m):
    """(first, more): the keys b - 1 and b of the last boundary of each tile size that m crosses, then those of every other
    boundary, from the last backwards (at most 40 in all); m - 1 is the `last` row's"""
    first = sorted({t for g in GRAN for t in (g * ((m - 1) // g) - 1, g * ((m - 1) // g)) if g * ((m - 1) // g) > 0} - {m - 1})
    more = list({t for g in GRAN for b in range(g, m, g) for t in (b - 1, b)} - set(first) - {m - 1})
    more.sort(reverse=True)
    return first, more[:max(0, 40 - len(first))]


def _solve_half(r):
    """L >= 0 with L = log sum_j exp(L r_j) for r_j < 1 (the target carries half of the weight)"""
    def f(L):
        z = L * r
        zm = z.max()
        return L - (zm + np.log(np.exp(z - zm).sum()))
    lo, hi = 0.0, 1.0
    while f(hi) <= 0:
        hi *= 2
        assert hi < 1e6
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) <= 0 else (lo, mid)
    return hi


def build_softmax(name, fact, seed, n, m, dim, H, vdim=None, scale=None, family="mha", same_keys=False):
    """q [n, dim * H], k [m, dim * H], v [m, vdim * H], dout [n, vdim * H] float32, scale (default 1 / sqrt(dim)),
    rows: list of dict(i, h, kind)"""
    rng = np.random.default_rng(seed)
    vdim = dim if vdim is None else vdim
    scale = float(F32(1.0) / np.sqrt(F32(dim))) if scale is None else float(scale)
    q = rng.standard_normal((n, dim, H))
    k = rng.standard_normal((m, dim, H))
    v = rng.standard_normal((m, vdim, H)).astype(F32)
    dout = rng.standard_normal((n, vdim, H)).astype(F32)
    k[:, 0, :] = phi(m)[:, None]
    if dim >= 2:
        k[:, 1, :] = 1.0
    first, more = target_keys(m) if dim >= 4 and m >= 3 and not same_keys else ([], [])
    fixed = 6 if dim >= 2 else 5                                  # the rows of the other kinds
    more = more[:max(0, n * H - fixed - len(first))]
    if dim - 2 < 16:
        more = more[:8]
    targets = first + more
    k = k.astype(F32).astype(np.float64)
    if targets:
        for h in range(H):
            norms = np.linalg.norm(k[:, 2:, h], axis=1)
            kmax = np.delete(norms, targets).max()
            for idx, t in enumerate(targets):
                if dim - 2 < 16:      # too few random channels for random directions to stay apart: spread them on a circle
                    ang = 2 * np.pi * idx / len(targets)
                    k[t, 2:, h] = 0.0
                    k[t, 2, h], k[t, 3, h] = 1.5 * kmax * np.cos(ang), 1.5 * kmax * np.sin(ang)
                else:
                    k[t, 2:, h] *= 1.5 * kmax / norms[t]
        k = k.astype(F32).astype(np.float64)
    for idx, t in enumerate(targets + [m - 1]):      # a planted key's first value channel stands clear of the others
        v[t, 0, :] = (3.0 + 0.25 * np.arange(H)) * (1 if idx % 2 == 0 else -1)
    kinds = (["last"] + [f"key:{t}" for t in first] + ["dominant", "tie", "first"] + (["offset"] if dim >= 2 else []) + ["firstdom"]
             + [f"key:{t}" for t in more])
    if m == 1:
        kinds = ["last", "tie"]
    if same_keys:                 # every key row is one row: every query ties; two of the random ones are designated
        k[:] = k[m // 2]
        kinds = ["tie", "tie"]
    rows = []
    inv = 1.0 / scale
    for r, kind in enumerate(kinds[:n * H]):
        i, h = r % n, (r // n) % H
        qr = np.zeros(dim)
        if kind in ("last", "offset"):
            qr[0] = inv
        elif kind == "dominant":
            qr[0] = GAP * inv
        elif kind == "first":
            qr[0] = -inv
        elif kind == "firstdom":
            qr[0] = -GAP * inv
        if kind in ("tie", "offset") and dim >= 2:
            qr[1] = OFFSET
        if same_keys:
            qr = q[i, :, h]
        if kind.startswith("key:"):
            t = int(kind[4:])
            kt = k[t, 2:, h]
            rr = np.delete(k[:, 2:, h] @ kt / (kt @ kt), t)
            qr[2:] = _solve_half(rr) * kt / ((kt @ kt) * scale)
        q[i, :, h] = qr
        rows.append(dict(i=i, h=h, kind=kind))
    c = lambda a: np.ascontiguousarray(a, F32).reshape(a.shape[0], -1)
    return dict(name=name, fact=fact, seed=seed, family=family, n=n, m=m, dim=dim, H=H, vdim=vdim, scale=scale, q=c(q), k=c(k),
                v=c(v), dout=c(dout), rows=rows, targets=targets, first_targets=first, same_keys=same_keys)


def rows_of(case, *kinds):
    return [r for r in case["rows"] if r["kind"] in kinds or (("key" in kinds) and r["kind"].startswith("key:"))]


# name: (edge it covers, seed, n, m, dim, heads)
_MHA = {
    "mha-n1-m1":        ("one query, one key, one head: a single workgroup, every softmax is 1", 101, 1, 1, 64, 1),
    "mha-n7-m255":      ("n = 7 (one short query block), m = 255: the key loop's last thread idle", 102, 7, 255, 64, 4),
    "mha-n8-m256":      ("n = 8 (a full query block), m = 256: exactly one trip of 256 threads; 3 heads", 103, 8, 256, 64, 3),
    "mha-n9-m257":      ("n = 9 (second block with one query), m = 257: second trip with one key; score area m > 256", 104, 9,
                         257, 64, 4),
    "mha-m15-d64":      ("dim 64: ngrp = 4, m = 4 ngrp - 1: one value step with its last slot empty", 105, 9, 15, 64, 1),
    "mha-m17-d64":      ("dim 64: m = 4 ngrp + 1: a second value step with one key", 106, 8, 17, 64, 3),
    "mha-m1856-d64":    ("dim 64: m = 1920 - 64 = 1856, the LDS limit", 107, 9, 1856, 64, 1),
    "mha-m63-d16":      ("dim 16: ngrp = 16, m = 4 ngrp - 1", 108, 7, 63, 16, 3),
    "mha-m65-d16":      ("dim 16: m = 4 ngrp + 1", 109, 9, 65, 16, 4),
    "mha-m1904-d16":    ("dim 16: m = 1920 - 16 = 1904, the LDS limit; one query", 110, 1, 1904, 16, 1),
    "mha-m255-d4":      ("dim 4: ngrp = 64, m = 4 ngrp - 1", 111, 9, 255, 4, 3),
    "mha-m257-d4":      ("dim 4: m = 4 ngrp + 1", 112, 8, 257, 4, 4),
    "mha-m3-d256":      ("dim 256: ngrp = 1, m = 4 ngrp - 1; the query load strides (8 * 256 values)", 113, 9, 3, 256, 1),
    "mha-m5-d256":      ("dim 256: m = 4 ngrp + 1; 3 heads", 114, 7, 5, 256, 3),
    "mha-samekeys":     ("identical key rows, n = 9, m = 257, 4 heads of 64: every row is the mean of v", 116, 9, 257, 64, 4),
    "mha-m1664-d256":   ("dim 256: m = 1920 - 256 = 1664, the LDS limit", 115, 8, 1664, 256, 1),
}
# dim 64: (edge, seed, n, m, heads)
_HEADMAJOR = {
    "hm-m1":    ("m = 1: one tile of one key, three waves see no tile; n = 17", 121, 17, 1, 1),
    "hm-m5":    ("m = 5: one tile, two of the four k-slots partly empty; n = 15", 122, 15, 5, 3),
    "hm-m15":   ("m = 15; n = 16: one full query block", 123, 16, 15, 4),
    "hm-m16":   ("m = 16: exactly one tile; n = 33: three blocks, the last with one query", 124, 33, 16, 1),
    "hm-m17":   ("m = 17: a last tile with a single key, two waves idle; n = 1", 125, 1, 17, 4),
    "hm-m63":   ("m = 63: four tiles, one per wave; n = 17", 126, 17, 63, 3),
    "hm-m64":   ("m = 64: four full tiles; n = 16", 127, 16, 64, 1),
    "hm-m65":   ("m = 65: wave 0 takes a second tile with a single key (one rescale, one prefetch); n = 15", 128, 15, 65, 4),
    "hm-m129":  ("m = 129: nine tiles; n = 33", 129, 33, 129, 3),
}
# (edge, seed, n, m, c)
_SMV = {
    "smv-c64-m257":   ("mfma c = 64; n = 1; m = 257: 17 tiles, wave 0 takes three", 131, 1, 257, 64),
    "smv-c32-m1":     ("mfma c = 32; n = 15; m = 1: 31 of the 32 partial triples saw no key", 132, 15, 1, 32),
    "smv-c128-m15":   ("mfma c = 128; n = 16; m = 15", 133, 16, 15, 128),
    "smv-c256-m16":   ("mfma c = 256; n = 17; m = 16: one full tile", 134, 17, 16, 256),
    "smv-c32-m17":    ("mfma c = 32; n = 1; m = 17: a tile with a single key", 135, 1, 17, 32),
    "smv-c64-m127":   ("mfma c = 64; n = 15; m = 127: eight tiles, one per wave", 136, 15, 127, 64),
    "smv-c128-m128":  ("mfma c = 128; n = 16; m = 128", 137, 16, 128, 128),
    "smv-c256-m129":  ("mfma c = 256; n = 17; m = 129: wave 0 takes a second tile (prefetch) with a single key", 138, 17, 129, 256),
    "smv-common":     ("mfma c = 64; n = 5; m = 129: the case every entry point runs directly", 139, 5, 129, 64),
    "smv-samekeys":   ("identical key rows; mfma c = 64, n = 17, m = 129", 146, 17, 129, 64),
    "smv-t-c20":      ("transposed c = 20; n = 1; m + c = 3840, the limit", 140, 1, 3820, 20),
    "smv-t-c33":      ("transposed c = 33; n = 3; m + c = 3840", 141, 3, 3807, 33),
    "smv-t-c96":      ("transposed c = 96; n = 4: one full query block; m + c = 3840", 142, 4, 3744, 96),
    "smv-t-c20-n5":   ("transposed c = 20; n = 5: second block with one query; m + c = 3840", 143, 5, 3820, 20),
    "smv-1-3841":     ("first kernel: m + c = 3841 with c = 20, one past the transposed form's limit; n = 5", 144, 5, 3821, 20),
    "smv-1-15360":    ("first kernel: m + c = 15360, its own limit; n = 5", 145, 5, 15340, 20),
}
# (edge, seed, n, m, dim, heads, vdim)
_TRAIN = {
    "tr-d1-m255":      ("dim 1, 3 heads; m = 255", 151, 5, 255, 1, 3, None),
    "tr-d64-m256":     ("dim 64, 3 heads; m = 256: exactly one trip", 152, 9, 256, 64, 3, None),
    "tr-d300-m257":    ("dim 300 > 256: the head-vector load strides; m = 257", 153, 4, 257, 300, 3, None),
    "tr-d1024-m1":     ("dim 1024, the limit; m = 1: every probability is 1, dS = 0", 154, 3, 1, 1024, 3, None),
    "tr-d1024-m257":   ("dim 1024, 3 heads; m = 257", 155, 2, 257, 1024, 3, None),
    "tr-sal-m257":     ("the cross-saliency form: one head, vdim 1, c = 64; m = 257", 156, 6, 257, 64, 1, 1),
    "tr-samekeys":     ("identical key rows; dim 64, 3 heads, m = 257: P = 1 / m, dS = 0 up to rounding", 159, 5, 257, 64, 3, None),
    "tr-sweep-row":    ("k_mha_rowmat past one sweep: n = 16400, H dim = 256 (4 198 400 > 16384 x 256 threads), m = 3", 157,
                        16400, 3, 64, 4, None),
    "tr-sweep-col":    ("k_mha_colmat past one sweep: m = 16400, H dim = 256, n = 3", 158, 3, 16400, 64, 4, None),
}


def temperature(c):
    return float(F32(0.4 * np.sqrt(c)))


_same = lambda name: name.endswith("samekeys")
MHA = {name: build_softmax(name, s[0], *s[1:], family="mha", same_keys=_same(name)) for name, s in _MHA.items()}
HEADMAJOR = {name: build_softmax(name, s[0], s[1], s[2], s[3], 64, s[4], family="headmajor") for name, s in _HEADMAJOR.items()}
SMV = {name: build_softmax(name, s[0], s[1], s[2], s[3], s[4], 1, vdim=1, scale=1.0 / temperature(s[4]), family="smv",
                           same_keys=_same(name)) for name, s in _SMV.items()}
TRAIN = {name: build_softmax(name, s[0], s[1], s[2], s[3], s[4], s[5], vdim=s[6], family="train", same_keys=_same(name))
         for name, s in _TRAIN.items()}
ATTENTION = {**MHA, **HEADMAJOR}
SOFTMAX = {**MHA, **HEADMAJOR, **SMV, **TRAIN}


def mha_takes(c):
    """apr_mha's own conditions, restated"""
    return c["dim"] <= 256 and 256 % c["dim"] == 0 and c["m"] <= 1920 - c["dim"]


def expected_route(n, m, c, aligned=True):
    """the dispatch of kp_ops.softmax_matvec, restated"""
    if c in (32, 64, 128, 256) and aligned:
        return "mfma"
    return "transposed" if m + c <= 3840 else "first"


REFUSED = {
    "mha-dim48": dict(fn="mha", n=5, m=9, dim=48, H=1), "mha-dim512": dict(fn="mha", n=5, m=9, dim=512, H=1),
    "mha-m1857": dict(fn="mha", n=5, m=1921 - 64, dim=64, H=1),
    "hm-dim32": dict(fn="headmajor", n=5, m=9, dim=32, H=2), "hm-misaligned": dict(fn="headmajor", n=5, m=9, dim=64, H=1, off=1),
    "smv-mfma-c48": dict(fn="smv_mfma", n=5, m=9, c=48, T=0.5), "smv-bt-3841": dict(fn="smv_bt", n=5, m=3841 - 20, c=20, T=0.5),
    "smv-15361": dict(fn="smv", n=5, m=15361 - 20, c=20, T=0.5), "smv-T0": dict(fn="smv", n=5, m=9, c=20, T=0.0),
    "train-dim1025": dict(fn="train", n=2, m=3, dim=1025, H=1),
}


# ------------------------------------------------------------------------------------------------------ edge kernels
def edge_case(name, fact, seed, n, c, k):
    """f [n, c]; knn [n, k] with planted entries: row 0 lists row 0 (itself and the first row) first, row 1 lists n - 1, row 2
    lists itself, row 3 lists its first neighbour again last; de [n * k, 2 c]"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, c)).astype(F32)
    knn = rng.integers(0, n, (n, k)).astype(np.int32)
    plants = {}
    knn[0, 0] = 0
    plants[0] = "row0+self"
    if n > 1:
        knn[1, 0] = n - 1
        plants[1] = "lastrow"
    if n > 2:
        knn[2, k - 1] = 2
        plants[2] = "self"
    if n > 3 and k >= 2:
        knn[3, k - 1] = knn[3, 0]
        plants[3] = "repeat"
    de = rng.standard_normal((n * k, 2 * c)).astype(F32)
    return dict(name=name, fact=fact, n=n, c=c, k=k, f=f, knn=knn, de=de, plants=plants)


EDGE = {name: edge_case(name, s[0], 170 + i, *s[1:]) for i, (name, s) in enumerate({
    "e-c1-k1":     ("c = 1, k = 1", 7, 1, 1),
    "e-c3-k6":     ("c = 3, k = 6", 9, 3, 6),
    "e-c64-k15":   ("c = 64, k = 15; more than one block", 33, 64, 15),
    "e-c256-k6":   ("c = 256, k = 6", 5, 256, 6),
    "e-c3-k15":    ("c = 3, k = 15: 45 values per point, no multiple of anything", 12, 3, 15),
    "e-c256-k1":   ("c = 256, k = 1", 4, 256, 1),
    "e-sweep":     ("edge features past one sweep: n = 1100, k = 15, c = 256 (4 224 000 > 16384 x 256 threads)", 1100, 256, 15),
}.items())}
EDGE_BWD_SWEEP = dict(n=16400, c=256, k=2, seed=190)      # group max and edge-features backward past one sweep


def group_case(name, fact, seed, n, c, k, affine, slope, ldy_extra=0, ldo_extra=0):
    """y [n * k, c], scale / shift [c] or None.  Group 0: every activation input negative; group 1 (n >= 2): the maximum is
    the group's last row."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n * k, c)).astype(F32)
    scale = rng.uniform(0.5, 1.5, c).astype(F32) if affine else None
    shift = rng.standard_normal(c).astype(F32) if affine else None
    sc = np.ones(c) if scale is None else scale.astype(np.float64)
    sh = np.zeros(c) if shift is None else shift.astype(np.float64)
    y[:k] = ((-np.abs(rng.standard_normal((k, c))) - 0.25 - sh) / sc).astype(F32)
    if n >= 2:
        y[2 * k - 1] = ((6.0 + rng.random(c) - sh) / sc).astype(F32)
    return dict(name=name, fact=fact, n=n, c=c, k=k, y=y, scale=scale, shift=shift, slope=slope, ldy_extra=ldy_extra,
                ldo_extra=ldo_extra)


GROUP = {name: group_case(name, s[0], 200 + i, *s[1:]) for i, (name, s) in enumerate({
    "g-c1-k1":        ("c = 1, k = 1, affine, slope 0.2", 7, 1, 1, True, 0.2),
    "g-c3-k6":        ("c = 3, k = 6, affine, slope 0.2", 9, 3, 6, True, 0.2),
    "g-c64-k15":      ("c = 64, k = 15, affine", 33, 64, 15, True, 0.2),
    "g-c256-k6":      ("c = 256, k = 6, affine", 5, 256, 6, True, 0.2),
    "g-noaffine-s0":  ("scale / shift absent, slope 0: the all-negative group gives exactly 0", 9, 3, 6, False, 0.0),
    "g-noaffine-s02": ("scale / shift absent, slope 0.2", 9, 64, 15, False, 0.2),
    "g-affine-s0":    ("affine, slope 0", 12, 3, 15, True, 0.0),
    "g-slices":       ("ldy > c and ldo > c: column slices of wider NaN-filled buffers", 9, 64, 6, True, 0.2, 8, 5),
    "g-sweep":        ("past one sweep: n = 16400, c = 256, k = 2", 16400, 256, 2, True, 0.2),
}.items())}


# ------------------------------------------------------------------------------------------------------- score head
SCORE_SPECIALS = {0: float("nan"), 1: float("inf"), 2: float("-inf"), 3: -200.0, 4: 200.0, 5: 0.0, 6: -0.0, 7: 88.0, 8: -88.0,
                  9: -90.0, 10: -104.0, 11: 17.0}


def score_case(n, seed=220):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 6).astype(F32)
    for i, val in SCORE_SPECIALS.items():
        if i < n:
            x[i] = val
    return x

"""Inputs for the fused KPConv forward (apr_kpconv_fused), shared by tests/test_kpconv_fused_cpu.py (which confirms the
facts stated here from the oracle's intermediates) and tests/test_kpconv_fused_gpu.py.  numpy only.

EXACT cases: every float32 evaluation, in any order, split into bf16 pieces or not, gives the float64 result.
* queries and supports on the lattice 2 Z^3 inside {0, 2, 4}^3, the 15 kernel points distinct points of {-2, 0, 2}^3 with
  kp[0] = 0, extent 1: s - q - kp has even integer components, so the distance is 0 (influence exactly 1) or >= 2
  (1 - d <= -1 clamps to exactly 0 whatever the square root rounds to);
* integer features; in every row the neighbours with a positive feature sum are trimmed to a power of two (the surplus
  becomes padding), so 1 / num is a power of two;
* integer weights.  Ordinary values have at most 8 significant bits (one bf16 piece).  Planted (ns >= 8): feature 257 in
  channel 1 of support 2 against weight 257 (h and m pieces on both sides); feature 65793 = 2^16 + 2^8 + 1 in channel 2 of
  support 3 (three pieces) against weight 2; feature 129 in channel 3 of support 4 (the channel's only non-zero) against the
  16-bit weight 32769.  A planted support appears at most once per row.  A missing cross term, a permuted kernel-point
  order or a wrong channel map changes an integer.
BOUND cases: every aligned MFMA case of kpconv_cases.FORWARD and kpconv_cases.build cases at the edges of the query tile
(16 queries per workgroup, 4 per wave) and of the neighbour loop (groups of 16 neighbours, index trips of 64 lanes), with
cin 64 and 512; weights from kpconv_cases.weights.
"""
import functools

import numpy as np

import kpconv_cases as K
import kpconv_oracle as O

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
PAD_KINDS = (0, -1, -7, 5)       # ns + 0, -1, -7, ns + 5

# name: (seed, cin, cout, H, nq, ns)
_EXACT = {
    "x-c64-H1-nq1-ns1":     (1, 64, 64, 1, 1, 1),
    "x-c64-H5-nq33-ns1":    (2, 64, 64, 5, 33, 1),
    "x-c64-H4-nq15":        (3, 64, 64, 4, 15, 27),
    "x-c64-H5-nq16":        (4, 64, 64, 5, 16, 40),
    "x-c64-H128-nq17":      (5, 64, 64, 128, 17, 60),
    "x-c128-H64-nq63":      (6, 128, 128, 64, 63, 50),
    "x-c128-H65-nq64":      (7, 128, 128, 65, 64, 50),
    "x-c256-H5-nq65":       (8, 256, 256, 5, 65, 40),
    "x-c256-H4-nq127":      (9, 256, 256, 4, 127, 40),
    "x-c512-H5-nq129":      (10, 512, 512, 5, 129, 40),
    "x-c64-o512-H4-nq200":  (11, 64, 512, 4, 200, 40),
    "x-c512-o64-H65-nq17":  (12, 512, 64, 65, 17, 50),
    "x-c512-H128-nq16":     (13, 512, 512, 128, 16, 30),
}


def build_exact(seed, cin, cout, H, nq, ns):
    rng = np.random.default_rng(5000 + seed)
    s = (2 * rng.integers(0, 3, (ns, 3))).astype(F32)
    q = (2 * rng.integers(0, 3, (nq, 3))).astype(F32)
    cube = np.array([[a, b, c] for a in (-2, 0, 2) for b in (-2, 0, 2) for c in (-2, 0, 2) if (a, b, c) != (0, 0, 0)], F32)
    kp = np.concatenate([np.zeros((1, 3), F32), cube[rng.permutation(26)[:14]]], 0)
    x = rng.integers(-2, 4, (ns, cin)).astype(F32)
    x[rng.random(ns) < 0.3] *= -1                                                  # rows whose sum is <= 0
    W = rng.integers(-2, 3, (15, cin, cout)).astype(F32)
    planted = ns >= 8
    if planted:
        x[:, 3] = 0.0                                                              # the 16-bit weights meet one feature per row
        x[2, 1], x[3, 2], x[4, 3] = 257.0, 65793.0, 129.0
        W[:, 1, 0::3], W[:, 2, 1::3], W[:, 3, 2::3] = 257.0, 2.0, 32769.0
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)                        # ns = padding
    if planted:
        for row in range(nq):
            for r in (2, 3, 4):
                hit = np.flatnonzero(nbr[row] == r)
                nbr[row, hit[1:]] = rng.integers(5, ns, len(hit) - 1) if len(hit) > 1 else nbr[row, hit[1:]]
    nbr[0, 0], q[0], x[0] = 0, s[0], np.abs(x[0]) + 1                              # row 0 sits on support 0: never all zero
    if nq >= 3:
        nbr[1] = ns                                                                # a row of nothing but padding
        for h in range(min(H, 4)):
            v = PAD_KINDS[(h + seed) % 4]
            nbr[2, h] = v if v < 0 else ns + v
    pos = x.astype(np.float64).sum(1) > 0
    for row in range(nq):                                                          # num -> a power of two
        real = (nbr[row] >= 0) & (nbr[row] < ns)
        counted = np.flatnonzero(real & pos[np.where(real, nbr[row], 0)])
        keep = 1 << (len(counted).bit_length() - 1) if len(counted) else 0
        nbr[row, counted[keep:]] = PAD_KINDS[row % 4] + (ns if PAD_KINDS[row % 4] >= 0 else 0)
    return dict(cin=cin, cout=cout, H=H, nq=nq, ns=ns, q=q, s=s, kp=kp, x=x, nbr=nbr, extent=1.0, W=W, layout="aligned")


@functools.lru_cache(maxsize=None)
def exact(name):
    return build_exact(*_EXACT[name])


EXACT = list(_EXACT)

# ----------------------------------------------------------------------------------------------------------- bound cases
_COUTS = (64, 128, 256, 512, 192, 320, 384, 448)
_MFMA = [n for n, c in K.FORWARD.items() if c["layout"] == "aligned" and c["cin"] % 64 == 0 and c["H"] <= 128]
# (cin, H, nq, ns, cout): the edges of the 16-query tile and of the neighbour groups / 64-lane index trips
_EDGES = [(64, 1, 1, 7, 64), (64, 4, 15, 30, 128), (64, 5, 16, 30, 64), (64, 64, 17, 90, 512), (64, 65, 63, 90, 64),
          (64, 128, 64, 150, 64), (64, 5, 65, 40, 256), (64, 4, 127, 40, 64), (64, 5, 129, 40, 64), (64, 4, 200, 40, 192),
          (512, 1, 17, 7, 64), (512, 4, 63, 30, 64), (512, 5, 64, 30, 128), (512, 64, 16, 90, 64), (512, 65, 15, 90, 512),
          (512, 128, 1, 150, 64), (512, 5, 65, 40, 64), (512, 4, 127, 40, 64), (512, 4, 129, 40, 256), (512, 5, 200, 40, 64)]
_BOUND = {n: (n, _COUTS[i % len(_COUTS)]) for i, n in enumerate(_MFMA)}
for _i, (_cin, _H, _nq, _ns, _cout) in enumerate(_EDGES):
    _BOUND[f"e-c{_cin}-H{_H}-nq{_nq}-o{_cout}"] = ((200 + _i, _cin, _H, _nq, _ns), _cout)
BOUND = list(_BOUND)


@functools.lru_cache(maxsize=None)
def bound_case(name):
    """-> the kpconv_cases dict plus W [15, cin, cout] and cout"""
    spec, cout = _BOUND[name]
    c = dict(K.FORWARD[spec]) if isinstance(spec, str) else K.build(name, "tile / neighbour-loop edge", *spec)
    c["W"], _ = K.weights(c, cout)
    c["cout"] = cout
    return c


def args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (out float64 [nq, cout], wf float64 [nq, 15 cin], num [nq], w [nq, 15, H]) of an exact or bound case"""
    c = exact(name) if name in _EXACT else bound_case(name)
    wf, num, w = O.weighted(*args(c))
    W2 = np.asarray(c["W"], np.float64).reshape(-1, c["cout"])
    return wf @ W2, wf, num, w


@functools.lru_cache(maxsize=None)
def element_bound(name):
    """|out - ref| <= bound_weighted @ |W| + 16 eps32 (|wf| @ |W|): the derived fp32 bound of the correlation carried through
    exact weights, plus the split contraction (8.03 of the 16 derived from the three dropped cross terms, the rest given to
    the fp32 accumulation of 15 cin terms inside the MFMA, whose internal rounding is not documented)."""
    c = bound_case(name)
    _, wf, _, _ = reference(name)
    aW = np.abs(np.asarray(c["W"], np.float64)).reshape(-1, c["cout"])
    return O.bound_weighted(*args(c)) @ aW + 16.0 * EPS32 * (np.abs(wf) @ aW)


def rows_rel_l2(got, ref):
    """the statistic of test_kpconv_function_end_to_end: per row |got - ref|_2 / max(|ref|_2, median row norm), no row
    excluded; rows that are exactly 0 in the reference must be exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    norms = np.linalg.norm(ref, axis=1)
    zero = norms == 0
    assert not got[zero].any(), "a row that is exactly 0 in the reference is not exactly 0"
    floor = np.median(norms)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(norms, floor if floor > 0 else 1.0)).max())


# ------------------------------------------------------------------------------------- the bf16 3-way split, restated
def _top8_trunc(x):
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3_trunc(x):
    """apr_split3 (csrc/bf3.h): x = h + m + l exactly, each piece the top 16 bits of what is left"""
    x = np.ascontiguousarray(x, np.float32)
    h = _top8_trunc(x)
    r = (x - h).astype(np.float32)
    m = _top8_trunc(r)
    t = (r - m).astype(np.float32)
    return h, m, _top8_trunc(t)


def _bf16_rn(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3_rn(w):
    """k_pack_weights_bf3 (csrc/spconv_ws.hip): the weight image's pieces, rounded to nearest"""
    w = np.ascontiguousarray(w, np.float32)
    h = _bf16_rn(w)
    r = (w - h).astype(np.float32)
    m = _bf16_rn(r)
    return h, m, _bf16_rn((r - m).astype(np.float32))

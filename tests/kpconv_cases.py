"""Named inputs for the KPConv kernels, the reverse table and the pools, each with the fact it exists for
(tests/test_kpconv_oracle_cpu.py confirms every fact from the oracle's own intermediates, so a case that stops reaching
its edge fails on the host and not on the GPU).  numpy only; everything is built from small integer seeds.

Kernel constants the cases are built around (apr_amd/csrc/kpconv.hip, revtable.hip):
* step 1 takes the MFMA kernel iff cin % 64 == 0, H <= 128, ldx % 4 == 0, ldwf % 4 == 0 and x / wf are 16-byte aligned:
  mfma<4> for cin >= 256 (passes of 4 groups of 64 channels: 320 = 4 + 1, 384 = 4 + 2), mfma<2> for cin == 128, mfma<1>
  otherwise (192 = three passes); every other input runs the generic kernel (8-channel chunks).  One wave per query, 4 per
  block, so ceil(nq / 4) blocks, re-ordered over the 8 XCDs; the index stage fills 128 LDS slots in two trips of 64 lanes,
  the MFMA walks (H + 3) >> 2 steps of 4 neighbours.
* the feature gradient keeps CPL = 1 / 2 / 4 / 8 channels per lane for cin <= 64 / 128 / 256 / 512 and refuses cin > 512
  and H > 128; KPConvFunction sums contribution rows over the reverse table when cin % 4 == 0, float atomics otherwise.
* the reverse table sorts keys of key_bits(ns) bits (a new bit at every power of two) with 256-thread key / start kernels.
* the pools walk H in steps of 8; apr_gather_pool has a 16-byte route (c % 4 == 0, aligned rows) and a scalar one.

Geometry: points in [-1, 1]^3, kernel points in [-1, 1]^3 with kp[0] = 0, extent 1.2.  Support ns - 1 is `far` (at
(9, 9, 9): beyond every kernel point of every query, positive features), support 0 has features that sum to exactly 0 in
any order (small integers; all zero for cin = 1), support 1 sums to a negative number (when ns >= 4).  Every feature row
is either such an exact zero or has |sum| >= 1e-3 * sum |x|: a float32 row sum in any order (error <= cin * 2^-24 *
sum |x| <= 3.1e-5 * sum |x|) then decides `> 0` as float64 does.  The module asserts this at import.

The first rows of every neighbour table are planted (PLANTS, rotated by the seed when nq < 7):
  allpad     every entry is padding (ns)
  padkinds   padding written as ns, -1, -7 and ns + 5 in the first slots
  dup        one near, positive support fills the whole row
  floor      only supports 1 (negative sum) and 0 (zero sum), both inside the extent: they contribute, nobody counts
  far        a near positive support, the far one and (H >= 3) the zero-sum one: num = 2, one of the counted contributes
  self       the query sits on its first neighbour: w = 1 at kp[0]; (H >= 3) the last slot lists that support again
  lastonly   padding everywhere but h = H - 1
"""
import numpy as np

F32 = np.float32
EXTENT = 1.2
PLANTS = ("allpad", "padkinds", "dup", "floor", "far", "self", "lastonly")
PAD_KINDS = (0, -1, -7, 5)      # ns + 0, -1, -7, ns + 5


def _features(rng, ns, cin, special):
    x = rng.standard_normal((ns, cin)).astype(F32)
    sign = np.where(rng.random(ns) < 0.25, -1.0, 1.0)
    if special:
        sign[1], sign[ns - 1] = -1.0, 1.0
    else:
        sign[:] = 1.0
    x = (x + 0.5 * sign[:, None]).astype(F32)
    for r in range(ns):
        tot, mag = float(x[r].astype(np.float64).sum()), float(np.abs(x[r]).astype(np.float64).sum())
        if tot * sign[r] < 0.05 * mag:
            x[r] = np.abs(x[r]) * F32(sign[r])
    if special:
        z = np.zeros(cin, F32)
        if cin >= 2:
            z[:cin - 1] = rng.integers(-4, 5, cin - 1)
            z[0] = 3.0 if z[0] == 0 else z[0]
            z[cin - 1] = -z[:cin - 1].sum()
        x[0] = z
    return x


def build(name, fact, seed, cin, H, nq, ns, layout="aligned"):
    rng = np.random.default_rng(seed)
    special = ns >= 4
    s = rng.uniform(-1, 1, (ns, 3)).astype(F32)
    q = rng.uniform(-1, 1, (nq, 3)).astype(F32)
    if special:
        s[ns - 1] = 9.0
    kp = rng.uniform(-1, 1, (15, 3)).astype(F32)
    kp[0] = 0.0
    x = _features(rng, ns, cin, special)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)                    # ns = padding
    positive = [r for r in range(ns) if x[r].astype(np.float64).sum() > 0 and not (special and r == ns - 1)]
    plants = {}
    for row in range(min(nq, len(PLANTS))):
        kind = PLANTS[(row + (seed if nq < len(PLANTS) else 0)) % len(PLANTS)]
        if kind in ("floor", "far") and not special:
            continue
        if kind == "far" and H < 2:
            continue
        near = positive[int(rng.integers(len(positive)))]
        off = np.array([0.25, -0.125, 0.0625], F32) * F32(1 + row % 3)
        if kind == "allpad":
            nbr[row] = ns
        elif kind == "padkinds":
            for h in range(min(H, 4)):
                v = PAD_KINDS[(h + seed) % 4]
                nbr[row, h] = v if v < 0 else ns + v
        elif kind == "dup":
            nbr[row] = near
            q[row] = s[near] + off
        elif kind == "floor":
            nbr[row] = ns
            nbr[row, 0] = 1
            if H > 1:
                nbr[row, H - 1] = 0
            q[row] = (s[1] + off if H == 1 else (s[0].astype(np.float64) + s[1]) / 2).astype(F32)
            if H > 1 and np.linalg.norm(s[0].astype(np.float64) - s[1]) > 1.6:
                s[0] = s[1] + np.array([0.5, 0.25, -0.5], F32)
                q[row] = s[1] + np.array([0.25, 0.125, -0.25], F32)
        elif kind == "far":
            nbr[row] = ns
            nbr[row, 0] = ns - 1
            nbr[row, H - 1] = near
            if H >= 3:
                nbr[row, 1] = 0                 # the zero-sum support: listed, not counted
            q[row] = s[near] + off
        elif kind == "self":
            nbr[row, 0] = near
            if H >= 3:
                nbr[row, H - 1] = near          # the same support listed twice among others
            q[row] = s[near]
        elif kind == "lastonly":
            nbr[row] = ns
            nbr[row, H - 1] = near
            q[row] = s[near] + off
        plants[row] = kind
    dwf = rng.standard_normal((nq, 15 * cin)).astype(F32)
    return dict(name=name, fact=fact, seed=seed, cin=cin, H=H, nq=nq, ns=ns, layout=layout, q=q, s=s, kp=kp, x=x, nbr=nbr,
                dwf=dwf, extent=EXTENT, plants=plants)


def expected_route(cin, H, layout):
    """the dispatch of apr_kpconv_weighted, restated (ldwf and wf are aligned in every case)"""
    if cin % 64 or H > 128 or layout != "aligned":
        return "generic"
    return "mfma4" if cin >= 256 else "mfma2" if cin == 128 else "mfma1"


def expected_cpl(cin):
    return 1 if cin <= 64 else 2 if cin <= 128 else 4 if cin <= 256 else 8


def blocks(nq):
    return (nq + 3) // 4


# name: (fact, seed, cin, H, nq, ns[, layout]);  route / grid / H facts are checked from these numbers, planted rows from
# the oracle's intermediates
_FORWARD = {
    # ---- generic kernel
    "g-c1":        ("cin = 1 (the first layer): generic kernel, one chunk of one channel", 1, 1, 5, 29, 40),
    "g-c3-ns1":    ("cin = 3, a single support point (ns = 1), H = 1", 2, 3, 1, 5, 1),
    "g-c8-H65":    ("cin = 8: exactly one 8-channel chunk; nq > ns; H = 65", 3, 8, 65, 33, 20),
    "g-c9-H129":   ("cin = 9: a chunk and a 1-channel tail; H = 129", 4, 9, 129, 4, 150),
    "g-c63":       ("cin = 63: the widest input below the MFMA width", 5, 63, 4, 61, 70),
    "g-c64-H129":  ("cin = 64 but H = 129 > the LDS table: generic kernel", 6, 64, 129, 3, 30),
    "g-c64-H130":  ("cin = 64, H = 130: generic kernel", 7, 64, 130, 5, 140),
    "g-c64-slice": ("the values of m1-c64 through a column slice big[:, 1:65]: misaligned, generic kernel", 8, 64, 5, 29, 40,
                    "slice1"),
    "g-c64-ldodd": ("the values of m1-c64 with ldx = 65 (ldx % 4 != 0): generic kernel", 8, 64, 5, 29, 40, "ldodd"),
    # ---- mfma<1>
    "m1-c64":      ("cin = 64 aligned: mfma<1>, 8 blocks (nb & 7 = 0)", 8, 64, 5, 29, 40),
    "m1-H1-nq1":   ("H = 1, one query, one block: a single MFMA step with three empty k-slots", 9, 64, 1, 1, 7),
    "m1-H2-nq3":   ("H = 2, 3 queries in one block (a wave without a query)", 10, 64, 2, 3, 9),
    "m1-H3-nq4":   ("H = 3, a full block", 11, 64, 3, 4, 12),
    "m1-H4-nq5":   ("H = 4: exactly one step; 2 blocks (nb < 8)", 12, 64, 4, 5, 11),
    "m1-H63-nq33": ("H = 63: last lane of the first index trip idle; 9 blocks (nb & 7 = 1)", 13, 64, 63, 33, 90),
    "m1-H64-nq61": ("H = 64: one full index trip, 16 steps; 16 blocks (nb & 7 = 0)", 14, 64, 64, 61, 80),
    "m1-H65-nq67": ("H = 65: second index trip with one lane, tail step of one; 17 blocks (nb & 7 = 1); nq = 67", 15, 64, 65,
                    67, 100),
    "m1-H127":     ("H = 127: tail step of three", 16, 64, 127, 29, 150),
    "m1-H128":     ("H = 128: the LDS table's last slot", 17, 64, 128, 33, 160),
    "m1-ns1":      ("ns = 1 on the MFMA route", 18, 64, 5, 9, 1),
    "m1-c192":     ("cin = 192: mfma<1>, three passes", 19, 192, 5, 29, 40),
    "m1-c192-H65": ("cin = 192, H = 65", 20, 192, 65, 5, 70),
    # ---- mfma<2>
    "m2-c128":     ("cin = 128: mfma<2>", 21, 128, 5, 29, 40),
    "m2-H1":       ("mfma<2>, H = 1, one query", 22, 128, 1, 1, 6),
    "m2-H3":       ("mfma<2>, H = 3", 23, 128, 3, 4, 30),
    "m2-H65":      ("mfma<2>, H = 65, 9 blocks", 24, 128, 65, 33, 80),
    "m2-H128":     ("mfma<2>, H = 128", 25, 128, 128, 5, 140),
    # ---- mfma<4>
    "m4-c256":     ("cin = 256: mfma<4>, one full pass", 26, 256, 5, 29, 40),
    "m4-c256-H128": ("mfma<4>, H = 128", 27, 256, 128, 4, 140),
    "m4-c320":     ("cin = 320 = 4 + 1 groups: the second pass holds one live group; 9 blocks", 28, 320, 5, 33, 40),
    "m4-c320-H65": ("cin = 320, H = 65", 29, 320, 65, 5, 70),
    "m4-c384":     ("cin = 384 = 4 + 2 groups", 30, 384, 3, 29, 40),
    "m4-c384-H127": ("cin = 384, H = 127", 31, 384, 127, 3, 130),
    "m4-c512":     ("cin = 512: two full passes; nq = 67 (17 blocks), ns = 200: the largest case", 32, 512, 4, 67, 200),
    "m4-c512-H64": ("cin = 512, H = 64, one query", 33, 512, 64, 1, 70),
    "m4-c512-H2":  ("cin = 512, H = 2, 61 queries (16 blocks), nq > ns", 34, 512, 2, 61, 30),
}

_BACKWARD = {
    # ---- atomic path (cin % 4 != 0)
    "b-c1":        ("cin = 1: atomic path, CPL 1, 63 idle lanes", 41, 1, 5, 29, 40),
    "b-c3-H65":    ("cin = 3: atomic path; ns = 200 > nq * H-ish: supports nobody points at", 42, 3, 65, 5, 200),
    "b-c130":      ("cin = 130: atomic path, CPL 4 with a 2-channel tail", 43, 130, 4, 33, 20),
    # ---- contribution path
    "b-c4-H1":     ("cin = 4, H = 1, one query", 44, 4, 1, 1, 7),
    "b-c4-ns1":    ("cin = 4, ns = 1", 45, 4, 5, 9, 1),
    "b-c60-H2":    ("cin = 60: CPL 1 with 4 idle lanes; H = 2", 46, 60, 2, 3, 9),
    "b-c60-H65":   ("cin = 60, H = 65 (second trip of the index loop), supports nobody points at", 47, 60, 65, 5, 200),
    "b-c64-H3":    ("cin = 64: CPL 1 full; H = 3", 48, 64, 3, 4, 12),
    "b-c64-H63":   ("cin = 64, H = 63, 9 blocks", 49, 64, 63, 33, 90),
    "b-c64-H64":   ("cin = 64, H = 64, 16 blocks", 50, 64, 64, 61, 80),
    "b-c64-H65":   ("cin = 64, H = 65, 17 blocks", 51, 64, 65, 67, 100),
    "b-c64-H127":  ("cin = 64, H = 127", 52, 64, 127, 5, 150),
    "b-c64-H128":  ("cin = 64, H = 128: the last LDS slot", 53, 64, 128, 29, 160),
    "b-c68":       ("cin = 68: CPL 2 with a 4-channel second register", 54, 68, 5, 29, 40),
    "b-c128-H4":   ("cin = 128: CPL 2 full; H = 4", 55, 128, 4, 5, 11),
    "b-c128-H65":  ("cin = 128, H = 65", 56, 128, 65, 9, 80),
    "b-c132":      ("cin = 132: CPL 4 with a 4-channel third register", 57, 132, 5, 33, 40),
    "b-c132-H128": ("cin = 132, H = 128", 58, 132, 128, 3, 140),
    "b-c256":      ("cin = 256: CPL 4 full", 59, 256, 5, 29, 40),
    "b-c256-H64":  ("cin = 256, H = 64", 60, 256, 64, 4, 70),
    "b-c260-H3":   ("cin = 260: CPL 8 with a 4-channel fifth register; 16 blocks", 61, 260, 3, 61, 40),
    "b-c260-H127": ("cin = 260, H = 127", 62, 260, 127, 4, 130),
    "b-c512":      ("cin = 512: CPL 8 full; nq = 67, ns = 200", 63, 512, 5, 67, 200),
    "b-c512-H128": ("cin = 512, H = 128", 64, 512, 128, 3, 140),
    "b-c192":      ("cin = 192 (the end-to-end width): CPL 4, one register idle", 65, 192, 5, 29, 40),
}


def _make(table):
    out = {}
    for name, spec in table.items():
        fact, seed, cin, H, nq, ns = spec[:6]
        out[name] = build(name, fact, seed, cin, H, nq, ns, spec[6] if len(spec) > 6 else "aligned")
    return out


FORWARD = _make(_FORWARD)
BACKWARD = _make(_BACKWARD)
ALL = {**FORWARD, **BACKWARD}
REFUSED = {"cin513": dict(cin=513, H=5, n_kp=15), "H129": dict(cin=64, H=129, n_kp=15), "nkp14": dict(cin=64, H=5, n_kp=14)}

# KPConvFunction end to end: case -> cout
END_TO_END = [("g-c1", 128), ("b-c3-H65", 34), ("m1-c64", 34), ("b-c68", 129), ("m1-c192", 64), ("m4-c320", 64),
              ("m4-c384", 128), ("m4-c512", 64)]


def weights(case, cout):
    rng = np.random.default_rng(1000 + case["seed"])
    cin = case["cin"]
    W = (rng.standard_normal((15, cin, cout)) / np.sqrt(15 * cin)).astype(F32)
    d_out = rng.standard_normal((case["nq"], cout)).astype(F32)
    return W, d_out


def features_are_decision_safe(x):
    x64 = x.astype(np.float64)
    tot, mag = x64.sum(1), np.abs(x64).sum(1)
    exact_zero = np.array([_sums_to_zero_in_any_order(r) for r in x64])
    return bool(np.all(exact_zero | (np.abs(tot) >= 1e-3 * mag))) and bool(np.all(exact_zero == (tot == 0)))


def _sums_to_zero_in_any_order(row):
    """small integers (every partial sum is an integer below 2^24: exact in float32) that cancel"""
    return bool(np.all(row == np.round(row)) and np.abs(row).sum() < 2 ** 20 and row.sum() == 0)


for _c in ALL.values():
    assert features_are_decision_safe(_c["x"]), _c["name"]
assert np.array_equal(FORWARD["g-c64-slice"]["x"], FORWARD["m1-c64"]["x"])
assert np.array_equal(FORWARD["g-c64-ldodd"]["nbr"], FORWARD["m1-c64"]["nbr"])


# ---------------------------------------------------------------------------------------------------- reverse table
def rev_case(ns, nq, H, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "allpad":
        nbr = np.full((nq, H), ns, np.int32)
    elif kind == "nopad":
        nbr = rng.integers(0, ns, (nq, H)).astype(np.int32)
    else:
        nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)
        if kind == "negatives":
            nbr[rng.random((nq, H)) < 0.3] = -1
            nbr.reshape(-1)[::7] = -7
            nbr.reshape(-1)[3::11] = ns + 5
    return dict(ns=ns, nq=nq, H=H, kind=kind, nbr=nbr)


# name: (ns, nq, H, kind): key_bits changes at ns = 1 | 2, 255 | 256; the key kernel's 256-thread tail at nq * H = 255 /
# 256 / 257, the start kernel's at ns + 1 = 256 / 257 / 258
REVERSE = {name: rev_case(*spec, seed=70 + i) for i, (name, spec) in enumerate({
    "ns1-t1": (1, 1, 1, "nopad"),
    "ns1-t257": (1, 257, 1, "mixed"),
    "ns2-t255": (2, 255, 1, "mixed"),
    "ns2-t256-nopad": (2, 16, 16, "nopad"),
    "ns255-t255": (255, 51, 5, "mixed"),
    "ns255-t255-allpad": (255, 85, 3, "allpad"),
    "ns256-t256": (256, 256, 1, "mixed"),
    "ns256-t256-nopad": (256, 64, 4, "nopad"),
    "ns257-t257": (257, 257, 1, "mixed"),
    "ns257-t257-negatives": (257, 1, 257, "negatives"),
    "ns256-t1": (256, 1, 1, "mixed"),
    "ns255-t256-negatives": (255, 32, 8, "negatives"),
}.items())}


# ------------------------------------------------------------------------------------------------------------ pools
def pool_case(c, H, nq, ns, layout, seed):
    """Features and gradients are multiples of 1/8 below 2^8: every sum is exact in float32, so the GPU must give the
    oracle's bits.  Planted rows (when they fit): 0: supports a != b with equal rows, the maximum of every column, at
    h = 0 and 3; 1: the same at h = 7 and 8; 2: neighbours whose column 0 is negative, and a shadow entry (maximum 0 at the
    shadow, gradient to nobody); 3: all shadow."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-40, 41, (ns, c)) / 8.0).astype(F32)
    inds = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)
    dout = (rng.integers(-16, 17, (nq, c)) / 4.0).astype(F32)
    plants = {}
    if ns >= 4:
        a, b = 1, ns - 2
        x[a] = x[b] = (50 + np.arange(c)).astype(F32)
        others = np.array([r for r in range(ns) if r not in (a, b)])
        inds[inds == a] = others[0]
        inds[inds == b] = others[-1]
        if H >= 4 and nq > 0:
            inds[0, 0], inds[0, 3] = a, b
            plants[0] = ("tie", 0, 3)
        if H >= 9 and nq > 1:
            inds[1, 7], inds[1, 8] = a, b
            plants[1] = ("tie", 7, 8)
        if H >= 2 and nq > 2:
            neg = others[:3]
            x[neg, 0] = -np.abs(x[neg, 0]) - F32(0.125)
            inds[2] = neg[np.arange(H) % 3]
            inds[2, H // 2] = ns
            plants[2] = ("shadowmax", H // 2)
        if nq > 3:
            inds[3] = ns
            plants[3] = ("allshadow",)
    return dict(c=c, H=H, nq=nq, ns=ns, layout=layout, x=x, inds=inds, dout=dout, plants=plants)


POOLS = {name: pool_case(*spec, seed=90 + i) for i, (name, spec) in enumerate({
    "c1-H1": (1, 1, 5, 6, "aligned"),
    "c3-H7": (3, 7, 9, 20, "aligned"),
    "c4-H8": (4, 8, 33, 50, "aligned"),
    "c5-H9": (5, 9, 9, 30, "aligned"),
    "c8-H255": (8, 255, 5, 300, "aligned"),
    "c4-H9-slice": (4, 9, 17, 40, "slice1"),
    "c8-H4": (8, 4, 7, 10, "aligned"),
    "c4-H255": (4, 255, 4, 100, "aligned"),
}.items())}

"""Named inputs for the deformable KPConv kernels (apr_amd/csrc/kpconv_deform.hip), each with the fact it exists for.
numpy only; everything is built from small integer seeds.

Geometry as tests/kpconv_cases.py: points in [-1, 1]^3, rigid kernel points kp in [-1, 1]^3 with kp[0] = 0, extent 1.2,
support ns - 1 `far` at (9, 9, 9) with positive features, support 0 summing to exactly 0, support 1 to a negative number
(ns >= 4).  dkp = kp + extent * offsets with offsets uniform in [-0.3, 0.3]; mod uniform in [0.2, 1.8].

Planted rows (PLANTS; rotated by the seed when nq is smaller than their number; the ones that need ns >= 4 or H >= 2 are left
out otherwise):
  allpad       every entry is padding: min_d2 from the padding point, output 0, num at its floor
  padkinds     padding written as ns, -1 and ns + 5 in the first slots
  deform_only  the far support, reached by a deformed kernel point (k = 3 moved next to it) and by no rigid one
  rigid_only   the far support (all 15 deformed points around it) and a positive support next to the query: inside the rigid
               ball of kp[0], outside every deformed one: it must not count (num = 1; the rigid rule says 2)
  none         real, positive neighbours next to the query, every deformed point moved away: nothing in range, output 0
  floor        the negative-sum and the zero-sum support, each with a deformed point next to it: they contribute, nobody
               counts
  dup          one near, positive support fills the row
  mod02        mod = 0 on kernel point 2 and 2 on kernel point 5
  mod0_only    the far support in range of kernel point 2 ALONE, whose mod is 0, and a positive support near the query
               with the other 14 points around it: both count (num = 2)
  zero_off     zero offsets (dkp = kp) and mod = 1

Every case asserts at import, in float64: |d / extent - 1| >= 1e-3 for every real (q, h, k) -- so the in-range and clamp
decisions are the same in float32, which sees up to 1 + 2^-20 --, d >= 0.05 extent for every in-ball triple, and the
row-sum margin of tests/kpconv_cases.py (a feature row sums to an exact 0 or |sum| >= 1e-3 sum |x|).
"""
import numpy as np

import kpconv_cases as KC
import kpconv_deform_oracle as DO

F32 = np.float32
EXTENT = KC.EXTENT
PLANTS = ("allpad", "padkinds", "deform_only", "rigid_only", "none", "floor", "dup", "mod02", "mod0_only", "zero_off")
NEAR = np.array([0.25, -0.125, 0.0625], F32)


def _cluster(rng, centre, n):
    """n points around `centre`, 0.1 .. 0.5 away from it"""
    v = rng.standard_normal((n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.1, 0.5, (n, 1))
    return (np.asarray(centre, np.float64) + v).astype(F32)


def _repair(rng, q, s, nbr, dkp, fixed):
    """move the deformed points of the triples that sit next to the edge of a ball or next to a kernel point"""
    for _ in range(200):
        g = DO.geometry(q, s, nbr, dkp, EXTENT)
        r = g["d"] / EXTENT
        bad = g["real"][:, :, None] & ((np.abs(r - 1.0) < 2e-3) | (r < 0.06))
        rows, ks = np.nonzero(bad.any(1))
        if len(rows) == 0:
            return dkp
        for row, k in zip(rows, ks):
            assert (row, k) not in fixed, (row, k)
            dkp[row, k] += rng.uniform(-0.05, 0.05, 3).astype(F32)
    raise AssertionError("no margin")


def build(name, fact, seed, cin, H, nq, ns):
    rng = np.random.default_rng(seed)
    special = ns >= 4
    s = rng.uniform(-1, 1, (ns, 3)).astype(F32)
    q = rng.uniform(-1, 1, (nq, 3)).astype(F32)
    if special:
        s[ns - 1] = 9.0
    kp = rng.uniform(-1, 1, (15, 3)).astype(F32)
    kp[0] = 0.0
    x = KC._features(rng, ns, cin, special)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)
    dkp = (kp[None] + F32(EXTENT) * rng.uniform(-0.3, 0.3, (nq, 15, 3)).astype(F32)).astype(F32)
    mod = rng.uniform(0.2, 1.8, (nq, 15)).astype(F32)
    positive = [r for r in range(ns) if x[r].astype(np.float64).sum() > 0 and not (special and r == ns - 1)]
    plants, fixed = {}, set()
    far = ns - 1
    for row in range(min(nq, len(PLANTS))):
        kind = PLANTS[(row + (seed if nq < len(PLANTS) else 0)) % len(PLANTS)]
        if kind in ("deform_only", "rigid_only", "floor", "mod0_only") and not special:
            continue
        if kind in ("rigid_only", "mod0_only", "floor") and H < 2:
            continue
        if not positive and kind in ("rigid_only", "none", "dup", "mod0_only"):
            continue
        near = positive[int(rng.integers(len(positive)))] if positive else 0
        if kind == "allpad":
            nbr[row] = ns
        elif kind == "padkinds":
            for h, v in enumerate((ns, -1, ns + 5)[:H]):
                nbr[row, h] = v
        elif kind == "deform_only":
            nbr[row] = ns
            nbr[row, H - 1] = far
            dkp[row, 3] = (s[far].astype(np.float64) - q[row] + np.array([0.3, 0.2, 0.1])).astype(F32)
        elif kind == "rigid_only":
            nbr[row] = ns
            nbr[row, 0], nbr[row, H - 1] = far, near
            q[row] = s[near] + NEAR
            dkp[row] = _cluster(rng, s[far].astype(np.float64) - q[row], 15)
        elif kind == "none":
            nbr[row] = near
            q[row] = s[near] + NEAR
            dkp[row] = (kp + F32(30.0)).astype(F32)
        elif kind == "floor":
            nbr[row] = ns
            nbr[row, 0], nbr[row, H - 1] = 1, 0
            q[row] = s[1] + NEAR
            dkp[row, 0] = (s[1].astype(np.float64) - q[row] + np.array([0.1, 0.1, 0.1])).astype(F32)
            dkp[row, 1] = (s[0].astype(np.float64) - q[row] + np.array([-0.1, 0.2, 0.1])).astype(F32)
        elif kind == "dup":
            nbr[row] = near
            q[row] = s[near] + NEAR
        elif kind == "mod02":
            mod[row, 2], mod[row, 5] = 0.0, 2.0
        elif kind == "mod0_only":
            nbr[row] = ns
            nbr[row, 0], nbr[row, H - 1] = far, near
            q[row] = s[near] + NEAR
            dkp[row] = _cluster(rng, s[near].astype(np.float64) - q[row], 15)
            dkp[row, 2] = (s[far].astype(np.float64) - q[row] + np.array([0.3, 0.2, 0.1])).astype(F32)
            mod[row, 2] = 0.0
        elif kind == "zero_off":
            dkp[row] = kp
            mod[row] = 1.0
        plants[row] = kind
        if kind in ("zero_off", "none"):
            fixed.update((row, k) for k in range(15))
    # zero_off keeps dkp = kp: move the QUERY instead when one of its triples sits next to an edge
    for row, kind in plants.items():
        if kind == "zero_off":
            for _ in range(200):
                g = DO.geometry(q[row:row + 1], s, nbr[row:row + 1], dkp[row:row + 1], EXTENT)
                r = g["d"] / EXTENT
                if not (g["real"][:, :, None] & ((np.abs(r - 1.0) < 2e-3) | (r < 0.06))).any():
                    break
                q[row] = rng.uniform(-1, 1, 3).astype(F32)
    dkp = _repair(rng, q, s, nbr, dkp, fixed)
    dwf = rng.standard_normal((nq, 15 * cin)).astype(F32)
    return dict(name=name, fact=fact, seed=seed, cin=cin, H=H, nq=nq, ns=ns, q=q, s=s, kp=kp, x=x, nbr=nbr, dkp=dkp, mod=mod,
                dwf=dwf, extent=EXTENT, plants=plants)


# name: (fact, seed, cin, H, nq, ns)
_CASES = {
    "d-c64-H5":        ("cin = 64 (one group, CPL 1): every planted row; 9 blocks (nb & 7 = 1)", 101, 64, 5, 33, 40),
    "d-c64-H1-nq1":    ("H = 1, one query: a single step with three empty k-slots, one tile with one row", 102, 64, 1, 1, 7),
    "d-c64-H3-nq4":    ("H = 3, one full block", 103, 64, 3, 4, 12),
    "d-c64-H4-nq5":    ("H = 4: exactly one step; 2 blocks, a block with one wave at work", 104, 64, 4, 5, 11),
    "d-c64-H63":       ("H = 63: the last lane of the index trip idle, a tile of 15 rows", 105, 64, 63, 33, 90),
    "d-c64-H64":       ("H = 64: one full index trip, 16 steps, 4 full tiles", 106, 64, 64, 5, 80),
    "d-c64-H65-nq67":  ("H = 65: a second index trip, a fifth tile of one row; 17 blocks", 107, 64, 65, 67, 100),
    "d-c128-H127":     ("cin = 128 (two groups, CPL 2), H = 127: tail step of three", 108, 128, 127, 5, 150),
    "d-c128-H128":     ("cin = 128, H = 128: the last LDS slot, 8 full tiles", 109, 128, 128, 33, 160),
    "d-c256-H5":       ("cin = 256: one pass of 4 groups, CPL 4, 4 chunks", 110, 256, 5, 33, 40),
    "d-c320-H65":      ("cin = 320 = 4 + 1 groups: a pass with one live group; CPL 8 with three idle registers", 111, 320, 65, 5,
                        70),
    "d-c512-H4-nq67":  ("cin = 512: two full passes, CPL 8, 8 chunks; nq = 67, ns = 200: the largest case", 112, 512, 4, 67, 200),
    "d-c64-ns1":       ("a single support point (ns = 1)", 113, 64, 5, 5, 1),
}

CASES = {name: build(name, *spec) for name, spec in _CASES.items()}
REFUSED = {"cin32": dict(cin=32), "cin96": dict(cin=96), "cin576": dict(cin=576), "H0": dict(H=0), "H129": dict(H=129),
           "nkp14": dict(n_kp=14), "ns0": dict(ns=0), "extent0": dict(extent=0.0), "nq_negative": dict(nq=-1)}
# the module (offset_conv included): case -> cout
MODULE = [("d-c64-H5", 64), ("d-c128-H127", 32), ("d-c256-H5", 64), ("d-c320-H65", 128)]

for _c in CASES.values():
    assert KC.features_are_decision_safe(_c["x"]), _c["name"]
    _edge, _ball = DO.margins(_c["q"], _c["s"], _c["nbr"], _c["dkp"], EXTENT)
    assert _edge >= 1e-3 and _ball >= 0.05, (_c["name"], _edge, _ball)


def weights(case, cout):
    rng = np.random.default_rng(2000 + case["seed"])
    W = (rng.standard_normal((15, case["cin"], cout)) / np.sqrt(15 * case["cin"])).astype(F32)
    d_out = rng.standard_normal((case["nq"], cout)).astype(F32)
    return W, d_out


def module_params(case, cout, modulated):
    """W, W_off, b_off, d_out for the module chain.  The offset weights are drawn (seed after seed) until the chain's own
    deformed points leave every neighbour's NEAREST kernel point |d / extent - 1| >= 1e-3 from the edge in float64: then
    the in-range flags and the count of a float32 chain, whose dkp differs by parts in 10^6, are the oracle's."""
    W, d_out = weights(case, cout)
    od = 60 if modulated else 45
    for t in range(64):
        rng = np.random.default_rng(3000 + 64 * case["seed"] + t + (32 if modulated else 0))
        W_off = (rng.standard_normal((15, case["cin"], od)) * 0.15 / np.sqrt(15 * case["cin"])).astype(F32)
        b_off = (rng.standard_normal(od) * 0.05).astype(F32)
        r = DO.chain(case["q"], case["s"], case["nbr"], case["x"], case["kp"], EXTENT, W, W_off, b_off, modulated)
        g = DO.geometry(case["q"], case["s"], case["nbr"], r["deformed_KP"], EXTENT)
        near = np.where(g["real"], (g["d"] / EXTENT).min(-1), 0.0)
        if (np.abs(near - 1.0)[g["real"]] >= 1e-3).all():
            return W, W_off, b_off, d_out
    raise AssertionError("no offset weights with a margin")

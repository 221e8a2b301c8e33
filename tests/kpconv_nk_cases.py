"""Named inputs for the rigid KPConv with any kernel-point count (apr_kpconv_weighted_nk, apr_kpconv_dfeat_contrib_nk;
apr_amd/csrc/kpconv_nk.hip), each with the fact it exists for.  numpy only; everything is built from small integer seeds.

Kernel constants the cases are built around:
* step 1 takes the MFMA kernel iff cin % 64 == 0, H <= 128 and the rows of x and wf are 16-byte aligned: ONE 16-row tile of
  kernel points for n_kp <= 16 with 4 / 2 / 1 channel groups per pass (cin >= 256 / == 128 / otherwise), TWO tiles for
  n_kp 17..32 with 2 / 1 groups (cin >= 128 / 64); lane r16 owns kernel points r16 and 16 + r16, rows k >= n_kp are not
  stored.  One wave per query, 4 per block, re-ordered over 8 XCDs.  Everything else: one thread per (query, kernel point).
* the feature gradient sizes its influence table and dwf registers by 16 (n_kp <= 16: 4 waves per block, 1 / 2 / 4 / 8
  channels per lane, one pass) or 32 (2 waves per block, 1 / 2 / 4 channels per lane, passes of 256 channels: cin = 320 takes
  two); the closest kernel point has five index bits.
So: n_kp 1 (one row of one tile), 7, 15 (the count kpconv.hip is built for: the same bits are demanded), 16 (a full tile), 17
(one row of the second tile), 20, 32 (both tiles full); H 1, 3 (a partly filled MFMA step), 64, 65 (the second trip of the
index stage), 128 (the last LDS slot); cin 64, 128, 320 (2 + 2 + 1 / 4 + 1 groups; the second channel pass of the gradient)
on the MFMA route and 1, 3, 32 and 64 through a misaligned slice on the generic one; nq 1, 5 (a partial block; three blocks of
the two-wave gradient) and 70 (18 blocks: more than the 8 XCDs).

Geometry: points in [-1, 1]^3, kernel points in [-1, 1]^3 with kp[0] = 0, extent 1.2; support ns - 1 is `far` at (9, 9, 9)
(beyond every ball; a gaussian argument that underflows), support 0 has features that sum to exactly 0, support 1 a negative
sum (ns >= 4; features of tests/kpconv_cases.py: every row sum is an exact zero or decided with a margin).  Planted rows:
  allpad     a query with no real neighbour (every entry is ns)
  padkinds   padding of every kind in the first slots: ns, -1, ns + 5 (and -7)
  dup        one near, positive support listed in every slot (twice at least when H >= 2)
  far        a near positive support and the far one
  tie        (n_kp >= 20) an exact float32 tie for the closest kernel point between kernel points 3 and 19: they sit at
             (+-0.5, 1, 0), the centred neighbour at (0, 1.25, 0.125), every coordinate dyadic so that each evaluation order
             gives d2 = 0.328125 for both; kernel point 3 wins
Margins, asserted at import in float64: every real (q, h, k) has |d / extent - 1| >= M_EDGE (the oracle's edge band), and
apart from the planted tie the two smallest d2 of every real (q, h) differ by at least 1e-3 extent^2 (the float32 d2 is off
by parts in 10^7), so the float32 argmin is the float64 one.  Entries of unplanted rows that miss a margin are turned into
padding; planted rows move their query.
"""
import numpy as np

import kpconv_cases as KC
import kpconv_nk_oracle as NO

F32 = np.float32
EXTENT = KC.EXTENT
PLANTS = ("allpad", "padkinds", "dup", "far", "tie")
TIE_Q = np.array([0.25, -0.5, 0.125], F32)
TIE_D = np.array([0.0, 1.25, 0.125], F32)
TIE_KP = (np.array([0.5, 1.0, 0.0], F32), np.array([-0.5, 1.0, 0.0], F32))
TIE_K = (3, 19)
TIE_D2 = 0.328125
GAP = 1e-3


def build(name, fact, seed, n_kp, cin, H, nq, ns, layout="aligned"):
    rng = np.random.default_rng(5000 + seed)
    special = ns >= 4
    s = rng.uniform(-1, 1, (ns, 3)).astype(F32)
    q = rng.uniform(-1, 1, (nq, 3)).astype(F32)
    if special:
        s[ns - 1] = 9.0
    kp = rng.uniform(-1, 1, (n_kp, 3)).astype(F32)
    kp[0] = 0.0
    x = KC._features(rng, ns, cin, special)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)
    positive = [r for r in range(ns) if x[r].astype(np.float64).sum() > 0 and not (special and r == ns - 1)]
    plants, exempt = {}, []
    order = [PLANTS[(i + (seed if nq < len(PLANTS) else 0)) % len(PLANTS)] for i in range(min(nq, len(PLANTS)))]
    if n_kp >= 20 and "tie" not in order:
        order[0] = "tie"
    used = set()
    for row, kind in enumerate(order):
        near = positive[int(rng.integers(len(positive)))]
        off = np.array([0.25, -0.125, 0.0625], F32) * F32(1 + row % 3)
        if kind == "allpad":
            nbr[row] = ns
        elif kind == "padkinds":
            for h, v in enumerate((0, -1, 5, -7)[:H]):
                nbr[row, (h + seed) % H] = v if v < 0 else ns + v
        elif kind == "dup":
            nbr[row] = near
            q[row] = s[near] + off
        elif kind == "far":
            if not special or H < 2:
                continue
            nbr[row] = ns
            nbr[row, 0], nbr[row, H - 1] = ns - 1, near
            q[row] = s[near] + off
        elif kind == "tie":
            free = [r for r in range(2, ns - 1) if r not in used and x[r].astype(np.float64).sum() > 0]
            if n_kp < 20 or not free:
                continue
            r = free[0]
            q[row], s[r] = TIE_Q, TIE_Q + TIE_D
            nbr[row] = ns
            nbr[row, H - 1] = r
            for k, p in zip(TIE_K, TIE_KP):
                kp[k] = p
            for k in range(n_kp):      # nobody else nearer than the tie plus a margin
                while k not in TIE_K and float(((TIE_D.astype(np.float64) - kp[k]) ** 2).sum()) < TIE_D2 + 0.05:
                    kp[k] = rng.uniform(-1, 1, 3).astype(F32)
            exempt.append((row, H - 1))
            used.add(r)
        used |= {int(v) for v in nbr[row] if 0 <= v < ns}
        plants[row] = kind
    for _ in range(400):
        g = NO.geometry(q, s, nbr, kp, EXTENT, NO.DEFAULT)
        bad = g["real"] & (np.abs(g["d"] / EXTENT - 1.0) < 2 * NO.M_EDGE).any(-1)
        if n_kp >= 2:
            two = np.sort(g["d2"], axis=-1)[:, :, :2]
            bad |= g["real"] & (two[:, :, 1] - two[:, :, 0] < 2 * GAP * EXTENT ** 2)
        for row, h in exempt:
            bad[row, h] = False
        if not bad.any():
            break
        for row, h in np.argwhere(bad):
            if row not in plants or plants[row] == "padkinds":
                nbr[row, h] = ns
            else:
                assert plants[row] != "tie", name
                q[row] += rng.uniform(-0.02, 0.02, 3).astype(F32)
    else:
        raise AssertionError(f"{name}: no margin")
    dwf = rng.standard_normal((nq, n_kp * cin)).astype(F32)
    return dict(name=name, fact=fact, seed=seed, n_kp=n_kp, cin=cin, H=H, nq=nq, ns=ns, layout=layout, q=q, s=s, kp=kp, x=x,
                nbr=nbr, dwf=dwf, extent=EXTENT, plants=plants, exempt=exempt)


def expected_route(c):
    """the dispatch of apr_kpconv_weighted_nk, restated (ldwf and wf are aligned in every case)"""
    if c["cin"] % 64 or c["H"] > 128 or c["layout"] != "aligned":
        return "generic"
    if c["n_kp"] <= 16:
        return "t1g4" if c["cin"] >= 256 else "t1g2" if c["cin"] == 128 else "t1g1"
    return "t2g2" if c["cin"] >= 128 else "t2g1"


# name: (fact, seed, n_kp, cin, H, nq, ns[, layout])
_CASES = {
    # ---- MFMA route
    "k1-c64-H3-nq5":     ("n_kp = 1: one live row of one tile; H = 3: a partly filled MFMA step", 1, 1, 64, 3, 5, 12),
    "k7-c64-H5-nq70":    ("n_kp = 7; 18 blocks (more than the 8 XCDs: the swizzle), 35 blocks of the gradient", 2, 7, 64, 5, 70, 40),
    "k7-c128-H65-nq5":   ("n_kp = 7, cin = 128 (two groups per pass), H = 65: the second trip of the index stage", 3, 7, 128, 65, 5, 100),
    "k15-c64-H5-nq5":    ("n_kp = 15: the bits of apr_kpconv_weighted_mode / apr_kpconv_dfeat_contrib_mode", 4, 15, 64, 5, 5, 40),
    "k15-c320-H64-nq5":  ("n_kp = 15, cin = 320 = 4 + 1 groups, 8 channels per lane in the gradient; H = 64", 5, 15, 320, 64, 5, 80),
    "k16-c128-H128-nq5": ("n_kp = 16: a full tile, no idle row; H = 128: the last LDS slot", 6, 16, 128, 128, 5, 160),
    "k17-c64-H1-nq1":    ("n_kp = 17: ONE row of the second tile; H = 1, one query", 7, 17, 64, 1, 1, 7),
    "k17-c320-H3-nq5":   ("n_kp = 17, cin = 320 = 2 + 2 + 1 groups of the two-tile form; two channel passes of the gradient", 8, 17,
                          320, 3, 5, 40),
    "k20-c64-H5-nq70":   ("n_kp = 20, one group per pass, 18 blocks; the tie between kernel points 3 and 19", 9, 20, 64, 5, 70, 40),
    "k20-c128-H65-nq5":  ("n_kp = 20, cin = 128, H = 65", 10, 20, 128, 65, 5, 100),
    "k32-c128-H128-nq5": ("n_kp = 32: both tiles full; H = 128; ns = 160", 11, 32, 128, 128, 5, 160),
    "k32-c320-H64-nq5":  ("n_kp = 32, cin = 320, H = 64: the most registers of either kernel; ns = 200", 12, 32, 320, 64, 5, 200),
    # ---- generic route
    "k1-c1-H1-nq1":      ("n_kp = 1, cin = 1, H = 1, one query: one thread", 13, 1, 1, 1, 1, 5),
    "k7-c1-H5-nq70":     ("cin = 1 (the first layer of a network) at n_kp = 7; 490 threads: two blocks", 14, 7, 1, 5, 70, 40),
    "k15-c3-H5-nq5":     ("n_kp = 15 on the generic route: the bits of apr_kpconv_weighted_mode", 15, 15, 3, 5, 5, 40),
    "k17-c32-H3-nq5":    ("cin = 32: four 8-channel chunks, below the MFMA width", 16, 17, 32, 3, 5, 20),
    "k20-c3-H65-nq5":    ("cin = 3: a 3-channel tail chunk; H = 65; the tie", 17, 20, 3, 65, 5, 100),
    "k32-c64-H5-slice":  ("cin = 64 through a column slice big[:, 1:65]: misaligned rows, generic route at n_kp = 32", 18, 32, 64,
                          5, 5, 40, "slice1"),
}
CASES = {name: build(name, *spec) for name, spec in _CASES.items()}
ALL_MODE_CASES = [n for n, c in CASES.items() if c["n_kp"] in (7, 15, 20)]      # every (influence, aggregation) runs on these
BIT_CASES = [n for n, c in CASES.items() if c["n_kp"] == 15]
MODULE = [("k7-c64-H5-nq70", 64), ("k20-c64-H5-nq70", 64)]


def case_modes(name):
    """all six modes at n_kp = 7 and 20 and at 15 (held to the 15-point entries' bits); elsewhere (linear, sum) and (gaussian, closest): the five index bits at n_kp = 32"""
    return list(NO.MODES) if name in ALL_MODE_CASES else [NO.DEFAULT, (NO.GAUSSIAN, 1)]


def weights(case, cout):
    rng = np.random.default_rng(1000 + case["seed"])
    K, cin = case["n_kp"], case["cin"]
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(F32)
    d_out = rng.standard_normal((case["nq"], cout)).astype(F32)
    return W, d_out


_seen = set()
for _c in CASES.values():
    assert _c["ns"] <= 200 and _c["nq"] <= 70 and _c["H"] <= 128 and _c["fact"], _c["name"]
    assert KC.features_are_decision_safe(_c["x"]), _c["name"]
    _a = (_c["q"], _c["s"], _c["nbr"], _c["kp"], EXTENT)
    assert NO.edge_margin(*_a) >= NO.M_EDGE, _c["name"]
    assert NO.closest_margin(*_a, _c["exempt"]) >= GAP, _c["name"]
    for _row, _h in _c["exempt"]:      # the tie is exact in float32 and in float64, and it is the minimum
        _d2 = NO.geometry(*_a, NO.DEFAULT)["d2"][_row, _h]
        assert _d2[3] == _d2[19] == TIE_D2 and np.sort(_d2)[2] >= TIE_D2 + GAP * EXTENT ** 2, (_c["name"], _d2)
        _e = (_c["s"][_c["nbr"][_row, _h]] - _c["q"][_row])[None] - _c["kp"][[3, 19]]
        assert _e.dtype == F32 and ((_e * _e).sum(1) == F32(TIE_D2)).all()
    _seen |= set(_c["plants"].values())
assert set(PLANTS) <= _seen, _seen
assert all(CASES[n]["exempt"] for n in CASES if CASES[n]["n_kp"] >= 20 and CASES[n]["nq"] >= 5), "a tie case without its tie"

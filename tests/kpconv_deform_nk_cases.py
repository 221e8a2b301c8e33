"""Named inputs for the deformable KPConv with any kernel-point count (apr_kpconv_deform_*_nk;
apr_amd/csrc/kpconv_deform_nk.hip), each with the fact it exists for.  numpy only; everything is built from small integer
seeds.

Kernel constants the cases are built around: one wave per query; the MFMA kernels carry ONE 16-row tile of kernel points for
n_kp <= 16 and TWO for 17..32 (lane r16 owns kernel points r16 and 16 + r16); step 1 runs 4 / 2 / 1 channel groups of 64 per
pass with one tile (cin >= 256 / == 128 / 64) and 2 / 1 with two (cin >= 128 / 64), four neighbours per MFMA step; the feature
gradient sizes its influence table by 16 (4 waves per block, 1 / 2 / 4 / 8 channels per lane) or 32 (2 waves per block,
1 / 2 / 4 channels per lane, channel passes of 256); the geometry gradient streams 16-neighbour tiles; the index stage fills 64
slots per trip; the closest kernel point has five index bits.
So: n_kp 1, 7, 15, 16 (a full tile), 17 (one row of the second tile), 20, 32; H 1, 3 (a partly filled MFMA step), 5, 64, 65
(a second index trip, a fifth neighbour tile of one row), 128 (the last LDS slot); cin 64, 128, 320 (4 + 1 / 2 + 2 + 1 groups;
the second channel pass of the two-tile gradient), 512; nq 1, 5 (a partial block), 70 (18 blocks: more than the 8 XCDs).

Geometry as tests/kpconv_deform_cases.py: points in [-1, 1]^3, rigid kernel points kp in [-1, 1]^3 with kp[0] = 0, extent 1.2,
support ns - 1 `far` at (9, 9, 9) with positive features, support 0 summing to exactly 0, support 1 to a negative number.
dkp = kp + extent * offsets with offsets uniform in [-0.3, 0.3]; mod uniform in [0.2, 1.8].

Planted rows: those of kpconv_deform_cases.PLANTS (allpad, padkinds, deform_only, rigid_only, none, floor, dup, mod02,
mod0_only, zero_off; a plant that names a kernel point the case does not have is left out) and, for n_kp >= 20,
  high_only  the far support in range of kernel point 17 and of no other, next to a near positive support inside the balls of
             the other kernel points: both count (num = 2); a flag that looks at the first tile alone counts one
  tie        an exact float32 tie for the closest kernel point between kernel points 3 and 19 ((+-0.5, 1, 0) seen from the
             centred neighbour (0, 1.25, 0.125): d2 = 0.328125 in every evaluation order); kernel point 3 wins
  min_high   one near support in every slot and kernel point n_kp - 1 moved next to it: the query's smallest d2 belongs to a
             kernel point of the second tile
Margins, asserted at import in float64: |d / extent - 1| >= 1e-3 for every real (q, h, k), d >= 0.05 extent inside a ball, the
row-sum margin of tests/kpconv_cases.py and, apart from the planted tie, the two smallest d2 of every real (q, h) at least
1e-3 extent^2 apart -- so every decision of a float32 evaluation is the float64 one.
"""
import numpy as np

import kpconv_cases as KC
import kpconv_deform_cases as DC
import kpconv_deform_nk_oracle as DNO

F32 = np.float32
EXTENT = KC.EXTENT
PLANTS = DC.PLANTS + ("high_only", "tie", "min_high")
HIGH_PLANTS = ("high_only", "tie", "min_high")
NEAR = DC.NEAR
TIE_D = np.array([0.0, 1.25, 0.125], F32)
TIE_KP = (np.array([0.5, 1.0, 0.0], F32), np.array([-0.5, 1.0, 0.0], F32))
TIE_K = (3, 19)
TIE_D2 = 0.328125
GAP = 1e-3
DROPPABLE = ("zero_off", "mod02", "padkinds")      # planted rows whose neighbour table is random: entries may turn into padding
_NEEDS_K = {"deform_only": 4, "floor": 2, "mod02": 6, "mod0_only": 3}


def build(name, fact, seed, n_kp, cin, H, nq, ns):
    rng = np.random.default_rng(8000 + seed)
    K = n_kp
    s = rng.uniform(-1, 1, (ns, 3)).astype(F32)
    q = rng.uniform(-1, 1, (nq, 3)).astype(F32)
    s[ns - 1] = 9.0
    kp = rng.uniform(-1, 1, (K, 3)).astype(F32)
    kp[0] = 0.0
    x = KC._features(rng, ns, cin, True)
    nbr = rng.integers(0, ns + 1, (nq, H)).astype(np.int32)
    dkp = (kp[None] + F32(EXTENT) * rng.uniform(-0.3, 0.3, (nq, K, 3)).astype(F32)).astype(F32)
    mod = rng.uniform(0.2, 1.8, (nq, K)).astype(F32)
    positive = [r for r in range(2, ns - 1) if x[r].astype(np.float64).sum() > 0]
    far = ns - 1
    kinds = list(PLANTS if K >= 20 else DC.PLANTS)
    if nq < len(kinds):      # a few rows only: the plants of the second tile first, then a rotation of the others
        rot = [DC.PLANTS[(i + seed) % len(DC.PLANTS)] for i in range(len(DC.PLANTS))]
        kinds = (list(HIGH_PLANTS) if K >= 20 else []) + rot
    plants, fixed, exempt, used = {}, set(), [], set()
    for row, kind in zip(range(nq), kinds):
        if kind in ("rigid_only", "mod0_only", "floor", "high_only") and H < 2:
            kind = "dup"      # one slot: it holds a real neighbour
        if _NEEDS_K.get(kind, 1) > K:
            continue
        near = positive[int(rng.integers(len(positive)))]
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
            dkp[row] = DC._cluster(rng, s[far].astype(np.float64) - q[row], K)
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
            dkp[row] = DC._cluster(rng, s[near].astype(np.float64) - q[row], K)
            dkp[row, 2] = (s[far].astype(np.float64) - q[row] + np.array([0.3, 0.2, 0.1])).astype(F32)
            mod[row, 2] = 0.0
        elif kind == "zero_off":
            dkp[row] = kp
            mod[row] = 1.0
        elif kind == "high_only":
            nbr[row] = ns
            nbr[row, 0], nbr[row, H - 1] = far, near
            q[row] = s[near] + NEAR
            dkp[row] = DC._cluster(rng, s[near].astype(np.float64) - q[row], K)
            dkp[row, 17] = (s[far].astype(np.float64) - q[row] + np.array([0.3, 0.2, 0.1])).astype(F32)
        elif kind == "tie":
            r = [v for v in positive if v != near and v not in used][0]      # a support no planted row before this one names
            q[row] = np.array([0.25, -0.5, 0.125], F32)
            s[r] = q[row] + TIE_D
            nbr[np.arange(nq) != row] = np.where(nbr[np.arange(nq) != row] == r, ns, nbr[np.arange(nq) != row])
            nbr[row] = ns
            nbr[row, H - 1] = r
            for k, p in zip(TIE_K, TIE_KP):
                dkp[row, k] = p
            for k in range(K):      # nobody else nearer than the tie plus a margin
                while k not in TIE_K and float(((TIE_D.astype(np.float64) - dkp[row, k]) ** 2).sum()) < TIE_D2 + 0.05:
                    dkp[row, k] = rng.uniform(-1, 1, 3).astype(F32)
            exempt.append((row, H - 1))
            positive = [v for v in positive if v != r]
        elif kind == "min_high":
            nbr[row] = near
            q[row] = s[near] + NEAR
            Dn = s[near].astype(np.float64) - q[row]
            for k in range(K - 1):
                while float(((Dn - dkp[row, k]) ** 2).sum()) < 0.3 ** 2:
                    dkp[row, k] = (kp[k] + F32(EXTENT) * rng.uniform(-0.3, 0.3, 3)).astype(F32)
            dkp[row, K - 1] = (Dn + np.array([0.1, 0.1, 0.1])).astype(F32)
        plants[row] = kind
        used |= {int(v) for v in nbr[row] if 0 <= v < ns}
        if kind in ("zero_off", "none", "tie", "min_high"):
            fixed.add(row)
    gap_min = 2 * GAP * EXTENT ** 2
    for _ in range(600):
        g = DNO.geometry(q, s, nbr, dkp, EXTENT)
        r = g["d"] / EXTENT
        bad = g["real"][:, :, None] & ((np.abs(r - 1.0) < 2e-3) | (r < 0.06))
        small = np.zeros(nbr.shape, bool)
        if K >= 2:
            two = np.sort(g["d2"], axis=-1)[:, :, :2]
            small = g["real"] & (two[:, :, 1] - two[:, :, 0] < gap_min)
        for row, h in exempt:
            small[row, h] = False
        if not bad.any() and not small.any():
            break
        for row, h, k in np.argwhere(bad):
            if row not in fixed or (plants[row] == "tie" and k not in TIE_K) or (plants[row] == "min_high" and k != K - 1):
                dkp[row, k] += rng.uniform(-0.05, 0.05, 3).astype(F32)
            elif row not in plants or plants[row] in DROPPABLE:
                nbr[row, h] = ns
            else:
                assert plants[row] not in ("tie", "min_high"), (name, plants[row])
                q[row] += rng.uniform(-0.02, 0.02, 3).astype(F32)
        for row, h in np.argwhere(small):
            if row not in plants or plants[row] in DROPPABLE:
                nbr[row, h] = ns
            elif plants[row] in ("tie", "min_high", "none", "dup"):      # the query is tied to its support: move a kernel point
                k = int(np.argsort(g["d2"][row, h])[1])
                assert plants[row] != "none", name
                dkp[row, k] += rng.uniform(-0.05, 0.05, 3).astype(F32)
            else:
                k = int(np.argsort(g["d2"][row, h])[1])
                dkp[row, k] += rng.uniform(-0.05, 0.05, 3).astype(F32)
    else:
        raise AssertionError(f"{name}: no margin")
    dwf = rng.standard_normal((nq, K * cin)).astype(F32)
    return dict(name=name, fact=fact, seed=seed, n_kp=K, cin=cin, H=H, nq=nq, ns=ns, q=q, s=s, kp=kp, x=x, nbr=nbr, dkp=dkp,
                mod=mod, dwf=dwf, extent=EXTENT, plants=plants, exempt=exempt)


def expected_route(c):
    """the dispatch of the three entries, restated: (step 1 <T, NG>, gradient <CPL, KT>, geometry <T>)"""
    K, cin = c["n_kp"], c["cin"]
    if K <= 16:
        return ((1, 4 if cin >= 256 else 2 if cin == 128 else 1), (1 if cin <= 64 else 2 if cin <= 128 else 4 if cin <= 256 else 8, 16),
                1)
    return (2, 2 if cin >= 128 else 1), (1 if cin <= 64 else 2 if cin <= 128 else 4, 32), 2


# name: (fact, seed, n_kp, cin, H, nq, ns)
_CASES = {
    "dk1-c64-H3-nq5":      ("n_kp = 1: one live row of one tile, no second-closest kernel point; H = 3", 1, 1, 64, 3, 5, 12),
    "dk7-c64-H5-nq70":     ("n_kp = 7: every plant of the first tile; 18 blocks (more than the 8 XCDs), 18 of the gradient", 2, 7, 64,
                            5, 70, 40),
    "dk7-c128-H65-nq5":    ("n_kp = 7, cin = 128 (two groups per pass), H = 65: a second index trip, a fifth neighbour tile", 3, 7,
                            128, 65, 5, 100),
    "dk7-c512-H3-nq5":     ("n_kp = 7, cin = 512: two passes of four groups, 8 channels per lane, 8 chunks of the geometry GEMM", 4,
                            7, 512, 3, 5, 40),
    "dk15-c64-H5-nq70":    ("n_kp = 15: the count kpconv_deform.hip is built for; every plant of the first tile", 5, 15, 64, 5, 70,
                            40),
    "dk15-c320-H64-nq5":   ("n_kp = 15, cin = 320 = 4 + 1 groups; H = 64: one full index trip, 4 full neighbour tiles", 6, 15, 320,
                            64, 5, 80),
    "dk16-c128-H128-nq5":  ("n_kp = 16: a full tile, no idle row; H = 128: the last LDS slot, 8 neighbour tiles", 7, 16, 128, 128,
                            5, 160),
    "dk17-c64-H1-nq1":     ("n_kp = 17: ONE row of the second tile; H = 1, one query", 8, 17, 64, 1, 1, 7),
    "dk17-c320-H3-nq5":    ("n_kp = 17, cin = 320 = 2 + 2 + 1 groups of the two-tile form; two channel passes of the gradient", 9,
                            17, 320, 3, 5, 40),
    "dk20-c64-H5-nq70":    ("n_kp = 20: every plant, the three of the second tile included; 18 blocks, 35 of the gradient", 10, 20,
                            64, 5, 70, 40),
    "dk20-c128-H65-nq5":   ("n_kp = 20, cin = 128, H = 65; high_only, tie, min_high", 11, 20, 128, 65, 5, 100),
    "dk20-c512-H5-nq5":    ("n_kp = 20, cin = 512: four passes of two groups, two channel passes of 256 of the gradient", 12, 20,
                            512, 5, 5, 40),
    "dk32-c128-H128-nq5":  ("n_kp = 32: both tiles full, five index bits; H = 128", 13, 32, 128, 128, 5, 160),
    "dk32-c320-H64-nq5":   ("n_kp = 32, cin = 320, H = 64: the most registers of every kernel", 14, 32, 320, 64, 5, 200),
}
CASES = {name: build(name, *spec) for name, spec in _CASES.items()}
ALL_MODE_CASES = [n for n, c in CASES.items() if c["n_kp"] in (7, 15, 20)]      # every (influence, aggregation) runs on these
K15_CASES = [n for n, c in CASES.items() if c["n_kp"] == 15]
# what every entry refuses (overrides of cin 64, H 5, n_kp 7, ns 9, extent 1.2, nq 5, mode m = (1, 0))
REFUSED = {"nkp0": dict(n_kp=0), "nkp33": dict(n_kp=33), "cin32": dict(cin=32), "cin96": dict(cin=96), "cin576": dict(cin=576),
           "H0": dict(H=0), "H129": dict(H=129), "ns0": dict(ns=0), "extent0": dict(extent=0.0), "nq_negative": dict(nq=-1),
           "influence3": dict(m=(3, 0)), "closest2": dict(m=(1, 2))}
MODULE = [("dk7-c64-H5-nq70", 64), ("dk7-c128-H65-nq5", 32), ("dk20-c64-H5-nq70", 64), ("dk20-c128-H65-nq5", 32)]


def case_modes(name):
    """all six modes at n_kp = 7, 15 and 20; elsewhere (linear, sum) and (gaussian, closest)"""
    return list(DNO.MODES) if name in ALL_MODE_CASES else [DNO.DEFAULT, (DNO.GAUSSIAN, 1)]


def weights(case, cout):
    rng = np.random.default_rng(2000 + case["seed"])
    K, cin = case["n_kp"], case["cin"]
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(F32)
    d_out = rng.standard_normal((case["nq"], cout)).astype(F32)
    return W, d_out


def module_params(case, cout, modulated, mode=DNO.DEFAULT):
    """W, W_off, b_off, d_out for the module chain.  The offset weights are drawn (seed after seed) until the chain's own
    deformed points leave every neighbour's NEAREST kernel point |d / extent - 1| >= 1e-3 from the edge in float64 (and, for
    closest, the two smallest d2 1e-3 extent^2 apart): then the in-range flags and the count of a float32 chain, whose dkp
    differs by parts in 10^6, are the oracle's."""
    W, d_out = weights(case, cout)
    K, cin = case["n_kp"], case["cin"]
    od = (4 if modulated else 3) * K
    for t in range(256):
        rng = np.random.default_rng(9000 + 256 * case["seed"] + t + (128 if modulated else 0) + 17 * mode[0] + 5 * mode[1])
        W_off = (rng.standard_normal((K, cin, od)) * 0.15 / np.sqrt(K * cin)).astype(F32)
        b_off = (rng.standard_normal(od) * 0.05).astype(F32)
        r = DNO.chain(case["q"], case["s"], case["nbr"], case["x"], case["kp"], EXTENT, W, W_off, b_off, modulated, mode)
        g = DNO.geometry(case["q"], case["s"], case["nbr"], r["deformed_KP"], EXTENT)
        near = np.where(g["real"], (g["d"] / EXTENT).min(-1), 0.0)
        if not (np.abs(near - 1.0)[g["real"]] >= 1e-3).all():
            continue
        if mode[1] and DNO.closest_margin(case["q"], case["s"], case["nbr"], r["deformed_KP"], EXTENT) < 1e-3:
            continue
        return W, W_off, b_off, d_out
    raise AssertionError("no offset weights with a margin")


_seen = set()
for _c in CASES.values():
    assert _c["ns"] <= 200 and _c["nq"] <= 70 and _c["H"] <= 128 and _c["fact"], _c["name"]
    assert KC.features_are_decision_safe(_c["x"]), _c["name"]
    _a = (_c["q"], _c["s"], _c["nbr"], _c["dkp"], EXTENT)
    _edge, _ball = DNO.margins(*_a)
    assert _edge >= 1e-3 and _ball >= 0.05, (_c["name"], _edge, _ball)
    assert DNO.closest_margin(*_a, _c["exempt"]) >= GAP, _c["name"]
    for _row, _h in _c["exempt"]:      # the tie is exact in float32 and in float64, and it is the minimum
        _d2 = DNO.geometry(*_a)["d2"][_row, _h]
        assert _d2[3] == _d2[19] == TIE_D2 and np.sort(_d2)[2] >= TIE_D2 + GAP * EXTENT ** 2, (_c["name"], _d2)
        _e = (_c["s"][_c["nbr"][_row, _h]] - _c["q"][_row])[None] - _c["dkp"][_row][[3, 19]]
        assert _e.dtype == F32 and ((_e * _e).sum(1) == F32(TIE_D2)).all()
    _seen |= set(_c["plants"].values())
assert set(PLANTS) <= _seen, _seen
assert all(set(HIGH_PLANTS) <= set(CASES[n]["plants"].values()) for n in CASES if CASES[n]["n_kp"] >= 20 and CASES[n]["nq"] >= 5)

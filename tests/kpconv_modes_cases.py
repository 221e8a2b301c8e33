"""Named inputs for KPConv's influence / aggregation modes (apr_kpconv_*_mode), each with the fact it exists for.  numpy
only; everything is built from small integer seeds.

Every case carries BOTH geometries: the rigid kernel points kp (apr_kpconv_weighted_mode, apr_kpconv_dfeat_contrib_mode) and
per-query deformed points dkp with modulations mod (apr_kpconv_deform_*_mode; cin % 64 == 0 only).  The base is the builder
of tests/kpconv_deform_cases.py (points in [-1, 1]^3, extent 1.2, the far support at (9, 9, 9), the zero-sum and the
negative-sum support) with its planted rows, which serve the modes as follows:
  allpad       all padding: output exactly 0 in every mode, num at its floor
  padkinds     the three kinds of padding (ns, -1, ns + 5): with the constant influence a padding slot still adds nothing
  rigid_only   a real, positive neighbour outside every deformed ball next to the far support inside one: on the deformed layer
               it must neither contribute nor count with the constant and the gaussian influence; on the rigid layer the same
               neighbour contributes, and the far support does too -- with the gaussian influence far beyond the extent,
               where its argument (~ 700) underflows
  deform_only  the far support inside ONE deformed ball: with `sum` it carries influence to all 15 kernel points (14 of them
               ~ 14 away: gaussian arguments that underflow), with `closest` to kernel point 3 alone
  mod0_only    the far support whose closest deformed kernel point (2) has mod = 0: `closest` gives it no output at all
  mod02, none, floor, dup, zero_off: as in the deform cases
and two more:
  tie          an exact float32 tie: kernel points 3 and 7 at (+-0.5, 1, 0), the centred neighbour at (0, 1.25, 0.125), every
               coordinate dyadic so that each evaluation order gives d2 = 0.328125 for both; kernel point 3 wins
  denormal     a support at (3, 2.75, 2.5) seen from a query at the origin: gaussian argument 88.01 for kernel point 0 -- the
               influence is a float32 denormal (or flushed)

Every case asserts at import, in float64: the margins of the deform cases on the deformed geometry (|d / extent - 1| >= 1e-3
for every real triple, d >= 0.05 extent inside a ball, the row-sum margin) and, for `closest`, on both geometries: apart from
the planted tie the two smallest d2 of every real (q, h) differ by at least 1e-3 extent^2, so the float32 argmin is the
float64 one.  Entries of unplanted rows that miss a margin are turned into padding; planted rows move their query.
"""
import numpy as np

import kpconv_cases as KC
import kpconv_deform_cases as DC
import kpconv_deform_oracle as DO
import kpconv_modes_oracle as MO

F32 = np.float32
EXTENT = DC.EXTENT
DROPPABLE = ("zero_off", "mod02", "padkinds")      # planted rows whose neighbour table is random: entries may turn into padding
TIE_Q = np.array([0.25, -0.5, 0.125], F32)
TIE_D = np.array([0.0, 1.25, 0.125], F32)
TIE_KP = (np.array([0.5, 1.0, 0.0], F32), np.array([-0.5, 1.0, 0.0], F32))
TIE_K = (3, 7)
DENORMAL_S = np.array([3.0, 2.75, 2.5], F32)


def _away(rng, pts, D, skip):
    """move the points of pts [15, 3] (but `skip`) that are nearer to D than the tie distance plus a margin"""
    tie = float(((TIE_D - TIE_KP[0]) ** 2).sum())
    for k in range(15):
        if k in skip:
            continue
        while float(((D.astype(np.float64) - pts[k]) ** 2).sum()) < tie + 0.05:
            pts[k] = rng.uniform(-1, 1, 3).astype(F32)


def build(name, fact, seed, cin, H, nq, ns):
    c = DC.build(name, fact, seed, cin, H, nq, ns)
    rng = np.random.default_rng(7000 + seed)
    q, s, kp, nbr, dkp, plants = c["q"], c["s"], c["kp"], c["nbr"], c["dkp"], c["plants"]
    used = set(int(v) for row in plants for v in nbr[row] if 0 <= v < ns) | {0, 1, ns - 1}
    free_rows = [r for r in range(nq) if r not in plants]
    free_sup = [r for r in range(ns) if r not in used]
    exempt = []
    if free_rows and free_sup:
        row, r = free_rows.pop(0), free_sup.pop(0)
        q[row], s[r] = TIE_Q, TIE_Q + TIE_D
        nbr[row] = ns
        nbr[row, H - 1] = r
        for k, p in zip(TIE_K, TIE_KP):
            kp[k] = p
            dkp[row, k] = p
        _away(rng, kp, TIE_D, TIE_K)
        _away(rng, dkp[row], TIE_D, TIE_K)
        plants[row] = "tie"
        exempt.append((row, H - 1))
    if free_rows and free_sup and ns >= 6:
        row, r = free_rows.pop(0), free_sup.pop(0)
        q[row], s[r] = 0.0, DENORMAL_S
        nbr[row] = ns
        nbr[row, 0] = r
        plants[row] = "denormal"
    fixed = {row for row, kind in plants.items() if kind in ("zero_off", "none", "tie")}
    gap_min = 2e-3 * EXTENT ** 2
    for _ in range(400):
        clean = True
        gd = DO.geometry(q, s, nbr, dkp, EXTENT)
        gr = DO.geometry(q, s, nbr, MO.rigid(kp, nq), EXTENT)
        r = gd["d"] / EXTENT
        bad = gd["real"][:, :, None] & ((np.abs(r - 1.0) < 2e-3) | (r < 0.06))
        small = np.zeros(nbr.shape, bool)
        for g in (gd, gr):
            two = np.sort(g["d2"], axis=-1)[:, :, :2]
            small |= g["real"] & (two[:, :, 1] - two[:, :, 0] < gap_min)
        for row, h in exempt:
            small[row, h] = False
        for row, h, k in np.argwhere(bad):
            clean = False
            if row not in fixed or (plants[row] == "tie" and k not in TIE_K):
                dkp[row, k] += rng.uniform(-0.05, 0.05, 3).astype(F32)
            elif row not in plants or plants[row] in DROPPABLE:
                nbr[row, h] = ns
            else:
                assert plants[row] != "tie", name
                q[row] += rng.uniform(-0.02, 0.02, 3).astype(F32)
        for row, h in np.argwhere(small):
            clean = False
            if row not in plants or plants[row] in DROPPABLE:
                nbr[row, h] = ns
            else:
                assert plants[row] != "tie", name
                q[row] += rng.uniform(-0.02, 0.02, 3).astype(F32)
        if clean:
            break
    else:
        raise AssertionError(f"{name}: no margin")
    c.update(exempt=exempt)
    return c


# name: (fact, seed, cin, H, nq, ns)
_CASES = {
    "k-c1-H5-nq37":   ("cin = 1 (the first layer): the generic kernel finds the closest kernel point per thread; rigid only", 201,
                       1, 5, 37, 40),
    "k-c64-H5-nq37":  ("cin = 64, H = 5 (a partly filled MFMA step), 10 blocks (more than 8: the XCD swizzle): every planted row",
                       202, 64, 5, 37, 40),
    "k-c64-H1-nq1":   ("H = 1, one query", 203, 64, 1, 1, 7),
    "k-c64-H65-nq5":  ("H = 65: the second pass of the index stage records mode bytes too; nq = 5: a partial block", 204, 64, 65,
                       5, 100),
    "k-c64-H128-nq5": ("H = 128: the last LDS slot of the mode bytes", 205, 64, 128, 5, 160),
    "k-c192-H5-nq5":  ("cin = 192: three channel passes read the same mode bytes; CPL 4 with an idle register", 206, 192, 5, 5, 40),
    "k-c320-H5-nq5":  ("cin = 320 = 4 + 1 groups: a pass with one live group", 207, 320, 5, 5, 40),
}
CASES = {name: build(name, *spec) for name, spec in _CASES.items()}
MODULE = [("k-c64-H5-nq37", 64)]

_seen = set()
for _c in CASES.values():
    assert KC.features_are_decision_safe(_c["x"]), _c["name"]
    _edge, _ball = DO.margins(_c["q"], _c["s"], _c["nbr"], _c["dkp"], EXTENT)
    assert _edge >= 1e-3 and _ball >= 0.05, (_c["name"], _edge, _ball)
    for _K in (_c["dkp"], MO.rigid(_c["kp"], _c["nq"])):
        assert MO.closest_margin(_c["q"], _c["s"], _c["nbr"], _K, EXTENT, _c["exempt"]) >= 1e-3, _c["name"]
    for _row, _h in _c["exempt"]:      # the tie is exact in float32 and in float64, on both geometries, and it is the minimum
        for _K in (_c["dkp"], MO.rigid(_c["kp"], _c["nq"])):
            _d2 = DO.geometry(_c["q"], _c["s"], _c["nbr"], _K, EXTENT)["d2"][_row, _h]
            assert _d2[3] == _d2[7] == 0.328125 and np.sort(_d2)[2] >= 0.328125 + 1e-3 * EXTENT ** 2, (_c["name"], _d2)
        _e = (_c["s"][_c["nbr"][_row, _h]] - _c["q"][_row])[None] - _c["kp"][[3, 7]]
        assert _e.dtype == F32 and ((_e * _e).sum(1) == F32(0.328125)).all()
    _seen |= set(_c["plants"].values())
assert {"tie", "denormal", "rigid_only", "deform_only", "mod0_only", "allpad", "padkinds", "zero_off"} <= _seen, _seen
_a = DO.geometry(CASES["k-c64-H5-nq37"]["q"], CASES["k-c64-H5-nq37"]["s"], CASES["k-c64-H5-nq37"]["nbr"],
                 MO.rigid(CASES["k-c64-H5-nq37"]["kp"], 37), EXTENT)
_arg = (_a["d2"] / MO.gauss_den(EXTENT))[_a["real"]]
assert ((_arg > 87.4) & (_arg < 103.0)).any() and (_arg > 104.0).any(), "no denormal / underflowing gaussian argument"

weights = DC.weights


def module_params(case, cout, modulated, mode):
    """W, W_off, b_off, d_out for the module chain in `mode`.  The offset weights are drawn until the chain's own deformed
    points keep the margins of this file: every neighbour's nearest kernel point 1e-3 off the edge and, for closest, the two
    smallest d2 1e-3 extent^2 apart -- then the decisions of a float32 chain, whose dkp differs by parts in 10^6, are the
    oracle's."""
    W, d_out = weights(case, cout)
    od = 60 if modulated else 45
    for t in range(256):
        rng = np.random.default_rng(9000 + 256 * case["seed"] + t + (128 if modulated else 0) + 17 * mode[0] + 5 * mode[1])
        W_off = (rng.standard_normal((15, case["cin"], od)) * 0.15 / np.sqrt(15 * case["cin"])).astype(F32)
        b_off = (rng.standard_normal(od) * 0.05).astype(F32)
        r = MO.chain(case["q"], case["s"], case["nbr"], case["x"], case["kp"], EXTENT, W, mode, W_off=W_off, b_off=b_off,
                     modulated=modulated)
        g = DO.geometry(case["q"], case["s"], case["nbr"], r["deformed_KP"], EXTENT)
        near = np.where(g["real"], (g["d"] / EXTENT).min(-1), 0.0)
        if not (np.abs(near - 1.0)[g["real"]] >= 1e-3).all():
            continue
        if mode[1] and MO.closest_margin(case["q"], case["s"], case["nbr"], r["deformed_KP"], EXTENT) < 1e-3:
            continue
        return W, W_off, b_off, d_out
    raise AssertionError("no offset weights with a margin")

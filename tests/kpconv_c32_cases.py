"""Inputs for apr_kpconv_weighted_c32 (cin = 32), built by tests/kpconv_cases.py's own builder (its geometry, features and
planted rows) plus one plant of this file: a neighbour at distance float32(extent) from kernel point 0 -- the extent the
kernel receives; in float64 that is 4e-8 beyond 1.2, so the exact influence is 0 where a float32 evaluation may see a last
bit of it.  numpy only.  The facts the GPU test relies on are asserted here from the oracle's own intermediates, at import.

k_kpconv_weighted_c32: one wave per query, 4 per block (ceil(nq / 4) blocks), the index stage fills 128 LDS slots in two trips
of 64 lanes, the MFMA walks (H + 3) >> 2 steps of 4 neighbours with the next step's row in flight.
"""
import numpy as np

import kpconv_cases as K
import kpconv_oracle as O

CIN = 32
# name: (fact, seed, nq, H, ns)
_SPECS = {
    "q1-H1-ns1":    ("one query, one neighbour, one support: a single MFMA step, three empty k-slots, nothing in flight", 2, 1, 1, 1),
    "q3-H3-ns7":    ("3 queries in one block (a wave without a query), H = 3: a partial step", 0, 3, 3, 7),
    "q4-H4-ns9":    ("a full block, H = 4: exactly one step", 3, 4, 4, 9),
    "q5-H5-ns40":   ("2 blocks, H = 5: two steps, the second with one neighbour", 1, 5, 5, 40),
    "q9-H63-ns50":  ("H = 63: last lane of the first index trip idle; 3 blocks", 13, 9, 63, 50),
    "q9-H64-ns50":  ("H = 64: one full index trip, 16 steps", 14, 9, 64, 50),
    "q6-H65-ns50":  ("H = 65: second index trip with one lane, tail step of one", 15, 6, 65, 50),
    "q5-H128-ns200": ("H = 128: the LDS table's last slot, 32 steps", 17, 5, 128, 200),
}
AT_EXTENT = ("q9-H63-ns50", "q9-H64-ns50")      # nq > the 7 planted rows: row 8 carries the plant of this file
EXTENT32 = float(np.float32(K.EXTENT))


def _plant_at_extent(c, row=8):
    """support r (positive features, no planted row leans on it) moves to q[row] + (float32(extent), 0, 0) with q[row] on
    dyadic coordinates: s - q is float32(extent) exactly, in float32 and in float64; kp[0] = 0"""
    nbr, H, ns = c["nbr"], c["H"], c["ns"]
    leaned = {0, 1, ns - 1}
    for r_, kind in c["plants"].items():
        leaned.update(int(v) for v in (nbr[r_, 0], nbr[r_, H - 1]) if 0 <= v < ns)
    r = next(i for i in range(ns) if i not in leaned and c["x"][i].astype(np.float64).sum() > 0)
    c["q"][row] = np.array([0.25, -0.5, 0.125], np.float32)
    c["s"][r] = c["q"][row] + np.array([np.float32(K.EXTENT), 0, 0], np.float32)
    nbr[row, 0] = r
    c["at_extent"] = (row, 0, r)


def _make():
    out = {}
    for name, (fact, seed, nq, H, ns) in _SPECS.items():
        c = K.build(name, fact, seed, CIN, H, nq, ns)
        if name in AT_EXTENT:
            _plant_at_extent(c)
        out[name] = c
    return out


CASES = _make()
END_TO_END = ("q9-H64-ns50", 128)      # KPConvFunction: case, cout


def args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


def facts():
    """which of the edges the issue names are reached, and where: {fact: [(case, query), ...]}"""
    hit = {"all_shadow": [], "on_kernel_point": [], "at_extent": [], "zero_sum_listed": [], "negative_sum_listed": [],
           "count_floor": []}
    for name, c in CASES.items():
        w, d, real, idx, _ = O.geometry(c["q"], c["s"], c["nbr"], c["kp"], c["extent"])
        _, raw = O.neighbour_count(c["nbr"], c["x"])
        sums = c["x"].astype(np.float64).sum(1)
        for qi in range(c["nq"]):
            if not real[qi].any():
                hit["all_shadow"].append((name, qi))
            if (w[qi] == 1.0).any():
                hit["on_kernel_point"].append((name, qi))
            if (real[qi][None, :] & (d[qi] == EXTENT32)).any():
                hit["at_extent"].append((name, qi))
            inside = real[qi] & (w[qi] > 0).any(0)
            if (inside & (sums[idx[qi]] == 0)).any():
                hit["zero_sum_listed"].append((name, qi))
            if (inside & (sums[idx[qi]] < 0)).any():
                hit["negative_sum_listed"].append((name, qi))
            if real[qi].any() and raw[qi] == 0:
                hit["count_floor"].append((name, qi))          # real neighbours, none counted: num = max(0, 1)
    return hit


FACTS = facts()
for _k, _v in FACTS.items():
    assert _v, f"no case reaches the edge '{_k}'"
for _c in CASES.values():
    assert K.features_are_decision_safe(_c["x"]), _c["name"]
    assert K.expected_route(CIN, _c["H"], "aligned") == "generic"      # what apr_kpconv_weighted itself does with these
for _n in AT_EXTENT:
    _row, _h, _r = CASES[_n]["at_extent"]
    _d = CASES[_n]["s"][_r].astype(np.float64) - CASES[_n]["q"][_row].astype(np.float64)
    assert _d[0] == EXTENT32 and _d[1] == 0 and _d[2] == 0

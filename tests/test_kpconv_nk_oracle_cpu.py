"""Host-side checks of the any-kernel-point-count KPConv tests: the K-general oracle (tests/kpconv_nk_oracle.py) against the
15-point oracles it restates, the cases' margins and coverage (tests/kpconv_nk_cases.py), a plain float32 NumPy evaluation
inside the bounds on EVERY row, the one-rule mutants outside them, and the refusals of apr_kpconv_weighted_nk /
apr_kpconv_dfeat_contrib_nk and of the one-call block (stand-in pointers: no device needed).

Worst float32 evaluation / bound over all cases (printed by test_print_worst_ratios): (linear, sum) 0.283, (linear, closest)
0.421, (constant, sum) 0.356, (constant, closest) 0.412, (gaussian, sum) 0.439, (gaussian, closest) 0.400.
"""
import ctypes as C

import numpy as np
import pytest

import kpconv_cases as KC
import kpconv_modes_cases as MC
import kpconv_modes_oracle as MO
import kpconv_nk_cases as NC
import kpconv_nk_oracle as NO
import kpconv_oracle as O

WORST = {}


def _args(c):
    return c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"]


# ------------------------------------------------------------------------------- the restatement against its sources
@pytest.mark.parametrize("name", ["m1-c64", "g-c1", "b-c68", "m4-c320"])
def test_k15_linear_sum_is_the_15_point_oracle(name):
    c = KC.ALL[name]
    a = _args(c)
    close = lambda x, y: np.allclose(x, y, rtol=1e-12, atol=1e-300)
    assert close(NO.weighted(*a)[0], O.weighted(*a)[0])
    assert close(NO.bound_weighted(*a), O.bound_weighted(*a))
    assert close(NO.contrib(*a, c["dwf"]), O.contrib(*a, c["dwf"]))
    assert close(NO.bound_contrib(*a, c["dwf"]), O.bound_contrib(*a, c["dwf"]))
    assert close(NO.d_x_from_dwf(*a, c["dwf"]), O.d_x_from_dwf(*a, c["dwf"]))
    assert close(NO.bound_dx(*a, c["dwf"]), O.bound_dx(*a, c["dwf"]))
    d_out = np.random.default_rng(3).standard_normal((c["nq"], 8))
    assert close(NO.d_W(*a, d_out), O.d_W(*a, d_out))


@pytest.mark.parametrize("mode", MO.MODES, ids=[MO.mode_name(m) for m in MO.MODES])
def test_k15_modes_are_the_modes_oracle(mode):
    c = MC.CASES["k-c64-H5-nq37"]
    a = _args(c)
    K = MO.rigid(c["kp"], c["nq"])
    b = (c["q"], c["s"], c["nbr"], c["x"], K, None, c["extent"])
    close = lambda x, y: np.allclose(x, y, rtol=1e-10, atol=1e-300)
    assert close(NO.weighted(*a, mode)[0], MO.weighted(*b, mode, False)[0])
    assert close(NO.bound_weighted(*a, mode), MO.bound_weighted(*b, mode, False))
    assert close(NO.contrib(*a, c["dwf"], mode), MO.contrib(*b, c["dwf"], mode, False))
    assert close(NO.bound_contrib(*a, c["dwf"], mode), MO.bound_contrib(*b, c["dwf"], mode, False))
    assert close(NO.bound_dx(*a, c["dwf"], mode), MO.bound_dx(*b, c["dwf"], mode, False))


def test_geometry_weighted_and_bound_of_the_15_point_oracle_are_general_in_k():
    """what kpconv_nk_oracle reuses as it is: at K = 7 and 20 they give the restated (linear, sum) statement"""
    for name in ("k7-c64-H5-nq70", "k20-c64-H5-nq70"):
        c = NC.CASES[name]
        a = _args(c)
        assert np.allclose(O.weighted(*a)[0], NO.weighted(*a)[0], rtol=1e-12, atol=1e-300)
        assert np.allclose(O.bound_weighted(*a), NO.bound_weighted(*a), rtol=1e-12, atol=1e-300)
        assert O.geometry(c["q"], c["s"], c["nbr"], c["kp"], c["extent"])[0].shape == (c["nq"], c["n_kp"], c["H"])


# ------------------------------------------------------------------------------------------------ cases and coverage
def test_cases_cover_the_parameters_and_routes():
    cs = list(NC.CASES.values())
    assert {c["n_kp"] for c in cs} == {1, 7, 15, 16, 17, 20, 32}
    assert {c["H"] for c in cs} >= {1, 3, 64, 65, 128}
    assert {c["nq"] for c in cs} == {1, 5, 70}
    mfma = [c for c in cs if NC.expected_route(c) != "generic"]
    gen = [c for c in cs if NC.expected_route(c) == "generic"]
    assert {c["cin"] for c in mfma} == {64, 128, 320}
    assert {c["cin"] for c in gen} == {1, 3, 32, 64} and any(c["layout"] == "slice1" for c in gen)
    assert {NC.expected_route(c) for c in mfma} == {"t1g1", "t1g2", "t1g4", "t2g1", "t2g2"}
    for K in (7, 20):      # both routes at the counts that run every mode
        assert {NC.expected_route(c) == "generic" for c in cs if c["n_kp"] == K} == {True, False}
    for K in (15,):
        assert {NC.expected_route(c) == "generic" for c in cs if c["n_kp"] == K} == {True, False}
    assert all(c["ns"] <= 200 for c in cs) and len(cs) <= 20


@pytest.mark.parametrize("name", list(NC.CASES))
def test_case_decides_with_a_margin_and_reaches_its_plants(name):
    c = NC.CASES[name]
    a = _args(c)
    geo = (c["q"], c["s"], c["nbr"], c["kp"], c["extent"])
    assert NO.edge_margin(*geo) >= NO.M_EDGE
    assert NO.closest_margin(*geo, c["exempt"]) >= NC.GAP
    assert KC.features_are_decision_safe(c["x"])
    real = O.real_mask(c["nbr"], c["ns"])
    wf, num, g = NO.weighted(*a)
    kinds = set()
    for row, kind in c["plants"].items():
        kinds.add(kind)
        if kind == "allpad":
            assert not real[row].any() and not wf[row].any() and num[row] == 1
        elif kind == "padkinds":
            vals = set(int(v) for v in c["nbr"][row][~real[row]])
            assert {c["ns"], -1, c["ns"] + 5}.issubset(vals) or c["H"] < 3
        elif kind == "dup":
            assert real[row].all() and len(set(c["nbr"][row])) == 1 and (c["H"] < 2 or num[row] == c["H"])
        elif kind == "far":
            assert c["nbr"][row, 0] == c["ns"] - 1 and not g["w"][row, :, 0].any() and g["w"][row, :, c["H"] - 1].any()
        elif kind == "tie":
            (r, h), = c["exempt"]
            assert r == row and g["cl"][row, h] == 3 and g["d2"][row, h, 3] == g["d2"][row, h, 19] == NC.TIE_D2
    if c["nq"] >= 5:
        assert {"allpad", "padkinds", "dup"} <= kinds and (c["n_kp"] < 20 or "tie" in kinds)
    if c["layout"] == "slice1":
        assert c["cin"] == 64


# --------------------------------------------------------------------------------- float32 evaluation and the mutants
@pytest.mark.parametrize("name", list(NC.CASES))
def test_float32_evaluation_is_inside_the_bounds_on_every_row(name):
    c = NC.CASES[name]
    a = _args(c)
    for mode in NC.case_modes(name):
        wf32, rows32 = NO.eval32(*a, c["dwf"], mode)
        ref_wf, ref_rows = NO.weighted(*a, mode)[0], NO.contrib(*a, c["dwf"], mode)
        bw, bc = NO.bound_weighted(*a, mode), NO.bound_contrib(*a, c["dwf"], mode)
        assert wf32.shape == ref_wf.shape == bw.shape == (c["nq"], c["n_kp"] * c["cin"])
        assert rows32.shape == ref_rows.shape == bc.shape == (c["nq"] * c["H"], c["cin"])      # no row is left out
        r1, at1 = NO.compare_rows(wf32, ref_wf, bw)
        r2, at2 = NO.compare_rows(rows32, ref_rows, bc)
        dx32 = O.scatter_rows(rows32.astype(np.float64), c["nbr"], c["ns"]).astype(np.float32)
        r3, at3 = NO.compare_rows(dx32, NO.d_x_from_dwf(*a, c["dwf"], mode), NO.bound_dx(*a, c["dwf"], mode))
        key = MO.mode_name(mode)
        WORST[key] = max(WORST.get(key, 0.0), r1, r2, r3)
        assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0, (name, mode, r1, at1, r2, at2, r3, at3)
        real = O.real_mask(c["nbr"], c["ns"]).reshape(-1)
        assert not ref_rows[~real].any() and not bc[~real].any()


def test_print_worst_ratios():
    print("worst float32 evaluation / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


MUTANT_CASES = {
    "tiles_swapped": [("k20-c64-H5-nq70", NO.DEFAULT), ("k17-c64-H1-nq1", NO.DEFAULT), ("k32-c128-H128-nq5", (2, 1))],
    "rows_ge16_dropped": [("k20-c64-H5-nq70", NO.DEFAULT), ("k17-c320-H3-nq5", NO.DEFAULT), ("k32-c64-H5-slice", (0, 0))],
    "stride_15cin": [("k7-c64-H5-nq70", NO.DEFAULT), ("k16-c128-H128-nq5", NO.DEFAULT), ("k20-c3-H65-nq5", (1, 1))],
    "tie_high": [("k20-c64-H5-nq70", (1, 1)), ("k20-c3-H65-nq5", (0, 1)), ("k32-c320-H64-nq5", (2, 1))],
}


@pytest.mark.parametrize("kind", NO.MUTANTS)
def test_mutant_is_rejected(kind):
    assert set(MUTANT_CASES) == set(NO.MUTANTS)
    for name, mode in MUTANT_CASES[kind]:
        c = NC.CASES[name]
        a = _args(c)
        wf32, rows32 = NO.eval32(*a, c["dwf"], mode, mutant=kind)
        r1, at1 = NO.compare_rows(wf32, NO.weighted(*a, mode)[0], NO.bound_weighted(*a, mode))
        r2, at2 = NO.compare_rows(rows32, NO.contrib(*a, c["dwf"], mode), NO.bound_contrib(*a, c["dwf"], mode))
        assert r1 > 1.0 and at1 is not None, (kind, name, "wf", r1)
        assert r2 > 1.0 and at2 is not None, (kind, name, "contrib", r2)


def test_identity_is_not_rejected():
    c = NC.CASES["k20-c64-H5-nq70"]
    a = _args(c)
    for mode in NO.MODES:
        wf = NO.weighted(*a, mode)[0]
        assert NO.compare_rows(wf, wf, NO.bound_weighted(*a, mode)) == (0.0, None)
        assert NO.compare_rows(wf.astype(np.float32), wf, NO.bound_weighted(*a, mode))[0] <= 1.0


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_entry_and_come_before_anything_is_read(lib):
    from apr_amd import _lib
    A = 0x10000      # stand-in pointers: every refusal comes before anything is read or launched

    def weighted(nq=5, ns=9, H=5, cin=64, ldx=64, n_kp=7, extent=1.2, ldwf=None, m=(1, 0), wf=A):
        return lib.apr_kpconv_weighted_nk(A, nq, A, ns, A, H, A, ldx, cin, A, n_kp, extent, A, wf,
                                          n_kp * cin if ldwf is None else ldwf, m[0], m[1], None)

    def contrib(nq=5, ns=9, H=5, cin=64, lddwf=None, n_kp=7, extent=1.2, m=(1, 0), out=A):
        return lib.apr_kpconv_dfeat_contrib_nk(A, nq, A, ns, A, H, A, n_kp * cin if lddwf is None else lddwf, cin, A, n_kp,
                                               extent, A, out, m[0], m[1], None)

    common = dict(nkp0=dict(n_kp=0), nkp33=dict(n_kp=33), nkp_negative=dict(n_kp=-1), influence3=dict(m=(3, 0)),
                  influence_negative=dict(m=(-1, 0)), closest2=dict(m=(1, 2)), closest_negative=dict(m=(2, -1)), H0=dict(H=0),
                  cin0=dict(cin=0, ldx=64), ns0=dict(ns=0), nq_negative=dict(nq=-1), extent0=dict(extent=0.0))
    for name, kw in {**common, "ldx_small": dict(ldx=60), "ldwf_small": dict(ldwf=7 * 64 - 1),
                     "ldwf_15_rows_at_20": dict(n_kp=20, ldwf=15 * 64)}.items():
        assert weighted(**kw) == -1, name                                   # APR_EINVAL
        assert b"apr_kpconv_weighted_nk" in lib.apr_last_error(), name
    for name, kw in {**common, "H129": dict(H=129), "cin513": dict(cin=513), "lddwf_small": dict(lddwf=7 * 64 - 1),
                     "null_contrib": dict(out=None)}.items():
        kw = {k: v for k, v in kw.items() if k != "ldx"}
        assert contrib(**kw) == -1, name
        assert b"apr_kpconv_dfeat_contrib_nk" in lib.apr_last_error(), name
    for n_kp in (1, 15, 32):
        assert weighted(nq=0, n_kp=n_kp) == 0 and contrib(nq=0, n_kp=n_kp) == 0      # nothing to do, nothing launched
    # the existing entries stay built for 15 kernel points
    assert lib.apr_kpconv_weighted_mode(A, 5, A, 9, A, 5, A, 64, 64, A, 14, 1.2, A, A, 14 * 64, 1, 0, None) == -1
    assert lib.apr_kpconv_dfeat_contrib_mode(A, 5, A, 9, A, 5, A, 14 * 64, 64, A, 14, 1.2, A, A, 1, 0, None) == -1
    # the one-call block: route 1 (the fused forward) with n_kp != 15 stays an argument error; the descriptor keeps its layout
    d = _lib.KpResnetDesc()
    d.x = d.q_pts = d.s_pts = d.nbr = d.w_kpconv = d.w_unary2 = d.kernel_points = d.out = d.scratch = d.w_unary1 = A
    d.ldx = d.ldo = 256
    d.n_in = d.n_out = 10
    d.in_dim, d.mid, d.out_dim, d.H, d.n_kp, d.extent, d.nseg = 256, 64, 256, 5, 7, 1.2, 1
    d.scratch_bytes = 1 << 30
    d.kpconv_route = 1
    assert lib.apr_kp_resnet_block(C.byref(d), None) == -1 and b"kpconv_route" in lib.apr_last_error()
    assert _lib.KpResnetDesc._fields_[-1][0] == "kpconv_route"
    d.kpconv_route = 0
    a7 = lib.apr_kp_resnet_scratch_bytes(C.byref(d))
    d.n_kp = 15
    assert 0 < a7 < lib.apr_kp_resnet_scratch_bytes(C.byref(d)), "the scratch walk does not follow n_kp"

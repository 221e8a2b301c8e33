"""Host-side checks of the any-kernel-point-count deformable KPConv tests: the K-general oracle
(tests/kpconv_deform_nk_oracle.py) against the 15-point modes oracle it restates (K = 15, all six modes, 1e-12) and against
the reference's own float64 results at K = 7 and 20 (tests/golden/kpconv_deform_nk_ref.npz, written by
tests/golden/make_kpconv_deform_nk_ref_golden.py), the cases' coverage and plants (tests/kpconv_deform_nk_cases.py), a plain
float32 NumPy evaluation inside the bounds on EVERY element, the one-rule mutants outside them, and the refusals of the three
apr_kpconv_deform_*_nk entry points (stand-in pointers: no device needed)."""
import os

import numpy as np
import pytest

import kpconv_deform_nk_cases as DNC
import kpconv_deform_nk_oracle as DNO
import kpconv_modes_cases as MC
import kpconv_modes_oracle as MO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kpconv_deform_nk_ref.npz")
WORST = {}


def _args(c, use_mod=True):
    return c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"] if use_mod else None, c["extent"]


# ------------------------------------------------------------------------------- the restatement against its sources
@pytest.mark.parametrize("mode", MO.MODES, ids=[MO.mode_name(m) for m in MO.MODES])
@pytest.mark.parametrize("name", ["k-c64-H5-nq37", "k-c64-H65-nq5"])
def test_k15_is_the_modes_oracle(name, mode):
    """every statement and every bound at K = 15 against tests/kpconv_modes_oracle.py on a deformed layer, 1e-12"""
    c = MC.CASES[name]
    a = _args(c)
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    close = lambda x, y: np.allclose(x, y, rtol=1e-12, atol=1e-300)
    assert close(DNO.weighted(*a, mode)[0], MO.weighted(*a, mode, True)[0])
    assert close(DNO.min_d2(*geo), MO.min_d2(*geo))
    assert close(DNO.contrib(*a, c["dwf"], mode), MO.contrib(*a, c["dwf"], mode, True))
    assert close(DNO.d_x(*a, c["dwf"], mode), MO.d_x(*a, c["dwf"], mode, True))
    for mine, theirs in zip(DNO.d_geom(*a, c["dwf"], mode), MO.d_geom(*a, c["dwf"], mode)):
        assert close(mine, theirs)
    d_out = np.random.default_rng(3).standard_normal((c["nq"], 8))
    assert close(DNO.d_W(*a, d_out, mode), MO.d_W(*a, d_out, mode, True))
    assert close(DNO.bound_weighted(*a, mode), MO.bound_weighted(*a, mode, True))
    assert close(DNO.bound_min_d2(*geo), MO.DO.bound_min_d2(*geo))
    assert close(DNO.bound_contrib(*a, c["dwf"], mode), MO.bound_contrib(*a, c["dwf"], mode, True))
    assert close(DNO.bound_dx(*a, c["dwf"], mode), MO.bound_dx(*a, c["dwf"], mode, True))
    for mine, theirs in zip(DNO.bound_d_geom(*a, c["dwf"], mode), MO.bound_d_geom(*a, c["dwf"], mode)):
        assert close(mine, theirs)


@pytest.mark.parametrize("mode", MO.MODES, ids=[MO.mode_name(m) for m in MO.MODES])
@pytest.mark.parametrize("modulated", [False, True])
def test_k15_chain_is_the_modes_oracle_chain(modulated, mode):
    c = MC.CASES["k-c64-H5-nq37"]
    W, W_off, b_off, d_out = MC.module_params(c, 64, modulated, mode)
    mine = DNO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, W_off, b_off, modulated, mode, d_out=d_out)
    theirs = MO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, mode, d_out=d_out, W_off=W_off, b_off=b_off,
                      modulated=modulated)
    for k in ("out", "min_d2", "deformed_KP", "offset_features", "d_x", "d_W", "d_W_off", "d_b_off", "d_dkp", "d_mod"):
        assert np.allclose(mine[k], theirs[k], rtol=1e-12, atol=1e-14 * max(1.0, np.abs(theirs[k]).max())), k


@pytest.mark.parametrize("m", [0, 1])
@pytest.mark.parametrize("tag", ["k7_center", "k20_none"])
def test_oracle_reproduces_the_reference_in_float64(tag, m):
    """the reference's KPConv(K, 3, 8, 8, 1.2, 1.5, fixed, deformable=True, modulated) cast to float64: out, min_d2,
    deformed_KP, offset_features and all four gradients at 1e-12"""
    gold = np.load(GOLD)
    i = {k: gold[f"in/{k}"] for k in ("q", "s", "nbr", "x", "G", "bias")}
    p = f"{tag}/m{m}"
    sd = {k[len(f"{p}/sd/"):]: gold[k] for k in gold.files if k.startswith(f"{p}/sd/")}
    K = int(tag[1:].split("_")[0])
    assert sd["kernel_points"].shape == (K, 3) and sd["weights"].shape == (K, 8, 8)
    od = (4 if m else 3) * K
    assert sd["offset_conv.weights"].shape == (K, 8, od)
    r = DNO.chain(i["q"], i["s"], i["nbr"], i["x"], sd["kernel_points"], 1.2, sd["weights"], sd["offset_conv.weights"],
                  i["bias"][:od], bool(m), d_out=i["G"], kp_off=sd["offset_conv.kernel_points"])
    pairs = dict(out="out", min_d2="min_d2", deformed_KP="deformed_KP", offset_features="offset_features", d_x="d_x",
                 d_W="d_weights", d_W_off="d_offset_conv_weights", d_b_off="d_offset_bias")
    for mine, theirs in pairs.items():
        ref = gold[f"{p}/{theirs}"]
        assert ref.dtype == np.float64 and ref.shape == r[mine].shape, mine
        scale = max(1.0, float(np.abs(ref).max()))
        err = np.abs(r[mine] - ref)
        if mine == "min_d2":                      # the padding row holds 3e12 next to rows below 1: per element, relative
            err, scale = err / np.maximum(1.0, np.abs(ref)), 1.0
        print(f"{p} {mine}: max err {err.max():.3g} (scale {scale:.3g})")
        assert err.max() <= 1e-12 * scale, (mine, err.max())
    assert not gold[f"{p}/out"][3].any() and not r["out"][3].any()       # nothing in range: an all-zero row
    assert (gold[f"{p}/min_d2"][3] > 1e11).all()                         # from the padding point


# ------------------------------------------------------------------------------------------------ cases and coverage
def test_cases_cover_the_parameters_and_routes():
    cs = list(DNC.CASES.values())
    assert {c["n_kp"] for c in cs} == {1, 7, 15, 16, 17, 20, 32}
    assert {c["H"] for c in cs} == {1, 3, 5, 64, 65, 128}
    assert {c["cin"] for c in cs} == {64, 128, 320, 512}
    assert {c["nq"] for c in cs} == {1, 5, 70}
    routes = [DNC.expected_route(c) for c in cs]
    assert {r[0] for r in routes} == {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2)}
    assert {r[1] for r in routes} == {(1, 16), (2, 16), (8, 16), (1, 32), (2, 32), (4, 32)}
    assert {c["cin"] for c in cs if c["n_kp"] > 16} >= {320, 512}      # a second channel pass of both two-tile kernels
    assert all(c["ns"] <= 200 for c in cs) and len(cs) <= 16
    for K in (7, 15, 20):
        assert any(c["n_kp"] == K and c["nq"] == 70 for c in cs)       # every mode meets every plant


def test_planted_rows_reach_their_edges():
    c = DNC.CASES["dk20-c64-H5-nq70"]
    assert set(c["plants"].values()) == set(DNC.PLANTS)
    row = {v: k for k, v in c["plants"].items()}
    a = _args(c)
    wf, num, g = DNO.weighted(*a)
    _, raw = DNO.count(g, c["x"])
    md = DNO.min_d2(c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    inr = g["d2"] < c["extent"] ** 2
    r = row["allpad"]
    assert not g["real"][r].any() and not wf[r].any() and raw[r] == 0 and num[r] == 1 and (md[r] > 1e11).all()
    r = row["padkinds"]
    assert list(c["nbr"][r, :3]) == [c["ns"], -1, c["ns"] + 5] and not g["real"][r, :3].any()
    r = row["deform_only"]
    assert wf[r].any() and raw[r] == 1 and list(np.nonzero(inr[r, c["H"] - 1])[0]) == [3]
    r = row["rigid_only"]
    assert raw[r] == 1 and not g["in_range"][r, c["H"] - 1] and g["real"][r].sum() == 2
    r = row["none"]
    assert g["real"][r].all() and not g["in_range"][r].any() and not wf[r].any() and num[r] == 1 and (md[r] < 1e5).all()
    r = row["floor"]
    assert raw[r] == 0 and g["in_range"][r].sum() == 2 and wf[r].any()
    r = row["dup"]
    assert len(set(c["nbr"][r])) == 1 and g["real"][r].all()
    r = row["mod02"]
    assert c["mod"][r, 2] == 0 and c["mod"][r, 5] == 2 and not wf[r].reshape(20, -1)[2].any()
    r = row["mod0_only"]
    assert raw[r] == 2 and list(np.nonzero(inr[r, 0])[0]) == [2] and c["mod"][r, 2] == 0
    r = row["zero_off"]
    assert np.array_equal(c["dkp"][r], c["kp"]) and (c["mod"][r] == 1).all()
    r = row["high_only"]
    assert raw[r] == 2 and list(np.nonzero(inr[r, 0])[0]) == [17] and inr[r, c["H"] - 1, :16].any()
    r = row["tie"]
    (rr, h), = c["exempt"]
    assert rr == r and g["cl"][r, h] == 3 and g["d2"][r, h, 3] == g["d2"][r, h, 19] == DNC.TIE_D2 and g["in_range"][r, h]
    r = row["min_high"]
    assert np.unravel_index(np.argmin(g["d2"][r]), g["d2"][r].shape)[1] == 19 and md[r].argmin() == 19
    for name in DNC.CASES:
        if DNC.CASES[name]["n_kp"] >= 20 and DNC.CASES[name]["nq"] >= 5:
            assert set(DNC.HIGH_PLANTS) <= set(DNC.CASES[name]["plants"].values()), name


# --------------------------------------------------------------------------------- float32 evaluation and the mutants
def ratios(c, got, mode, use_mod=True):
    """-> {quantity: (worst |got - oracle| / bound, where)} over EVERY element"""
    a = _args(c, use_mod)
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    ref_dd, ref_dm = DNO.d_geom(*a, c["dwf"], mode)
    bd, bm = DNO.bound_d_geom(*a, c["dwf"], mode)
    n = len(bd)
    table = dict(wf=(got["wf"], DNO.weighted(*a, mode)[0], DNO.bound_weighted(*a, mode)),
                 min_d2=(got["min_d2"], DNO.min_d2(*geo), DNO.bound_min_d2(*geo)),
                 contrib=(got["contrib"], DNO.contrib(*a, c["dwf"], mode), DNO.bound_contrib(*a, c["dwf"], mode)),
                 d_mod=(got["d_mod"], ref_dm, bm),
                 d_dkp=(got["d_dkp"].reshape(n, -1), ref_dd.reshape(n, -1), bd.reshape(n, -1)))
    out = {}
    for k, (g, r, b) in table.items():
        assert g.shape == r.shape == b.shape, (c["name"], k, g.shape, r.shape, b.shape)
        out[k] = DNO.compare_rows(g, r, b)
    return out


@pytest.mark.parametrize("name", list(DNC.CASES))
def test_float32_evaluation_is_inside_the_bounds_on_every_element(name):
    c = DNC.CASES[name]
    for mode in DNC.case_modes(name):
        for use_mod in (True, False):
            got = DNO.eval32(*_args(c, use_mod), c["dwf"], mode)
            res = ratios(c, got, mode, use_mod)
            key = MO.mode_name(mode)
            WORST[key] = max(WORST.get(key, 0.0), max(v[0] for v in res.values()))
            assert all(v[0] <= 1.0 for v in res.values()), (name, mode, use_mod, res)
            if mode[0] == DNO.CONSTANT:
                assert not got["d_dkp"].any()


def test_print_worst_ratios():
    print("worst float32 evaluation / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())


# mutant -> [(case, mode, the quantity it shows in)]
MUTANT_CASES = {
    "inrange_tile0_only": [("dk20-c64-H5-nq70", DNO.DEFAULT, "wf"), ("dk20-c64-H5-nq70", (2, 0), "wf"),
                           ("dk32-c128-H128-nq5", DNO.DEFAULT, "contrib")],
    "min_rows_ge16_dropped": [("dk17-c64-H1-nq1", DNO.DEFAULT, "min_d2"), ("dk20-c64-H5-nq70", DNO.DEFAULT, "min_d2"),
                              ("dk32-c320-H64-nq5", DNO.DEFAULT, "min_d2")],
    "mod_stride_15": [("dk7-c64-H5-nq70", DNO.DEFAULT, "wf"), ("dk16-c128-H128-nq5", DNO.DEFAULT, "contrib"),
                      ("dk20-c128-H65-nq5", (2, 1), "d_dkp")],
    "tiles_swapped": [("dk20-c64-H5-nq70", DNO.DEFAULT, "wf"), ("dk17-c64-H1-nq1", DNO.DEFAULT, "wf"),
                      ("dk32-c128-H128-nq5", (2, 1), "d_mod")],
    "tie_high": [("dk20-c64-H5-nq70", (1, 1), "wf"), ("dk20-c128-H65-nq5", (0, 1), "contrib"),
                 ("dk32-c320-H64-nq5", (2, 1), "d_dkp")],
    "count_rigid": [("dk7-c64-H5-nq70", DNO.DEFAULT, "wf"), ("dk20-c64-H5-nq70", (2, 1), "contrib"),
                    ("dk15-c64-H5-nq70", DNO.DEFAULT, "d_mod")],
}


@pytest.mark.parametrize("kind", DNO.MUTANTS)
def test_mutant_is_rejected(kind):
    assert set(MUTANT_CASES) == set(DNO.MUTANTS)
    for name, mode, what in MUTANT_CASES[kind]:
        c = DNC.CASES[name]
        res = ratios(c, DNO.eval32(*_args(c), c["dwf"], mode, mutant=kind), mode)
        print(kind, name, mode, {k: round(v[0], 3) for k, v in res.items()})
        assert res[what][0] > 1.0 and res[what][1] is not None, (kind, name, mode, what, res[what])


def test_identity_is_not_rejected():
    c = DNC.CASES["dk20-c64-H5-nq70"]
    for mode in DNO.MODES:
        wf = DNO.weighted(*_args(c), mode)[0]
        assert DNO.compare_rows(wf, wf, DNO.bound_weighted(*_args(c), mode)) == (0.0, None)


@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("name,cout", DNC.MODULE)
def test_module_cases_keep_their_margin(name, cout, modulated):
    c = DNC.CASES[name]
    W, W_off, b_off, d_out = DNC.module_params(c, cout, modulated)
    r = DNO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, W_off, b_off, modulated, d_out=d_out)
    moved = np.linalg.norm(r["deformed_KP"] - c["kp"][None], axis=-1)
    assert moved.max() > 0.05 and np.isfinite(r["d_W_off"]).all() and np.abs(r["d_W_off"]).max() > 0
    assert r["offset_features"].shape[1] == (4 if modulated else 3) * c["n_kp"]
    if modulated:
        assert np.ptp(r["mod"]) > 0.05


# ---------------------------------------------------------------------------------------------------------- refusals
REFUSED = DNC.REFUSED


def refusal_calls(lib, A=0x10000):
    """the three entries with stand-in arguments -> {tag: fn(**overrides)}; shared with the GPU refusal test"""

    def weighted(nq=5, ns=9, H=5, x=A, ldx=64, cin=64, n_kp=7, extent=1.2, wf=A, ldwf=None, m=(1, 0), bufs=None):
        p = bufs or {}
        return lib.apr_kpconv_deform_weighted_nk(p.get("q", A), nq, p.get("s", A), ns, p.get("nbr", A), H, p.get("x", x), ldx,
                                                 cin, p.get("dkp", A), p.get("mod", A), n_kp, extent, p.get("rs", A),
                                                 p.get("wf", wf), n_kp * cin if ldwf is None else ldwf, p.get("md", A), m[0],
                                                 m[1], None)

    def contrib(nq=5, ns=9, H=5, dwf=A, lddwf=None, cin=64, n_kp=7, extent=1.2, out=A, m=(1, 0), bufs=None, **_):
        p = bufs or {}
        return lib.apr_kpconv_deform_dfeat_contrib_nk(p.get("q", A), nq, p.get("s", A), ns, p.get("nbr", A), H, p.get("dwf", dwf),
                                                      n_kp * cin if lddwf is None else lddwf, cin, p.get("dkp", A),
                                                      p.get("mod", A), n_kp, extent, p.get("rs", A), p.get("contrib", out), m[0],
                                                      m[1], None)

    def dgeom(nq=5, ns=9, H=5, x=A, ldx=64, cin=64, dwf=A, lddwf=None, n_kp=7, extent=1.2, d_dkp=A, m=(1, 0), bufs=None):
        p = bufs or {}
        return lib.apr_kpconv_deform_dgeom_nk(p.get("q", A), nq, p.get("s", A), ns, p.get("nbr", A), H, p.get("x", x), ldx, cin,
                                              p.get("dwf", dwf), n_kp * cin if lddwf is None else lddwf, p.get("dkp", A),
                                              p.get("mod", A), n_kp, extent, p.get("rs", A), p.get("d_dkp", d_dkp),
                                              p.get("d_mod", A), m[0], m[1], None)

    return {b"apr_kpconv_deform_weighted_nk": weighted, b"apr_kpconv_deform_dfeat_contrib_nk": contrib,
            b"apr_kpconv_deform_dgeom_nk": dgeom}


def test_refusals_come_before_anything_is_read(lib):
    A = 0x10000      # stand-in pointers: every refusal comes before anything is read or launched
    calls = refusal_calls(lib, A)
    weighted, contrib, dgeom = calls.values()
    for tag, fn in calls.items():
        for name, kw in REFUSED.items():
            kw = dict(kw)
            if "cin" in kw and fn is not contrib:
                kw["ldx"] = max(64, (kw["cin"] + 3) // 4 * 4)
            assert fn(**kw) == -1, (tag, name)                             # APR_EINVAL
            assert tag in lib.apr_last_error(), (tag, name)
        for n_kp in (1, 15, 32):
            assert fn(nq=0, n_kp=n_kp) == 0                                # nothing to do, nothing launched
    for name, kw in dict(ldx_small=dict(ldx=60), ldx_odd=dict(ldx=66), x_misaligned=dict(x=A + 4), x_null=dict(x=None)).items():
        assert weighted(**kw) == -1 and dgeom(**kw) == -1, name
    for kw in (dict(ldwf=7 * 64 - 4), dict(ldwf=7 * 64 + 2), dict(wf=A + 8), dict(wf=None), dict(n_kp=20, ldwf=15 * 64)):
        assert weighted(**kw) == -1, kw
    for kw in (dict(lddwf=7 * 64 - 4), dict(dwf=None), dict(n_kp=20, lddwf=15 * 64)):
        assert contrib(**kw) == -1 and dgeom(**kw) == -1, kw
    assert contrib(out=None) == -1 and dgeom(d_dkp=None) == -1 and dgeom(dwf=A + 4) == -1 and dgeom(lddwf=7 * 64 + 2) == -1
    # the existing entries stay built for 15 kernel points
    assert lib.apr_kpconv_deform_weighted_mode(A, 5, A, 9, A, 5, A, 64, 64, A, A, 14, 1.2, A, A, 14 * 64, A, 1, 0, None) == -1

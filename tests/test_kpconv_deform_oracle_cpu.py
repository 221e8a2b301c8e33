"""Host-side checks of the deformable KPConv: the float64 oracle (tests/kpconv_deform_oracle.py) against the reference's
own float64 results (tests/golden/kpconv_deform_ref.npz, written by tests/golden/make_kpconv_deform_ref_golden.py), a plain
float32 restatement inside every bound, the mutants of the oracle each rejected at the bound by a named case, the module's
construction under the reference's seeds, block_decider, and the refusals of the three entry points (no device needed)."""
import os

import numpy as np
import pytest
import torch

import kpconv_deform_cases as DC
import kpconv_deform_oracle as DO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kpconv_deform_ref.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("m", [0, 1])
def test_oracle_reproduces_the_reference_in_float64(gold, m):
    """out, min_d2, deformed_KP, offset_features and all four gradients at 1e-12 (every reference statement ran)."""
    i = {k: gold[f"in/{k}"] for k in ("q", "s", "nbr", "x", "G", "bias")}
    sd = {k[len(f"m{m}/sd/"):]: gold[k] for k in gold.files if k.startswith(f"m{m}/sd/")}
    od = 60 if m else 45
    r = DO.chain(i["q"], i["s"], i["nbr"], i["x"], sd["kernel_points"], 1.2, sd["weights"], sd["offset_conv.weights"],
                 i["bias"][:od], bool(m), d_out=i["G"], kp_off=sd["offset_conv.kernel_points"])
    assert not np.array_equal(sd["kernel_points"], sd["offset_conv.kernel_points"])      # each draws its own rotation
    pairs = dict(out="out", min_d2="min_d2", deformed_KP="deformed_KP", offset_features="offset_features", d_x="d_x",
                 d_W="d_weights", d_W_off="d_offset_conv_weights", d_b_off="d_offset_bias")
    for mine, theirs in pairs.items():
        ref = gold[f"m{m}/{theirs}"]
        assert ref.dtype == np.float64 and ref.shape == r[mine].shape, mine
        scale = max(1.0, float(np.abs(ref).max()))
        err = np.abs(r[mine] - ref)
        if mine == "min_d2":                      # the padding row holds 3e12 next to rows below 1: per element, relative
            err, scale = err / np.maximum(1.0, np.abs(ref)), 1.0
        print(f"m{m} {mine}: max err {err.max():.3g} (scale {scale:.3g})")
        assert err.max() <= 1e-12 * scale, (mine, err.max())
    assert not gold[f"m{m}/out"][3].any() and not r["out"][3].any()       # nothing in range: an all-zero row
    assert (gold[f"m{m}/min_d2"][3] > 1e11).all()                         # from the padding point


# ------------------------------------------------------------------------------------------- float32 restatement
def f32_restatement(c, use_mod=True):
    """the contract in plain float32 numpy, one rounding per operation, sums in numpy's order"""
    q, s, nbr, x, dkp, dwf = c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["dwf"]
    mod = c["mod"] if use_mod else np.ones_like(c["mod"])
    ns, ext = len(s), F32(c["extent"])
    nq, H = nbr.shape
    real = (nbr >= 0) & (nbr < ns)
    idx = np.where(real, nbr, 0)
    D = (np.where(real[:, :, None], s[idx], F32(1e6)) - q[:, None, :]).astype(F32)
    diff = (D[:, :, None, :] - dkp[:, None, :, :]).astype(F32)
    d2 = ((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]).astype(F32)
    d = np.sqrt(d2).astype(F32)
    w = (np.maximum(F32(0), F32(1) - d * (F32(1) / ext)) * real[:, :, None]).astype(F32)            # [nq, H, 15]
    in_range = real & (d2 < ext * ext).any(-1)
    rs = x.sum(1, dtype=F32)
    num = np.maximum((in_range & (rs[idx] > 0)).sum(1), 1).astype(F32)
    inv = (F32(1) / num).astype(F32)
    xg = (x[idx] * real[:, :, None]).astype(F32)
    f = (mod * inv[:, None]).astype(F32)
    wf = (np.einsum("qhk,qhc->qkc", w, xg).astype(F32) * f[:, :, None]).astype(F32).reshape(nq, -1)
    g = (dwf.reshape(nq, 15, -1) * f[:, :, None]).astype(F32)
    contrib = np.einsum("qhk,qkc->qhc", w, g).astype(F32).reshape(nq * H, -1)
    P = np.einsum("qhc,qkc->qhk", xg, dwf.reshape(nq, 15, -1)).astype(F32)
    dm = ((w * P).sum(1, dtype=F32) * inv[:, None]).astype(F32)
    live = real[:, :, None] & (w > 0) & (d > 0)
    coef = np.where(live, P / np.where(live, d * ext, F32(1)), F32(0)).astype(F32)
    dd = ((diff * coef[..., None]).sum(1, dtype=F32) * f[:, :, None]).astype(F32)
    return dict(wf=wf, min_d2=d2.min(1), contrib=contrib, d_mod=dm, d_dkp=dd, real=real)


def check_against_bounds(c, got, use_mod=True):
    """-> {quantity: worst |err| / bound}; asserts each <= 1"""
    a = (c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"] if use_mod else None, c["extent"])
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    ref_dd, ref_dm = DO.d_geom(*a, c["dwf"])
    bd, bm = DO.bound_d_geom(*a, c["dwf"])
    real = got["real"].reshape(-1)
    table = dict(wf=(got["wf"], DO.weighted(*a)[0], DO.bound_weighted(*a)),
                 min_d2=(got["min_d2"], DO.min_d2(*geo), DO.bound_min_d2(*geo)),
                 contrib=(got["contrib"][real], DO.contrib(*a, c["dwf"])[real], DO.bound_contrib(*a, c["dwf"])[real]),
                 d_mod=(got["d_mod"], ref_dm, bm),
                 d_dkp=(got["d_dkp"].reshape(len(bd), -1), ref_dd.reshape(len(bd), -1), bd.reshape(len(bd), -1)))
    worst = {}
    for name, (g, r, b) in table.items():
        worst[name], at = DO.compare_rows(g, r, b)
        assert worst[name] <= 1.0, (c["name"], name, worst[name], at)
    return worst


@pytest.mark.parametrize("name", list(DC.CASES))
def test_float32_restatement_stays_inside_every_bound(name):
    c = DC.CASES[name]
    worst = check_against_bounds(c, f32_restatement(c))
    print(name, {k: round(v, 3) for k, v in worst.items()})


def test_planted_rows_reach_their_edges():
    c = DC.CASES["d-c64-H5"]
    assert set(c["plants"].values()) == set(DC.PLANTS)
    row = {v: k for k, v in c["plants"].items()}
    a = (c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"], c["extent"])
    wf, S, num, g = DO.weighted(*a)
    _, raw = DO.count(g, c["x"])
    rigid = DO.O.geometry(c["q"], c["s"], c["nbr"], c["kp"], c["extent"])[0]               # w [nq, 15, H]
    md = DO.min_d2(c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    r = row["allpad"]
    assert not g["real"][r].any() and not wf[r].any() and raw[r] == 0 and num[r] == 1 and (md[r] > 1e11).all()
    r = row["padkinds"]
    assert list(c["nbr"][r, :3]) == [c["ns"], -1, c["ns"] + 5] and not g["real"][r, :3].any()
    r = row["deform_only"]
    assert wf[r].any() and not rigid[r].any() and raw[r] == 1
    r = row["rigid_only"]
    assert raw[r] == 1 and rigid[r, :, c["H"] - 1].any() and not g["in_range"][r, c["H"] - 1] and g["real"][r].sum() == 2
    r = row["none"]
    assert g["real"][r].all() and not g["in_range"][r].any() and not wf[r].any() and num[r] == 1 and (md[r] < 1e5).all()
    r = row["floor"]
    assert raw[r] == 0 and g["in_range"][r].sum() == 2 and wf[r].any()
    r = row["dup"]
    assert len(set(c["nbr"][r])) == 1 and g["real"][r].all()
    r = row["mod02"]
    assert c["mod"][r, 2] == 0 and c["mod"][r, 5] == 2 and not wf[r].reshape(15, -1)[2].any()
    r = row["mod0_only"]
    inr = g["d2"][r] < c["extent"] ** 2
    assert raw[r] == 2 and list(np.nonzero(inr[0])[0]) == [2] and c["mod"][r, 2] == 0
    r = row["zero_off"]
    assert np.array_equal(c["dkp"][r], c["kp"]) and (c["mod"][r] == 1).all()
    assert (raw != DO.count(g, c["x"], mutant="rigid_count")[1]).sum() >= 3


# mutant -> (the case that rejects it, the quantity it shows in)
REJECTED_BY = {"rigid_count": ("d-c64-H5", "wf"), "count_no_sum": ("d-c64-H5", "wf"), "min_no_pad": ("d-c64-H5", "min_d2"),
               "no_mod": ("d-c64-H5", "wf"), "mod_before_count": ("d-c64-H5", "wf"), "offsets_unscaled": ("d-c64-H5", "wf"),
               "ddkp_sign": ("d-c64-H5", "d_dkp"), "ddkp_no_num": ("d-c64-H5", "d_dkp"), "ddkp_no_mod": ("d-c64-H5", "d_dkp"),
               "drop_k14": ("d-c64-H5", "wf"), "drop_h64": ("d-c64-H65-nq67", "wf")}


@pytest.mark.parametrize("mutant", DO.MUTANTS)
def test_mutants_of_the_oracle_are_rejected_at_the_bound(mutant):
    name, what = REJECTED_BY[mutant]
    c = DC.CASES[name]
    a = [c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"], c["extent"]]
    m = list(a)
    if mutant == "offsets_unscaled":
        offsets = (c["dkp"].astype(np.float64) - c["kp"]) / c["extent"]
        assert np.abs(DO.deformed_points(c["kp"], offsets, c["extent"]) - c["dkp"]).max() < 1e-12
        m[4] = DO.deformed_points(c["kp"], offsets, c["extent"], mutant)
    if what == "wf":
        got, ref, b = DO.weighted(*m, mutant=mutant)[0], DO.weighted(*a)[0], DO.bound_weighted(*a)
    elif what == "min_d2":
        geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
        got, ref, b = DO.min_d2(*geo, mutant=mutant), DO.min_d2(*geo), DO.bound_min_d2(*geo)
        got = np.where(np.isfinite(got), got, 0.0)
    else:
        got, ref, b = DO.d_geom(*m, c["dwf"], mutant=mutant)[0], DO.d_geom(*a, c["dwf"])[0], DO.bound_d_geom(*a, c["dwf"])[0]
        got, ref, b = (v.reshape(len(v), -1) for v in (got, ref, b))
    ratio, at = DO.compare_rows(got, ref, b)
    print(mutant, name, what, ratio, at)
    assert ratio > 1.0 and at is not None


# ------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("m", [0, 1])
def test_module_construction_under_the_reference_seeds(gold, m):
    from apr_amd.predator.models import blocks
    sd_ref = {k[len(f"m{m}/sd/"):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(f"m{m}/sd/")}
    np.random.seed(1)
    torch.manual_seed(1)
    conv = blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, deformable=True, modulated=bool(m))
    sd = conv.state_dict()
    assert sorted(sd) == sorted(["weights", "kernel_points", "offset_bias", "offset_conv.weights", "offset_conv.kernel_points"])
    assert list(sd) == list(sd_ref)
    assert conv.offset_dim == (60 if m else 45) and tuple(sd["offset_conv.weights"].shape) == (15, 8, conv.offset_dim)
    for k in sd:
        assert sd[k].shape == sd_ref[k].shape and torch.equal(sd[k], sd_ref[k]), k
    assert not conv.kernel_points.requires_grad and conv.offset_bias.requires_grad and not sd["offset_bias"].any()
    torch.manual_seed(99)
    other = blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, deformable=True, modulated=bool(m))
    assert not torch.equal(other.weights, sd_ref["weights"])
    other.load_state_dict(sd_ref, strict=True)
    assert torch.equal(other.weights, sd_ref["weights"]) and torch.equal(other.offset_conv.weights, sd_ref["offset_conv.weights"])
    assert conv.min_d2 is None and conv.deformed_KP is None and conv.offset_features is None


def test_modulated_rigid_builds_and_other_settings_raise():
    from apr_amd.predator.models import blocks
    conv = blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, modulated=True)
    assert conv.offset_conv is None and conv.offset_bias is None and conv.offset_dim is None
    assert sorted(conv.state_dict()) == ["kernel_points", "weights"]
    for kw in (dict(KP_influence="gaussian"), dict(KP_influence="constant"), dict(aggregation_mode="closest")):
        for deformable in (False, True):
            with pytest.raises(NotImplementedError):
                blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, deformable=deformable, **kw)


@pytest.mark.parametrize("modulated", [False, True])
def test_block_decider_returns_the_four_deformable_blocks(modulated):
    from apr_amd.predator.configs.models import kitti_config
    from apr_amd.predator.models import blocks
    cfg = kitti_config(modulated=modulated)
    want = dict(simple_deformable=blocks.SimpleBlock, simple_deformable_strided=blocks.SimpleBlock,
                resnetb_deformable=blocks.ResnetBottleneckBlock, resnetb_deformable_strided=blocks.ResnetBottleneckBlock)
    for name, cls in want.items():
        b = blocks.block_decider(name, 2.5, 64, 128, 1, cfg)
        assert type(b) is cls and b.KPConv.deformable and b.KPConv.modulated == modulated
        assert b.KPConv.offset_conv is not None and not b.KPConv.offset_conv.deformable
        assert b.KPConv.offset_dim == (60 if modulated else 45)
        if cls is blocks.ResnetBottleneckBlock:
            assert not b._fused_ok(torch.zeros(4, 64), torch.zeros(4, 3, dtype=torch.int32))
        assert not b.KPConv._fused_route(100, 20, True)
    rigid = blocks.block_decider("resnetb", 2.5, 64, 128, 1, cfg)
    assert not rigid.KPConv.deformable and rigid.KPConv.offset_conv is None
    with pytest.raises(NotImplementedError):
        blocks.block_decider("resnetb_invariant", 2.5, 64, 128, 1, cfg)


def test_refusals_come_before_anything_is_read(lib):
    A = 0x10000      # stand-in pointers: every refusal comes before anything is read or launched

    def weighted(nq=5, ns=9, H=5, x=A, ldx=64, cin=64, n_kp=15, extent=1.2, wf=A, ldwf=960):
        return lib.apr_kpconv_deform_weighted(A, nq, A, ns, A, H, x, ldx, cin, A, A, n_kp, extent, A, wf, ldwf, A, None)

    def contrib(nq=5, ns=9, H=5, dwf=A, lddwf=960, cin=64, n_kp=15, extent=1.2, out=A):
        return lib.apr_kpconv_deform_dfeat_contrib(A, nq, A, ns, A, H, dwf, lddwf, cin, A, A, n_kp, extent, A, out, None)

    def dgeom(nq=5, ns=9, H=5, x=A, ldx=64, cin=64, dwf=A, lddwf=960, n_kp=15, extent=1.2, d_dkp=A):
        return lib.apr_kpconv_deform_dgeom(A, nq, A, ns, A, H, x, ldx, cin, dwf, lddwf, A, A, n_kp, extent, A, d_dkp, A, None)

    for fn, tag in ((weighted, b"apr_kpconv_deform_weighted"), (contrib, b"apr_kpconv_deform_dfeat_contrib"),
                    (dgeom, b"apr_kpconv_deform_dgeom")):
        for name, kw in DC.REFUSED.items():
            kw = dict(kw)
            if "cin" in kw and fn is not contrib:
                kw["ldx"] = max(64, (kw["cin"] + 3) // 4 * 4)
            assert fn(**kw) == -1, (tag, name)                             # APR_EINVAL
            assert tag in lib.apr_last_error(), (tag, name)
        assert fn(nq=0) == 0                                               # nothing to do, nothing launched
    for name, kw in dict(ldx_small=dict(ldx=60), ldx_odd=dict(ldx=66), x_misaligned=dict(x=A + 4), x_null=dict(x=None)).items():
        assert weighted(**kw) == -1 and dgeom(**kw) == -1, name
    for kw in (dict(ldwf=956), dict(ldwf=962), dict(wf=A + 8), dict(wf=None)):
        assert weighted(**kw) == -1, kw
    for kw in (dict(lddwf=956), dict(dwf=None)):
        assert contrib(**kw) == -1 and dgeom(**kw) == -1, kw
    assert contrib(out=None) == -1 and dgeom(d_dkp=None) == -1 and dgeom(dwf=A + 4) == -1 and dgeom(lddwf=962) == -1


@pytest.mark.parametrize("modulated", [False, True])
@pytest.mark.parametrize("name,cout", DC.MODULE)
def test_module_cases_keep_their_margin(name, cout, modulated):
    """the offset weights of the module cases exist (tests/kpconv_deform_cases.py:module_params finds a draw whose chain keeps
    every neighbour's nearest deformed point off the edge), and the chain moves the kernel points and the modulations"""
    c = DC.CASES[name]
    W, W_off, b_off, d_out = DC.module_params(c, cout, modulated)
    r = DO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, W_off, b_off, modulated, d_out=d_out)
    moved = np.linalg.norm(r["deformed_KP"] - c["kp"][None], axis=-1)
    assert moved.max() > 0.05 and np.isfinite(r["d_W_off"]).all() and np.abs(r["d_W_off"]).max() > 0
    if modulated:
        assert np.ptp(r["mod"]) > 0.05

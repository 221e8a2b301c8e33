"""KPConv's influence / aggregation modes without a GPU: the float64 oracle (tests/kpconv_modes_oracle.py) against the
reference's own outputs (tests/golden/kpconv_modes_ref.npz), the module's constructor and parameters, its torch formulation
on the CPU against the same fixture, the refusals of the five *_mode entry points, and the mutants that show the oracle's
bounds have teeth on the cases of tests/kpconv_modes_cases.py."""
import os

import numpy as np
import pytest
import torch

import kpconv_modes_cases as MC
import kpconv_modes_oracle as MO
from apr_amd.predator import kp_ops

GOLD = os.path.join(os.path.dirname(__file__), "golden", "kpconv_modes_ref.npz")
PAIRS = [("constant", "sum"), ("constant", "closest"), ("linear", "closest"), ("gaussian", "sum"), ("gaussian", "closest")]
KINDS = {"r": (False, False), "d": (True, False), "dm": (True, True)}
ENTRIES = [(i, a, k) for i, a in PAIRS for k in KINDS]
IDS = [f"{i}-{a}-{k}" for i, a, k in ENTRIES]
GRADS = {"d_x": "d_x", "d_weights": "d_W", "d_offset_conv_weights": "d_W_off", "d_offset_bias": "d_b_off"}


@pytest.fixture(autouse=True)
def modes_on(monkeypatch):
    """the modes are behind blocks.KPCONV_MODES (APR_KPCONV_MODES=1), off by default: every test here runs with it on"""
    from apr_amd.predator.models import blocks
    monkeypatch.setattr(blocks, "KPCONV_MODES", True)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_switch_off_keeps_the_constructor_refusing(monkeypatch):
    """the default: the constructor refuses the new combinations as it always did, naming the switch; linear / sum builds,
    an unknown value is a ValueError either way"""
    from apr_amd.predator.models import blocks
    monkeypatch.setattr(blocks, "KPCONV_MODES", False)
    for kw in (dict(KP_influence="gaussian"), dict(KP_influence="constant"), dict(aggregation_mode="closest")):
        for deformable in (False, True):
            with pytest.raises(NotImplementedError, match="APR_KPCONV_MODES"):
                blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, deformable=deformable, **kw)
    assert blocks.KPConv(15, 3, 8, 8, 1.2, 1.5)._mode == kp_ops.DEFAULT_MODE
    with pytest.raises(ValueError):
        blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence="foo")


@pytest.fixture(scope="module")
def lib():
    from apr_amd import _lib
    return _lib.load()


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())


def _chain(gold, inf, agg, kind, d_out=True):
    p = f"{inf}-{agg}/{kind}"
    deformable, modulated = KINDS[kind]
    mode = kp_ops.kpconv_mode(inf, agg)
    sd = lambda k: gold[f"{p}/sd/{k}"]
    kw = {}
    if deformable:
        od = 60 if modulated else 45
        kw = dict(W_off=sd("offset_conv.weights"), b_off=gold["in/bias"][:od], modulated=modulated,
                  kp_off=sd("offset_conv.kernel_points"))
    return MO.chain(gold["in/q"], gold["in/s"], gold["in/nbr"], gold["in/x"], sd("kernel_points"), 1.2, sd("weights"), mode,
                    d_out=gold["in/G"] if d_out else None, **kw)


@pytest.mark.parametrize("inf,agg,kind", ENTRIES, ids=IDS)
def test_oracle_chain_reproduces_the_reference(gold, inf, agg, kind):
    p = f"{inf}-{agg}/{kind}"
    r = _chain(gold, inf, agg, kind)
    assert _rel(r["out"], gold[f"{p}/out"]) <= 1e-12
    if KINDS[kind][0]:
        for k in ("min_d2", "deformed_KP", "offset_features"):
            assert _rel(r[k], gold[f"{p}/{k}"]) <= 1e-12, k
    if int(gold[f"{p}/no_backward"]):
        assert (inf, agg) == ("gaussian", "closest") and KINDS[kind][0]      # the reference's own backward raises there
        return
    for k, mine in GRADS.items():
        if f"{p}/{k}" not in gold.files:
            continue
        if int(gold[f"{p}/none/{k}"]):
            assert inf == "constant" and not np.asarray(r[mine]).any(), (k, "the reference gives None: the oracle must give 0")
        assert _rel(r[mine], gold[f"{p}/{k}"]) <= 1e-12, k


def test_constructor_takes_the_six_combinations_and_refuses_others():
    from apr_amd.predator.models import blocks
    for inf in ("constant", "linear", "gaussian"):
        for agg in ("sum", "closest"):
            for deformable in (False, True):
                conv = blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence=inf, aggregation_mode=agg, deformable=deformable)
                assert (conv.KP_influence, conv.aggregation_mode) == (inf, agg)
                assert conv._mode == (kp_ops.INFLUENCES[inf], kp_ops.AGGREGATIONS[agg])
                if deformable:      # offset_conv inherits both (blocks.py:184-192 of the reference)
                    assert conv.offset_conv._mode == conv._mode and conv.offset_conv.KP_influence == inf
                assert conv._fused_route(100, 20, True) is False or (inf, agg) == ("linear", "sum")
    with pytest.raises(ValueError, match="Unknown influence function type"):
        blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence="foo")
    with pytest.raises(ValueError, match="Unknown convolution mode"):
        blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, aggregation_mode="foo")
    with pytest.raises(ValueError):
        blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence="foo", deformable=True)


def test_config_reaches_every_kpconv_of_the_network():
    """kitti_config passes both keys through; block_decider and KPFCNN hand them to every KPConv; the one-call block plan
    and the fused forward decline a mode that is not the default"""
    from apr_amd.predator.configs.models import kitti_config
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    cfg = kitti_config(KP_influence="gaussian", aggregation_mode="closest")
    assert (cfg.KP_influence, cfg.aggregation_mode) == ("gaussian", "closest")
    b = blocks.block_decider("resnetb", 2.5, 64, 256, 1, cfg)
    assert b.KPConv._mode == (2, 1)
    assert not b._fused_ok(torch.zeros(4, 64), torch.zeros(4, 3, dtype=torch.int32))
    np.random.seed(0)
    torch.manual_seed(0)
    net = KPFCNN(cfg)
    convs = [m for m in net.modules() if isinstance(m, blocks.KPConv)]
    assert len(convs) >= 10 and all(m._mode == (2, 1) for m in convs)


def _module(gold, inf, agg, kind, seed=1):
    from apr_amd.predator.models import blocks
    deformable, modulated = KINDS[kind]
    np.random.seed(seed)
    torch.manual_seed(seed)
    return blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence=inf, aggregation_mode=agg, deformable=deformable,
                         modulated=modulated)


@pytest.mark.parametrize("inf,agg,kind", ENTRIES, ids=IDS)
def test_state_dict_keys_and_draws_are_the_reference_s(gold, inf, agg, kind):
    p = f"{inf}-{agg}/{kind}/sd/"
    ref = {k[len(p):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith(p)}
    sd = _module(gold, inf, agg, kind).state_dict()
    assert list(sd) == list(ref)
    for k in sd:
        assert sd[k].shape == ref[k].shape and torch.equal(sd[k], ref[k]), k
    other = _module(gold, inf, agg, kind, seed=5)
    other.load_state_dict(ref, strict=True)
    assert torch.equal(other.weights, ref["weights"])


@pytest.mark.parametrize("inf,agg,kind", ENTRIES, ids=IDS)
def test_torch_formulation_on_the_cpu_matches_the_reference(gold, inf, agg, kind):
    """cin = 8: the shapes the kernels refuse run the torch formulation (forward and backward) -- float32, 1e-5 of the
    reference's float64.  Where the reference's own backward raises, the gradients are held to the oracle chain."""
    p = f"{inf}-{agg}/{kind}"
    deformable, modulated = KINDS[kind]
    conv = _module(gold, inf, agg, kind)
    if deformable:
        with torch.no_grad():
            conv.offset_bias.copy_(torch.from_numpy(gold["in/bias"][:conv.offset_dim]))
    t = lambda k: torch.from_numpy(gold[f"in/{k}"])
    x = t("x").clone().requires_grad_(True)
    y = conv(t("q"), t("s"), t("nbr"), x)
    (y * t("G")).sum().backward()
    assert _rel(y.detach().numpy(), gold[f"{p}/out"]) <= 1e-5
    if deformable:
        assert _rel(conv.min_d2.numpy(), gold[f"{p}/min_d2"]) <= 1e-5 and not conv.min_d2.requires_grad
        assert _rel(conv.deformed_KP.detach().numpy(), gold[f"{p}/deformed_KP"]) <= 1e-5
    ref = _chain(gold, inf, agg, kind) if int(gold[f"{p}/no_backward"]) else None
    got = dict(d_x=x.grad, d_weights=conv.weights.grad)
    if deformable:
        got.update(d_offset_conv_weights=conv.offset_conv.weights.grad, d_offset_bias=conv.offset_bias.grad)
    for k, g in got.items():
        want = ref[GRADS[k]] if ref is not None else gold[f"{p}/{k}"]
        if ref is None and int(gold[f"{p}/none/{k}"]):
            assert g is None or not g.any(), k      # documented: None, as in the reference (all-zero would do as well)
            continue
        assert g is not None and _rel(g.numpy(), want) <= 1e-5, k


# ------------------------------------------------------------------------------------------------------- refusals
def test_mode_entries_refuse_bad_modes_and_bad_shapes_before_anything_is_read(lib):
    A = 0x10000      # stand-in pointers: every refusal comes before anything is read or launched

    def weighted(nq=5, H=5, cin=64, n_kp=15, extent=1.2, ldx=64, m=(2, 1)):
        return lib.apr_kpconv_weighted_mode(A, nq, A, 9, A, H, A, ldx, cin, A, n_kp, extent, A, A, 15 * cin, m[0], m[1], None)

    def contrib(nq=5, H=5, cin=64, n_kp=15, extent=1.2, m=(2, 1), out=A):
        return lib.apr_kpconv_dfeat_contrib_mode(A, nq, A, 9, A, H, A, 15 * cin, cin, A, n_kp, extent, A, out, m[0], m[1], None)

    def d_weighted(nq=5, H=5, cin=64, n_kp=15, extent=1.2, m=(2, 1)):
        return lib.apr_kpconv_deform_weighted_mode(A, nq, A, 9, A, H, A, max(cin, 64), cin, A, A, n_kp, extent, A, A, 15 * cin, A,
                                                   m[0], m[1], None)

    def d_contrib(nq=5, H=5, cin=64, n_kp=15, extent=1.2, m=(2, 1)):
        return lib.apr_kpconv_deform_dfeat_contrib_mode(A, nq, A, 9, A, H, A, 15 * cin, cin, A, A, n_kp, extent, A, A, m[0], m[1],
                                                        None)

    def d_geom(nq=5, H=5, cin=64, n_kp=15, extent=1.2, m=(2, 1)):
        return lib.apr_kpconv_deform_dgeom_mode(A, nq, A, 9, A, H, A, max(cin, 64), cin, A, 15 * cin, A, A, n_kp, extent, A, A, A,
                                                m[0], m[1], None)

    fns = {b"apr_kpconv_weighted_mode": weighted, b"apr_kpconv_dfeat_contrib_mode": contrib,
           b"apr_kpconv_deform_weighted_mode": d_weighted, b"apr_kpconv_deform_dfeat_contrib_mode": d_contrib,
           b"apr_kpconv_deform_dgeom_mode": d_geom}
    for tag, fn in fns.items():
        for m in ((3, 0), (-1, 0), (1, 2), (0, -1), (7, 7)):
            assert fn(m=m) == -1, (tag, m)                                  # APR_EINVAL
            assert tag in lib.apr_last_error(), (tag, m)
        for m in MO.MODES:
            assert fn(nq=0, m=m) == 0                                       # nothing to do, nothing launched
            assert fn(n_kp=14, m=m) == -1 and fn(extent=0.0, m=m) == -1 and fn(nq=-1, m=m) == -1 and fn(H=0, m=m) == -1
    for m in MO.MODES:
        assert contrib(H=129, m=m) == -1 and contrib(cin=513, m=m) == -1 and contrib(out=None, m=m) == -1
        for fn in (d_weighted, d_contrib, d_geom):
            assert fn(H=129, m=m) == -1 and fn(cin=32, m=m) == -1 and fn(cin=576, m=m) == -1


# -------------------------------------------------------------------------------------------------------- mutants
def _args(c, deformable, use_mod=True):
    K = c["dkp"] if deformable else MO.rigid(c["kp"], c["nq"])
    return c["q"], c["s"], c["nbr"], c["x"], K, (c["mod"] if (deformable and use_mod) else None), c["extent"]


MUTANT_PROBES = {      # mutant -> (quantity, mode, deformable): where it must leave its bound on at least one case
    "gauss_sigma_extent": ("wf", (2, 0), False),
    "gauss_clipped": ("wf", (2, 0), False),
    "const_out_of_range": ("wf", (0, 0), True),
    "closest_last_tie": ("wf", (1, 1), False),
    "closest_grad_unmasked": ("d_dkp", (1, 1), True),
    "ddkp_gauss_half": ("d_dkp", (2, 0), True),
    "const_ddkp_linear": ("d_dkp", (0, 0), True),
}


@pytest.mark.parametrize("mutant", MO.MUTANTS)
def test_every_mutant_leaves_its_bound_on_some_case(mutant):
    what, mode, deformable = MUTANT_PROBES[mutant]
    worst = 0.0
    for name, c in MC.CASES.items():
        if deformable and c["cin"] % 64:
            continue
        a = _args(c, deformable)
        if what == "wf":
            got = MO.weighted(*a, mode, deformable, mutant=mutant)[0]
            ref, b = MO.weighted(*a, mode, deformable)[0], MO.bound_weighted(*a, mode, deformable)
        else:
            got, ref = MO.d_geom(*a, c["dwf"], mode, mutant=mutant)[0], MO.d_geom(*a, c["dwf"], mode)[0]
            b = MO.bound_d_geom(*a, c["dwf"], mode)[0]
            got, ref, b = (v.reshape(len(v), -1) for v in (got, ref, b))
        ratio, at = MO.compare_rows(got, ref, b)
        print(mutant, name, what, ratio, at)
        worst = max(worst, ratio)
    assert worst > 1.0, (mutant, worst)
    assert set(MUTANT_PROBES) == set(MO.MUTANTS)


def test_the_default_mode_is_the_deform_and_rigid_oracles():
    """(linear, sum) through the modes oracle is the statement the existing oracles make: same values; bounds no tighter"""
    import kpconv_deform_oracle as DO
    import kpconv_oracle as O
    c = MC.CASES["k-c64-H5-nq37"]
    a = _args(c, True)
    assert np.array_equal(MO.weighted(*a, (1, 0), True)[0], DO.weighted(*a)[0])
    assert np.array_equal(MO.contrib(*a, c["dwf"], (1, 0), True), DO.contrib(*a, c["dwf"]))
    for mine, theirs in zip(MO.d_geom(*a, c["dwf"], (1, 0)), DO.d_geom(*a, c["dwf"])):
        assert np.allclose(mine, theirs, rtol=1e-14, atol=0)
    assert np.allclose(MO.bound_weighted(*a, (1, 0), True), DO.bound_weighted(*a), rtol=1e-12)
    assert np.allclose(MO.bound_contrib(*a, c["dwf"], (1, 0), True), DO.bound_contrib(*a, c["dwf"]), rtol=1e-12)
    for mine, theirs in zip(MO.bound_d_geom(*a, c["dwf"], (1, 0)), DO.bound_d_geom(*a, c["dwf"])):
        assert np.allclose(mine, theirs, rtol=1e-12)
    r = (c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"])
    assert np.allclose(MO.weighted(*_args(c, False), (1, 0), False)[0], O.weighted(*r)[0], rtol=1e-14, atol=0)
    assert np.allclose(MO.bound_weighted(*_args(c, False), (1, 0), False), O.bound_weighted(*r), rtol=1e-12)
    assert np.allclose(MO.bound_contrib(*_args(c, False), c["dwf"], (1, 0), False), O.bound_contrib(*r, c["dwf"]), rtol=1e-12)


def test_planted_rows_state_their_facts():
    c = MC.CASES["k-c64-H5-nq37"]
    rows = {kind: row for row, kind in c["plants"].items()}
    for mode in MO.MODES:
        wf_d, num_d, g_d = MO.weighted(*_args(c, True), mode, True)
        wf_r, num_r, g_r = MO.weighted(*_args(c, False), mode, False)
        assert not wf_d[rows["allpad"]].any() and not wf_r[rows["allpad"]].any()
        ro = rows["rigid_only"]      # the near neighbour (last slot): outside every deformed ball, inside a rigid one
        assert g_d["real"][ro, -1] and not g_d["take"][ro, -1] and not g_d["w"][ro, :, -1].any() and num_d[ro] == 1
        assert g_r["w"][ro, :, -1].any() and num_r[ro] == 2
        if mode[1]:
            t = rows["tie"]
            assert g_r["cl"][t, -1] == 3 and g_d["cl"][t, -1] == 3 and not g_r["w"][t, 7].any()
            m0 = rows["mod0_only"]
            assert g_d["cl"][m0, 0] == 2 and c["mod"][m0, 2] == 0 and not wf_d[m0, 2 * 64:3 * 64].any()
    g = MO.geometry(*_args(c, False)[:3], MO.rigid(c["kp"], c["nq"]), c["extent"], (2, 0), False)
    far = g["w"][ro, :, 0]      # the far support on the rigid gaussian layer: beyond the extent, underflowing
    assert (g["d"][ro, 0] > 10 * c["extent"]).all() and (far < 2.0 ** -149).all()

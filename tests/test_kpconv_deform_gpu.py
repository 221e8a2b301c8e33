"""The deformable / modulated KPConv on the GPU (apr_amd/csrc/kpconv_deform.hip): step 1 with min_d2, the contribution rows
and their ordered sum, the geometry gradient -- element by element against the float64 oracle (tests/kpconv_deform_oracle.py)
on the named cases of tests/kpconv_deform_cases.py at the oracle's derived bounds (ratio 1) --, the refusals, the module
(offset_conv included) against the oracle chain at the rigid module's bars, and KPFCNN with two deformable blocks against the
reference's own outputs (tests/golden/kpconv_deform_ref.npz).

Worst |kernel - oracle| / bound measured on the MI355X over all cases (records, not thresholds; printed by
test_print_worst_ratios):  wf 0.251,  min_d2 0.632,  contrib 0.225,  d_x 0.182,  d_mod 0.210,  d_dkp 0.627.
"""
import os

import numpy as np
import pytest
import torch

import kpconv_deform_cases as DC
import kpconv_deform_oracle as DO
from apr_amd import _lib
from apr_amd.predator import kp_ops
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "kpconv_deform_ref.npz")
WORST = {"wf": 0.0, "min_d2": 0.0, "contrib": 0.0, "d_x": 0.0, "d_mod": 0.0, "d_dkp": 0.0}
P = _lib.ptr


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _args(c, use_mod):
    return c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"] if use_mod else None, c["extent"]


def _record(key, got, ref, bound, what):
    ratio, at = DO.compare_rows(got, ref, bound)
    print(f"{what}: worst {key} ratio {ratio:.4f}")
    WORST[key] = max(WORST[key], ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _dev_inputs(c, dev, use_mod):
    d = dict(q=_t(c["q"], dev), s=_t(c["s"], dev), nbr=_t(c["nbr"], dev), x=_t(c["x"], dev), dkp=_t(c["dkp"], dev),
             mod=_t(c["mod"], dev) if use_mod else None)
    d["rs"] = kp_ops.row_sums(d["x"])
    return d


def _padded(values, pad, dev):
    """[n, c] values in a NaN-filled [n, c + pad] buffer -> (buffer, ld)"""
    n, c = values.shape
    big = torch.full((n, c + pad), NAN, dtype=torch.float32, device=dev)
    big[:, :c] = _t(values, dev)
    return big, c + pad


# ----------------------------------------------------------------------------------------------------------- step 1
@pytest.mark.parametrize("use_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("name", list(DC.CASES))
def test_step1_every_element_within_bound(dev, name, use_mod):
    c = DC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    d = _dev_inputs(c, dev, use_mod)
    kk = 15 * cin

    def run():
        wf = torch.full((nq, kk + 32), NAN, dtype=torch.float32, device=dev)
        md = torch.full((nq + 1, 15), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_weighted(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["dkp"]),
                                                  P(d["mod"]), 15, c["extent"], P(d["rs"]), P(wf), kk + 32, P(md), _lib.stream()))
        torch.cuda.synchronize()
        return wf.cpu().numpy(), md.cpu().numpy()

    wf, md = run()
    assert np.isnan(wf[:, kk:]).all() and np.isnan(md[nq]).all(), "guard columns / rows were touched"
    a = _args(c, use_mod)
    ref, _, num, g = DO.weighted(*a)
    _record("wf", wf[:, :kk], ref, DO.bound_weighted(*a), name)
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    _record("min_d2", md[:nq], DO.min_d2(*geo), DO.bound_min_d2(*geo), name)
    for row, kind in c["plants"].items():
        if kind in ("allpad", "none"):
            assert not wf[row, :kk].any(), (kind, "not exactly 0")
        if kind == "allpad":
            assert (md[row] > 1e11).all()
    wf2, md2 = run()
    assert wf2.tobytes() == wf.tobytes() and md2.tobytes() == md.tobytes(), "two runs, other bits"
    # without min_d2 (NULL): the same wf
    out = torch.full((nq, kk), NAN, dtype=torch.float32, device=dev)
    _lib.check(lib.apr_kpconv_deform_weighted(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["dkp"]),
                                              P(d["mod"]), 15, c["extent"], P(d["rs"]), P(out), kk, None, _lib.stream()))
    assert out.cpu().numpy().tobytes() == np.ascontiguousarray(wf[:, :kk]).tobytes()


# --------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("use_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("name", list(DC.CASES))
def test_contribution_rows_ordered_sum_and_geometry_gradient(dev, name, use_mod):
    c = DC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    d = _dev_inputs(c, dev, use_mod)
    a = _args(c, use_mod)
    dwf, lddwf = _padded(c["dwf"], 4, dev)

    def contrib_rows(q0, q1, buf):
        _lib.check(lib.apr_kpconv_deform_dfeat_contrib(P(d["q"][q0:q1]), q1 - q0, P(d["s"]), ns, P(d["nbr"][q0:q1]), H,
                                                       P(dwf[q0:q1]), lddwf, cin, P(d["dkp"][q0:q1]),
                                                       P(None if d["mod"] is None else d["mod"][q0:q1]), 15, c["extent"],
                                                       P(d["rs"]), P(buf), _lib.stream()))

    contrib = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
    contrib_rows(0, nq, contrib)
    rows = contrib.cpu().numpy()
    real = DO.O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    ref, bound = DO.contrib(*a, c["dwf"]), DO.bound_contrib(*a, c["dwf"])
    _record("contrib", rows[real], ref[real], bound[real], name)

    rev, start = kp_ops.reverse_table(d["nbr"], ns)
    ldo = cin + 4

    def summed(qc):
        out = torch.full((ns, ldo), NAN, dtype=torch.float32, device=dev)
        buf = torch.full((min(nq, qc) * H, cin), NAN, dtype=torch.float32, device=dev)
        for q0 in range(0, nq, qc):
            q1 = min(nq, q0 + qc)
            contrib_rows(q0, q1, buf)
            _lib.check(lib.apr_reverse_gather_range(P(buf), cin, P(rev), P(start), ns, q0 * H, q1 * H, int(q0 > 0), P(out), ldo,
                                                    _lib.stream()))
        return out.cpu().numpy()

    whole = summed(nq)
    assert np.isnan(whole[:, cin:]).all() and not np.isnan(whole[:, :cin]).any()
    for qc in (1, 3):
        assert summed(qc)[:, :cin].tobytes() == whole[:, :cin].tobytes(), f"chunks of {qc} queries: other bits than one gather"
    _record("d_x", whole[:, :cin], DO.d_x(*a, c["dwf"]), DO.bound_dx(*a, c["dwf"]), name)

    def geom():
        dd = torch.full((nq + 1, 15, 3), NAN, dtype=torch.float32, device=dev)
        dm = torch.full((nq + 1, 15), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_dgeom(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(dwf), lddwf,
                                               P(d["dkp"]), P(d["mod"]), 15, c["extent"], P(d["rs"]), P(dd), P(dm), _lib.stream()))
        torch.cuda.synchronize()
        return dd.cpu().numpy(), dm.cpu().numpy()

    dd, dm = geom()
    assert np.isnan(dd[nq]).all() and np.isnan(dm[nq]).all() and not np.isnan(dd[:nq]).any() and not np.isnan(dm[:nq]).any()
    ref_dd, ref_dm = DO.d_geom(*a, c["dwf"])
    bd, bm = DO.bound_d_geom(*a, c["dwf"])
    _record("d_mod", dm[:nq], ref_dm, bm, name)
    _record("d_dkp", dd[:nq].reshape(nq, -1), ref_dd.reshape(nq, -1), bd.reshape(nq, -1), name)
    dd2, dm2 = geom()
    assert dd2.tobytes() == dd.tobytes() and dm2.tobytes() == dm.tobytes(), "two runs, other bits"


@pytest.mark.parametrize("name", list(DC.REFUSED))
def test_refusals_leave_the_outputs_untouched(dev, name):
    r = dict(cin=64, H=5, n_kp=15, ns=9, extent=1.2, nq=5)
    r.update(DC.REFUSED[name])
    lib = _lib.load()
    cin, H, n_kp, ns, nq = r["cin"], r["H"], r["n_kp"], r["ns"], r["nq"]
    rng = np.random.default_rng(7)
    cw, Hb, nb = (cin + 3) // 4 * 4, max(H, 1), 9
    q, s = _t(rng.uniform(-1, 1, (5, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (nb, 3)).astype(np.float32), dev)
    dkp = _t(rng.uniform(-1, 1, (5, 15, 3)).astype(np.float32), dev)
    mod = _t(rng.uniform(0, 2, (5, 15)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, nb + 1, (5, Hb)).astype(np.int32), dev)
    x = _t(rng.standard_normal((nb, cw)).astype(np.float32), dev)
    dwf = _t(rng.standard_normal((5, 15 * cw)).astype(np.float32), dev)
    rs = kp_ops.row_sums(x)
    pattern = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    wf, md, contrib = pattern(5 * 15 * cw * 4), pattern(5 * 15 * 4), pattern(5 * Hb * cw * 4)
    dd, dm = pattern(5 * 45 * 4), pattern(5 * 15 * 4)
    ext = r["extent"]
    calls = [
        lambda: lib.apr_kpconv_deform_weighted(P(q), nq, P(s), ns, P(nbr), H, P(x), cw, cin, P(dkp), P(mod), n_kp, ext, P(rs),
                                               P(wf), 15 * cw, P(md), _lib.stream()),
        lambda: lib.apr_kpconv_deform_dfeat_contrib(P(q), nq, P(s), ns, P(nbr), H, P(dwf), 15 * cw, cin, P(dkp), P(mod), n_kp,
                                                    ext, P(rs), P(contrib), _lib.stream()),
        lambda: lib.apr_kpconv_deform_dgeom(P(q), nq, P(s), ns, P(nbr), H, P(x), cw, cin, P(dwf), 15 * cw, P(dkp), P(mod), n_kp,
                                            ext, P(rs), P(dd), P(dm), _lib.stream()),
    ]
    for call in calls:
        assert call() == -1                                     # APR_EINVAL
        assert b"apr_kpconv_deform" in lib.apr_last_error()
    torch.cuda.synchronize()
    for buf in (wf, md, contrib, dd, dm):
        assert bool((buf == 0xA5).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------- the module
def _rows_rel_l2(got, ref):
    """per row: |got - ref|_2 / max(|ref|_2, median row norm); rows that are exactly 0 in the reference must be exactly 0"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    norms = np.linalg.norm(ref, axis=1)
    zero = norms == 0
    assert not got[zero].any(), "a row that is exactly 0 in the reference is not exactly 0"
    floor = np.median(norms)
    return float((np.linalg.norm(got - ref, axis=1) / np.maximum(norms, floor if floor > 0 else 1.0)).max())


def _module(c, cout, modulated, params, dev):
    from apr_amd.predator.models import blocks
    W, W_off, b_off, _ = params
    conv = blocks.KPConv(15, 3, c["cin"], cout, c["extent"], 1.0, deformable=True, modulated=modulated)
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(W))
        conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_conv.weights.copy_(torch.from_numpy(W_off))
        conv.offset_conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_bias.copy_(torch.from_numpy(b_off))
    return conv.to(dev)


def _module_run(conv, c, d_out, dev, hip):
    """-> inference out, training out, min_d2, gradients (x, W, W_off, b_off) as numpy"""
    from apr_amd.predator.models import blocks
    q, s, nbr = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev)
    saved = blocks.KPCONV_DEFORM_HIP
    blocks.KPCONV_DEFORM_HIP = hip
    try:
        with torch.no_grad():
            inf = conv(q, s, nbr, _t(c["x"], dev)).cpu().numpy()
        md_inf, dkp_inf = conv.min_d2.cpu().numpy(), conv.deformed_KP.cpu().numpy()
        assert not conv.min_d2.requires_grad and tuple(conv.deformed_KP.shape) == (c["nq"], 15, 3)
        conv.zero_grad()
        x = _t(c["x"], dev).requires_grad_(True)
        out = conv(q, s, nbr, x)
        assert not conv.min_d2.requires_grad and conv.offset_features.requires_grad
        out.backward(_t(d_out, dev))
    finally:
        blocks.KPCONV_DEFORM_HIP = saved
    g = dict(d_x=x.grad, d_W=conv.weights.grad, d_W_off=conv.offset_conv.weights.grad, d_b_off=conv.offset_bias.grad)
    res = {k: v.cpu().numpy() for k, v in g.items()}
    res.update(inf=inf, out=out.detach().cpu().numpy(), min_d2=md_inf, min_d2_train=conv.min_d2.cpu().numpy(),
               dkp=conv.deformed_KP.detach().cpu().numpy(), dkp_inf=dkp_inf, of=conv.offset_features.detach().cpu().numpy())
    return res


def _module_errors(r, ref):
    e = dict(inf=_rows_rel_l2(r["inf"], ref["out"]), out=_rows_rel_l2(r["out"], ref["out"]),
             d_x=_rows_rel_l2(r["d_x"], ref["d_x"]),
             d_W=_rows_rel_l2(r["d_W"].reshape(15, -1), ref["d_W"].reshape(15, -1)),
             d_W_off=_rows_rel_l2(r["d_W_off"].reshape(15, -1), ref["d_W_off"].reshape(15, -1)),
             d_b_off=_rows_rel_l2(r["d_b_off"].reshape(1, -1), ref["d_b_off"].reshape(1, -1)))
    return e


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "modulated"])
@pytest.mark.parametrize("name,cout", DC.MODULE)
def test_module_against_the_oracle_chain(dev, name, cout, modulated):
    """Inference out, training out and every gradient of KPConv(deformable=True) against the float64 chain (offset_conv
    included): out at the rigid module's 5e-6, gradients at 1e-4, per row / per W slice, relative L2 floored at the median
    row norm.  The forced torch branch is held to the same bars and to the HIP branch.
    The module takes the reference's neighbour tables, where padding is written as ns and nothing else: offset_conv's
    training path (45 or 60 output channels: torch ops) indexes with them as the reference does.  The other spellings of
    padding (-1, ns + 5) are the kernels' business and stay in the kernel tests above."""
    c = dict(DC.CASES[name])
    c["nbr"] = np.where(DO.O.real_mask(c["nbr"], c["ns"]), c["nbr"], c["ns"]).astype(np.int32)
    params = DC.module_params(c, cout, modulated)
    W, W_off, b_off, d_out = params
    ref = DO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, W_off, b_off, modulated, d_out=d_out)
    conv = _module(c, cout, modulated, params, dev)
    hip = _module_run(conv, c, d_out, dev, True)
    tor = _module_run(conv, c, d_out, dev, False)
    e_hip, e_tor = _module_errors(hip, ref), _module_errors(tor, ref)
    print(f"{name} cout {cout} modulated {modulated}: HIP {({k: float(f'{v:.3g}') for k, v in e_hip.items()})}")
    print(f"{name} cout {cout} modulated {modulated}: torch {({k: float(f'{v:.3g}') for k, v in e_tor.items()})}")
    for e in (e_hip, e_tor):
        assert e["inf"] < 5e-6 and e["out"] < 5e-6, e
        assert max(e["d_x"], e["d_W"], e["d_W_off"], e["d_b_off"]) < 1e-4, e
    assert _rows_rel_l2(hip["out"], tor["out"].astype(np.float64)) < 5e-6
    for k in ("d_x", "d_W", "d_W_off", "d_b_off"):
        n = 15 if k in ("d_W", "d_W_off") else (1 if k == "d_b_off" else len(hip[k]))
        assert _rows_rel_l2(hip[k].reshape(n, -1), tor[k].reshape(n, -1).astype(np.float64)) < 1e-4, k
    for r in (hip, tor):
        for key, pts in (("min_d2", "dkp_inf"), ("min_d2_train", "dkp")):     # of the deformed points that very pass made
            geo = (c["q"], c["s"], c["nbr"], r[pts], c["extent"])
            ratio, at = DO.compare_rows(r[key], DO.min_d2(*geo), DO.bound_min_d2(*geo))
            assert ratio <= 1.0, (key, ratio, at)
    assert np.abs(hip["dkp"] - ref["deformed_KP"]).max() < 1e-5 and np.abs(hip["of"] - ref["offset_features"]).max() < 1e-5


# ------------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("m", [0, 1], ids=["plain", "modulated"])
def test_kpfcnn_with_deformable_blocks_matches_the_reference(dev, m):
    """KPFCNN, KITTI architecture with its two coarsest encoder blocks deformable, against the outputs of the reference's
    own KPFCNN on the committed pair, at predator_small's bars."""
    from apr_amd.predator.configs.models import kitti_config
    from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    g = np.load(GOLD)
    cfg = kitti_config(modulated=bool(m))
    arch = list(cfg.architecture)
    for i in g["net/enc_deform"]:
        assert arch[int(i)] == "resnetb"
        arch[int(i)] = "resnetb_deformable"
    cfg.architecture = arch
    np.random.seed(0)
    torch.manual_seed(0)
    model = KPFCNN(cfg)
    wsum = float(sum(v.double().abs().sum() for v in model.state_dict().values()))
    assert abs(wsum - float(g[f"n{m}/weight_abs_sum"])) <= 1e-6 * wsum, "same seeds must give the reference's parameters"
    model = model.to(dev).eval()
    deform = [mod for mod in model.modules() if isinstance(mod, blocks.KPConv) and mod.deformable]
    assert len(deform) == 2 and all(d.modulated == bool(m) and d.in_channels == 512 for d in deform)
    src, tgt = g["net/src"], g["net/tgt"]
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg,
                                  [int(v) for v in g["net/limits"]])
    assert [len(p) for p in batch["points"]] == [int(v) for v in g[f"n{m}/level_sizes"]]
    feats, ov, sal = model(batch)
    assert all(d.min_d2 is not None and tuple(d.min_d2.shape) == (len(batch["points"][3]), 15) for d in deform)
    r_f = rel_l2(feats.cpu(), g[f"n{m}/feats"])
    e_ov, e_sal = np.abs(ov.cpu().numpy() - g[f"n{m}/overlap"]).max(), np.abs(sal.cpu().numpy() - g[f"n{m}/saliency"]).max()
    print(f"modulated {m}: feats rel-L2 {r_f:.3g}, overlap {e_ov:.3g}, saliency {e_sal:.3g}")
    assert r_f < 1e-4 and e_ov < 1e-4 and e_sal < 1e-4
    f2, ov2, sal2 = model(batch)
    assert torch.equal(f2, feats) and torch.equal(ov2, ov) and torch.equal(sal2, sal), "two eval runs, other bits"
    model.train()
    ft, ovt, salt = model(batch)
    assert ft.requires_grad
    assert rel_l2(ft.detach().cpu(), feats.cpu()) < 1e-4
    assert (ovt.detach() - ov).abs().max().item() < 1e-4 and (salt.detach() - sal).abs().max().item() < 1e-4


def test_print_worst_ratios():
    print("worst |kernel - oracle| / bound over the cases run:", {k: round(v, 4) for k, v in WORST.items()})

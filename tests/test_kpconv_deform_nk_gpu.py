"""Deformable / modulated KPConv with any kernel-point count on the GPU (apr_kpconv_deform_weighted_nk,
apr_kpconv_deform_dfeat_contrib_nk, apr_kpconv_deform_dgeom_nk; csrc/kpconv_deform_nk.hip): wf, min_d2, the contribution rows,
their ordered sum d_x, d_dkp and d_mod element by element against the float64 oracle (tests/kpconv_deform_nk_oracle.py) on the
named cases of tests/kpconv_deform_nk_cases.py at the oracle's derived bounds (ratio 1; every mode at n_kp = 7, 15 and 20,
(linear, sum) and (gaussian, closest) elsewhere; with and without mod), two runs bit for bit, n_kp = 15 against the *_mode
entries inside twice the bound, refusals that leave pre-filled outputs untouched, blocks.KPConv(7 / 20, deformable) against the
float64 chain on the kernels and on the torch formulation, KPFCNN with two deformable blocks at K = 7 against its all-torch
route, and one training iteration.

Worst |kernel - oracle| / bound measured on the MI355X over all cases and modes (records, not thresholds; printed by
test_print_worst_ratios with the last-bit counts at n_kp = 15; by mode in DESIGN section 40):  wf 0.583,  min_d2 0.683,
contrib 0.502,  d_x 0.469,  d_mod 0.192,  d_dkp 0.786.
"""
import numpy as np
import pytest
import torch

import kpconv_deform_nk_cases as DNC
import kpconv_deform_nk_oracle as DNO
from apr_amd import _lib
from apr_amd.predator import kp_ops
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
REFUSED = DNC.REFUSED
NAN = float("nan")
WORST = {}
LASTBIT = {}
P = _lib.ptr
CASE_MODES = [(n, m) for n in DNC.CASES for m in DNC.case_modes(n)]
CASE_MODE_IDS = [f"{n}-{DNO.mode_name(m)}" for n, m in CASE_MODES]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _args(c, use_mod):
    return c["q"], c["s"], c["nbr"], c["x"], c["dkp"], c["mod"] if use_mod else None, c["extent"]


def _record(key, mode, got, ref, bound, what):
    ratio, at = DNO.compare_rows(got, ref, bound)
    print(f"{what} {DNO.mode_name(mode)}: worst {key} ratio {ratio:.4f}")
    k = (key, DNO.mode_name(mode))
    WORST[k] = max(WORST.get(k, 0.0), ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, mode, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _dev_inputs(c, dev, use_mod):
    d = dict(q=_t(c["q"], dev), s=_t(c["s"], dev), nbr=_t(c["nbr"], dev), x=_t(c["x"], dev), dkp=_t(c["dkp"], dev),
             mod=_t(c["mod"], dev) if use_mod else None)
    d["rs"] = kp_ops.row_sums(d["x"])
    return d


def _agree_at_15(key, new, old, bound, what):
    """both entries lie inside the bound of the same oracle value, so they differ by at most twice it; the elements a last
    bit (or more) apart are counted"""
    diff = np.abs(new.astype(np.float64) - old.astype(np.float64))
    assert (diff <= 2.0 * bound).all(), (what, key, float((diff - 2.0 * bound).max()))
    n = int((new.view(np.uint32) != old.view(np.uint32)).sum())
    LASTBIT[key] = tuple(a + b for a, b in zip(LASTBIT.get(key, (0, 0)), (n, new.size)))
    print(f"{what}: n_kp = 15, {key}: {n} of {new.size} elements differ from the _mode entry")


# --------------------------------------------------------------------------------------- the three entries, every case
@pytest.mark.parametrize("use_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("name,mode", CASE_MODES, ids=CASE_MODE_IDS)
def test_every_element_within_bound(dev, name, mode, use_mod):
    c = DNC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin, K = c["nq"], c["ns"], c["H"], c["cin"], c["n_kp"]
    d = _dev_inputs(c, dev, use_mod)
    a = _args(c, use_mod)
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    kk = K * cin
    what = f"{name}/{'mod' if use_mod else 'nomod'}"

    def step1(fn):
        wf = torch.full((nq, kk + 32), NAN, dtype=torch.float32, device=dev)
        md = torch.full((nq + 1, K), NAN, dtype=torch.float32, device=dev)
        _lib.check(fn(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["dkp"]), P(d["mod"]), K, c["extent"],
                      P(d["rs"]), P(wf), kk + 32, P(md), mode[0], mode[1], _lib.stream()))
        return wf.cpu().numpy(), md.cpu().numpy()

    wf, md = step1(lib.apr_kpconv_deform_weighted_nk)
    assert np.isnan(wf[:, kk:]).all() and np.isnan(md[nq]).all(), "guard columns / rows were touched"
    bw, bmin = DNO.bound_weighted(*a, mode), DNO.bound_min_d2(*geo)
    _record("wf", mode, wf[:, :kk], DNO.weighted(*a, mode)[0], bw, what)
    _record("min_d2", mode, md[:nq], DNO.min_d2(*geo), bmin, what)
    for row, kind in c["plants"].items():
        if kind in ("allpad", "none"):
            assert not wf[row, :kk].any(), (kind, "not exactly 0")
        if kind == "allpad":
            assert (md[row] > 1e11).all()
    wf2, md2 = step1(lib.apr_kpconv_deform_weighted_nk)
    assert wf2.tobytes() == wf.tobytes() and md2.tobytes() == md.tobytes(), "step 1: two runs, other bits"
    out = torch.full((nq, kk), NAN, dtype=torch.float32, device=dev)      # without min_d2 (NULL): the same wf
    _lib.check(lib.apr_kpconv_deform_weighted_nk(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["dkp"]),
                                                 P(d["mod"]), K, c["extent"], P(d["rs"]), P(out), kk, None, mode[0], mode[1],
                                                 _lib.stream()))
    assert out.cpu().numpy().tobytes() == np.ascontiguousarray(wf[:, :kk]).tobytes()
    if K == 15:
        wf_o, md_o = step1(lib.apr_kpconv_deform_weighted_mode)
        _agree_at_15("wf", np.ascontiguousarray(wf[:, :kk]), np.ascontiguousarray(wf_o[:, :kk]), bw, what)
        _agree_at_15("min_d2", np.ascontiguousarray(md[:nq]), np.ascontiguousarray(md_o[:nq]), bmin, what)

    lddwf = kk + 4
    dwf = torch.full((nq, lddwf), NAN, dtype=torch.float32, device=dev)
    dwf[:, :kk] = _t(c["dwf"], dev)

    def contrib_rows(fn, q0, q1, buf):
        _lib.check(fn(P(d["q"][q0:q1]), q1 - q0, P(d["s"]), ns, P(d["nbr"][q0:q1]), H, P(dwf[q0:q1]), lddwf, cin,
                      P(d["dkp"][q0:q1]), P(None if d["mod"] is None else d["mod"][q0:q1]), K, c["extent"], P(d["rs"]), P(buf),
                      mode[0], mode[1], _lib.stream()))

    def all_rows(fn):
        buf = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
        contrib_rows(fn, 0, nq, buf)
        return buf.cpu().numpy()

    rows = all_rows(lib.apr_kpconv_deform_dfeat_contrib_nk)
    real = DNO.O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    bc = DNO.bound_contrib(*a, c["dwf"], mode)
    _record("contrib", mode, rows[real], DNO.contrib(*a, c["dwf"], mode)[real], bc[real], what)
    assert all_rows(lib.apr_kpconv_deform_dfeat_contrib_nk).tobytes() == rows.tobytes(), "contribution rows: two runs, other bits"
    if K == 15:
        _agree_at_15("contrib", np.ascontiguousarray(rows[real]),
                     np.ascontiguousarray(all_rows(lib.apr_kpconv_deform_dfeat_contrib_mode)[real]), bc[real], what)

    rev, start = kp_ops.reverse_table(d["nbr"], ns)
    ldo = cin + 4

    def summed(qc):
        o = torch.full((ns, ldo), NAN, dtype=torch.float32, device=dev)
        buf = torch.full((min(nq, qc) * H, cin), NAN, dtype=torch.float32, device=dev)
        for q0 in range(0, nq, qc):
            q1 = min(nq, q0 + qc)
            contrib_rows(lib.apr_kpconv_deform_dfeat_contrib_nk, q0, q1, buf)
            _lib.check(lib.apr_reverse_gather_range(P(buf), cin, P(rev), P(start), ns, q0 * H, q1 * H, int(q0 > 0), P(o), ldo,
                                                    _lib.stream()))
        return o.cpu().numpy()

    whole = summed(nq)
    assert np.isnan(whole[:, cin:]).all() and not np.isnan(whole[:, :cin]).any()
    if nq > 1:
        assert summed(3)[:, :cin].tobytes() == whole[:, :cin].tobytes(), "chunks of 3 queries: other bits than one gather"
    _record("d_x", mode, whole[:, :cin], DNO.d_x(*a, c["dwf"], mode), DNO.bound_dx(*a, c["dwf"], mode), what)

    def geom(fn):
        dd = torch.full((nq + 1, K, 3), NAN, dtype=torch.float32, device=dev)
        dm = torch.full((nq + 1, K), NAN, dtype=torch.float32, device=dev)
        _lib.check(fn(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(dwf), lddwf, P(d["dkp"]), P(d["mod"]), K,
                      c["extent"], P(d["rs"]), P(dd), P(dm), mode[0], mode[1], _lib.stream()))
        return dd.cpu().numpy(), dm.cpu().numpy()

    dd, dm = geom(lib.apr_kpconv_deform_dgeom_nk)
    assert np.isnan(dd[nq]).all() and np.isnan(dm[nq]).all() and not np.isnan(dd[:nq]).any() and not np.isnan(dm[:nq]).any()
    ref_dd, ref_dm = DNO.d_geom(*a, c["dwf"], mode)
    bd, bm = DNO.bound_d_geom(*a, c["dwf"], mode)
    _record("d_mod", mode, dm[:nq], ref_dm, bm, what)
    _record("d_dkp", mode, dd[:nq].reshape(nq, -1), ref_dd.reshape(nq, -1), bd.reshape(nq, -1), what)
    if mode[0] == DNO.CONSTANT:
        assert not dd[:nq].any(), "constant influence: d_dkp must be exactly 0"
    dd2, dm2 = geom(lib.apr_kpconv_deform_dgeom_nk)
    assert dd2.tobytes() == dd.tobytes() and dm2.tobytes() == dm.tobytes(), "geometry gradient: two runs, other bits"
    if K == 15:
        dd_o, dm_o = geom(lib.apr_kpconv_deform_dgeom_mode)
        _agree_at_15("d_mod", np.ascontiguousarray(dm[:nq]), np.ascontiguousarray(dm_o[:nq]), bm, what)
        _agree_at_15("d_dkp", np.ascontiguousarray(dd[:nq]).reshape(nq, -1), np.ascontiguousarray(dd_o[:nq]).reshape(nq, -1),
                     bd.reshape(nq, -1), what)


@pytest.mark.parametrize("name", list(REFUSED) + ["x_misaligned", "ldwf_small"])
def test_refusals_leave_the_outputs_untouched(dev, name):
    r = dict(cin=64, H=5, n_kp=7, ns=9, extent=1.2, nq=5, m=(1, 0), off=0, ld_cut=0)
    r.update(dict(x_misaligned=dict(off=1), ldwf_small=dict(ld_cut=4)).get(name) or REFUSED[name])
    lib = _lib.load()
    cin, H, n_kp, ns, nq, m = r["cin"], r["H"], r["n_kp"], r["ns"], r["nq"], r["m"]
    rng = np.random.default_rng(7)
    cw, Hb, nb, Kb = (cin + 3) // 4 * 4, max(H, 1), 9, max(n_kp, 1)
    q, s = _t(rng.uniform(-1, 1, (5, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (nb, 3)).astype(np.float32), dev)
    dkp = _t(rng.uniform(-1, 1, (5, Kb, 3)).astype(np.float32), dev)
    mod = _t(rng.uniform(0, 2, (5, Kb)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, nb + 1, (5, Hb)).astype(np.int32), dev)
    x = _t(rng.standard_normal((nb * cw + 4,)).astype(np.float32), dev)[r["off"]:r["off"] + nb * cw].view(nb, cw)
    dwf = _t(rng.standard_normal((5 * Kb * cw + 4,)).astype(np.float32), dev)[r["off"]:r["off"] + 5 * Kb * cw].view(5, Kb * cw)
    rs = _t(rng.standard_normal(nb).astype(np.float32), dev)
    pattern = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    wf, md, contrib = pattern(5 * Kb * cw * 4), pattern(5 * Kb * 4), pattern(5 * Hb * cw * 4)
    dd, dm = pattern(5 * Kb * 12), pattern(5 * Kb * 4)
    ext, ld = r["extent"], Kb * cw - r["ld_cut"]
    calls = [
        lambda: lib.apr_kpconv_deform_weighted_nk(P(q), nq, P(s), ns, P(nbr), H, P(x), cw, cin, P(dkp), P(mod), n_kp, ext, P(rs),
                                                  P(wf), ld, P(md), m[0], m[1], _lib.stream()),
        lambda: lib.apr_kpconv_deform_dfeat_contrib_nk(P(q), nq, P(s), ns, P(nbr), H, P(dwf), ld, cin, P(dkp), P(mod), n_kp, ext,
                                                       P(rs), P(contrib), m[0], m[1], _lib.stream()),
        lambda: lib.apr_kpconv_deform_dgeom_nk(P(q), nq, P(s), ns, P(nbr), H, P(x), cw, cin, P(dwf), ld, P(dkp), P(mod), n_kp, ext,
                                               P(rs), P(dd), P(dm), m[0], m[1], _lib.stream()),
    ]
    for i, call in enumerate(calls):
        if name == "x_misaligned" and i == 1:      # the contribution entry reads dwf with scalar loads: no alignment rule
            continue
        assert call() == -1, i                                  # APR_EINVAL
        assert b"apr_kpconv_deform" in lib.apr_last_error() and b"_nk" in lib.apr_last_error()
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


def _spy(monkeypatch, blocks):
    calls = []
    orig = blocks.KPConv._forward_autograd_deformable

    def spy(self, *a):
        calls.append(self.K)
        return orig(self, *a)

    monkeypatch.setattr(blocks.KPConv, "_forward_autograd_deformable", spy)
    return calls


@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "modulated"])
@pytest.mark.parametrize("name,cout", DNC.MODULE)
def test_module_against_the_oracle_chain(dev, name, cout, modulated, monkeypatch):
    """blocks.KPConv(7 / 20, .., deformable=True) at cin = 64 and 128: inference out, training out and every gradient against
    the float64 chain (offset_conv included): out at 5e-6, gradients at 1e-4, per row / per W slice, relative L2 floored at
    the median row norm -- the bars of every KPConv module test here -- on the kernels and, with KPCONV_NK_HIP off, on the
    torch formulation.  With the switch on the deformed convolution never reaches _forward_autograd_deformable.  Padding is
    spelled ns, as the reference's tables spell it."""
    from apr_amd.predator.models import blocks
    c = dict(DNC.CASES[name])
    K = c["n_kp"]
    c["nbr"] = np.where(DNO.O.real_mask(c["nbr"], c["ns"]), c["nbr"], c["ns"]).astype(np.int32)
    W, W_off, b_off, d_out = DNC.module_params(c, cout, modulated)
    ref = DNO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, W_off, b_off, modulated, d_out=d_out)
    np.random.seed(1)
    conv = blocks.KPConv(K, 3, c["cin"], cout, c["extent"], 1.0, deformable=True, modulated=modulated)
    assert conv.offset_dim == (4 if modulated else 3) * K
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(W))
        conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_conv.weights.copy_(torch.from_numpy(W_off))
        conv.offset_conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        conv.offset_bias.copy_(torch.from_numpy(b_off))
    conv = conv.to(dev)
    calls = _spy(monkeypatch, blocks)
    q, s, nbr = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev)
    res = {}
    for hip in (True, False):
        monkeypatch.setattr(blocks, "KPCONV_NK_HIP", hip)
        del calls[:]
        with torch.no_grad():
            inf = conv(q, s, nbr, _t(c["x"], dev)).cpu().numpy()
        md_inf, dkp_inf = conv.min_d2.cpu().numpy(), conv.deformed_KP.cpu().numpy()
        assert tuple(md_inf.shape) == (c["nq"], K) and tuple(dkp_inf.shape) == (c["nq"], K, 3)
        conv.zero_grad()
        x = _t(c["x"], dev).requires_grad_(True)
        out = conv(q, s, nbr, x)
        assert not conv.min_d2.requires_grad and conv.offset_features.requires_grad
        out.backward(_t(d_out, dev))
        assert len(calls) == (0 if hip else 2), "the deformed convolution did not take the route the switch names"
        r = dict(inf=inf, out=out.detach().cpu().numpy(), d_x=x.grad.cpu().numpy(), d_W=conv.weights.grad.cpu().numpy().reshape(K, -1),
                 d_W_off=conv.offset_conv.weights.grad.cpu().numpy().reshape(K, -1),
                 d_b_off=conv.offset_bias.grad.cpu().numpy().reshape(1, -1))
        e = dict(inf=_rows_rel_l2(r["inf"], ref["out"]), out=_rows_rel_l2(r["out"], ref["out"]), d_x=_rows_rel_l2(r["d_x"], ref["d_x"]),
                 d_W=_rows_rel_l2(r["d_W"], ref["d_W"].reshape(K, -1)), d_W_off=_rows_rel_l2(r["d_W_off"], ref["d_W_off"].reshape(K, -1)),
                 d_b_off=_rows_rel_l2(r["d_b_off"], ref["d_b_off"].reshape(1, -1)))
        print(f"{name} cout {cout} modulated {modulated} {'HIP' if hip else 'torch'}: {({k: float(f'{v:.3g}') for k, v in e.items()})}")
        assert e["inf"] < 5e-6 and e["out"] < 5e-6, e
        assert max(e["d_x"], e["d_W"], e["d_W_off"], e["d_b_off"]) < 1e-4, e
        for key, pts in ((md_inf, dkp_inf), (conv.min_d2.cpu().numpy(), conv.deformed_KP.detach().cpu().numpy())):
            geo = (c["q"], c["s"], c["nbr"], pts, c["extent"])      # min_d2 of the deformed points that very pass made
            ratio, at = DNO.compare_rows(key, DNO.min_d2(*geo), DNO.bound_min_d2(*geo))
            assert ratio <= 1.0, ("min_d2", ratio, at)
        assert np.abs(conv.deformed_KP.detach().cpu().numpy() - ref["deformed_KP"]).max() < 1e-5
        res[hip] = r
    for k in res[True]:
        assert _rows_rel_l2(res[True][k], res[False][k]) < (5e-6 if k in ("inf", "out") else 1e-4), k


# ------------------------------------------------------------------------------------------------------ the network
def _deform_config(modulated, **kw):
    from apr_amd.predator.configs.models import kitti_config
    cfg = kitti_config(modulated=bool(modulated), num_kernel_points=7, **kw)
    arch = list(cfg.architecture)
    for i in (9, 10):      # the two coarsest encoder blocks
        assert arch[i] == "resnetb"
        arch[i] = "resnetb_deformable"
    cfg.architecture = arch
    return cfg


@pytest.mark.parametrize("m", [0, 1], ids=["plain", "modulated"])
def test_kpfcnn_k7_with_deformable_blocks_matches_its_all_torch_route(dev, m, monkeypatch):
    """KPFCNN(kitti_config(num_kernel_points=7)) with its two coarsest resnetb blocks deformable on a pair of a few
    hundred points (synth.make_pair at 4 beams, one point per 0.3 m cell): the kernels against the route with
    KPCONV_NK_HIP off (every K = 7 layer on torch ops), features, overlap and saliency at 1e-4."""
    from apr_amd import synth
    from apr_amd.predator import point_ops
    from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    cfg = _deform_config(m)
    np.random.seed(0)
    torch.manual_seed(0)
    model = KPFCNN(cfg).to(dev).eval()
    deform = [mod for mod in model.modules() if isinstance(mod, blocks.KPConv) and mod.deformable]
    assert len(deform) == 2 and all(d.K == 7 and d.modulated == bool(m) and d.in_channels == 512 for d in deform)
    a, b, _ = synth.make_pair(11, n_beams=4, n_azimuth=200)
    pts, lens = point_ops.grid_subsample(torch.cat([torch.from_numpy(a), torch.from_numpy(b)]).to(dev),
                                         np.array([len(a), len(b)], np.int32), 0.3)
    src, tgt = pts[:lens[0]].cpu().numpy(), pts[lens[0]:].cpu().numpy()
    assert 300 <= len(src) <= 800 and 300 <= len(tgt) <= 800
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg,
                                  [35, 33, 34, 36])
    calls = _spy(monkeypatch, blocks)
    out = {}
    for hip in (True, False):
        monkeypatch.setattr(blocks, "KPCONV_NK_HIP", hip)
        del calls[:]
        with torch.no_grad():
            out[hip] = [v.cpu().numpy() for v in model(batch)]
        assert len(calls) == (0 if hip else 2)
        assert all(tuple(d.min_d2.shape) == (len(batch["points"][3]), 7) for d in deform)
    e = (rel_l2(out[True][0], out[False][0]), float(np.abs(out[True][1] - out[False][1]).max()),
         float(np.abs(out[True][2] - out[False][2]).max()))
    print(f"KPFCNN K = 7, two deformable blocks, modulated {m}: kernels vs all-torch (feats rel L2, overlap, saliency): {e}")
    assert np.isfinite(out[True][0]).all() and out[True][0].any()
    assert e[0] < 1e-4 and e[1] < 1e-4 and e[2] < 1e-4


def test_one_training_iteration_with_deformable_k7_blocks_is_finite_and_repeats_bit_for_bit(dev, monkeypatch):
    from apr_amd.predator.lib.trainer import PredatorPairTrainStep
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    from apr_amd.predator.models.mlp import GenerativeMLP_98
    from oracle import predator_points_oracle as PREF
    from tests.predator_loss_fixture import collated, small_pair, train_config
    if not PREF.available():
        pytest.skip("oracle/_ref not built")
    pair = small_pair()
    calls = _spy(monkeypatch, blocks)
    runs = []
    for _ in range(2):
        np.random.seed(7)
        torch.manual_seed(7)
        cfg = train_config()
        cfg.update(num_kernel_points=7, modulated=True)
        arch = list(cfg.architecture)
        arch[9] = arch[10] = "resnetb_deformable"
        cfg.architecture = arch
        model = KPFCNN(cfg).to(dev)
        gen = GenerativeMLP_98(in_channel=cfg.final_feats_dim, out_points=cfg.point_generation_ratio, radius=None,
                               bn_momentum=cfg.batch_norm_momentum).to(dev)
        opt = torch.optim.SGD([{"params": model.parameters()}, {"params": gen.parameters()}], lr=0.01, momentum=0.98,
                              weight_decay=1e-6)
        step = PredatorPairTrainStep(model, gen, opt, cfg)
        batch = collated(pair, cfg, [30, 30, 30, 30], dev)
        grads = []
        hooks = [p.register_hook(lambda g: grads.append(g.detach().clone())) for p in model.parameters() if p.requires_grad]
        np.random.seed(5)
        stats = step(batch)[0]
        for h in hooks:
            h.remove()
        runs.append((stats, grads, [p.detach().clone() for p in model.parameters()]))
    assert not calls, "a deformable K = 7 layer left the kernels in training"
    stats, grads, _ = runs[0]
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    assert len(grads) > 50 and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
    for k in stats:
        assert float(stats[k]) == float(runs[1][0][k]), k
    assert all(torch.equal(a, b) for a, b in zip(grads, runs[1][1])) and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


def test_print_worst_ratios():
    table = {}
    for (key, mode), v in sorted(WORST.items()):
        table.setdefault(key, {})[mode] = round(v, 4)
    for key, row in table.items():
        print(f"worst |kernel - oracle| / bound, {key}: {row}")
    for key, (n, total) in LASTBIT.items():
        print(f"n_kp = 15, {key}: {n} of {total} elements differ from the _mode entries")

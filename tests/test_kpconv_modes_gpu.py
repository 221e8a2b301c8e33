"""KPConv's influence / aggregation modes on the GPU (apr_kpconv_*_mode; csrc/kpconv.hip, csrc/kpconv_deform.hip): step 1
(with min_d2 on deformed layers), the contribution rows and their ordered sum, the geometry gradient -- element by element
against the float64 oracle (tests/kpconv_modes_oracle.py) on the named cases of tests/kpconv_modes_cases.py, every mode,
with and without modulations, at the oracle's derived bounds (ratio 1) --, (linear, sum) bit for bit against the entry
points without a mode, the refusals, the module against the oracle chain and against the reference's own outputs
(tests/golden/kpconv_modes_ref.npz), and a KPFCNN built from a gaussian / closest config.

Worst |kernel - oracle| / bound measured on the MI355X over all cases and modes (records, not thresholds; printed by
test_print_worst_ratios; the table per mode is in DESIGN section 34):  rigid wf 0.397, contrib 0.416, d_x 0.416;  deformed wf
0.399, min_d2 0.570, contrib 0.420, d_x 0.435, d_mod 0.099, d_dkp 0.256 (constant: exactly 0).
"""
import os

import numpy as np
import pytest
import torch

import kpconv_modes_cases as MC
import kpconv_modes_oracle as MO
from apr_amd import _lib
from apr_amd.predator import kp_ops
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "kpconv_modes_ref.npz")
NET = os.path.join(os.path.dirname(__file__), "golden", "kpconv_deform_ref.npz")
WORST = {}
P = _lib.ptr
MODE_IDS = [MO.mode_name(m) for m in MO.MODES]
DEFORM_CASES = [n for n, c in MC.CASES.items() if c["cin"] % 64 == 0]
DEFAULT = (1, 0)


@pytest.fixture(autouse=True)
def modes_on(monkeypatch):
    """the modes are behind blocks.KPCONV_MODES (APR_KPCONV_MODES=1), off by default: every test here runs with it on"""
    from apr_amd.predator.models import blocks
    monkeypatch.setattr(blocks, "KPCONV_MODES", True)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _record(key, mode, got, ref, bound, what):
    ratio, at = MO.compare_rows(got, ref, bound)
    print(f"{what} {MO.mode_name(mode)}: worst {key} ratio {ratio:.4f}")
    k = (key, MO.mode_name(mode))
    WORST[k] = max(WORST.get(k, 0.0), ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, mode, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _dev_inputs(c, dev, use_mod):
    d = dict(q=_t(c["q"], dev), s=_t(c["s"], dev), nbr=_t(c["nbr"], dev), x=_t(c["x"], dev), kp=_t(c["kp"], dev),
             dkp=_t(c["dkp"], dev), mod=_t(c["mod"], dev) if use_mod else None)
    d["rs"] = kp_ops.row_sums(d["x"])
    return d


def _oargs(c, deformable, use_mod):
    K = c["dkp"] if deformable else MO.rigid(c["kp"], c["nq"])
    return c["q"], c["s"], c["nbr"], c["x"], K, (c["mod"] if (deformable and use_mod) else None), c["extent"]


def _padded(values, pad, dev):
    n, cc = values.shape
    big = torch.full((n, cc + pad), NAN, dtype=torch.float32, device=dev)
    big[:, :cc] = _t(values, dev)
    return big, cc + pad


def _ordered_sum(lib, c, d, dev, contrib_rows):
    """the contribution rows summed per support row over the reverse table, whole and in chunks of 3 queries: the same bits"""
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    rev, start = kp_ops.reverse_table(d["nbr"], ns)

    def summed(qc):
        out = torch.full((ns, cin + 4), NAN, dtype=torch.float32, device=dev)
        buf = torch.full((min(nq, qc) * H, cin), NAN, dtype=torch.float32, device=dev)
        for q0 in range(0, nq, qc):
            q1 = min(nq, q0 + qc)
            contrib_rows(q0, q1, buf)
            _lib.check(lib.apr_reverse_gather_range(P(buf), cin, P(rev), P(start), ns, q0 * H, q1 * H, int(q0 > 0), P(out),
                                                    cin + 4, _lib.stream()))
        return out.cpu().numpy()

    whole = summed(nq)
    assert np.isnan(whole[:, cin:]).all() and not np.isnan(whole[:, :cin]).any()
    assert summed(3)[:, :cin].tobytes() == whole[:, :cin].tobytes(), "chunks of 3 queries: other bits than one gather"
    return whole[:, :cin]


# ------------------------------------------------------------------------------------------------------ rigid layers
@pytest.mark.parametrize("mode", MO.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(MC.CASES))
def test_rigid_step1_and_feature_gradient_within_bound(dev, name, mode):
    c = MC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    d = _dev_inputs(c, dev, False)
    kk = 15 * cin
    ld = (kk + 3) // 4 * 4 + 32
    a = _oargs(c, False, False)

    def step1():
        wf = torch.full((nq, ld), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_weighted_mode(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["kp"]), 15,
                                                c["extent"], P(d["rs"]), P(wf), ld, mode[0], mode[1], _lib.stream()))
        return wf

    wf_t = step1()
    wf = wf_t.cpu().numpy()
    assert np.isnan(wf[:, kk:]).all(), "guard columns were touched"
    ref, _, g = MO.weighted(*a, mode, False)
    _record("rigid wf", mode, wf[:, :kk], ref, MO.bound_weighted(*a, mode, False), name)
    for row, kind in c["plants"].items():
        if kind == "allpad":
            assert not wf[row, :kk].any(), "all padding: not exactly 0"
    assert torch.equal(step1()[:, :kk], wf_t[:, :kk]), "two runs, other bits"
    if mode == DEFAULT:
        old = torch.full((nq, ld), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_weighted(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["kp"]), 15,
                                           c["extent"], P(d["rs"]), P(old), ld, _lib.stream()))
        assert torch.equal(old[:, :kk], wf_t[:, :kk]), "(linear, sum): other bits than apr_kpconv_weighted"

    dwf, lddwf = _padded(c["dwf"], 4, dev)

    def contrib_rows(q0, q1, buf):
        _lib.check(lib.apr_kpconv_dfeat_contrib_mode(P(d["q"][q0:q1]), q1 - q0, P(d["s"]), ns, P(d["nbr"][q0:q1]), H, P(dwf[q0:q1]),
                                                     lddwf, cin, P(d["kp"]), 15, c["extent"], P(d["rs"]), P(buf), mode[0], mode[1],
                                                     _lib.stream()))

    contrib = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
    contrib_rows(0, nq, contrib)
    rows = contrib.cpu().numpy()
    real = MO.O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    _record("rigid contrib", mode, rows[real], MO.contrib(*a, c["dwf"], mode, False)[real],
            MO.bound_contrib(*a, c["dwf"], mode, False)[real], name)
    if mode == DEFAULT:
        old = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_dfeat_contrib(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(dwf), lddwf, cin, P(d["kp"]), 15,
                                                c["extent"], P(d["rs"]), P(old), _lib.stream()))
        assert old.cpu().numpy().tobytes() == rows.tobytes(), "(linear, sum): other bits than apr_kpconv_dfeat_contrib"
    if cin % 4 == 0:      # the ordered sum reads 16-byte rows
        dx = _ordered_sum(lib, c, d, dev, contrib_rows)
        _record("rigid d_x", mode, dx, MO.d_x(*a, c["dwf"], mode, False), MO.bound_dx(*a, c["dwf"], mode, False), name)


# --------------------------------------------------------------------------------------------------- deformed layers
@pytest.mark.parametrize("use_mod", [True, False], ids=["mod", "nomod"])
@pytest.mark.parametrize("mode", MO.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", DEFORM_CASES)
def test_deformed_step1_and_gradients_within_bound(dev, name, mode, use_mod):
    c = MC.CASES[name]
    lib = _lib.load()
    nq, ns, H, cin = c["nq"], c["ns"], c["H"], c["cin"]
    d = _dev_inputs(c, dev, use_mod)
    kk = 15 * cin
    a = _oargs(c, True, use_mod)

    def step1():
        wf = torch.full((nq, kk + 32), NAN, dtype=torch.float32, device=dev)
        md = torch.full((nq + 1, 15), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_weighted_mode(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin,
                                                       P(d["dkp"]), P(d["mod"]), 15, c["extent"], P(d["rs"]), P(wf), kk + 32,
                                                       P(md), mode[0], mode[1], _lib.stream()))
        return wf, md

    wf_t, md_t = step1()
    wf, md = wf_t.cpu().numpy(), md_t.cpu().numpy()
    assert np.isnan(wf[:, kk:]).all() and np.isnan(md[nq]).all(), "guard columns / rows were touched"
    ref, _, g = MO.weighted(*a, mode, True)
    _record("deform wf", mode, wf[:, :kk], ref, MO.bound_weighted(*a, mode, True), name)
    geo = (c["q"], c["s"], c["nbr"], c["dkp"], c["extent"])
    _record("min_d2", mode, md[:nq], MO.min_d2(*geo), MO.DO.bound_min_d2(*geo), name)
    for row, kind in c["plants"].items():
        if kind in ("allpad", "none"):
            assert not wf[row, :kk].any(), (kind, "not exactly 0")
    wf2, md2 = step1()
    assert torch.equal(wf2[:, :kk], wf_t[:, :kk]) and torch.equal(md2[:nq], md_t[:nq]), "two runs, other bits"
    dwf, lddwf = _padded(c["dwf"], 4, dev)

    def contrib_rows(q0, q1, buf):
        _lib.check(lib.apr_kpconv_deform_dfeat_contrib_mode(P(d["q"][q0:q1]), q1 - q0, P(d["s"]), ns, P(d["nbr"][q0:q1]), H,
                                                            P(dwf[q0:q1]), lddwf, cin, P(d["dkp"][q0:q1]),
                                                            P(None if d["mod"] is None else d["mod"][q0:q1]), 15, c["extent"],
                                                            P(d["rs"]), P(buf), mode[0], mode[1], _lib.stream()))

    contrib = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
    contrib_rows(0, nq, contrib)
    rows = contrib.cpu().numpy()
    real = MO.O.real_mask(c["nbr"], ns).reshape(-1)
    assert np.isnan(rows[~real]).all(), "rows of padding neighbours are documented as untouched"
    _record("deform contrib", mode, rows[real], MO.contrib(*a, c["dwf"], mode, True)[real],
            MO.bound_contrib(*a, c["dwf"], mode, True)[real], name)
    dx = _ordered_sum(lib, c, d, dev, contrib_rows)
    _record("deform d_x", mode, dx, MO.d_x(*a, c["dwf"], mode, True), MO.bound_dx(*a, c["dwf"], mode, True), name)

    def geom():
        dd = torch.full((nq + 1, 15, 3), NAN, dtype=torch.float32, device=dev)
        dm = torch.full((nq + 1, 15), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_dgeom_mode(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(dwf),
                                                    lddwf, P(d["dkp"]), P(d["mod"]), 15, c["extent"], P(d["rs"]), P(dd), P(dm),
                                                    mode[0], mode[1], _lib.stream()))
        return dd, dm

    dd_t, dm_t = geom()
    dd, dm = dd_t.cpu().numpy(), dm_t.cpu().numpy()
    assert np.isnan(dd[nq]).all() and np.isnan(dm[nq]).all() and not np.isnan(dd[:nq]).any() and not np.isnan(dm[:nq]).any()
    ref_dd, ref_dm = MO.d_geom(*a, c["dwf"], mode)
    bd, bm = MO.bound_d_geom(*a, c["dwf"], mode)
    _record("d_mod", mode, dm[:nq], ref_dm, bm, name)
    _record("d_dkp", mode, dd[:nq].reshape(nq, -1), ref_dd.reshape(nq, -1), bd.reshape(nq, -1), name)
    if mode[0] == 0:
        assert not dd[:nq].any(), "constant influence: d_dkp must be exactly 0"
    dd2, dm2 = geom()
    assert torch.equal(dd2[:nq], dd_t[:nq]) and torch.equal(dm2[:nq], dm_t[:nq]), "two runs, other bits"
    if mode == DEFAULT:      # the entry points without a mode: the same bits
        o_wf = torch.full((nq, kk + 32), NAN, dtype=torch.float32, device=dev)
        o_md = torch.full((nq + 1, 15), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_weighted(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(d["dkp"]),
                                                  P(d["mod"]), 15, c["extent"], P(d["rs"]), P(o_wf), kk + 32, P(o_md),
                                                  _lib.stream()))
        assert torch.equal(o_wf[:, :kk], wf_t[:, :kk]) and torch.equal(o_md[:nq], md_t[:nq])
        o_c = torch.full((nq * H, cin), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_deform_dfeat_contrib(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(dwf), lddwf, cin,
                                                       P(d["dkp"]), P(d["mod"]), 15, c["extent"], P(d["rs"]), P(o_c),
                                                       _lib.stream()))
        assert o_c.cpu().numpy().tobytes() == rows.tobytes()
        o_dd, o_dm = torch.empty_like(dd_t), torch.empty_like(dm_t)
        _lib.check(lib.apr_kpconv_deform_dgeom(P(d["q"]), nq, P(d["s"]), ns, P(d["nbr"]), H, P(d["x"]), cin, cin, P(dwf), lddwf,
                                               P(d["dkp"]), P(d["mod"]), 15, c["extent"], P(d["rs"]), P(o_dd), P(o_dm),
                                               _lib.stream()))
        assert torch.equal(o_dd[:nq], dd_t[:nq]) and torch.equal(o_dm[:nq], dm_t[:nq])


@pytest.mark.parametrize("bad", [(3, 0), (-1, 0), (1, 2), (2, -1)], ids=str)
def test_unknown_modes_are_refused_with_the_outputs_untouched(dev, bad):
    lib = _lib.load()
    rng = np.random.default_rng(7)
    cin, H, ns, nq = 64, 5, 9, 5
    q, s = _t(rng.uniform(-1, 1, (nq, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (ns, 3)).astype(np.float32), dev)
    kp = _t(rng.uniform(-1, 1, (15, 3)).astype(np.float32), dev)
    dkp = _t(rng.uniform(-1, 1, (nq, 15, 3)).astype(np.float32), dev)
    mod = _t(rng.uniform(0, 2, (nq, 15)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, ns + 1, (nq, H)).astype(np.int32), dev)
    x = _t(rng.standard_normal((ns, cin)).astype(np.float32), dev)
    dwf = _t(rng.standard_normal((nq, 15 * cin)).astype(np.float32), dev)
    rs = kp_ops.row_sums(x)
    pattern = lambda n: torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    wf, md, contrib = pattern(nq * 15 * cin * 4), pattern(nq * 15 * 4), pattern(nq * H * cin * 4)
    dd, dm = pattern(nq * 45 * 4), pattern(nq * 15 * 4)
    i, cl = bad
    st = _lib.stream()
    calls = {
        b"apr_kpconv_weighted_mode": lambda: lib.apr_kpconv_weighted_mode(P(q), nq, P(s), ns, P(nbr), H, P(x), cin, cin, P(kp), 15,
                                                                          1.2, P(rs), P(wf), 15 * cin, i, cl, st),
        b"apr_kpconv_dfeat_contrib_mode": lambda: lib.apr_kpconv_dfeat_contrib_mode(P(q), nq, P(s), ns, P(nbr), H, P(dwf), 15 * cin,
                                                                                    cin, P(kp), 15, 1.2, P(rs), P(contrib), i, cl,
                                                                                    st),
        b"apr_kpconv_deform_weighted_mode": lambda: lib.apr_kpconv_deform_weighted_mode(P(q), nq, P(s), ns, P(nbr), H, P(x), cin,
                                                                                        cin, P(dkp), P(mod), 15, 1.2, P(rs), P(wf),
                                                                                        15 * cin, P(md), i, cl, st),
        b"apr_kpconv_deform_dfeat_contrib_mode": lambda: lib.apr_kpconv_deform_dfeat_contrib_mode(
            P(q), nq, P(s), ns, P(nbr), H, P(dwf), 15 * cin, cin, P(dkp), P(mod), 15, 1.2, P(rs), P(contrib), i, cl, st),
        b"apr_kpconv_deform_dgeom_mode": lambda: lib.apr_kpconv_deform_dgeom_mode(P(q), nq, P(s), ns, P(nbr), H, P(x), cin, cin,
                                                                                  P(dwf), 15 * cin, P(dkp), P(mod), 15, 1.2, P(rs),
                                                                                  P(dd), P(dm), i, cl, st),
    }
    for tag, call in calls.items():
        assert call() == -1                                     # APR_EINVAL
        assert tag in lib.apr_last_error()
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


def _grad(p, like):
    """a gradient the graph does not reach (the constant influence moves no kernel point) may be None or all-zero"""
    return np.zeros(tuple(like.shape), np.float32) if p is None else p.cpu().numpy()


def _module_run(conv, c, d_out, dev, hip):
    from apr_amd.predator.models import blocks
    q, s, nbr = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev)
    saved = blocks.KPCONV_DEFORM_HIP, blocks.KPCONV_TRAIN_HIP
    blocks.KPCONV_DEFORM_HIP = blocks.KPCONV_TRAIN_HIP = hip
    try:
        with torch.no_grad():
            inf = conv(q, s, nbr, _t(c["x"], dev)).cpu().numpy()
        conv.zero_grad()
        x = _t(c["x"], dev).requires_grad_(True)
        out = conv(q, s, nbr, x)
        out.backward(_t(d_out, dev))
    finally:
        blocks.KPCONV_DEFORM_HIP, blocks.KPCONV_TRAIN_HIP = saved
    res = dict(inf=inf, out=out.detach().cpu().numpy(), d_x=x.grad.cpu().numpy(), d_W=conv.weights.grad.cpu().numpy())
    if conv.deformable:
        res.update(d_W_off=_grad(conv.offset_conv.weights.grad, conv.offset_conv.weights),
                   d_b_off=_grad(conv.offset_bias.grad, conv.offset_bias), min_d2=conv.min_d2.cpu().numpy(),
                   dkp=conv.deformed_KP.detach().cpu().numpy())
    return res


@pytest.mark.parametrize("kind", ["rigid", "deformable", "modulated"])
@pytest.mark.parametrize("mode", MO.NEW_MODES, ids=[MO.mode_name(m) for m in MO.NEW_MODES])
@pytest.mark.parametrize("name,cout", MC.MODULE)
def test_module_against_the_oracle_chain(dev, name, cout, mode, kind):
    """blocks.KPConv at cin = 64, cout = 64 in every new mode: inference out, training out and every gradient against the
    float64 chain at the bars of the deformable module's test (out 5e-6, gradients 1e-4, per row / per W slice, relative L2
    floored at the median row norm), on the HIP kernels and on the forced torch formulation.  Padding is spelled ns, as the
    reference's tables spell it."""
    from apr_amd.predator.models import blocks
    c = dict(MC.CASES[name])
    c["nbr"] = np.where(MO.O.real_mask(c["nbr"], c["ns"]), c["nbr"], c["ns"]).astype(np.int32)
    deformable, modulated = kind != "rigid", kind == "modulated"
    inf_name, agg_name = MO.NAMES[mode[0]], "closest" if mode[1] else "sum"
    conv = blocks.KPConv(15, 3, c["cin"], cout, c["extent"], 1.0, KP_influence=inf_name, aggregation_mode=agg_name,
                         deformable=deformable, modulated=modulated)
    if deformable:
        W, W_off, b_off, d_out = MC.module_params(c, cout, modulated, mode)
        kw = dict(W_off=W_off, b_off=b_off, modulated=modulated)
    else:
        (W, d_out), kw = MC.weights(c, cout), {}
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(W))
        conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
        if deformable:
            conv.offset_conv.weights.copy_(torch.from_numpy(W_off))
            conv.offset_conv.kernel_points.copy_(torch.from_numpy(c["kp"]))
            conv.offset_bias.copy_(torch.from_numpy(b_off))
    conv = conv.to(dev)
    ref = MO.chain(c["q"], c["s"], c["nbr"], c["x"], c["kp"], c["extent"], W, mode, d_out=d_out, **kw)
    keys = ["d_x", "d_W"] + (["d_W_off", "d_b_off"] if deformable else [])
    rows = lambda k, v: v.reshape(15, -1) if k in ("d_W", "d_W_off") else (v.reshape(1, -1) if k == "d_b_off" else v)
    for hip in (True, False):
        r = _module_run(conv, c, d_out, dev, hip)
        e = dict(inf=_rows_rel_l2(r["inf"], ref["out"]), out=_rows_rel_l2(r["out"], ref["out"]))
        e.update({k: _rows_rel_l2(rows(k, r[k]), rows(k, ref[k])) for k in keys})
        print(f"{name} {MO.mode_name(mode)} {kind} {'HIP' if hip else 'torch'}: {({k: float(f'{v:.3g}') for k, v in e.items()})}")
        assert e["inf"] < 5e-6 and e["out"] < 5e-6, e
        assert max(e[k] for k in keys) < 1e-4, e
        if deformable:
            geo = (c["q"], c["s"], c["nbr"], r["dkp"], c["extent"])
            ratio, at = MO.compare_rows(r["min_d2"], MO.min_d2(*geo), MO.DO.bound_min_d2(*geo))
            assert ratio <= 1.0, ("min_d2", ratio, at)
            assert np.abs(r["dkp"] - ref["deformed_KP"]).max() < 1e-5


PAIRS = [("constant", "sum"), ("constant", "closest"), ("linear", "closest"), ("gaussian", "sum"), ("gaussian", "closest")]


@pytest.mark.parametrize("kind", ["r", "d", "dm"])
@pytest.mark.parametrize("inf,agg", PAIRS, ids=[f"{i}-{a}" for i, a in PAIRS])
def test_cin8_module_matches_the_reference_fixture(dev, inf, agg, kind):
    """cin = 8 (no MFMA form): inference on the generic kernel / the torch formulation, training on the torch formulation,
    against the reference's own float64 outputs and gradients at 1e-5 of the largest element"""
    from apr_amd.predator.models import blocks
    g = np.load(GOLD)
    p = f"{inf}-{agg}/{kind}"
    deformable, modulated = kind != "r", kind == "dm"
    conv = blocks.KPConv(15, 3, 8, 8, 1.2, 1.5, KP_influence=inf, aggregation_mode=agg, deformable=deformable, modulated=modulated)
    conv.load_state_dict({k[len(p) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + "/sd/")}, strict=True)
    if deformable:
        with torch.no_grad():
            conv.offset_bias.copy_(torch.from_numpy(g["in/bias"][:conv.offset_dim]))
    conv = conv.to(dev)
    t = lambda k: _t(g[f"in/{k}"], dev)
    rel = lambda got, ref: float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))
    with torch.no_grad():
        assert rel(conv(t("q"), t("s"), t("nbr"), t("x")).cpu().numpy(), g[f"{p}/out"]) <= 1e-5
    x = t("x").clone().requires_grad_(True)
    y = conv(t("q"), t("s"), t("nbr"), x)
    (y * t("G")).sum().backward()
    assert rel(y.detach().cpu().numpy(), g[f"{p}/out"]) <= 1e-5
    if deformable:
        assert rel(conv.min_d2.cpu().numpy(), g[f"{p}/min_d2"]) <= 1e-5
    if int(g[f"{p}/no_backward"]):
        return      # the reference's own backward raises there; the CPU test holds these gradients to the oracle chain
    got = dict(d_x=x.grad, d_weights=conv.weights.grad)
    if deformable:
        got.update(d_offset_conv_weights=conv.offset_conv.weights.grad, d_offset_bias=conv.offset_bias.grad)
    for k, v in got.items():
        if int(g[f"{p}/none/{k}"]):
            assert v is None or not v.any(), k
        else:
            assert rel(v.cpu().numpy(), g[f"{p}/{k}"]) <= 1e-5, k


# ------------------------------------------------------------------------------------------------------ the network
def test_kpfcnn_from_a_gaussian_closest_config(dev):
    """KPFCNN built from kitti_config(KP_influence='gaussian', aggregation_mode='closest') on the tiny committed pair: eval()
    on the per-op HIP path (the one-call block plan and the fused forward decline the mode) against the torch formulation
    (train() with KPCONV_TRAIN_HIP off: eval() never leaves the kernels) at 1e-4 relative L2, and one train() step on the
    kernels with finite outputs and gradients."""
    from apr_amd.predator.configs.models import kitti_config
    from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
    from apr_amd.predator.models import blocks
    from apr_amd.predator.models.architectures import KPFCNN
    g = np.load(NET)
    cfg = kitti_config(KP_influence="gaussian", aggregation_mode="closest")
    np.random.seed(0)
    torch.manual_seed(0)
    model = KPFCNN(cfg).to(dev).eval()
    assert all(m._mode == (2, 1) for m in model.modules() if isinstance(m, blocks.KPConv))
    src, tgt = g["net/src"], g["net/tgt"]
    batch = collate_fn_descriptor([(src, tgt, np.ones((len(src), 1), np.float32), np.ones((len(tgt), 1), np.float32))], cfg,
                                  [int(v) for v in g["net/limits"]])
    with torch.no_grad():
        feats, ov, sal = model(batch)
        f2, ov2, sal2 = model(batch)
    assert torch.isfinite(feats).all() and torch.isfinite(ov).all() and torch.isfinite(sal).all()
    assert torch.equal(f2, feats) and torch.equal(ov2, ov) and torch.equal(sal2, sal), "two eval runs, other bits"
    model.train()      # (the norms are InstanceNorm: train() changes the route, not the function)
    routes = []
    saved, saved_fn = blocks.KPCONV_TRAIN_HIP, blocks.KPConv._forward_autograd
    blocks.KPCONV_TRAIN_HIP = False

    def spy(self, *a):
        routes.append(self)
        return saved_fn(self, *a)

    blocks.KPConv._forward_autograd = spy
    try:
        ft, ovt, salt = model(batch)      # parameters tracked, the switch off: the torch formulation of every KPConv
    finally:
        blocks.KPCONV_TRAIN_HIP, blocks.KPConv._forward_autograd = saved, saved_fn
    n_conv = sum(isinstance(m, blocks.KPConv) for m in model.modules())
    assert ft.requires_grad and len(routes) == n_conv, "the torch formulation did not run in every KPConv"
    e = rel_l2(feats.cpu(), ft.detach().cpu()), rel_l2(ov.cpu(), ovt.detach().cpu()), rel_l2(sal.cpu(), salt.detach().cpu())
    print("per-op HIP vs torch formulation, relative L2 (feats, overlap, saliency):", e)
    assert max(e) <= 1e-4
    model.zero_grad()
    fo, oo, so = model(batch)
    assert fo.requires_grad and torch.isfinite(fo).all() and torch.isfinite(oo).all() and torch.isfinite(so).all()
    (fo.square().sum() + oo.sum() + so.sum()).backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert sum(gr is not None for gr in grads) >= 10 and all(torch.isfinite(gr).all() for gr in grads if gr is not None)
    assert any(gr.abs().max() > 0 for gr in grads if gr is not None)


def test_print_worst_ratios():
    table = {}
    for (key, mode), v in sorted(WORST.items()):
        table.setdefault(key, {})[mode] = round(v, 4)
    for key, row in table.items():
        print(f"worst |kernel - oracle| / bound, {key}: {row}")

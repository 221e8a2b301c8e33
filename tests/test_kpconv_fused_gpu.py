"""apr_kpconv_fused (correlation and contraction of the rigid KPConv in one kernel) on the GPU against the float64 oracle.

a. EXACT cases (tests/kpconv_fused_cases.py; tests/test_kpconv_fused_cpu.py shows that they are exact): the float64 result,
   value for value.
b. BOUND cases: the project's row statistic for this arithmetic (< 5e-6, test_kpconv_function_end_to_end) and element by
   element |out - ref| <= bound_weighted @ |W| + 16 eps32 (|wf| @ |W|), no row excluded.
c. the same bits on a second call; misaligned rows and the refused shapes raise through kp_ops.kpconv_fused.
d. the network with blocks.FUSED_KPCONV = 2.
`out` is NaN-filled with 8 guard columns behind cout, which must still be NaN afterwards.

Record (MI355X): worst rows rel-L2 over the bound cases 2.32e-06, worst |err| / bound 0.0803.
"""
import os

import numpy as np
import pytest
import torch

import kpconv_fused_cases as F
from apr_amd import _lib, ops, synth
from apr_amd.predator import kp_ops
from apr_amd.predator.configs.models import kitti_config
from apr_amd.predator.datasets.dataloader import collate_fn_descriptor
from apr_amd.predator.models import blocks
from apr_amd.predator.models.architectures import KPFCNN
from tests.helpers import rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 8
GOLD = os.path.join(os.path.dirname(__file__), "golden")
WORST = {"rows": 0.0, "element": 0.0}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _view(values, layout, dev):
    """the values [n, c] aligned, as the column slice big[:, 1:c + 1] (base 4 bytes off) or with a row stride of c + 1"""
    n, c = values.shape
    if layout == "aligned":
        return _t(values, dev)
    big = torch.full((n, c + 8 if layout == "slice1" else c + 1), NAN, dtype=torch.float32, device=dev)
    view = big[:, 1:c + 1] if layout == "slice1" else big[:, :c]
    view.copy_(_t(values, dev))
    return view


def _fused_direct(dev, c, calls=1):
    """-> the `calls` outputs [nq, cout] of the library entry on NaN-filled buffers, guard columns checked"""
    lib = _lib.load()
    nq, ns, H, cin, cout = c["nq"], c["ns"], c["H"], c["cin"], c["cout"]
    q, s, nbr, kp, x = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev), _t(c["kp"], dev), _t(c["x"], dev)
    w_bf3 = ops.pack_weights_bf3(_t(c["W"].reshape(1, 15 * cin, cout), dev))
    assert w_bf3 is not None
    rs = kp_ops.row_sums(x)
    outs = []
    for _ in range(calls):
        out = torch.full((nq, cout + GUARD), NAN, dtype=torch.float32, device=dev)
        _lib.check(lib.apr_kpconv_fused(_lib.ptr(q), nq, _lib.ptr(s), ns, _lib.ptr(nbr), H, _lib.ptr(x), cin, cin, _lib.ptr(kp), 15,
                                        float(c["extent"]), _lib.ptr(rs), _lib.ptr(w_bf3), cout, _lib.ptr(out), cout + GUARD,
                                        _lib.stream()))
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.isnan(out[:, cout:]).all(), "columns behind cout were written"
        outs.append(out[:, :cout])
    return outs


@pytest.mark.parametrize("name", F.EXACT)
def test_exact_cases_equal_the_float64_result(dev, name):
    c = F.exact(name)
    ref = F.reference(name)[0]
    got, = _fused_direct(dev, c)
    assert not np.isnan(got).any(), "a row or column group that no wave wrote"
    bad = np.argwhere(got.astype(np.float64) != ref)
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), [(float(got[tuple(b)]), float(ref[tuple(b)])) for b in bad[:4]])


@pytest.mark.parametrize("name", F.BOUND)
def test_bound_cases_rows_and_every_element(dev, name):
    c = F.bound_case(name)
    ref = F.reference(name)[0]
    got, again = _fused_direct(dev, c, calls=2)
    assert got.tobytes() == again.tobytes(), "a second call gave other bits"
    r = F.rows_rel_l2(got, ref)
    ratio, at = F.O.compare_rows(got, ref, F.element_bound(name))
    print(f"{name}: rows rel-L2 {r:.3g}, worst |err| / bound {ratio:.4f}")
    WORST["rows"], WORST["element"] = max(WORST["rows"], r), max(WORST["element"], ratio if np.isfinite(ratio) else 1e30)
    assert r < 5e-6, r
    assert ratio <= 1.0, (ratio, at, None if at is None else (float(got[at]), float(ref[at])))


def test_print_worst_figures():
    print("fused kpconv, worst over the bound cases:", {k: float(f"{v:.3g}") for k, v in WORST.items()})
    assert WORST["rows"] < 5e-6 and WORST["element"] <= 1.0


def _wrapper_inputs(dev, cin=64, cout=64, H=5, n_kp=15, nq=9, ns=12):
    rng = np.random.default_rng(3)
    q, s = _t(rng.uniform(-1, 1, (nq, 3)).astype(np.float32), dev), _t(rng.uniform(-1, 1, (ns, 3)).astype(np.float32), dev)
    kp = _t(rng.uniform(-1, 1, (n_kp, 3)).astype(np.float32), dev)
    nbr = _t(rng.integers(0, ns + 1, (nq, H)).astype(np.int32), dev)
    x = rng.standard_normal((ns, cin)).astype(np.float32)
    W = _t((rng.standard_normal((n_kp * cin, cout)) / 30).astype(np.float32), dev)
    return q, s, nbr, x, kp, W


def test_wrapper_same_bits_twice_and_refusals(dev):
    """kp_ops.kpconv_fused: the direct call's bits, twice, also into a caller's aligned column slice; rows of x off the
    16-byte grid (slice1, ldodd) and every shape outside apr_kpconv_fused_ok raise, nothing falls back"""
    c = F.bound_case("m1-c64")
    direct, = _fused_direct(dev, c)
    q, s, nbr, kp = _t(c["q"], dev), _t(c["s"], dev), _t(c["nbr"], dev), _t(c["kp"], dev)
    w_info = kp_ops.pack_linear(_t(c["W"].reshape(15 * c["cin"], c["cout"]), dev))
    a = kp_ops.kpconv_fused(q, s, nbr, _t(c["x"], dev), kp, c["extent"], w_info)
    big = torch.full((c["nq"], c["cout"] + 8), NAN, dtype=torch.float32, device=dev)
    b = kp_ops.kpconv_fused(q, s, nbr, _t(c["x"], dev), kp, c["extent"], w_info, out=big[:, 4:4 + c["cout"]])
    assert a.cpu().numpy().tobytes() == direct.tobytes() and torch.equal(a, b)
    assert torch.isnan(big[:, :4]).all() and torch.isnan(big[:, 4 + c["cout"]:]).all()
    for layout in ("slice1", "ldodd"):
        with pytest.raises(_lib.AprHipError):
            kp_ops.kpconv_fused(q, s, nbr, _view(c["x"], layout, dev), kp, c["extent"], w_info)
    with pytest.raises(_lib.AprHipError):
        kp_ops.kpconv_fused(q, s, nbr, _t(c["x"], dev), kp, c["extent"], w_info, out=big[:, 1:1 + c["cout"]])
    with pytest.raises(_lib.AprHipError):
        kp_ops.kpconv_fused(q.cpu(), s.cpu(), nbr.cpu(), torch.from_numpy(c["x"]), kp.cpu(), c["extent"], w_info)
    for kw in (dict(H=129), dict(cin=576), dict(cout=576), dict(cin=32), dict(cout=96), dict(n_kp=14)):
        q, s, nbr, x, kp, W = _wrapper_inputs(dev, **kw)
        with pytest.raises(_lib.AprHipError):
            kp_ops.kpconv_fused(q, s, nbr, _t(x, dev), kp, 1.2, kp_ops.pack_linear(W))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the network
def _with_flags(fused_kpconv, fused_block, fn):
    """fn() under the two module flags; -> (result, levels whose ResnetBottleneckBlock took the fused route)"""
    saved = blocks.FUSED_KPCONV, blocks.FUSED_BLOCK, blocks.KPCONV_ROUTE_HOOK
    taken = []
    blocks.FUSED_KPCONV, blocks.FUSED_BLOCK = fused_kpconv, fused_block
    blocks.KPCONV_ROUTE_HOOK = lambda mod, nq, cin, cout, H: taken.append(mod)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        blocks.FUSED_KPCONV, blocks.FUSED_BLOCK, blocks.KPCONV_ROUTE_HOOK = saved
    return res, taken


def _levels(model, taken):
    level_of = {id(m.KPConv): m.layer_ind for m in model.modules() if isinstance(m, blocks.ResnetBottleneckBlock)}
    return {level_of[id(k)] for k in taken if id(k) in level_of}, set(level_of.values())


def test_network_on_the_golden_pair(dev):
    """KPFCNN on the committed small pair with every eligible KPConv on the fused kernel: the reference's own outputs at the
    thresholds of test_kpfcnn_matches_reference_golden, flag 0 at the project's 2e-5, the same bits run to run, and the
    block call against the modular path.  Under flag 2 both paths run the same KPConv kernel; the unary layers take their
    InstanceNorm statistics from the GEMM's tiles in the block call and from k_bn_partial in the modular path (the note in
    test_fused_resnet_block_call_equals_the_modular_path), so that comparison is held to the same 2e-5, not to equal bits."""
    g = np.load(os.path.join(GOLD, "predator_small.npz"))
    np.random.seed(0)
    torch.manual_seed(0)
    model = KPFCNN(kitti_config()).to(dev).eval()
    wsum = float(sum(v.double().abs().sum() for v in model.state_dict().values()))
    assert abs(wsum - float(g["weight_abs_sum"])) <= 1e-6 * wsum, "RNG streams differ from the fixture's"
    cfg = kitti_config()
    batch = collate_fn_descriptor([(g["src"], g["tgt"], np.ones((len(g["src"]), 1), np.float32),
                                   np.ones((len(g["tgt"]), 1), np.float32))], cfg, [int(v) for v in g["limits"]])
    run = lambda: [t.clone() for t in model(batch)]
    with torch.no_grad():
        (feats, ov, sal), taken = _with_flags(2, True, run)
        again, _ = _with_flags(2, True, run)
        modular, taken_mod = _with_flags(2, False, run)
        plain, none = _with_flags(0, True, run)
    got, want = _levels(model, taken)
    assert got == want and len(want) >= 3, (got, want)          # a block of every level took route 1
    assert _levels(model, taken_mod)[0] == want and not none
    assert feats.shape == g["feats"].shape
    assert rel_l2(feats.cpu(), g["feats"]) < 1e-4
    assert np.abs(ov.cpu().numpy() - g["overlap"]).max() < 1e-4
    assert np.abs(sal.cpu().numpy() - g["saliency"]).max() < 1e-4
    for a, b in zip((feats, ov, sal), again):
        assert torch.equal(a, b)
    for other in (plain, modular):
        for a, b in zip((feats, ov, sal), other):
            assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 2e-5, rel_l2(a.cpu().numpy(), b.cpu().numpy())


def test_network_stacked_pairs_equal_one_at_a_time(dev):
    """two pairs through one forward (per-pair InstanceNorm segments behind the fused kernel) against one pair at a time"""
    from apr_amd.predator.pipeline import PredatorRegistration
    cfg = kitti_config()
    np.random.seed(4)
    torch.manual_seed(4)
    model = KPFCNN(cfg).to(dev).eval()
    pipe = PredatorRegistration(model, cfg, [38, 36, 36, 38], max_iteration=20000)
    pairs = []
    for s in range(2):
        a, b, _ = synth.make_pair(40 + s, n_beams=32, n_azimuth=800 + 150 * s)
        pairs.append((torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)))
    single, taken1 = _with_flags(2, True, lambda: [pipe.encode(*p) for p in pairs])
    stacked, taken2 = _with_flags(2, True, lambda: pipe.encode_batch(pairs))
    want = _levels(model, taken1)[1]
    assert _levels(model, taken1)[0] == want and _levels(model, taken2)[0] == want
    for one, many in zip(single, stacked):
        assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])
        assert rel_l2(many[2].cpu().numpy(), one[2].cpu().numpy()) < 2e-5
        assert torch.allclose(one[3], many[3], atol=2e-5) and torch.allclose(one[4], many[4], atol=2e-5)

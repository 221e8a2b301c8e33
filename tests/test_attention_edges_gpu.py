"""The kernels of the overlap-attention module on the GPU -- edge features and their backward, group max, apr_mha,
apr_mha_headmajor, the three softmax-matvec kernels, the attention's training path and the score head -- element by
element against the float64 oracle (tests/attention_oracle.py) on the named cases of tests/attention_cases.py.  Every
threshold is a derived bound of the oracle at ratio 1, or exact equality where the oracle says exact; no element is
excused.  Inputs are the first rows of taller NaN-filled allocations (a read past the end poisons the result, where a clamp
does not), outputs are NaN-filled with guard rows that must still be NaN.  tests/test_attention_oracle_cpu.py shows on the
host that the cases hold their planted rows, that the bounds hold for float32 evaluations in three orders and that they
reject one-rule mutants.

Worst |kernel - oracle| / bound measured on the MI355X over all cases (records, not thresholds; printed by
test_print_worst_ratios):  mha 0.025,  mha_mfma 0.022,  smv 0.013,  smv_t 0.014,  smv_mfma 0.009,  P 0.116,  O 0.038,  dq 0.017,
dk 0.113,  dv 0.019,  group_max 0.489,  d_center 0.662,  score 0.432.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cases as K
import attention_oracle as O
from apr_amd import _lib
from apr_amd.predator import kp_ops
from apr_amd.predator.models import gcn

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 2
WORST = {key: 0.0 for key in ("mha", "mha_mfma", "smv", "smv_t", "smv_mfma", "P", "O", "dq", "dk", "dv", "group_max", "d_center",
                              "score")}
_REF = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _tall(values, dev, extra=3):
    """the values as the first rows of a taller NaN-filled allocation"""
    values = np.asarray(values, np.float32)
    big = torch.full((values.shape[0] + extra,) + values.shape[1:], NAN, dtype=torch.float32, device=dev)
    big[:values.shape[0]] = _t(values, dev)
    return big[:values.shape[0]]


def _view(values, extra, dev):
    """the values [r, c] as the column slice big[:, 1:c + 1] of a NaN-filled [r + 3, c + extra] buffer -> (view, ld)"""
    r, c = values.shape
    big = torch.full((r + 3, c + extra), NAN, dtype=torch.float32, device=dev)
    view = big[:r, 1:c + 1]
    view.copy_(_t(values, dev))
    return view, big.stride(0)


def _out(shape, dev):
    """NaN-filled, with GUARD rows behind the first dimension"""
    return torch.full((shape[0] + GUARD,) + tuple(shape[1:]), NAN, dtype=torch.float32, device=dev)


def _split(buf, what):
    got = buf.cpu().numpy()
    assert np.isnan(got[-GUARD:]).all(), f"{what}: the guard rows behind the output were written"
    return got[:-GUARD]


def _record(key, got, ref, bound, what):
    ratio, at = O.compare_rows(got, ref, bound)
    print(f"{what}: worst {key} ratio {ratio:.4f}")
    WORST[key] = max(WORST[key], ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _twice(run, what):
    """the kernel's result, after a second run gave the same bits"""
    a, b = run(), run()
    assert a.tobytes() == b.tobytes(), f"{what}: two runs of the same kernel differ"
    return a


def _mha_ref(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = O.mha(c["q"], c["k"], c["v"], c["H"])
    return _REF[c["name"]]


_PERM = {}


def _module_perm(ch, H, dev):
    """the permutation the module applies to its projections (gcn.py, _PackedHeadMajor): read off a bias of 0 .. ch - 1"""
    if (ch, H) not in _PERM:
        conv = torch.nn.Conv1d(ch, ch, kernel_size=1).to(dev)
        with torch.no_grad():
            conv.bias.copy_(torch.arange(ch, dtype=torch.float32, device=dev))
        _PERM[(ch, H)] = gcn._PackedHeadMajor().get(conv, H)[1].cpu().numpy().astype(np.int64)
    return _PERM[(ch, H)]


# -------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("name", list(K.ATTENTION))
def test_attention_every_element_within_bound(dev, name):
    """apr_mha on every case, apr_mha_headmajor on every case of dim 64 (inputs through the module's permutation)"""
    c = K.ATTENTION[name]
    lib = _lib.load()
    n, m, dim, H = c["n"], c["m"], c["dim"], c["H"]
    ref, bound, _ = _mha_ref(c)
    assert K.mha_takes(c)
    q, k, v = (_tall(c[key], dev) for key in ("q", "k", "v"))

    def scalar():
        out = _out((n, dim * H), dev)
        _lib.check(lib.apr_mha(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), n, m, dim, H, _lib.ptr(out), _lib.stream()))
        return _split(out, name)

    _record("mha", _twice(scalar, name), ref, bound, name)
    if dim != 64:
        return
    perm = _module_perm(dim * H, H, dev)
    assert np.array_equal(perm, O.headmajor_perm(dim * H, H)), "the module's head-major permutation changed"
    qm, km, vm = (_tall(c[key][:, perm], dev) for key in ("q", "k", "v"))

    def mfma():
        out = _out((n, dim * H), dev)
        _lib.check(lib.apr_mha_headmajor(_lib.ptr(qm), _lib.ptr(km), _lib.ptr(vm), n, m, dim, H, _lib.ptr(out), _lib.stream()))
        return _split(out, name + "/headmajor")

    _record("mha_mfma", _twice(mfma, name + "/headmajor"), ref, bound, name + "/headmajor")


def test_attention_wrappers_meet_the_oracle(dev):
    c = K.MHA["mha-n9-m257"]
    ref, bound, _ = _mha_ref(c)
    q, k, v = (_tall(c[key], dev) for key in ("q", "k", "v"))
    _record("mha", kp_ops.mha(q, k, v, c["H"]).cpu().numpy(), ref, bound, "kp_ops.mha")
    perm = O.headmajor_perm(c["dim"] * c["H"], c["H"])
    qm, km, vm = (_tall(c[key][:, perm], dev) for key in ("q", "k", "v"))
    _record("mha_mfma", kp_ops.mha_headmajor(qm, km, vm, c["H"]).cpu().numpy(), ref, bound, "kp_ops.mha_headmajor")


# --------------------------------------------------------------------------------------------------- softmax-matvec
@pytest.mark.parametrize("name", list(K.SMV))
def test_softmax_matvec_every_element_within_bound(dev, name, monkeypatch):
    """every entry point that takes the shape, called directly; then kp_ops.softmax_matvec, whose route is asserted"""
    c = K.SMV[name]
    lib = _lib.load()
    n, m, ch = c["n"], c["m"], c["dim"]
    T = K.temperature(ch)
    assert c["scale"] == 1.0 / T
    if name not in _REF:
        _REF[name] = O.softmax_matvec(c["q"], c["k"], c["v"][:, 0], T)
    ref, bound = _REF[name]
    a, b, w = _tall(c["q"], dev), _tall(c["k"], dev), _tall(c["v"][:, 0], dev)
    bt = _tall(np.ascontiguousarray(c["k"].T), dev)
    entries = [("smv", lib.apr_softmax_matvec, b)]
    if m + ch <= 3840:
        entries.append(("smv_t", lib.apr_softmax_matvec_bt, bt))
    if ch in (32, 64, 128, 256):
        entries.append(("smv_mfma", lib.apr_softmax_matvec_mfma, b))
    if name == "smv-common":
        assert len(entries) == 3
    for key, fn, keys in entries:
        def run():
            out = _out((n,), dev)
            _lib.check(fn(_lib.ptr(a), _lib.ptr(keys), _lib.ptr(w), n, m, ch, T, _lib.ptr(out), _lib.stream()))
            return _split(out, f"{name}/{key}")
        _record(key, _twice(run, f"{name}/{key}"), ref, bound, f"{name}/{key}")
    called = []
    for route, fname in (("first", "apr_softmax_matvec"), ("transposed", "apr_softmax_matvec_bt"), ("mfma", "apr_softmax_matvec_mfma")):
        real = getattr(lib, fname)
        monkeypatch.setattr(lib, fname, lambda *args, _r=route, _f=real: (called.append(_r), _f(*args))[1], raising=False)
    got = kp_ops.softmax_matvec(a, b, w, T).cpu().numpy()
    route = K.expected_route(n, m, ch)
    assert called == [route], (called, route)
    _record({"first": "smv", "transposed": "smv_t", "mfma": "smv_mfma"}[route], got, ref, bound, f"{name}/kp_ops")


# ---------------------------------------------------------------------------------------------------- training path
@pytest.mark.parametrize("name", list(K.TRAIN))
def test_training_path_every_element_within_bound(dev, name):
    c = K.TRAIN[name]
    lib = _lib.load()
    n, m, dim, H, vdim = c["n"], c["m"], c["dim"], c["H"], c["vdim"]
    ref = O.mha_train(c["q"], c["k"], c["v"], c["dout"], H)
    q, k, v, g = (_tall(c[key], dev) for key in ("q", "k", "v", "dout"))

    def run():
        P, out = _out((H, n, m), dev), _out((n, vdim * H), dev)
        _lib.check(lib.apr_mha_train_forward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), n, m, dim, H, vdim, _lib.ptr(P), _lib.ptr(out),
                                             _lib.stream()))
        dS = _out((H, n, m), dev)
        dq, dk, dv = _out((n, dim * H), dev), _out((m, dim * H), dev), _out((m, vdim * H), dev)
        _lib.check(lib.apr_mha_train_backward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(P), _lib.ptr(g), n, m, dim, H, vdim,
                                              _lib.ptr(dS), _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.stream()))
        res = {key: _split(buf, f"{name}/{key}") for key, buf in (("P", P), ("O", out), ("dS", dS), ("dq", dq), ("dk", dk), ("dv", dv))}
        return res

    first, second = run(), run()
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), f"{name}/{key}: two runs differ"
    for key in ("P", "O", "dq", "dk", "dv"):
        _record(key, first[key], *ref[key], f"{name}/{key}")
    # the same through the autograd function (for vdim 1: MHAFunction.apply(q, b, w[:, None], 1), the cross-saliency call)
    qa, ka, va = (_tall(c[key], dev).requires_grad_(True) for key in ("q", "k", "v"))
    out = kp_ops.MHAFunction.apply(qa, ka, va, H)
    assert tuple(out.shape) == (n, vdim * H)
    out.backward(g)
    for key, got in (("O", out.detach()), ("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        _record(key, got.cpu().numpy(), *ref[key], f"{name}/MHAFunction/{key}")


# ----------------------------------------------------------------------------------------------------- edge kernels
@pytest.mark.parametrize("name", list(K.EDGE))
def test_edge_features_exact(dev, name):
    c = K.EDGE[name]
    lib = _lib.load()
    n, ch, k = c["n"], c["c"], c["k"]
    knn = _t(c["knn"], dev)
    ref = O.edge_features_f32(c["f"], c["knn"])
    for layout, (f, ldf) in (("rows", (_tall(c["f"], dev), ch)), ("slice", _view(c["f"], 8, dev))):
        out = _out((n * k, 2 * ch), dev)
        _lib.check(lib.apr_edge_features(_lib.ptr(f), ldf, n, ch, _lib.ptr(knn), k, _lib.ptr(out), _lib.stream()))
        got = _split(out, name)
        assert np.array_equal(got[:, :ch], ref[:, :ch]), (name, layout, "the centre half is not f[i]")
        assert np.array_equal(got[:, ch:], ref[:, ch:]), (name, layout, "the second half is not the float32 f[knn] - f[i]")
        assert not np.isnan(got).any()
    assert np.array_equal(kp_ops.edge_features(_tall(c["f"], dev), knn).cpu().numpy(), ref)


def _edge_backward(dev, name, n, ch, k, de_host):
    lib = _lib.load()
    dc_ref, contrib_ref, bound = O.edge_features_backward(de_host, n, k)
    de = _tall(de_host, dev)
    ldd = ch + 3

    def run():
        dc = torch.full((n + GUARD, ldd), NAN, dtype=torch.float32, device=dev)
        contrib = _out((n * k, ch), dev)
        _lib.check(lib.apr_edge_features_backward(_lib.ptr(de), n, ch, k, _lib.ptr(dc), ldd, _lib.ptr(contrib), _lib.stream()))
        dc = _split(dc, name + "/d_center")
        assert np.isnan(dc[:, ch:]).all(), "columns behind c were written"
        return np.ascontiguousarray(dc[:, :ch]), _split(contrib, name + "/contrib")

    dc, contrib = run()
    dc2, contrib2 = run()
    assert dc.tobytes() == dc2.tobytes() and contrib.tobytes() == contrib2.tobytes()
    assert np.array_equal(contrib, contrib_ref.astype(np.float32))
    _record("d_center", dc, dc_ref, bound, name)


@pytest.mark.parametrize("name", [n for n in K.EDGE if n != "e-sweep"])
def test_edge_features_backward(dev, name):
    c = K.EDGE[name]
    _edge_backward(dev, name, c["n"], c["c"], c["k"], c["de"])


def test_edge_features_backward_past_one_sweep(dev):
    s = K.EDGE_BWD_SWEEP
    de = np.random.default_rng(s["seed"]).standard_normal((s["n"] * s["k"], 2 * s["c"]), dtype=np.float32)
    _edge_backward(dev, "e-bwd-sweep", s["n"], s["c"], s["k"], de)


@pytest.mark.parametrize("name", list(K.GROUP))
def test_group_max_every_element_within_bound(dev, name):
    c = K.GROUP[name]
    lib = _lib.load()
    n, k, ch = c["n"], c["k"], c["c"]
    ref, bound = O.group_max(c["y"], n, k, c["scale"], c["shift"], c["slope"])
    y, ldy = _view(c["y"], c["ldy_extra"], dev) if c["ldy_extra"] else (_tall(c["y"], dev), ch)
    scale = None if c["scale"] is None else _tall(c["scale"], dev)
    shift = None if c["shift"] is None else _tall(c["shift"], dev)
    ldo = ch + c["ldo_extra"]
    out = torch.full((n + GUARD, ldo), NAN, dtype=torch.float32, device=dev)
    _lib.check(lib.apr_group_max(_lib.ptr(y), ldy, n, k, ch, _lib.ptr(scale), _lib.ptr(shift), c["slope"], _lib.ptr(out), ldo,
                                 _lib.stream()))
    got = _split(out, name)
    assert np.isnan(got[:, ch:]).all(), "columns behind c were written"
    _record("group_max", got[:, :ch], ref, bound, name)
    if c["slope"] == 0.0:
        assert not got[0, :ch].any(), "an all-negative group under slope 0 is exactly 0"
    if not c["ldy_extra"]:
        _record("group_max", kp_ops.group_max(y, n, k, scale, shift, c["slope"]).cpu().numpy(), ref, bound, name + "/kp_ops")


# ------------------------------------------------------------------------------------------------------- score head
def test_score_head(dev):
    lib = _lib.load()
    n = 257
    x = K.score_case(n)
    ref, bound = O.score_head(x)
    big = torch.full((n + 3, 5), NAN, dtype=torch.float32, device=dev)
    big[:n, 2] = _t(x, dev)
    col = big[:n, 2]
    out = _out((n,), dev)
    _lib.check(lib.apr_score_head(_lib.ptr(col), 5, 0, _lib.ptr(out), _lib.stream()))
    assert np.isnan(out.cpu().numpy()).all(), "n = 0 wrote something"
    _lib.check(lib.apr_score_head(_lib.ptr(col), 5, n, _lib.ptr(out), _lib.stream()))
    got = _split(out, "score")
    exact = sorted(i for i, val in K.SCORE_SPECIALS.items() if not np.isfinite(val) or abs(val) == 200.0)
    assert np.array_equal(got[exact], ref[exact].astype(np.float32)), (got[exact], ref[exact])
    assert got[0] == 0 and got[1] == 1 and got[2] == 0 and got[3] == 0 and got[4] == 1
    fin = np.isfinite(x)
    _record("score", got[fin], ref[fin], bound[fin], "score")
    _record("score", kp_ops.score_head(col).cpu().numpy()[fin], ref[fin], bound[fin], "score/kp_ops")


# --------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", list(K.REFUSED))
def test_refusals(dev, name):
    """the argument error as it stands, and nothing written to the output"""
    r = K.REFUSED[name]
    lib = _lib.load()
    rng = np.random.default_rng(5)
    rand = lambda *shape: _t(rng.standard_normal(shape).astype(np.float32), dev)
    pattern = lambda count: torch.full((count * 4,), 0xA5, dtype=torch.uint8, device=dev)
    n, m, fn = r["n"], r["m"], r["fn"]
    outs = []
    if fn in ("mha", "headmajor", "train"):
        ch = r["dim"] * r["H"]
        q, k, v = rand(n, ch + 4), rand(m, ch + 4), rand(m, ch + 4)
        off = 4 * r.get("off", 0)
        qp = C.c_void_p(q.data_ptr() + off)
        outs = [pattern(n * ch)]
        if fn == "train":
            outs.append(pattern(r["H"] * n * m))
            rc = lib.apr_mha_train_forward(qp, _lib.ptr(k), _lib.ptr(v), n, m, r["dim"], r["H"], 0, _lib.ptr(outs[1]), _lib.ptr(outs[0]),
                                           _lib.stream())
        else:
            call = lib.apr_mha if fn == "mha" else lib.apr_mha_headmajor
            rc = call(qp, _lib.ptr(k), _lib.ptr(v), n, m, r["dim"], r["H"], _lib.ptr(outs[0]), _lib.stream())
    else:
        ch = r["c"]
        a, b, w = rand(n, ch), rand(m, ch), rand(m)
        outs = [pattern(n)]
        call = {"smv": lib.apr_softmax_matvec, "smv_bt": lib.apr_softmax_matvec_bt, "smv_mfma": lib.apr_softmax_matvec_mfma}[fn]
        rc = call(_lib.ptr(a), _lib.ptr(b), _lib.ptr(w), n, m, ch, r["T"], _lib.ptr(outs[0]), _lib.stream())
    assert rc == -1                                     # APR_EINVAL
    assert lib.apr_last_error().decode()
    torch.cuda.synchronize()
    for buf in outs:
        assert bool((buf == 0xA5).all()), "a refused call wrote to its output"


def test_print_worst_ratios():
    print("worst kernel / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())

"""The kernels of the geometric cross attention ('cross_cat', apr_amd/csrc/attention_cat.hip) on the GPU -- apr_mha_cat_headmajor,
apr_mha_cat_train_forward and apr_mha_cat_train_backward -- element by element against the float64 oracle
(tests/attention_cat_oracle.py) on the named cases of tests/attention_cat_cases.py.  Every case runs through every entry that
takes its shape; every threshold is the oracle's derived bound at ratio 1, the inference kernel and the training forward each
held to the oracle, not to each other.  Inputs are the first rows of taller NaN-filled allocations, outputs are NaN-filled with
guard rows behind them and guard columns between (dim + 7) * H and ldy that must still be NaN; each entry runs twice and the
two results must agree bit for bit.  tests/test_attention_cat_oracle_cpu.py shows on the host that the cases hold their planted
rows, that the bounds hold for float32 evaluations in two orders and that they reject one-rule mutants.

Worst |kernel - oracle| / bound measured on the MI355X over all cases (records, not thresholds; printed by
test_print_worst_ratios):  y_mfma 0.022,  y_train 0.137,  dq 0.028,  dk 0.040,  dv 0.060.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_cat_cases as K
import attention_cat_oracle as CO
import attention_oracle as O
from apr_amd import _lib
from apr_amd.predator import kp_ops

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 2
WORST = {key: 0.0 for key in ("y_mfma", "y_train", "dq", "dk", "dv")}
_REF = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _tall(values, dev, extra=3):
    """the values as the first rows of a taller NaN-filled allocation"""
    values = np.asarray(values, np.float32)
    big = torch.full((values.shape[0] + extra,) + values.shape[1:], NAN, dtype=torch.float32, device=dev)
    big[:values.shape[0]] = _t(values, dev)
    return big[:values.shape[0]]


def _wide(values, ld, dev):
    """the values [r, c] as the first rows and columns of a NaN-filled [r + 3, ld] buffer (the whole buffer is returned)"""
    r, c = values.shape
    big = torch.full((r + 3, ld), NAN, dtype=torch.float32, device=dev)
    big[:r, :c] = _t(np.asarray(values, np.float32), dev)
    return big


def _out(shape, dev):
    """NaN-filled, with GUARD rows behind the first dimension"""
    return torch.full((shape[0] + GUARD,) + tuple(shape[1:]), NAN, dtype=torch.float32, device=dev)


def _split(buf, what, cols=None):
    got = buf.cpu().numpy()
    assert np.isnan(got[-GUARD:]).all(), f"{what}: the guard rows behind the output were written"
    got = got[:-GUARD]
    if cols is not None:
        assert np.isnan(got[:, cols:]).all(), f"{what}: the guard columns behind (dim + 7) * H were written"
        got = np.ascontiguousarray(got[:, :cols])
    return got


def _record(key, got, ref, bound, what):
    ratio, at = O.compare_rows(got, ref, bound)
    print(f"{what}: worst {key} ratio {ratio:.4f}")
    WORST[key] = max(WORST[key], ratio if np.isfinite(ratio) else 1e30)
    assert ratio <= 1.0, (what, key, ratio, at, None if at is None else (float(got[at]), float(ref[at]), float(bound[at])))


def _ref(c):
    """the oracle's values and bounds, computed once per case and left unchanged"""
    if c["name"] not in _REF:
        _REF[c["name"]] = CO.train(c["q"], c["k"], c["v"], c["c0"], c["c1"], c["dy"], c["H"])
    return _REF[c["name"]]


def _planted(c, y, what):
    """the planted zero: aug1 and aug2 of the zero rows are exactly 0 in every head"""
    dim, H = c["dim"], c["H"]
    for i in c["zero_rows"]:
        assert not y[i, (dim + 3) * H:(dim + 7) * H].any(), f"{what}: aug1 / aug2 of the planted row are not exactly 0"
        assert np.array_equal(y[i, dim * H:(dim + 3) * H].reshape(3, H), np.repeat(c["c1"][0][:, None], H, 1)), \
            f"{what}: one key, but soft is not c1[0]"


@pytest.mark.parametrize("name", list(K.CASES))
def test_every_element_within_bound(dev, name):
    c = K.CASES[name]
    lib = _lib.load()
    n, m, dim, H = c["n"], c["m"], c["dim"], c["H"]
    cy = (dim + 7) * H
    ref = _ref(c)
    q, k, v, c0, c1 = (_tall(c[key], dev) for key in ("q", "k", "v", "c0", "c1"))

    if dim == 64:
        perm = O.headmajor_perm(dim * H, H)
        qm, km, vm = (_tall(c[key][:, perm], dev) for key in ("q", "k", "v"))
        ld = 288                                    # the rows the module hands to the merge GEMM: 284 columns and 4 of pad

        def mfma():
            y = _out((n, ld), dev)
            _lib.check(lib.apr_mha_cat_headmajor(_lib.ptr(qm), _lib.ptr(km), _lib.ptr(vm), _lib.ptr(c0), _lib.ptr(c1), n, m, dim, H,
                                                 _lib.ptr(y), ld, _lib.stream()))
            return _split(y, name + "/headmajor", cy)

        a, b = mfma(), mfma()
        assert a.tobytes() == b.tobytes(), f"{name}/headmajor: two runs differ"
        _record("y_mfma", a, *ref["y"], name + "/headmajor")
        _planted(c, a, name + "/headmajor")

    ld = cy + 5
    g = _wide(c["dy"], ld, dev)

    def train():
        P, y = _out((H, n, m), dev), _out((n, ld), dev)
        _lib.check(lib.apr_mha_cat_train_forward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(c0), _lib.ptr(c1), n, m, dim, H,
                                                 _lib.ptr(P), _lib.ptr(y), ld, _lib.stream()))
        dS = _out((H, n, m), dev)
        dq, dk, dv = _out((n, dim * H), dev), _out((m, dim * H), dev), _out((m, dim * H), dev)
        _lib.check(lib.apr_mha_cat_train_backward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(c0), _lib.ptr(c1), _lib.ptr(P),
                                                  _lib.ptr(y), _lib.ptr(g), ld, n, m, dim, H, _lib.ptr(dS), _lib.ptr(dq), _lib.ptr(dk),
                                                  _lib.ptr(dv), _lib.stream()))
        res = {key: _split(buf, f"{name}/{key}") for key, buf in (("P", P), ("dS", dS), ("dq", dq), ("dk", dk), ("dv", dv))}
        res["y"] = _split(y, f"{name}/y", cy)
        return res

    first, second = train(), train()
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), f"{name}/{key}: two runs differ"
    _record("y_train", first["y"], *ref["y"], name + "/train")
    _planted(c, first["y"], name + "/train")
    for key in ("dq", "dk", "dv"):
        assert np.isfinite(first[key]).all()
        _record(key, first[key], *ref[key], f"{name}/{key}")
    if m == 1:
        assert not first["dS"].any() and not first["dq"].any() and not first["dk"].any(), "one key: dS = 0"

    # the same through the autograd function and the wrappers
    qa, ka, va = (_tall(c[key], dev).requires_grad_(True) for key in ("q", "k", "v"))
    y = kp_ops.MHACatFunction.apply(qa, ka, va, c0, c1, H)
    assert tuple(y.shape) == (n, cy)
    y.backward(_t(c["dy"], dev))
    for key, got in (("y_train", y.detach()), ("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        _record(key, got.cpu().numpy(), *ref["y" if key == "y_train" else key], f"{name}/MHACatFunction/{key}")
    if dim == 64:
        yp = kp_ops.mha_cat_headmajor(qm, km, vm, c0, c1, H, padded=True)
        assert tuple(yp.shape) == (n, 288) and not yp[:, cy:].any(), "the pad columns of the wrapper's rows must be zero"
        _record("y_mfma", yp[:, :cy].cpu().numpy(), *ref["y"], name + "/kp_ops.mha_cat_headmajor")
        assert torch.equal(kp_ops.mha_cat_headmajor(qm, km, vm, c0, c1, H), yp[:, :cy])


@pytest.mark.parametrize("name", ["cat-n16-m16", "cat-n15-m15", "cat-n33-m63"])
@pytest.mark.parametrize("form", ["float64", "transposed"])
def test_wrappers_convert_both_coordinate_tensors(dev, name, form):
    """coordinates the wrappers have to copy -- float64, or the [N, 3] view of the reference's [3, N] layout -- BOTH at once:
    each converted copy must live until the kernel has been launched (n == m: two copies of one size, where a freed first
    copy would be handed out again for the second)"""
    c = K.CASES[name]
    H, cy = c["H"], (c["dim"] + 7) * c["H"]
    ref = _ref(c)
    if form == "float64":
        c0, c1 = _t(c["c0"], dev).double(), _t(c["c1"], dev).double()
    else:
        c0, c1 = _t(np.ascontiguousarray(c["c0"].T), dev).t(), _t(np.ascontiguousarray(c["c1"].T), dev).t()
        assert not c0.is_contiguous() or c["n"] == 1
    perm = O.headmajor_perm(c["dim"] * H, H)
    qm, km, vm = (_tall(c[key][:, perm], dev) for key in ("q", "k", "v"))
    for padded in (False, True):
        y = kp_ops.mha_cat_headmajor(qm, km, vm, c0, c1, H, padded=padded)
        _record("y_mfma", y[:, :cy].cpu().numpy(), *ref["y"], f"{name}/{form}/mha_cat_headmajor")
    q, k, v = (_tall(c[key], dev) for key in ("q", "k", "v"))
    with torch.no_grad():
        y = kp_ops.mha_cat(q, k, v, c0, c1, H)
    _record("y_train", y.cpu().numpy(), *ref["y"], f"{name}/{form}/mha_cat")


def test_torch_statement_meets_the_oracle(dev):
    """the torch-op statement of the layer (the route when the HIP training switch is off), values and gradients"""
    c = K.CASES["cat-d16-n33-m130"]
    ref = _ref(c)
    qa, ka, va = (_t(c[key], dev).double().requires_grad_(True) for key in ("q", "k", "v"))
    y = kp_ops.mha_cat_torch(qa, ka, va, _t(c["c0"], dev).double(), _t(c["c1"], dev).double(), c["H"])
    y.backward(_t(c["dy"], dev).double())
    for key, got in (("y", y.detach()), ("dq", qa.grad), ("dk", ka.grad), ("dv", va.grad)):
        assert np.allclose(got.cpu().numpy(), ref[key][0], rtol=1e-9, atol=1e-9), key


@pytest.mark.parametrize("name", list(K.REFUSED))
def test_refusals(dev, name):
    """the argument error as it stands, and nothing written to any output"""
    r = K.REFUSED[name]
    lib = _lib.load()
    rng = np.random.default_rng(5)
    rand = lambda *shape: _t(rng.standard_normal(shape).astype(np.float32), dev)
    pattern = lambda count: torch.full((count * 4,), 0xA5, dtype=torch.uint8, device=dev)
    n, m, dim, H = r["n"], r["m"], r["dim"], 4
    ch, cy = dim * H, (dim + 7) * H
    ldy = r.get("ldy", cy)
    q, k, v, c0, c1 = rand(n, ch + 4), rand(m, ch + 4), rand(m, ch + 4), rand(n, 3), rand(m, 3)
    qp = C.c_void_p(q.data_ptr() + 4 * r.get("off", 0))
    y = pattern(n * cy)
    outs = [y]
    if r["fn"] == "headmajor":
        rc = lib.apr_mha_cat_headmajor(qp, _lib.ptr(k), _lib.ptr(v), _lib.ptr(c0), _lib.ptr(c1), n, m, dim, H, _lib.ptr(y), ldy,
                                       _lib.stream())
    else:
        P = pattern(H * n * m)
        outs.append(P)
        rc = lib.apr_mha_cat_train_forward(qp, _lib.ptr(k), _lib.ptr(v), _lib.ptr(c0), _lib.ptr(c1), n, m, dim, H, _lib.ptr(P),
                                           _lib.ptr(y), ldy, _lib.stream())
        assert rc == -1
        grads = [pattern(H * n * m), pattern(n * ch), pattern(m * ch), pattern(m * ch)]
        outs += grads
        rc = lib.apr_mha_cat_train_backward(qp, _lib.ptr(k), _lib.ptr(v), _lib.ptr(c0), _lib.ptr(c1), _lib.ptr(P), _lib.ptr(y),
                                            _lib.ptr(y), ldy, n, m, dim, H, *(_lib.ptr(b) for b in grads), _lib.stream())
    assert rc == -1                                     # APR_EINVAL
    assert lib.apr_last_error().decode()
    torch.cuda.synchronize()
    for buf in outs:
        assert bool((buf == 0xA5).all()), "a refused call wrote to its output"


def test_print_worst_ratios():
    print("worst kernel / bound:", {k: round(v, 4) for k, v in WORST.items()})
    assert all(v <= 1.0 for v in WORST.values())

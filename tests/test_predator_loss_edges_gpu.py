"""Every entry point of apr_amd/csrc/metric_loss.hip on the GPU, row by row and element by element against the float64 oracle
(tests/predator_loss_edges_oracle.py) on the named cases of tests/predator_loss_edges_cases.py.  The library entries are
called directly into sentinel-filled buffers; one more pass goes through the ops wrappers and MetricLoss.

Thresholds are the oracle's derived bounds (ratio 1) and equality where the oracle says exact (index lists, counts, flags,
labels, gathered rows, arg-min, arg-max).  Nothing is excluded: no row, no arg-max.  tests/
test_predator_loss_edges_oracle_cpu.py shows on the host that every case decides with a margin above its bound, that a float32
evaluation in the kernels' structure stays inside the bounds, and that they reject the planted faults.

Worst |kernel - oracle| / bound measured on the MI355X (records, not thresholds; every test prints its own, `pytest -s`): the
table in DESIGN.md, section 39.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import predator_loss_edges_cases as K
import predator_loss_edges_oracle as O
from apr_amd import _lib, ops

pytestmark = pytest.mark.gpu
SF, SI = -7.5, -77                 # sentinels: no kernel output takes these values
PAD = 3
ptr, check = _lib.ptr, _lib.check


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _f(shape, dev):
    return torch.full(shape, SF, dtype=torch.float32, device=dev)


def _i(shape, dev):
    return torch.full(shape, SI, dtype=torch.int32, device=dev)


def _np(d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def _same_bits(a, b):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{k} differs between two calls"


def _report(name, v):
    k, x = K.worst(v)
    bounded = {k: x for k, x in v.items() if 0 < x < np.inf}
    print(f"{name}: worst ratio {x:.4f} ({k}); " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(bounded.items())))
    assert x <= 1.0, (name, {k: x for k, x in v.items() if x > 1.0})


def _params(q):
    return (C.c_float * 7)(*O.param_vec(q))


# ------------------------------------------------------------------------------------------------------ direct calls
def _select_direct(dev, c):
    lib = _lib.load()
    corr = _t(c["corr"], dev)
    src, tgt, rot, trans = (_t(c[k], dev) for k in ("src_pcd", "tgt_pcd", "rot", "trans"))
    n = len(c["corr"])
    filt, count = _i((max(n, 1) + PAD,), dev), _i((1,), dev)
    check(lib.apr_circle_select(ptr(corr), n, ptr(src), len(c["src_pcd"]), ptr(tgt), len(c["tgt_pcd"]), ptr(rot), ptr(trans),
                                float(c["thresh"]), ptr(filt), ptr(count), _lib.stream()))
    return dict(filt=filt, count=count), (corr, src, tgt, rot, trans)


def _anchors_direct(dev, c):
    lib = _lib.load()
    sel, (corr, src, tgt, rot, trans) = _select_direct(dev, c)
    sf, tf, choice = _t(c["src_feats"], dev), _t(c["tgt_feats"], dev), _t(c["choice"], dev)
    P, D = c["P"], O.D
    g = dict(a_row=_i((P + PAD,), dev), b_row=_i((P + PAD,), dev), a_pts=_f((P + PAD, 3), dev), b_pts=_f((P + PAD, 3), dev),
             a_feats=_f((P + PAD, D), dev), b_feats=_f((P + PAD, D), dev))
    check(lib.apr_circle_gather(ptr(corr), ptr(sel["filt"]), ptr(sel["count"]), ptr(choice), P, ptr(src), ptr(tgt), ptr(sf), ptr(tf), D,
                                ptr(rot), ptr(trans), ptr(g["a_row"]), ptr(g["b_row"]), ptr(g["a_pts"]), ptr(g["b_pts"]),
                                ptr(g["a_feats"]), ptr(g["b_feats"]), _lib.stream()))
    st_a, st_b, out4, nn = _f((P + PAD, 8), dev), _f((P + PAD, 8), dev), _f((4 + PAD,), dev), _i((P + PAD,), dev)
    q = _params(c["q"])
    check(lib.apr_circle_forward(ptr(g["a_feats"]), ptr(g["a_pts"]), ptr(g["a_row"]), P, ptr(g["b_feats"]), ptr(g["b_pts"]),
                                 ptr(g["b_row"]), P, None, None, q, ptr(st_a), ptr(st_b), ptr(out4), ptr(nn), _lib.stream()))
    go = _t(np.array([c["grad_out"]], np.float32), dev)
    d_a, d_b = _f((P + PAD, D), dev), _f((P + PAD, D), dev)
    check(lib.apr_circle_backward(ptr(g["a_feats"]), ptr(g["a_pts"]), ptr(g["a_row"]), P, ptr(g["b_feats"]), ptr(g["b_pts"]),
                                  ptr(g["b_row"]), P, None, None, q, ptr(st_a), ptr(st_b), ptr(out4), ptr(go), ptr(d_a), ptr(d_b),
                                  None, _lib.stream()))
    n_src, n_tgt = len(c["src_pcd"]), len(c["tgt_pcd"])
    d_src, d_tgt = torch.zeros((n_src + PAD, D), device=dev), torch.zeros((n_tgt + PAD, D), device=dev)
    d_src[n_src:], d_tgt[n_tgt:] = SF, SF
    check(lib.apr_circle_scatter(ptr(d_a), ptr(g["a_row"]), P, D, ptr(d_src), n_src, _lib.stream()))
    check(lib.apr_circle_scatter(ptr(d_b), ptr(g["b_row"]), P, D, ptr(d_tgt), n_tgt, _lib.stream()))
    raw = _np(dict(g, filt=sel["filt"], count=sel["count"], st_a=st_a, st_b=st_b, out4=out4, nn=nn, d_a=d_a, d_b=d_b, d_src=d_src,
                   d_tgt=d_tgt))
    tails = {k: (raw[k][P:] if k not in ("filt", "count", "out4", "d_src", "d_tgt", "st_a", "st_b", "nn") else None) for k in raw}
    tails.update(out4=raw["out4"][4:], d_src=raw["d_src"][n_src:], d_tgt=raw["d_tgt"][n_tgt:])
    got = dict(raw, count=int(raw["count"][0]), out4=raw["out4"][:4], d_src=raw["d_src"][:n_src], d_tgt=raw["d_tgt"][:n_tgt])
    for k in ("a_row", "b_row", "a_pts", "b_pts", "a_feats", "b_feats", "d_a", "d_b"):
        got[k] = raw[k][:P]
    return got, raw, tails


@pytest.mark.parametrize("name", K.NAMES["anchors"])
def test_anchor_route_every_record_and_gradient_element(dev, name):
    """select -> gather -> forward -> backward -> scatter through the library entries: lists, rows, flags and arg-min exact,
    every record element, out4 and every gradient element inside its bound, NaN where the oracle has NaN, absent and
    untouched rows exactly zero, every sentinel behind a count or a length intact, a second call bit-identical."""
    c = K.get(name)
    got, raw, tails = _anchors_direct(dev, c)
    for k, t in tails.items():
        if t is not None:
            assert (t == (SI if t.dtype.kind == "i" else SF)).all(), f"{k}: written behind its length"
    _report(name, K.judge_anchors(name, got, SF, SI))
    _same_bits(raw, _anchors_direct(dev, c)[1])


def _dense_direct(dev, c):
    lib = _lib.load()
    na, nb = c["na"], c["nb"]
    cd, fd = _t(c["cd"], dev), _t(c["fd"], dev)
    st_a, st_b, out4, nn = _f((na + PAD, 8), dev), _f((nb + PAD, 8), dev), _f((4 + PAD,), dev), _i((na + PAD,), dev)
    q = _params(c["q"])
    check(lib.apr_circle_forward(None, None, None, na, None, None, None, nb, ptr(cd), ptr(fd), q, ptr(st_a), ptr(st_b), ptr(out4),
                                 ptr(nn), _lib.stream()))
    go = _t(np.array([c["grad_out"]], np.float32), dev)
    d_fd = _f((na * nb + PAD,), dev)
    check(lib.apr_circle_backward(None, None, None, na, None, None, None, nb, ptr(cd), ptr(fd), q, ptr(st_a), ptr(st_b), ptr(out4),
                                  ptr(go), None, None, ptr(d_fd), _lib.stream()))
    raw = _np(dict(st_a=st_a, st_b=st_b, out4=out4, nn=nn, d_fd=d_fd))
    assert (raw["out4"][4:] == SF).all() and (raw["d_fd"][na * nb:] == SF).all()
    return dict(raw, out4=raw["out4"][:4], d_fd=raw["d_fd"][:na * nb].reshape(na, nb)), raw


@pytest.mark.parametrize("name", K.NAMES["dense"])
def test_dense_route_every_record_and_gradient_element(dev, name):
    """the two distance matrices, not square, with the strides swapped for the column pass; entries on and next to the two
    radii decide exactly as float32 comparisons do"""
    c = K.get(name)
    got, raw = _dense_direct(dev, c)
    _report(name, K.judge_dense(name, got, SF, SI))
    _same_bits(raw, _dense_direct(dev, c)[1])


def _labels_direct(dev, c):
    lib = _lib.load()
    ns, nt, n = c["n_src"], c["n_tgt"], len(c["corr"])
    corr = _t(c["corr"], dev)
    gt, src_idx, tgt_idx, counts = _f((ns + nt + PAD,), dev), _i((ns + PAD,), dev), _i((nt + PAD,), dev), _i((3 + PAD,), dev)
    check(lib.apr_overlap_labels(ptr(corr), n, ns, nt, ptr(gt), ptr(src_idx), ptr(tgt_idx), ptr(counts), _lib.stream()))
    sel, _ = _select_direct(dev, c)
    raw = _np(dict(gt=gt, src_idx=src_idx, tgt_idx=tgt_idx, counts=counts, filt=sel["filt"], count=sel["count"]))
    assert (raw["gt"][ns + nt:] == SF).all() and (raw["counts"][3:] == SI).all()
    return dict(raw, gt=raw["gt"][:ns + nt], counts=raw["counts"][:3], count=int(raw["count"][0])), raw


@pytest.mark.parametrize("name", K.NAMES["select"])
def test_overlap_labels_and_select_lists_are_exact(dev, name):
    """apr_overlap_labels and apr_circle_select called directly: gt, the ascending lists, the filtered list in input order and
    the counts equal the oracle's; the tails of the three lists keep their sentinel"""
    c = K.get(name)
    got, raw = _labels_direct(dev, c)
    _report(name, K.judge_select(name, got, SI))
    _same_bits(raw, _labels_direct(dev, c)[1])


def _argmax_direct(dev, a, a_idx, na_dev, b, b_idx, nb_dev):
    lib = _lib.load()
    ta, tb, ia, ib = _t(a, dev), _t(b, dev), _t(a_idx, dev, torch.int32), _t(b_idx, dev, torch.int32)
    nad, nbd = _t(np.array([na_dev], np.int32), dev), _t(np.array([nb_dev], np.int32), dev)
    row, col = _i((len(a_idx) + PAD,), dev), _i((len(b_idx) + PAD,), dev)
    check(lib.apr_gathered_argmax(ptr(ta), ptr(ia), ptr(nad), len(a_idx), ptr(tb), ptr(ib), ptr(nbd), len(b_idx), O.D, ptr(row),
                                  ptr(col), _lib.stream()))
    return _np(dict(row_arg=row, col_arg=col))


@pytest.mark.parametrize("name", K.NAMES["argmax"])
def test_gathered_argmax_equals_the_oracle_everywhere(dev, name):
    """every arg-max of both directions (the oracle's margin exceeds the score bound everywhere, by construction), planted
    ties on the lowest index, all-negative rows not won by a padded column, nothing written past min(n_dev, length)"""
    c = K.get(name)
    got = _argmax_direct(dev, c["a"], c["a_idx"], c["na_dev"], c["b"], c["b_idx"], c["nb_dev"])
    _report(name, K.judge_argmax(name, got, SI))
    _same_bits(got, _argmax_direct(dev, c["a"], c["a_idx"], c["na_dev"], c["b"], c["b_idx"], c["nb_dev"]))


def _saliency_direct(dev, c, r):
    lib = _lib.load()
    lab, am = r["lab"], r["am"]
    ns, nt = c["n_src"], c["n_tgt"]
    pad_i = lambda v, n: np.concatenate([v, np.full(n - len(v), SI)]).astype(np.int32)
    args = [_t(c[k], dev) for k in ("src_pcd", "tgt_pcd", "rot", "trans")]
    args += [_t(pad_i(lab["src_idx"], ns), dev), _t(pad_i(lab["tgt_idx"], nt), dev), _t(lab["counts"].astype(np.int32), dev),
             _t(pad_i(am["row_arg"], ns), dev), _t(pad_i(am["col_arg"], nt), dev), _t(c["scores"], dev)]
    out = dict(labels=_f((ns + nt,), dev), sel=_f((ns + nt,), dev), pos=_i((ns + nt,), dev), dist=_f((ns + nt,), dev))
    check(lib.apr_saliency_labels(*[ptr(t) for t in args], ns, nt, float(c["radius"]), ptr(out["labels"]), ptr(out["sel"]),
                                  ptr(out["pos"]), ptr(out["dist"]), _lib.stream()))
    return _np(out)


@pytest.mark.parametrize("name", K.NAMES["saliency"])
def test_saliency_labels_driven_by_the_oracle_argmaxes(dev, name):
    """first the kernels' own arg-maxes on the oracle's lists equal the oracle's, then apr_saliency_labels on the oracle's lists
    and arg-maxes: labels on either side of matchability_radius, gathered scores and positions exact, distances bounded, the
    outputs past counts[2] untouched"""
    c, r = K.get(name), K.saliency_oracle(name)
    lab, am = r["lab"], r["am"]
    arg = _argmax_direct(dev, c["src_feats"], lab["src_idx"], lab["counts"][0], c["tgt_feats"], lab["tgt_idx"], lab["counts"][1])
    assert np.array_equal(arg["row_arg"][:am["na"]], am["row_arg"]) and np.array_equal(arg["col_arg"][:am["nb"]], am["col_arg"])
    got = _saliency_direct(dev, c, r)
    _report(name, K.judge_saliency(name, got, SF, SI))
    _same_bits(got, _saliency_direct(dev, c, r))


def _bce_direct(dev, c, n_dev, scatter):
    lib = _lib.load()
    n = c["n"]
    pred, gt = _t(c["pred"], dev), _t(c["gt"], dev)
    nd = None if n_dev is None else _t(np.array([n_dev], np.int32), dev)
    sb = int(lib.apr_weighted_bce_scratch_bytes())
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    out8 = _f((8 + PAD,), dev)
    check(lib.apr_weighted_bce_forward(ptr(pred), ptr(gt), n, ptr(nd), ptr(out8), ptr(scratch), sb, _lib.stream()))
    go = _t(np.array([c["grad_out"]], np.float32), dev)
    d = _f((n + 9 if scatter else n,), dev)
    sp = _t(c["scatter_pos"], dev) if scatter else None
    check(lib.apr_weighted_bce_backward(ptr(pred), ptr(gt), n, ptr(nd), ptr(out8), ptr(go), ptr(sp), ptr(d), _lib.stream()))
    return _np(dict(out8=out8, d=d))


@pytest.mark.parametrize("name", K.NAMES["bce"])
def test_weighted_bce_every_output_and_gradient_element(dev, name):
    """forward and backward for n_dev absent, 0, 1, n - 1, n, n + 5 and -3, the backward plain and through a scatter_pos
    permutation into a longer sentinel-filled vector: all eight outputs and every gradient element inside their bounds, NaN
    only where the oracle has it (an empty vector), every element past the count untouched"""
    c = K.get(name)
    v = {}
    for n_dev in K.bce_n_devs(c["n"]):
        for scatter in (False, True):
            got = _bce_direct(dev, c, n_dev, scatter)
            assert (got["out8"][8:] == SF).all()
            for k, x in K.judge_bce(name, n_dev, got["out8"][:8], got["d"], scatter, SF).items():
                v[f"{k}[{n_dev}]"] = max(v.get(f"{k}[{n_dev}]", 0.0), x)
            if n_dev in (None, c["n"] - 1):
                _same_bits(got, _bce_direct(dev, c, n_dev, scatter))
    _report(name, v)


def test_scatter_direct_shared_absent_and_out_of_range_rows(dev):
    """apr_circle_scatter on its own: rows under 1, 2 and 40 anchors, absent anchors (-1) and rows >= n_rows; the ordered float32
    sum is restated exactly, every other row of the sentinel-filled target is untouched"""
    lib = _lib.load()
    rng = np.random.default_rng(7)
    P, n_rows = 77, 50
    row = rng.integers(0, n_rows - 10, P)
    row[5:45], row[50:52], row[[0, 60]], row[[1, 61]] = 7, 9, -1, [n_rows, n_rows + 3]
    d = (rng.standard_normal((P, O.D)) * 10.0 ** rng.integers(-3, 4, (P, 1))).astype(np.float32)
    out, td, trow = _f((n_rows + PAD, O.D), dev), _t(d, dev), _t(row, dev, torch.int32)
    check(lib.apr_circle_scatter(ptr(td), ptr(trow), P, O.D, ptr(out), n_rows, _lib.stream()))
    torch.cuda.synchronize()
    ref = O.circle_scatter(d, row, n_rows, np.full((n_rows + PAD, O.D), SF, np.float32))
    assert np.array_equal(out.cpu().numpy(), ref)
    assert (ref[7] != SF).all() and (ref[n_rows - 1] == SF).all() and (ref[n_rows:] == SF).all()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_uncovered_shapes_and_null_arguments_are_refused_before_any_launch(dev):
    lib = _lib.load()
    D = O.D
    f, i = _f((520 * D,), dev), _i((1024,), dev)
    l64 = torch.zeros(1024, dtype=torch.int64, device=dev)
    q, st = _params(K.Q), _lib.stream()
    one = _t(np.array([1], np.int32), dev)
    bad = {
        "argmax d=16": lambda: lib.apr_gathered_argmax(ptr(f), ptr(one), ptr(one), 1, ptr(f), ptr(one), ptr(one), 1, 16, ptr(i), ptr(i), st),
        "argmax misaligned": lambda: lib.apr_gathered_argmax(C.c_void_p(f.data_ptr() + 4), ptr(one), ptr(one), 1, ptr(f), ptr(one),
                                                              ptr(one), 1, D, ptr(i), ptr(i), st),
        "argmax NULL list": lambda: lib.apr_gathered_argmax(ptr(f), None, ptr(one), 1, ptr(f), ptr(one), ptr(one), 1, D, ptr(i), ptr(i), st),
        "argmax NULL out": lambda: lib.apr_gathered_argmax(ptr(f), ptr(one), ptr(one), 1, ptr(f), ptr(one), ptr(one), 1, D, None, ptr(i), st),
        "gather d=16": lambda: lib.apr_circle_gather(ptr(l64), ptr(i), ptr(one), ptr(l64), 4, ptr(f), ptr(f), ptr(f), ptr(f), 16, ptr(f),
                                                      ptr(f), ptr(i), ptr(i), ptr(f), ptr(f), ptr(f), ptr(f), st),
        "gather P=0": lambda: lib.apr_circle_gather(ptr(l64), ptr(i), ptr(one), ptr(l64), 0, ptr(f), ptr(f), ptr(f), ptr(f), D, ptr(f),
                                                     ptr(f), ptr(i), ptr(i), ptr(f), ptr(f), ptr(f), ptr(f), st),
        "gather P=513": lambda: lib.apr_circle_gather(ptr(l64), ptr(i), ptr(one), ptr(l64), 513, ptr(f), ptr(f), ptr(f), ptr(f), D, ptr(f),
                                                       ptr(f), ptr(i), ptr(i), ptr(f), ptr(f), ptr(f), ptr(f), st),
        "forward P=0": lambda: lib.apr_circle_forward(ptr(f), ptr(f), ptr(i), 0, ptr(f), ptr(f), ptr(i), 0, None, None, q, ptr(f), ptr(f),
                                                      ptr(f), ptr(i), st),
        "forward P=513": lambda: lib.apr_circle_forward(ptr(f), ptr(f), ptr(i), 513, ptr(f), ptr(f), ptr(i), 513, None, None, q, ptr(f),
                                                        ptr(f), ptr(f), ptr(i), st),
        "forward dense 513x4": lambda: lib.apr_circle_forward(None, None, None, 513, None, None, None, 4, ptr(f), ptr(f), q, ptr(f), ptr(f),
                                                              ptr(f), ptr(i), st),
        "forward NULL params": lambda: lib.apr_circle_forward(ptr(f), ptr(f), ptr(i), 4, ptr(f), ptr(f), ptr(i), 4, None, None, None, ptr(f),
                                                              ptr(f), ptr(f), ptr(i), st),
        "forward NULL features": lambda: lib.apr_circle_forward(None, ptr(f), ptr(i), 4, ptr(f), ptr(f), ptr(i), 4, None, None, q, ptr(f),
                                                                ptr(f), ptr(f), ptr(i), st),
        "forward dense NULL feats_dist": lambda: lib.apr_circle_forward(None, None, None, 4, None, None, None, 4, ptr(f), None, q, ptr(f),
                                                                        ptr(f), ptr(f), ptr(i), st),
        "backward P=513": lambda: lib.apr_circle_backward(ptr(f), ptr(f), ptr(i), 513, ptr(f), ptr(f), ptr(i), 513, None, None, q, ptr(f),
                                                          ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), None, st),
        "backward dense 513x4": lambda: lib.apr_circle_backward(None, None, None, 513, None, None, None, 4, ptr(f), ptr(f), q, ptr(f), ptr(f),
                                                                ptr(f), ptr(f), None, None, ptr(f), st),
        "backward NULL d_a": lambda: lib.apr_circle_backward(ptr(f), ptr(f), ptr(i), 4, ptr(f), ptr(f), ptr(i), 4, None, None, q, ptr(f),
                                                             ptr(f), ptr(f), ptr(f), None, ptr(f), None, st),
        "scatter d=16": lambda: lib.apr_circle_scatter(ptr(f), ptr(i), 4, 16, ptr(f), 10, st),
        "scatter P=0": lambda: lib.apr_circle_scatter(ptr(f), ptr(i), 0, D, ptr(f), 10, st),
        "scatter P=513": lambda: lib.apr_circle_scatter(ptr(f), ptr(i), 513, D, ptr(f), 10, st),
    }
    for what, call in bad.items():
        with pytest.raises(_lib.AprHipError):
            check(call())
        torch.cuda.synchronize()
        assert bool((f == SF).all()) and bool((i == SI).all()), f"{what}: something was launched"


# ------------------------------------------------------------------------------------- the wrappers, on a subset of cases
def _metric_loss(dev):
    from apr_amd.predator.configs.models import kitti_config
    from apr_amd.predator.lib.loss import MetricLoss
    import predator_loss_oracle as T
    keys = ("pos_margin", "neg_margin", "max_points", "safe_radius", "matchability_radius", "pos_radius")
    m = MetricLoss(kitti_config(**{k: T.KITTI[k] for k in keys})).to(dev)
    m.keep_intermediates = True
    return m


@pytest.mark.parametrize("name", ["anc-p65", "anc-p129-choice", "anc-p443"])
def test_ops_wrappers_and_metric_loss_on_the_anchor_route(dev, name):
    """ops.circle_select / gather / forward / backward / scatter and MetricLoss.forward(choice=...) give what the direct calls
    gave: same judgement, and the autograd gradients of the two feature matrices inside the scattered bounds"""
    c, r = K.get(name), K.anchors_oracle(name)
    corr, src, tgt, rot, trans, sf, tf = (_t(c[k], dev) for k in ("corr", "src_pcd", "tgt_pcd", "rot", "trans", "src_feats", "tgt_feats"))
    filt, count = ops.circle_select(corr, src, tgt, rot, trans, c["thresh"])
    g = ops.circle_gather(corr, filt, count, _t(c["choice"], dev), src, tgt, sf, tf, rot, trans)
    out4, st_a, st_b, nn = ops.circle_forward(O.param_vec(c["q"]), anchors=g)
    go = _t(np.array(c["grad_out"], np.float32), dev)
    d_a, d_b = ops.circle_backward(O.param_vec(c["q"]), st_a, st_b, out4, go, anchors=g)
    d_src, d_tgt = ops.circle_scatter(d_a, g["a_row"], len(c["src_pcd"])), ops.circle_scatter(d_b, g["b_row"], len(c["tgt_pcd"]))
    got = _np(dict(g, filt=filt, count=count, st_a=st_a, st_b=st_b, out4=out4, nn=nn, d_a=d_a, d_b=d_b, d_src=d_src, d_tgt=d_tgt))
    cnt = int(got["count"][0])
    got.update(count=cnt, filt=np.concatenate([got["filt"][:cnt], np.full(PAD, SI)]))        # the wrapper's tail is its own
    _report(name + " (ops)", K.judge_anchors(name, got, SF, SI))

    m = _metric_loss(dev)
    rng = np.random.default_rng(3)
    n_src, n_tgt = len(c["src_pcd"]), len(c["tgt_pcd"])
    so, ss = (rng.uniform(0.01, 0.99, n_src + n_tgt).astype(np.float32) for _ in range(2))
    sf, tf, tso = sf.requires_grad_(True), tf.requires_grad_(True), _t(so, dev).requires_grad_(True)
    stats = m(src, tgt, sf, tf, corr, rot, trans, tso, _t(ss, dev), choice=_t(c["choice"], dev))
    (stats["circle_loss"] * c["grad_out"]).backward() if np.isfinite(r["fw"]["out4"][0]) else None
    (stats["overlap_loss"] * c["grad_out"]).backward()
    fw = r["fw"]
    lab = O.overlap_labels(c["corr"], n_src, n_tgt)
    ref8, b8 = O.weighted_bce(so, lab["gt"])
    d8, bd8 = O.weighted_bce_backward(so, lab["gt"], c["grad_out"])
    v = {"circle_loss": O.worst_ratio(np.array([float(stats["circle_loss"].detach()), float(stats["recall"])]), fw["out4"][:2], fw["out4_bound"][:2])[0],
         "overlap": O.worst_ratio(np.array([float(stats[k]) for k in ("overlap_loss", "overlap_precision", "overlap_recall")]),
                                  ref8[[0, 2, 3]], b8[[0, 2, 3]])[0],
         "d_scores": O.worst_ratio(tso.grad.cpu().numpy(), d8, bd8)[0],
         "d_src": O.worst_ratio(sf.grad.cpu().numpy(), r["d_src"][0], r["d_src"][1])[0],
         "d_tgt": O.worst_ratio(tf.grad.cpu().numpy(), r["d_tgt"][0], r["d_tgt"][1])[0],
         "gt": K._exact(m.last["gt"].cpu().numpy(), lab["gt"])}
    _report(name + " (MetricLoss)", v)


@pytest.mark.parametrize("name", K.NAMES["saliency"])
def test_metric_loss_saliency_branch_on_the_saliency_cases(dev, name):
    """MetricLoss.forward on a case whose arg-maxes and labels have margins: index lists, arg-maxes and labels as the oracle's,
    the saliency BCE (device count, gathered scores, scatter_pos backward) inside the BCE bounds"""
    c, r = K.get(name), K.saliency_oracle(name)
    lab, am, sal = r["lab"], r["am"], r["sal"]
    m = _metric_loss(dev)
    rng = np.random.default_rng(4)
    so = _t(rng.uniform(0.01, 0.99, c["n_src"] + c["n_tgt"]).astype(np.float32), dev)
    ss = _t(c["scores"], dev).requires_grad_(True)
    stats = m(*[_t(c[k], dev) for k in ("src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "corr", "rot", "trans")], so, ss,
              choice=torch.arange(512, device=dev))
    stats["saliency_loss"].backward()
    last, n = m.last, sal["n"]
    ns, nt = lab["counts"][0], lab["counts"][1]
    ref8, b8 = O.weighted_bce(sal["sel"], sal["labels"])
    d, bd = O.weighted_bce_backward(sal["sel"], sal["labels"], 1.0)
    full, fullb = np.zeros(c["n_src"] + c["n_tgt"]), np.zeros(c["n_src"] + c["n_tgt"])
    full[sal["pos"]], fullb[sal["pos"]] = d, bd
    v = {"lists": max(K._exact(last["src_idx"].cpu().numpy()[:ns], lab["src_idx"]), K._exact(last["tgt_idx"].cpu().numpy()[:nt], lab["tgt_idx"])),
         "argmax": max(K._exact(last["row_arg"].cpu().numpy()[:ns], am["row_arg"]), K._exact(last["col_arg"].cpu().numpy()[:nt], am["col_arg"])),
         "labels": K._exact(last["saliency_labels"].cpu().numpy()[:n], sal["labels"]),
         "pos": K._exact(last["saliency_pos"].cpu().numpy()[:n], sal["pos"]),
         "dist": O.worst_ratio(last["saliency_dist"].cpu().numpy()[:n], sal["dist"], sal["dist_bound"])[0],
         "saliency": O.worst_ratio(np.array([float(stats[k]) for k in ("saliency_loss", "saliency_precision", "saliency_recall")]),
                                   ref8[[0, 2, 3]], b8[[0, 2, 3]])[0],
         "d_scores": O.worst_ratio(ss.grad.cpu().numpy(), full, fullb)[0]}
    _report(name + " (MetricLoss)", v)


@pytest.mark.parametrize("name", ["dense-17x65", "dense-443x3", "dense-64x16-rows-only"])
def test_metric_loss_dense_entry_points(dev, name):
    """get_circle_loss (with autograd into feats_dist) and get_recall on the dense matrices"""
    c, r = K.get(name), K.dense_oracle(name)
    m = _metric_loss(dev)
    cd, fd = _t(c["cd"], dev), _t(c["fd"], dev).requires_grad_(True)
    loss = m.get_circle_loss(cd, fd)
    (loss * c["grad_out"]).backward()
    rec = m.get_recall(cd, fd)
    fw, bw = r["fw"], r["bw"]
    _report(name + " (MetricLoss)", {"out4": O.worst_ratio(np.array([float(loss.detach()), float(rec)]), fw["out4"][:2], fw["out4_bound"][:2])[0],
                                     "d_fd": O.worst_ratio(fd.grad.cpu().numpy(), bw["d_fd"], bw["d_fd_bound"])[0]})


@pytest.mark.parametrize("name", ["bce-n255", "bce-n65537"])
def test_metric_loss_weighted_bce_entry_point(dev, name):
    c = K.get(name)
    m = _metric_loss(dev)
    p = _t(c["pred"], dev).requires_grad_(True)
    loss, prec, rec = m.get_weighted_bce_loss(p, _t(c["gt"], dev))
    (loss * c["grad_out"]).backward()
    ref8, b8 = O.weighted_bce(c["pred"], c["gt"])
    d, bd = O.weighted_bce_backward(c["pred"], c["gt"], c["grad_out"])
    _report(name + " (MetricLoss)", {"out": O.worst_ratio(np.array([float(loss.detach()), float(prec), float(rec)]), ref8[[0, 2, 3]], b8[[0, 2, 3]])[0],
                                     "d": O.worst_ratio(p.grad.cpu().numpy(), d, bd)[0]})

"""The descriptor-loss edge suite without a GPU: the float64 oracle (tests/predator_loss_edges_oracle.py) against torch
float64 autograd of tests/predator_loss_oracle.py, the cases (tests/predator_loss_edges_cases.py) against their stated facts
and margins, a float32 host restatement in the kernels' structure (tests/predator_loss_edges_host32.py) against every bound,
and that restatement with one planted fault at a time against the named case that must reject it.

Worst |float32 host - oracle| / bound over all cases, as printed by test_host_float32_stays_inside_every_bound (records, not
thresholds): see the table in DESIGN.md, section 39.
"""
import numpy as np
import pytest
import torch

import predator_loss_edges_cases as K
import predator_loss_edges_host32 as H
import predator_loss_edges_oracle as O
import predator_loss_oracle as T

F64 = torch.float64
E20 = float(np.exp(-20.0))


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=F64, requires_grad=grad)


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert (np.isnan(a) == np.isnan(b)).all(), "NaN in different places"
    m = ~np.isnan(a)
    assert (np.abs(a[m] - b[m]) <= tol * np.maximum(1.0, np.abs(b[m]))).all(), float(np.abs(a[m] - b[m]).max())


# ------------------------------------------------------------------------------------------- oracle against autograd
def _torch_circle(q, cd, fd, grad_out, nn=None):
    p = dict(T.KITTI, **q)
    loss = T.circle_loss(cd, fd, p)
    rec = T.recall(cd, fd, p, None if nn is None else torch.as_tensor(nn))
    loss.backward(torch.tensor(grad_out, dtype=F64))
    return float(loss.detach()), float(rec)


@pytest.mark.parametrize("name", K.NAMES["anchors"])
def test_anchor_oracle_equals_autograd_on_the_present_anchors(name):
    """circle_loss and recall of the reference restatement on the present anchors, feats_dist built by square_distance from
    leaf feature tensors: values and both feature gradients to 1e-12 with torch's softplus backward, and the kernel's
    convention (sigmoid on both sides of the threshold) within e^-20 of it entry by entry."""
    c, r = K.get(name), K.anchors_oracle(name)
    g, fw = r["g"], r["fw"]
    pres = g["present"]
    if not pres.any():
        assert np.isnan(fw["out4"][0]) and fw["out4"][1] == 0 and not fw["A"]["st"].any() and not r["bw"]["d_a"].any()
        return
    a, b = _t(g["a_feats"][pres], True), _t(g["b_feats"][pres], True)
    cd = _t(fw["cd"][pres][:, pres])
    fd = torch.sqrt(T.square_distance(a[None], b[None], normalised=True)).squeeze(0)
    remap = np.cumsum(pres) - 1
    loss, rec = _torch_circle(c["q"], cd, fd, c["grad_out"], remap[fw["A"]["nn"][pres]] if fw["A"]["nn_tied"].any() else None)
    _close(fw["out4"][0], loss)
    _close(fw["out4"][1], rec)
    if not fw["A"]["nn_tied"].any():
        assert np.array_equal(remap[fw["A"]["nn"][pres]], fd.detach().numpy().argmin(1))
    bt = O.circle_backward(c["q"], fw, c["grad_out"], g["a_feats"], g["b_feats"], softplus_grad="torch")
    _close(bt["d_a"][pres], a.grad.numpy())
    _close(bt["d_b"][pres], b.grad.numpy())
    assert not bt["d_a"][~pres].any() and not bt["d_b"][~pres].any() and not fw["A"]["st"][~pres].any()
    bk, Gs = r["bw"], np.abs(bt["Gs"])
    assert (np.abs(bk["d_a"] - bt["d_a"]) <= E20 * (Gs @ np.abs(g["b_feats"])) + 1e-300).all()
    assert (np.abs(bk["d_b"] - bt["d_b"]) <= E20 * (Gs.T @ np.abs(g["a_feats"])) + 1e-300).all()
    if ((fw["A"]["z"] > 20) & (fw["A"]["z"] < 30) & fw["A"]["sel"]).any():      # 1 - sigmoid(z) is a float64 zero from z ~ 37
        assert (bk["d_a"] != bt["d_a"]).any(), "a row just above the softplus threshold has to see the two conventions differ"


@pytest.mark.parametrize("name", K.NAMES["dense"])
def test_dense_oracle_equals_autograd(name):
    c, r = K.get(name), K.dense_oracle(name)
    fw = r["fw"]
    cd, fd = _t(c["cd"]), _t(c["fd"], True)
    loss, rec = _torch_circle(c["q"], cd, fd, c["grad_out"], fw["A"]["nn"])
    _close(fw["out4"][0], loss)
    _close(fw["out4"][1], rec)
    bt = O.circle_backward(c["q"], fw, c["grad_out"], softplus_grad="torch")
    _close(bt["d_fd"], fd.grad.numpy())
    assert (np.abs(r["bw"]["d_fd"] - bt["d_fd"]) <= E20 * np.abs(bt["d_fd"]) * 2 + 1e-300).all()


@pytest.mark.parametrize("name", K.NAMES["bce"])
def test_bce_oracle_equals_autograd(name):
    c = K.get(name)
    for n_dev in K.bce_n_devs(c["n"]):
        n = O.bce_n(c["n"], n_dev)
        out, _ = O.weighted_bce(c["pred"], c["gt"], n_dev)
        d, _ = O.weighted_bce_backward(c["pred"], c["gt"], c["grad_out"], n_dev)
        if n == 0:
            assert np.isnan(out[0]) and not out[2:].any() and len(d) == 0
            continue
        p, g = _t(c["pred"][:n], True), _t(c["gt"][:n])
        loss, prec, rec = T.weighted_bce(p, g)
        loss.backward(torch.tensor(c["grad_out"], dtype=F64))
        _close(out[0], float(loss.detach()))
        _close(out[2:4], [float(prec), float(rec)])
        _close(d, p.grad.numpy())
        assert out[7] == n and out[4] + out[6] == g.sum()


FINITE = [n for n in K.NAMES["anchors"] if "loss_nan" not in K._ANCHORS[n][1].get("expect", {})]


@pytest.mark.parametrize("name", FINITE)
def test_oracle_chain_equals_the_reference_forward(name):
    """the whole restated forward (labels, both BCEs, arg-maxes, saliency labels, select, choice, circle loss, recall) on every
    anchor case with a finite loss, to 1e-12: the case's in-range correspondences (the reference indexes with every row),
    the entries of `choice` inside the filtered list (the reference indexes with every entry; an absent anchor drops its row
    and column, so the present anchors in their order give the same loss), float32-rounded parameters"""
    c, r = K.get(name), K.anchors_oracle(name)
    assert np.isfinite(r["fw"]["out4"][0])
    corr = c["corr"][r["sel"]["in_range"]]
    pres = r["g"]["present"]
    remap = np.cumsum(pres) - 1
    n_src, n_tgt = len(c["src_pcd"]), len(c["tgt_pcd"])
    rng = np.random.default_rng(5)
    so, ss = (rng.uniform(0.01, 0.99, n_src + n_tgt).astype(np.float32) for _ in range(2))
    p = dict(T.KITTI, **c["q"])
    p.update(max_points=0, matchability_radius=O.f32r(T.KITTI["matchability_radius"]))
    keep = {}
    stats = T.forward(_t(c["src_pcd"]), _t(c["tgt_pcd"]), _t(c["src_feats"]), _t(c["tgt_feats"]), torch.as_tensor(corr), _t(c["rot"]),
                      _t(c["trans"]).reshape(3, 1), _t(so), _t(ss), p, choice=c["choice"][pres],
                      pins={"nn": torch.as_tensor(remap[r["fw"]["A"]["nn"][pres]])}, keep=keep)
    lab = O.overlap_labels(corr, n_src, n_tgt)
    assert np.array_equal(lab["src_idx"], keep["src_idx"].numpy()) and np.array_equal(lab["tgt_idx"], keep["tgt_idx"].numpy())
    assert np.array_equal(lab["gt"], keep["overlap_gt"].numpy())
    _close(O.weighted_bce(so, lab["gt"])[0][[0, 2, 3]], [float(stats[k]) for k in ("overlap_loss", "overlap_precision", "overlap_recall")])
    am = O.gathered_argmax(c["src_feats"], lab["src_idx"], lab["counts"][0], c["tgt_feats"], lab["tgt_idx"], lab["counts"][1])
    assert np.array_equal(am["row_arg"][~am["row_tied"]], keep["row_arg"].numpy()[~am["row_tied"]])
    assert np.array_equal(am["col_arg"][~am["col_tied"]], keep["col_arg"].numpy()[~am["col_tied"]])
    sal = O.saliency_labels(c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], lab["src_idx"], lab["tgt_idx"], lab["counts"],
                            keep["row_arg"].numpy(), keep["col_arg"].numpy(), ss, T.KITTI["matchability_radius"])
    _close(sal["dist"], keep["saliency_dist"].numpy())
    assert np.array_equal(sal["labels"], keep["saliency_labels"].numpy())
    _close(O.weighted_bce(sal["sel"], sal["labels"])[0][[0, 2, 3]], [float(stats[k]) for k in ("saliency_loss", "saliency_precision", "saliency_recall")])
    assert keep["n_filtered"] == r["sel"]["count"]
    _close(r["fw"]["out4"][:2], [float(stats["circle_loss"]), float(stats["recall"])])


# --------------------------------------------------------------------------------------------------- facts and margins
@pytest.mark.parametrize("name", K.NAMES["anchors"])
def test_anchor_case_meets_its_fact_and_margins(name):
    c, r = K.get(name), K.anchors_oracle(name)
    sel, g, fw, bw, e = r["sel"], r["g"], r["fw"], r["bw"], c["expect"]
    A = fw["A"]
    assert sel["count"] == c["nfilt"] and (sel["slack"] > 0).all() and (~sel["in_range"]).sum() == 5
    assert 0 < sel["count"] < sel["in_range"].sum() or c["nfilt"] == 0, "the select has to reject something"
    assert (fw["mask_slack"] > 0).all() and (A["nn_slack"] > 0).all()
    assert not bw["clamp_unsure"].any()
    assert bool(A["nn_tied"].any()) == bool(e.get("nn_tie", False)), "exact fd ties only where the case names them"
    if e.get("nn_tie"):                      # a tie is between bitwise identical rows, so the kernel sees equal numbers too
        for i in np.nonzero(A["nn_tied"])[0]:
            cols = np.nonzero((fw["fd"][i] == fw["fd"][i].min()) & fw["pb"])[0]
            assert A["nn"][i] == cols[0] and len(cols) > 1 and (g["b_feats"][cols] == g["b_feats"][cols[0]]).all()
    assert np.isnan(fw["out4"][0]) == bool(e.get("loss_nan", False))
    assert (~g["present"]).sum() == e.get("absent", 0)
    if e.get("zero_grad"):
        assert not bw["d_a"].any() and not bw["d_b"].any()
    elif "loss_nan" not in e:
        assert np.abs(bw["d_a"]).max() > 1e-4 and np.abs(bw["d_b"]).max() > 1e-4
    if e.get("pos_no_neg"):
        assert ((A["st"][:, 4] == 1) & (A["st"][:, 3] == 0)).any()
    if e.get("some_sel"):
        assert 0 < fw["out4"][2] < c["P"]
    assert int(bw["clamped"].sum()) == e.get("clamped", 0)
    if e.get("clamped"):                     # the clamped pair is a negative with weight, so a kept gradient would be huge
        i, j = np.argwhere(bw["clamped"])[0]
        assert fw["E"]["neg"][i, j] and fw["E"]["nw"][i, j] > 1.0 and fw["fd"][i, j] == 1e-6 and fw["bfd"][i, j] < 1e-12
    if e.get("near"):
        assert ((np.abs(fw["fd"] - 2.0 ** -10) < 1e-12) & (fw["bfd"] < 1e-9) & fw["E"]["neg"]).any()
    if e.get("zgt20"):
        assert (A["z"] > 20).any()
    if "lds_over" in e:
        assert (148 * c["P"] > 65536) == e["lds_over"]
    if e.get("shared"):
        cnt = np.bincount(g["a_row"][g["present"]])
        assert {1, 2, 40} <= set(cnt[cnt > 0]) and np.bincount(g["b_row"]).max() == 3
        for k in np.nonzero(cnt > 1)[0]:
            assert len(set(g["b_row"][g["a_row"] == k])) == cnt[k], "shared a_row, distinct b_row"
    if name == "anc-p129-choice":
        ch = c["choice"]
        assert (ch >= sel["count"]).sum() == 3 and (ch < 0).sum() == 2 and len(set(ch)) < len(ch)
    assert 0 < A["st"][:, 5].sum() < A["st"][:, 4].sum() or c["P"] < 16, "recall neither 0 nor 1"


@pytest.mark.parametrize("name", K.NAMES["dense"])
def test_dense_case_meets_its_fact(name):
    c, fw, bw = K.get(name), K.dense_oracle(name)["fw"], K.dense_oracle(name)["bw"]
    e, q = c["expect"], c["q"]
    assert np.isnan(fw["out4"][0]) == (fw["out4"][2] == 0 or fw["out4"][3] == 0)
    if "loss_nan" in e:
        assert np.isnan(fw["out4"][0])
    if "cd" in c["planted"]:
        v = c["cd"].reshape(-1)[c["planted"]["cd"]].astype(np.float64)
        pr, sr = q["pos_radius"], q["safe_radius"]
        assert v[0] == pr and v[1] < pr < v[2] and v[3] == sr and v[4] < sr < v[5]
        assert pr < T.KITTI["pos_radius"], "float32(0.21) is below the Python double: a double threshold would call v[0] positive"
        E = fw["E"]
        at = c["planted"]["cd"]
        assert list(E["pos"].reshape(-1)[at]) == [False, True, False, False, False, False]
        assert list(E["neg"].reshape(-1)[at]) == [False, False, False, False, False, True]
    if "fd" in c["planted"]:
        assert list(c["fd"].reshape(-1)[c["planted"]["fd"]]) == [0.0, np.float32(1e-6), 2.0]
    if e.get("zero_grad"):
        assert not bw["d_fd"].any()
    if e.get("rows_only"):
        assert fw["out4"][2] == 1 and fw["out4"][3] == 0 and np.abs(bw["d_fd"][0]).max() > 1e-3 and not bw["d_fd"][1:].any()
    if e.get("neg_no_pos"):
        assert ((fw["A"]["st"][:, 4] == 0) & fw["E"]["neg"].any(1)).any()
    if "zlt" in e:
        assert fw["A"]["z"][0] < e["zlt"] and fw["A"]["st"][0, 2] > 0 and fw["A"]["st"][0, 6] > 0
    if c["na"] * c["nb"] > 64 and "loss_nan" not in e:
        assert (fw["A"]["z"] > 20).any()


@pytest.mark.parametrize("name", K.NAMES["select"])
def test_select_case_meets_its_margins(name):
    c, r = K.get(name), K.select_oracle(name)
    lab, sel = r["lab"], r["sel"]
    assert (sel["slack"] > 0).all()
    assert (lab["counts"][0] == 0) == (lab["counts"][1] == 0), "one empty list next to a filled one is a precondition, not a case"
    if len(sel["slack"]) > 100:
        d = sel["dist"][sel["in_range"]]
        assert ((d < sel["thr"]) & (d > sel["thr"] - 5e-4)).any() and ((d > sel["thr"]) & (d < sel["thr"] + 8e-4)).any()
        assert len(np.unique(c["corr"], axis=0)) < len(c["corr"]) and (name == "sel-all" or not sel["in_range"].all())
    if name == "sel-all":
        assert lab["counts"][0] == c["n_src"] and lab["counts"][1] == c["n_tgt"]


@pytest.mark.parametrize("name", K.NAMES["argmax"])
def test_argmax_case_meets_its_fact_and_margins(name):
    c, r = K.get(name), K.argmax_oracle(name)
    assert (r["row_slack"] > 0).all() and (r["col_slack"] > 0).all()
    sc = r["scores"]
    for i in c["neg_rows"]:
        assert sc[i].max() < 0
    if c["neg_rows"]:
        assert r["nb"] % 64 != 0
    for i, c1, c2 in c["row_ties"]:
        assert r["row_tied"][i] and r["row_arg"][i] == min(c1, c2) and sc[i, c1] == sc[i, c2] == sc[i].max()
    for j, r1, r2 in c["col_ties"]:
        assert r["col_tied"][j] and r["col_arg"][j] == min(r1, r2) and sc[r1, j] == sc[r2, j] == sc[:, j].max()
    planted = {t[0] for t in c["row_ties"]}
    for i in np.nonzero(r["row_tied"])[0]:                  # any other tie is between the same identical rows
        cols = np.nonzero(sc[i] == sc[i].max())[0]
        assert (c["b"][c["b_idx"][cols]] == c["b"][c["b_idx"][cols[0]]]).all(), (i, planted)
    if c["last_col_row"] is not None:
        assert r["row_arg"][c["last_col_row"]] == r["nb"] - 1
    # which rule settles a tie: keys on one lane of the 16-lane group (equal index & 15) meet in the running strict >, in
    # two tiles of a 64-block or in two blocks; keys on two lanes meet in the closing shuffle
    ties = [(c1, c2) for _, c1, c2 in c["row_ties"]] + [(r1, r2) for _, r1, r2 in c["col_ties"]]
    one_lane = [(x, y) for x, y in ties if x % 16 == y % 16]
    if name == "am-65x129":
        assert any(x // 64 == y // 64 for x, y in one_lane) and any(x // 64 != y // 64 for x, y in one_lane)
        assert any(x % 16 != y % 16 and x // 16 == y // 16 for x, y in ties) and any(x % 16 != y % 16 and x // 64 != y // 64 for x, y in ties)
    if name == "am-130x17-neg":
        assert one_lane and all(x // 64 != y // 64 for x, y in one_lane) and (c["b"][c["b_idx"]] > 0).all()


@pytest.mark.parametrize("name", K.NAMES["saliency"])
def test_saliency_case_meets_its_margins(name):
    r = K.saliency_oracle(name)
    assert (r["am"]["row_slack"] > 0).all() and (r["am"]["col_slack"] > 0).all() and (r["sal"]["slack"] > 0).all()
    d, rad = r["sal"]["dist"], O.f32r(T.KITTI["matchability_radius"])
    assert ((d < rad) & (d > rad - 3e-4)).any() and ((d > rad) & (d < rad + 3e-4)).any()
    assert r["lab"]["counts"][0] < len(K.get(name)["src_pcd"])


def test_every_case_has_a_fact():
    assert all(len(K.FACTS[n]) > 20 for n in K.ALL) and len(set(K.ALL)) == len(K.ALL)
    assert sorted(K.get(n)["P"] for n in K.NAMES["anchors"] if n.startswith("anc-p") and "-" not in n[5:]) == \
        [1, 16, 63, 64, 65, 442, 443, 512]


# ------------------------------------------------------------------------------ the float32 host run and planted faults
def host_anchors(name, fault=None):
    c = K.get(name)
    filt, cnt = H.circle_select(c["corr"], c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], c["thresh"], fault)
    g = H.circle_gather(c["corr"], filt, cnt, c["choice"], c["src_pcd"], c["tgt_pcd"], c["src_feats"], c["tgt_feats"], c["rot"], c["trans"])
    st_a, st_b, out4, nn = H.circle_forward(c["q"], g=g, fault=fault)
    P = c["P"]
    d_a, d_b = H.circle_backward(c["q"], st_a[:P], st_b[:P], out4, c["grad_out"], g=g, fault=fault)
    zs, zt = np.zeros((len(c["src_pcd"]), O.D), np.float32), np.zeros((len(c["tgt_pcd"]), O.D), np.float32)
    got = dict(g, filt=filt, count=cnt, st_a=st_a, st_b=st_b, out4=out4, nn=nn, d_a=d_a, d_b=d_b,
               d_src=H.circle_scatter(d_a, g["a_row"], len(zs), zs, fault), d_tgt=H.circle_scatter(d_b, g["b_row"], len(zt), zt, fault))
    return K.judge_anchors(name, got, H.SENT_F, H.SENT_I)


def host_dense(name, fault=None):
    c = K.get(name)
    st_a, st_b, out4, nn = H.circle_forward(c["q"], cd=c["cd"], fd=c["fd"], fault=fault)
    d_fd = H.circle_backward(c["q"], st_a[:c["na"]], st_b[:c["nb"]], out4, c["grad_out"], cd=c["cd"], fd=c["fd"], fault=fault)
    return K.judge_dense(name, dict(st_a=st_a, st_b=st_b, out4=out4, nn=nn, d_fd=d_fd), H.SENT_F, H.SENT_I)


def host_select(name, fault=None):
    c = K.get(name)
    got = H.overlap_labels(c["corr"], c["n_src"], c["n_tgt"], fault)
    got["filt"], got["count"] = H.circle_select(c["corr"], c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], c["thresh"], fault)
    return K.judge_select(name, got, H.SENT_I)


def host_argmax(name, fault=None):
    c = K.get(name)
    row, col = H.gathered_argmax(c["a"], c["a_idx"], c["na_dev"], c["b"], c["b_idx"], c["nb_dev"], fault)
    return K.judge_argmax(name, dict(row_arg=row, col_arg=col), H.SENT_I)


def host_saliency(name, fault=None):
    c, r = K.get(name), K.saliency_oracle(name)
    lab, am = r["lab"], r["am"]
    row, col = H.gathered_argmax(c["src_feats"], lab["src_idx"], lab["counts"][0], c["tgt_feats"], lab["tgt_idx"], lab["counts"][1], fault)
    assert np.array_equal(row, am["row_arg"]) and np.array_equal(col, am["col_arg"])
    s = H.saliency_labels(c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], lab["src_idx"], lab["tgt_idx"], lab["counts"], row, col,
                          c["scores"], c["radius"])
    n, tot = r["sal"]["n"], c["n_src"] + c["n_tgt"]
    got = {k: np.concatenate([s[k], np.full(tot - n, H.SENT_I if k == "pos" else H.SENT_F)]) for k in ("labels", "sel", "pos", "dist")}
    return K.judge_saliency(name, got, H.SENT_F, H.SENT_I)


def host_bce(name, fault=None):
    c = K.get(name)
    n, v = c["n"], {}
    pad_p, pad_g = np.concatenate([c["pred"], np.full(16, 0.25, np.float32)]), np.concatenate([c["gt"], np.ones(16, np.float32)])
    for n_dev in K.bce_n_devs(n):
        out8 = H.weighted_bce(pad_p, pad_g, n, n_dev, fault)
        for scatter in (False, True):
            d = np.full(n + 9 if scatter else n, H.SENT_F, np.float32)
            if n:
                H.weighted_bce_backward(c["pred"], c["gt"], n, out8, c["grad_out"], n_dev, c["scatter_pos"] if scatter else None, d)
            for k, x in K.judge_bce(name, n_dev, out8, d, scatter, H.SENT_F).items():
                v[f"{k}[{n_dev}]"] = max(v.get(f"{k}[{n_dev}]", 0.0), x)
    return v


HOST = {"anchors": host_anchors, "dense": host_dense, "select": host_select, "argmax": host_argmax, "saliency": host_saliency,
        "bce": host_bce}
KIND = {n: kind for kind in K.NAMES for n in K.NAMES[kind]}


def test_host_float32_stays_inside_every_bound():
    worst = {}
    for name in K.ALL:
        v = HOST[KIND[name]](name)
        k, x = K.worst(v)
        assert x <= 1.0, (name, k, x)
        for k, x in v.items():
            key = KIND[name] + "/" + k.split("[")[0]
            if x > worst.get(key, (0.0, ""))[0]:
                worst[key] = (x, name)
    for key in sorted(worst):
        print(f"host float32 worst ratio {key:28s} {worst[key][0]:.4f}  ({worst[key][1]})")


# fault -> the named cases that must reject it
KILLERS = {
    "pad_wins": ["am-1x65-neg", "am-130x17-neg"],
    "argmax_tie_high_lane": ["am-65x129", "am-130x17-neg"],
    "argmax_tie_high_shuffle": ["am-65x129"],
    "argmin_tie_high": ["anc-p64", "anc-p65", "anc-p129-choice"],
    "pos_le": ["dense-17x65", "dense-64x16"],
    "neg_ge": ["dense-17x65", "dense-443x3"],
    "absent_col_kept": ["anc-p129-choice"],
    "dense_col_rowstrides": ["dense-17x65", "dense-1x512", "dense-443x3"],
    "clt_short": ["anc-p512", "dense-1x512"],
    "last_block_skipped": ["anc-p17-mixed", "anc-p1", "dense-17x65", "anc-p443"],
    "scatter_first_only": ["anc-p64-shared"],
    "clamp_grad_kept": ["anc-p16", "anc-p65"],
    "bce_one_trip": ["bce-n65537", "bce-n70001"],
    "ndev_unclamped": ["bce-n255", "bce-n1"],
    "half_is_one": ["bce-n255", "bce-n70001"],
    "compact_order": ["sel-n1025", "sel-n5000", "sel-all"],
}


@pytest.mark.parametrize("fault", H.FAULTS)
def test_planted_fault_is_rejected_by_its_named_cases(fault):
    """the float32 restatement with one fault leaves at least one bound (or one exact output) on every case named for it"""
    assert set(KILLERS) == set(H.FAULTS)
    for name in KILLERS[fault]:
        assert K.worst(HOST[KIND[name]](name))[1] <= 1.0, "the unfaulted run has to pass"
        k, x = K.worst(HOST[KIND[name]](name, fault))
        print(f"fault {fault:22s} rejected by {name:18s} through {k} (ratio {x:.3g})")
        assert x > 1.0, (fault, name, "not rejected")

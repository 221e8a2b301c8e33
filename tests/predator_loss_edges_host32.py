"""A float32 NumPy restatement of apr_amd/csrc/metric_loss.hip in the kernels' own structure, for the CPU test of the
oracle's bounds and cases (tests/test_predator_loss_edges_oracle_cpu.py): lane-strided columns (j = lane + 64 t) and the
xor-butterfly order for the circle rows, 64-column blocks of four 16-column tiles with a running strict > for the arg-max,
per-thread chunks and an exclusive scan for the two compactions, a grid-stride loop over at most 256 blocks of 256 for the
BCE.  Products and sums are rounded separately where the kernels fuse them (inside every bound either way).

Borrowed, not restated: outputs that are pure copying or indexing are taken from the oracle itself (the gt vector of
overlap_labels, circle_gather's rows, tgt points and features, the `pos` and `sel` of saliency_labels, and the unfaulted
circle_scatter, which the oracle restates exactly).  Their host ratios are 0 by construction and are no independent evidence;
the GPU test is the check of those outputs.  What is restated here is everything with arithmetic or ordering in it: the two
compactions, the float32 distances, the circle rows and their backward, the closing block, the BCE sums and the arg-max.

`fault` switches on one planted fault (FAULTS); the CPU test shows that each is rejected by a named case.
"""
import numpy as np

import predator_loss_edges_oracle as O

F32 = np.float32
SENT_I = -77
SENT_F = F32(-7.5)
FAULTS = ("pad_wins", "argmax_tie_high_lane", "argmax_tie_high_shuffle", "argmin_tie_high", "pos_le", "neg_ge", "absent_col_kept", "dense_col_rowstrides",
          "clt_short", "last_block_skipped", "scatter_first_only", "clamp_grad_kept", "bce_one_trip", "ndev_unclamped",
          "half_is_one", "compact_order")
XOR = {d: np.arange(64) ^ d for d in (32, 16, 8, 4, 2, 1)}


def _q32(q):
    return {k: F32(v) for k, v in q.items()}


# --------------------------------------------------------------------------------------------------------- compactions
def compact(flags, fault=None, threads=1024):
    """k_labels_compact / k_circle_select: thread t owns [t per, (t + 1) per), counts, scans, writes from its offset"""
    n = len(flags)
    per = (n + threads - 1) // threads if n else 0
    idx = np.nonzero(flags)[0]
    if not len(idx):
        return idx.astype(np.int64), 0
    th = idx // per
    cnt = np.bincount(th, minlength=threads)
    off = np.cumsum(cnt) - cnt
    rank = np.arange(len(idx)) - off[th]
    use = off.copy()
    if fault == "compact_order":                      # a thread pair's offsets the wrong way round
        use[0::2], use[1::2] = off[0::2] + cnt[1::2], off[0::2]
    out = np.full(len(idx), SENT_I, np.int64)
    out[use[th] + rank] = idx
    return out, len(idx)


def overlap_labels(corr, n_src, n_tgt, fault=None):
    ref = O.overlap_labels(corr, n_src, n_tgt)
    gt = ref["gt"].astype(F32)
    src, tgt = np.full(n_src, SENT_I, np.int64), np.full(n_tgt, SENT_I, np.int64)
    s, ns = compact(gt[:n_src] != 0, fault)
    t, nt = compact(gt[n_src:] != 0, fault)
    src[:ns], tgt[:nt] = s, t
    return dict(gt=gt, src_idx=src, tgt_idx=tgt, counts=np.array([ns, nt, ns + nt]))


def rigid32(rot, trans, p):
    R, t, p = np.asarray(rot, F32).reshape(3, 3), np.asarray(trans, F32).reshape(3), np.asarray(p, F32).reshape(-1, 3)
    return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)


def dist32(q, b):
    e = q - np.asarray(b, F32)
    return np.sqrt(e[:, 2] * e[:, 2] + (e[:, 1] * e[:, 1] + e[:, 0] * e[:, 0]))


def circle_select(corr, src_pcd, tgt_pcd, rot, trans, thresh, fault=None):
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    s, t = corr[:, 0], corr[:, 1]
    ok = (s >= 0) & (s < len(src_pcd)) & (t >= 0) & (t < len(tgt_pcd))
    keep = np.zeros(len(corr), bool)
    if ok.any():
        keep[ok] = dist32(rigid32(rot, trans, src_pcd[s[ok]]), tgt_pcd[t[ok]]) < F32(thresh)
    filt = np.full(max(len(corr), 1), SENT_I, np.int64)
    f, n = compact(keep, fault)
    filt[:n] = f
    return filt, n


def circle_gather(corr, filt, count, choice, src_pcd, tgt_pcd, src_feats, tgt_feats, rot, trans):
    g = O.circle_gather(corr, filt, count, choice, src_pcd, tgt_pcd, src_feats, tgt_feats, rot, trans)
    ok = g["present"]
    a_pts = np.zeros((len(ok), 3), F32)
    if ok.any():
        a_pts[ok] = rigid32(rot, trans, np.asarray(src_pcd, F32)[g["a_row"][ok]])
    return dict(a_row=g["a_row"], b_row=g["b_row"], a_pts=a_pts, b_pts=g["b_pts"].astype(F32), a_feats=g["a_feats"].astype(F32),
                b_feats=g["b_feats"].astype(F32))


# -------------------------------------------------------------------------------------------------------------- circle
def _entries(q, side, fault):
    """every (i, j) of one direction in float32 -> dict of [na, nb] arrays; side: dict(na, nb, and dense cd / fd / si / sj, or
    aF / aP / bF / bP)"""
    na, nb = side["na"], side["nb"]
    if "cd" in side:
        i, j = np.arange(na)[:, None], np.arange(nb)[None, :]
        at = (i * side["si"] + j * side["sj"]) % side["cd"].size        # a wrong stride wraps here, it faults on the device
        cd, fd, s = side["cd"].reshape(-1)[at], side["fd"].reshape(-1)[at], np.zeros((na, nb), F32)
    else:
        aP, bP, aF, bF = side["aP"], side["bP"], side["aF"], side["bF"]
        dx, dy, dz = (aP[:, None, k] - bP[None, :, k] for k in range(3))
        cd = np.sqrt(np.maximum(dz * dz + (dy * dy + dx * dx), F32(1e-12)))
        s = np.zeros((na, nb), F32)
        for k in range(O.D):
            s = aF[:, k:k + 1] * bF[None, :, k] + s
        fd = np.sqrt(np.maximum(F32(2) - F32(2) * s, F32(1e-12)))
        at = None
    pos = cd <= q["pos_radius"] if fault == "pos_le" else cd < q["pos_radius"]
    neg = cd >= q["safe_radius"] if fault == "neg_ge" else cd > q["safe_radius"]
    pw = np.maximum(F32(0), (fd - np.where(pos, F32(0), F32(1e5))) - q["pos_optimal"])
    nw = np.maximum(F32(0), q["neg_optimal"] - (fd + np.where(neg, F32(0), F32(1e5))))
    ap = q["log_scale"] * (fd - q["pos_margin"]) * pw
    an = q["log_scale"] * (q["neg_margin"] - fd) * nw
    return dict(cd=cd, fd=fd, s=s, pos=pos, neg=neg, pw=pw, nw=nw, ap=ap, an=an, at=at)


def _lanes(x, fill):
    """[na, nb] -> [na, 8, 64]: column j = lane + 64 t at [t, lane]"""
    na, nb = x.shape
    out = np.full((na, 512), fill, x.dtype)
    out[:, :nb] = x
    return out.reshape(na, 8, 64)


def _bfly_sum(v):
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., XOR[d]]
    return v[..., 0]


def _valid(side, fault):
    v = np.ones(side["nb"], bool)
    if side.get("b_row") is not None and fault != "absent_col_kept":
        v = side["b_row"] >= 0
    if fault == "clt_short":
        v = v & (np.arange(side["nb"]) < 448)
    return v


def circle_rows(q, side, st, nn, fault=None):
    """k_circle_rows: writes the records of rows < na into st (and nn)"""
    na = side["na"]
    E = _entries(q, side, fault)
    valid = _lanes(np.broadcast_to(_valid(side, fault), E["cd"].shape), False)
    ninf = F32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ap, an = np.where(valid, _lanes(E["ap"], 0), ninf), np.where(valid, _lanes(E["an"], 0), ninf)
        mp, mn = ap.max((1, 2)), an.max((1, 2))
        sp, sn = np.zeros((na, 64), F32), np.zeros((na, 64), F32)
        for t in range(8):
            sp = sp + np.where(valid[:, t], np.exp(ap[:, t] - mp[:, None]), F32(0))
            sn = sn + np.where(valid[:, t], np.exp(an[:, t] - mn[:, None]), F32(0))
        sp, sn = _bfly_sum(sp), _bfly_sum(sn)
        anyp = (valid & _lanes(E["pos"], False)).any((1, 2))
        anyn = (valid & _lanes(E["neg"], False)).any((1, 2))
        fd, cd = _lanes(E["fd"], 0), _lanes(E["cd"], 0)
        bd, bj, bc = np.full((na, 64), np.inf, F32), np.full((na, 64), 0x7fffffff, np.int64), np.zeros((na, 64), F32)
        high = fault == "argmin_tie_high"
        for t in range(8):
            better = valid[:, t] & ((fd[:, t] <= bd) if high else (fd[:, t] < bd))
            bd, bc = np.where(better, fd[:, t], bd), np.where(better, cd[:, t], bc)
            bj = np.where(better, np.arange(64)[None, :] + 64 * t, bj)
        for d in (32, 16, 8, 4, 2, 1):
            od, oj, oc = bd[:, XOR[d]], bj[:, XOR[d]], bc[:, XOR[d]]
            better = (od < bd) | ((od == bd) & ((oj > bj) if high else (oj < bj)))
            bd, bj, bc = np.where(better, od, bd), np.where(better, oj, bj), np.where(better, oc, bc)
        bj, bc = bj[:, 0], bc[:, 0]
        lp, ln = mp + np.log(sp), mn + np.log(sn)
        z = lp + ln
        loss = np.where(z > F32(20), z, np.log1p(np.exp(z))) / q["log_scale"]
        sig = F32(1) / (F32(1) + np.exp(-z))
    rec = np.stack([lp, ln, loss, (anyp & anyn).astype(F32), anyp.astype(F32), (anyp & (bc < q["pos_radius"])).astype(F32), sig,
                    np.zeros(na, F32)], 1).astype(F32)
    arg = np.where(bj == 0x7fffffff, 0, bj)
    if side.get("a_row") is not None:
        rec[side["a_row"] < 0], arg[side["a_row"] < 0] = 0, 0
    rows = np.arange(na) < (16 * (na // 16) if fault == "last_block_skipped" else na)
    st[:na][rows] = rec[rows]
    if nn is not None:
        nn[:na][rows] = arg[rows]


def circle_final(st_a, na, st_b, nb):
    a, b = st_a[:na].astype(np.float64), st_b[:nb].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ra, rb = a[:, 3] != 0, b[:, 3] != 0
        out = [(a[ra, 2].sum() / ra.sum() + b[rb, 2].sum() / rb.sum()) / 2.0, a[:, 5].sum() / (a[:, 4].sum() + 1e-12), ra.sum(), rb.sum()]
    return np.array(out).astype(F32)


def _sides(q, g=None, cd=None, fd=None, fault=None):
    if g is not None:
        A = dict(na=len(g["a_row"]), nb=len(g["b_row"]), aF=g["a_feats"], aP=g["a_pts"], bF=g["b_feats"], bP=g["b_pts"],
                 a_row=g["a_row"], b_row=g["b_row"])
        B = dict(na=A["nb"], nb=A["na"], aF=g["b_feats"], aP=g["b_pts"], bF=g["a_feats"], bP=g["a_pts"], a_row=g["b_row"],
                 b_row=g["a_row"])
    else:
        na, nb = cd.shape
        A = dict(na=na, nb=nb, cd=cd, fd=fd, si=nb, sj=1)
        B = dict(na=nb, nb=na, cd=cd, fd=fd, si=1, sj=nb)
        if fault == "dense_col_rowstrides":
            B.update(si=nb, sj=1)
    return A, B


def circle_forward(q, g=None, cd=None, fd=None, fault=None, pad=3):
    """apr_circle_forward -> (st_a, st_b, out4, nn): records have `pad` sentinel rows behind them"""
    q = _q32(q)
    A, B = _sides(q, g, cd, fd, fault)
    st_a, st_b = np.full((A["na"] + pad, 8), SENT_F, F32), np.full((B["na"] + pad, 8), SENT_F, F32)
    nn = np.full(A["na"] + pad, SENT_I, np.int64)
    circle_rows(q, A, st_a, nn, fault)
    circle_rows(q, B, st_b, None, fault)
    return st_a, st_b, circle_final(st_a, A["na"], st_b, B["na"]), nn


def _bwd_rows(q, side, stA, stB, nA, nB, grad_out, fault):
    na, nb = side["na"], side["nb"]
    E = _entries(q, side, fault)
    valid = np.broadcast_to(_valid(side, fault), (na, nb))
    g = F32(0.5) * F32(grad_out)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ca = np.where((stA[:na, 3] != 0) & (nA > 0), g * stA[:na, 6] / nA, F32(0)).astype(F32)
        cb = np.where((stB[:nb, 3] != 0) & (nB > 0), g * stB[:nb, 6] / nB, F32(0)).astype(F32)
        G = ca[:, None] * (np.exp(E["ap"] - stA[:na, 0:1]) * E["pw"] - np.exp(E["an"] - stA[:na, 1:2]) * E["nw"]) + \
            cb[None, :] * (np.exp(E["ap"] - stB[None, :nb, 0]) * E["pw"] - np.exp(E["an"] - stB[None, :nb, 1]) * E["nw"])
        G = np.where(valid, G, F32(0)).astype(F32)
        if "cd" in side:
            return G, E["at"]
        live = (F32(2) - F32(2) * E["s"] > F32(1e-12)) | (fault == "clamp_grad_kept")
        Gs = np.where(live & valid, -G / E["fd"], F32(0)).astype(F32)
        Gl = _lanes(Gs, 0)
        bF = np.zeros((512, O.D), F32)
        bF[:nb] = side["bF"]
        bF = bF.reshape(8, 64, O.D)
        acc = np.zeros((na, 64, O.D), F32)
        for t in range(8):
            acc = Gl[:, t, :, None] * bF[None, t] + acc
        for d in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, XOR[d]]
    dA = acc[:, 0].copy()
    if side.get("a_row") is not None:
        dA[side["a_row"] < 0] = 0
    return dA


def circle_backward(q, st_a, st_b, out4, grad_out, g=None, cd=None, fd=None, fault=None):
    q = _q32(q)
    A, B = _sides(q, g, cd, fd, None)
    if g is None:
        G, at = _bwd_rows(q, A, st_a, st_b, out4[2], out4[3], grad_out, fault)
        out = np.full(cd.size, SENT_F, F32)
        out[at.reshape(-1)] = G.reshape(-1)
        return out.reshape(cd.shape)
    return (_bwd_rows(q, A, st_a, st_b, out4[2], out4[3], grad_out, fault),
            _bwd_rows(q, B, st_b, st_a, out4[3], out4[2], grad_out, fault))


def circle_scatter(d_anchor, row, n_rows, init, fault=None):
    if fault != "scatter_first_only":
        return O.circle_scatter(d_anchor, row, n_rows, init)
    out = np.array(init, dtype=F32, copy=True)
    row = np.asarray(row, np.int64)
    for r in np.unique(row[(row >= 0) & (row < n_rows)]):
        out[r] = np.asarray(d_anchor, F32)[np.nonzero(row == r)[0][0]]
    return out


# ------------------------------------------------------------------------------------------------------- weighted BCE
def weighted_bce(pred, gt, n_max, n_dev=None, fault=None, slack=16):
    """-> out8 float32.  pred / gt may be longer than n_max (what lies behind the vectors, for the unclamped fault)"""
    def count(n_dev):
        if n_dev is None:
            return n_max
        if fault == "ndev_unclamped":
            return max(int(n_dev), 0)
        return max(0, min(int(n_dev), n_max))
    n = min(count(n_dev), len(pred))
    nblocks = min(max((n_max + 255) // 256, 1), 256)
    i = np.arange(n)
    if fault == "bce_one_trip":
        i = i[i < nblocks * 256]
    p32 = np.asarray(pred, F32)[i]
    p, g = p32.astype(np.float64), np.asarray(gt, F32)[i].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = -(g * np.maximum(np.log(p), -100.0) + (1.0 - g) * np.maximum(np.log(1.0 - p), -100.0))
        pos = g >= 0.5
        hat = p32 >= F32(0.5) if fault == "half_is_one" else p32 > F32(0.5)
        block = (i // 256) % nblocks
        part = np.zeros((nblocks, 6))
        for k, v in enumerate((g, np.where(pos, l, 0.0), np.where(pos, 0.0, l), pos & hat, ~pos & hat, pos & ~hat)):
            part[:, k] = np.bincount(block, weights=v.astype(np.float64), minlength=nblocks)
        s = part.sum(0)
        nd = float(count(n_dev))
        w_neg = s[0] / nd
        out = [((1.0 - w_neg) * s[1] + w_neg * s[2]) / nd, w_neg, s[3] / (s[3] + s[4]) if s[3] + s[4] > 0 else 0.0,
               s[3] / (s[3] + s[5]) if s[3] + s[5] > 0 else 0.0, s[3], s[4], s[5], nd]
    return np.array(out).astype(F32)


def weighted_bce_backward(pred, gt, n_max, out8, grad_out, n_dev=None, scatter_pos=None, dpred=None):
    n = O.bce_n(n_max, n_dev)
    p, g = np.asarray(pred, F32)[:n].astype(np.float64), np.asarray(gt, F32)[:n].astype(np.float64)
    w_neg = float(out8[1])
    w = np.where(g >= 0.5, 1.0 - w_neg, w_neg)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = float(F32(grad_out)) * w / float(n) * (p - g) / np.maximum((1.0 - p) * p, 1e-12)
    dpred[np.arange(n) if scatter_pos is None else np.asarray(scatter_pos)[:n]] = d.astype(F32)
    return dpred


# ------------------------------------------------------------------------------------------------ arg-max and saliency
def _argmax_dir(A, B, na, nb, out, fault):
    if na <= 0:
        return
    nblk = (max(nb, 0) + 63) // 64
    Bp = np.zeros((nblk * 64, O.D), F32)
    Bp[:nb] = B[:nb]
    sc = np.zeros((na, nblk * 64), F32)
    for j in range(O.D // 4):
        acc = np.zeros_like(sc)
        for kq in range(4):
            acc = A[:na, 4 * j + kq][:, None] * Bp[None, :, 4 * j + kq] + acc
        sc = sc + acc
    ok = (np.arange(nblk * 64) < nb) | (fault == "pad_wins")
    sc, ok = sc.reshape(na, nblk * 4, 16), np.broadcast_to(ok, (na, nblk * 64)).reshape(na, nblk * 4, 16)
    lane_high, shuffle_high = fault == "argmax_tie_high_lane", fault == "argmax_tie_high_shuffle"
    bv, bi = np.full((na, 16), -np.inf, F32), np.full((na, 16), 0x7fffffff, np.int64)
    for t in range(nblk * 4):
        better = ok[:, t] & ((sc[:, t] >= bv) if lane_high else (sc[:, t] > bv))
        bv, bi = np.where(better, sc[:, t], bv), np.where(better, 16 * t + np.arange(16)[None, :], bi)
    for d in (1, 2, 4, 8):
        x = np.arange(16) ^ d
        ov, oi = bv[:, x], bi[:, x]
        better = (ov > bv) | ((ov == bv) & ((oi > bi) if shuffle_high else (oi < bi)))
        bv, bi = np.where(better, ov, bv), np.where(better, oi, bi)
    out[:na] = np.where(bi[:, 0] == 0x7fffffff, 0, bi[:, 0])


def gathered_argmax(a, a_idx, na_dev, b, b_idx, nb_dev, fault=None):
    na, nb = min(int(na_dev), len(a_idx)), min(int(nb_dev), len(b_idx))
    row, col = np.full(len(a_idx), SENT_I, np.int64), np.full(len(b_idx), SENT_I, np.int64)
    A, B = np.asarray(a, F32)[np.asarray(a_idx)[:max(na, 0)]], np.asarray(b, F32)[np.asarray(b_idx)[:max(nb, 0)]]
    _argmax_dir(A, B, na, nb, row, fault)
    _argmax_dir(B, A, nb, na, col, fault)
    return row, col


def saliency_labels(src_pcd, tgt_pcd, rot, trans, src_idx, tgt_idx, counts, row_arg, col_arg, scores, radius):
    ref = O.saliency_labels(src_pcd, tgt_pcd, rot, trans, src_idx, tgt_idx, counts, row_arg, col_arg, scores, radius)
    ns, nt = int(counts[0]), int(counts[1])
    si, ti = np.asarray(src_idx, np.int64)[:ns], np.asarray(tgt_idx, np.int64)[:nt]
    s = np.concatenate([si, si[np.asarray(col_arg, np.int64)[:nt]]])
    t = np.concatenate([ti[np.asarray(row_arg, np.int64)[:ns]], ti])
    d = dist32(rigid32(rot, trans, np.asarray(src_pcd, F32)[s]), np.asarray(tgt_pcd, F32)[t])
    return dict(labels=(d < F32(radius)).astype(F32), dist=d, pos=ref["pos"], sel=ref["sel"].astype(F32))

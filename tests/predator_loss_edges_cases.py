"""Named inputs for the descriptor-loss kernels (apr_amd/csrc/metric_loss.hip), each with the line of the kernel it presses.
NumPy only; D = 32 and KITTI's parameters throughout (one named dense case departs from them, see `dense-1x1-zneg`).

Margins are a condition of every case, asserted in tests/test_predator_loss_edges_oracle_cpu.py from the oracle alone:
every decision a GPU test holds the kernels to (pos / neg masks, hit, row arg-min, select, saliency label, arg-max) is
further from its boundary in float64 than its float32 bound, so the GPU tests exclude nothing.  The named exceptions are
planted exact ties (bitwise identical rows: both sides see the same float32 number) and, on the dense route, planted
exact-threshold entries (the comparison is of the given float32 numbers themselves).

Two shapes the anchor route cannot produce and that therefore live on the dense route: a row with a negative and no positive
(an anchor's own pair passed the select, so it is a positive), and 'rows selected, no column selected' (a negative in
column j is also a negative of column j, whose own pair is its positive).  With pos_margin == pos_optimal and neg_margin
== neg_optimal both exponents are >= 0, so z >= 0 under KITTI's parameters; z < -20 needs a single column and other
margins: `dense-1x1-zneg`.

Not built, for any GPU test: a correspondence list that leaves one cloud's index list empty and the other's not (every t
out of range while some s is valid): k_saliency_labels would read tgt_idx[0] of an unwritten list; the reference raises.
"""
import functools

import numpy as np

import predator_loss_edges_oracle as O
import predator_loss_oracle as T

F32 = np.float32
KITTI = T.KITTI
Q = O.params(KITTI)
SELECT_THRESH = KITTI["pos_radius"] - 0.001          # the Python double MetricLoss.select hands to the library
D = O.D


def _rot():
    ax = np.array([0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * K @ K).astype(F32)


ROT, TRANS = _rot(), np.array([1.5, -2.25, 0.75], F32)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _dirs(rng, n):
    return _unit(rng.standard_normal((n, 3)))


def _partner(src_pts, off):
    """R s + t + off in float64 (rounded to float32 by the caller)"""
    return O.f64(src_pts) @ O.f64(ROT).T + O.f64(TRANS) + off


# ----------------------------------------------------------------------------------------------------- circle, anchors
DYADIC = np.zeros(D)
DYADIC[[1, 6, 17, 30]] = 0.5                          # |row| = 1, every product and partial sum exact: s == 1, x == 0
E5 = np.zeros(D)
E5[5] = 1.0
E5_NEAR = E5 * (1.0 - 2.0 ** -21)                     # s = 1 - 2^-21 exactly: x = 2^-20, fd = 2^-10 ~ 9.8e-4


def build_anchors(name, fact, seed, P, nfilt=None, ncl=None, one_ball=False, share_a=(), share_b=(), choice=None,
                  plants=(), grad_out=1.0, expect=None):
    """`nfilt` correspondences pass the select (rank k = their order in corr), interleaved with far and out-of-range rows.
    Rank k sits in group (k % ncl, (k // ncl) % 3): superclusters 3 apart on a line, three groups per supercluster at
    0 / 0.5 / 1.0 along it, jitter +-0.03 (src) and +-0.01 (partner): same group < 0.13 (positive), neighbouring groups
    0.38 .. 0.62 (neither), everything else > 0.88 (negative).  share_a / share_b: lists of ranks that share one src / tgt
    point.  plants: ("identical" | "near" | "tie", k1, k2) on ranks."""
    rng = np.random.default_rng(seed)
    nfilt = P if nfilt is None else nfilt
    ncl = max(1, min(8, nfilt // 6)) if ncl is None else ncl
    k = np.arange(nfilt)
    cen = np.zeros((nfilt, 3))
    if not one_ball:
        cen[:, 0] = 3.0 * (k % ncl) + 0.5 * ((k // ncl) % 3)
    own_a, own_b = k.copy(), k.copy()
    for grp in share_a:
        own_a[list(grp)] = grp[0]
    for grp in share_b:
        own_b[list(grp)] = grp[0]
        cen[list(grp)] = cen[grp[0]]
    sp = cen + rng.uniform(-0.03, 0.03, (nfilt, 3))
    sp = sp[own_a]
    for grp in share_b:                                # anchors of one tgt point: their src points around its pre-image
        sp[list(grp)] = sp[grp[0]] + rng.uniform(-0.01, 0.01, (len(grp), 3))
    sp = sp.astype(F32)
    tp = _partner(sp, rng.uniform(-0.01, 0.01, (nfilt, 3)))
    tp = tp[own_b].astype(F32)
    sigma = np.array([0.15, 0.3, 1.0, 3.0])[k % 4] if nfilt else np.zeros(0)
    for p in plants:
        if p[0] == "tie":
            sigma[p[1]] = 0.15
    fa = _unit(rng.standard_normal((nfilt, D)))[own_a]
    fb = _unit(fa + sigma[:, None] * _unit(rng.standard_normal((nfilt, D))))[own_b]
    # far pairs (0.3 apart: rejected by the select) and the clouds' unused points
    n_far = max(1, nfilt // 4)
    fs = np.stack([-5.0 - 2.0 * np.arange(n_far), np.full(n_far, 3.0), np.zeros(n_far)], 1).astype(F32)
    ft = _partner(fs, 0.3 * _dirs(rng, n_far)).astype(F32)
    ua, ia = np.unique(own_a, return_inverse=True)
    ub, ib = np.unique(own_b, return_inverse=True)
    n_src, n_tgt = len(ua) + n_far + 3, len(ub) + n_far + 5
    ps, pt = rng.permutation(n_src), rng.permutation(n_tgt)
    src_pcd, tgt_pcd = rng.uniform(20, 30, (n_src, 3)).astype(F32), rng.uniform(-30, -20, (n_tgt, 3)).astype(F32)
    src_feats = _unit(rng.standard_normal((n_src, D))).astype(F32)
    tgt_feats = _unit(rng.standard_normal((n_tgt, D))).astype(F32)
    s_of, t_of = ps[ia], pt[ib]                        # cloud rows of rank k
    src_pcd[s_of], tgt_pcd[t_of] = sp, tp
    src_feats[s_of], tgt_feats[t_of] = fa.astype(F32), fb.astype(F32)
    fs_of, ft_of = ps[len(ua):len(ua) + n_far], pt[len(ub):len(ub) + n_far]
    src_pcd[fs_of], tgt_pcd[ft_of] = fs, ft
    for kind, k1, k2 in plants:
        if kind == "identical":
            src_feats[s_of[k1]] = tgt_feats[t_of[k2]] = DYADIC.astype(F32)
        elif kind == "near":
            src_feats[s_of[k1]], tgt_feats[t_of[k2]] = E5.astype(F32), E5_NEAR.astype(F32)
        elif kind == "tie":
            tgt_feats[t_of[k2]] = tgt_feats[t_of[k1]]
    bad = np.array([[-1, t_of[0] if nfilt else 0], [n_src, 1], [2, -1], [0, n_tgt], [-4, n_tgt + 9]], np.int64)
    rows = np.concatenate([np.stack([s_of, t_of], 1).reshape(-1, 2), np.stack([fs_of, ft_of], 1), bad]).astype(np.int64)
    kindv = np.concatenate([np.zeros(nfilt, int), np.ones(n_far + len(bad), int)])
    C = len(rows)
    other = np.sort(rng.choice(C, n_far + len(bad), replace=False))
    slot = np.ones(C, bool)
    slot[other] = False
    corr = np.zeros((C, 2), np.int64)
    corr[slot], corr[~slot] = rows[kindv == 0], rows[kindv == 1][rng.permutation(n_far + len(bad))]
    if choice is None:
        choice = rng.permutation(nfilt)[:P]
    choice = np.asarray(choice(rng, nfilt) if callable(choice) else choice, dtype=np.int64)
    assert len(choice) == P
    return dict(name=name, fact=fact, kind="anchors", P=P, nfilt=nfilt, src_pcd=src_pcd, tgt_pcd=tgt_pcd, src_feats=src_feats,
                tgt_feats=tgt_feats, corr=corr, rot=ROT, trans=TRANS, choice=choice, thresh=SELECT_THRESH, q=Q,
                grad_out=float(F32(grad_out)), expect=expect or {}, s_of=s_of, t_of=t_of)


def _choice_edges(rng, nfilt):
    c = rng.permutation(nfilt)[:129]
    c[[3, 40, 128]] = [nfilt, nfilt + 1000, 2 ** 40]       # >= count
    c[[0, 77]] = [-1, -2 ** 33]                            # negative
    c[[10, 90, 91]] = c[[5, 5, 6]]                         # duplicates: identical anchors (an exact tie in every row)
    return c


_ANCHORS = {
    # name: (fact, kwargs)
    "anc-p1": ("P = 1: one wave, 63 idle lanes; the one pair is positive, no negative: nothing selected, loss NaN, zero gradient",
               dict(seed=11, P=1, expect=dict(loss_nan=True, zero_grad=True))),
    "anc-p15-ball": ("P = 15 (a short block of CL_ROWS) in one ball: every row has a positive and no negative, NaN, zero gradient",
                     dict(seed=12, P=15, one_ball=True, expect=dict(loss_nan=True, zero_grad=True, pos_no_neg=True))),
    "anc-p16": ("P = 16: exactly one block of CL_ROWS waves", dict(seed=13, P=16, ncl=2, plants=(("identical", 0, 1),),
                                                                  expect=dict(clamped=1))),
    "anc-p17-mixed": ("P = 17: a second block with one wave; one supercluster, so the middle group's rows have a positive and "
                      "no negative next to selected rows", dict(seed=14, P=17, ncl=1, expect=dict(pos_no_neg=True, some_sel=True))),
    "anc-p63": ("P = 63: lane 63 idle in every trip", dict(seed=15, P=63, plants=(("near", 2, 3),), expect=dict(near=True))),
    "anc-p64": ("P = 64: a full first trip, no second", dict(seed=16, P=64, plants=(("tie", 4, 9),), expect=dict(nn_tie=True))),
    "anc-p65": ("P = 65: lane 0 alone in the second trip; identical rows across the clouds (clamp binds), fd ~ 1e-3 rows and "
                "an exact fd tie", dict(seed=17, P=65, plants=(("identical", 0, 1), ("near", 2, 3), ("tie", 4, 9)), grad_out=0.75,
                                        expect=dict(clamped=1, near=True, nn_tie=True, zgt20=True))),
    "anc-p64-shared": ("anchors sharing a row: one src row under 40 anchors, one under 2, the rest under 1; one tgt row under 3 "
                       "(k_circle_scatter's ordered sum)",
                       dict(seed=18, P=64, share_a=(tuple(range(8, 48)), (50, 51)), share_b=((2, 3, 4),), expect=dict(shared=40, nn_tie=True))),
    "anc-p129-choice": ("choice with entries >= count, negative and duplicated: absent anchors (row -1) drop their row and column",
                        dict(seed=19, P=129, nfilt=150, choice=_choice_edges, expect=dict(absent=5, nn_tie=True))),
    "anc-p1-empty": ("no filtered correspondence: count = 0, choice = [0], one absent anchor",
                     dict(seed=20, P=1, nfilt=0, choice=[0], expect=dict(absent=1, loss_nan=True, zero_grad=True))),
    "anc-p442": ("P = 442: 148 * 442 = 65 416 bytes of dynamic LDS, the last size under 64 KB", dict(seed=21, P=442, expect=dict(lds_over=False))),
    "anc-p443": ("P = 443: 65 564 bytes, the first size that needs hipFuncSetAttribute", dict(seed=22, P=443, expect=dict(lds_over=True))),
    "anc-p512": ("P = 512 = ML_MAXP: all CL_T = 8 trips full, 32 blocks", dict(seed=23, P=512, grad_out=0.75, expect=dict(lds_over=True, zgt20=True))),
}


# ------------------------------------------------------------------------------------------------------- circle, dense
def build_dense(name, fact, seed, na, nb, thresholds=False, fd_plants=False, mode="random", over=None, grad_out=1.0,
                expect=None):
    rng = np.random.default_rng(seed)
    q = O.params(KITTI, **(over or {}))
    level = rng.choice([0.1, 0.5, 1.0], size=(na, nb), p=[0.15, 0.45, 0.4])
    cd = (level * rng.uniform(0.9, 1.1, (na, nb))).astype(F32)
    fd = rng.uniform(0.05, 1.9, (na, nb)).astype(F32)
    planted = {}
    if mode == "rows-only":
        cd[:] = F32(0.5)
        cd[0, 0], cd[0, 1] = F32(0.1), F32(1.0)
    elif mode == "pos":
        cd[:] = F32(0.1)
    elif mode == "zneg":
        cd[:], fd[:] = F32(0.1), F32(0.8)
    flat_c, flat_f = cd.reshape(-1), fd.reshape(-1)
    if thresholds:
        pr, sr = F32(q["pos_radius"]), F32(q["safe_radius"])
        vals = [pr, np.nextafter(pr, F32(0)), np.nextafter(pr, F32(9)), sr, np.nextafter(sr, F32(0)), np.nextafter(sr, F32(9))]
        at = (np.arange(len(vals)) * (cd.size // len(vals)) + 1) % cd.size
        flat_c[at] = vals
        planted["cd"] = at
    if fd_plants:
        at = (np.arange(3) * (cd.size // 3) + 2) % cd.size
        flat_f[at] = [F32(0), F32(1e-6), F32(2)]
        flat_c[at] = [F32(1.0), F32(0.1), F32(0.1)]      # fd = 0 under a negative (nw = 1.4), 1e-6 and 2 under positives
        planted["fd"] = at
    return dict(name=name, fact=fact, kind="dense", na=na, nb=nb, cd=cd, fd=fd, q=q, grad_out=float(F32(grad_out)),
                planted=planted, expect=expect or {})


_DENSE = {
    "dense-1x1": ("1 x 1: one positive entry, nothing selected on either side: NaN, zero gradient",
                  dict(seed=41, na=1, nb=1, mode="pos", expect=dict(loss_nan=True, zero_grad=True))),
    "dense-1x1-zneg": ("1 x 1 with log_scale = 64, pos_margin = 1.5 (NOT KITTI's): z = 64 (0.8 - 1.5) 0.7 = -31 < -20 in softplus "
                       "and sigmoid", dict(seed=42, na=1, nb=1, mode="zneg", over=dict(log_scale=64, pos_margin=1.5),
                                           expect=dict(loss_nan=True, zlt=-20.0))),
    "dense-1x512": ("1 x 512: the row pass has one wave with 8 full trips, the column pass 512 waves of one entry, strides swapped",
                    dict(seed=43, na=1, nb=512, thresholds=True, fd_plants=True)),
    "dense-512x1": ("512 x 1: the mirror image; sj = nb = 1 equals si", dict(seed=44, na=512, nb=1, thresholds=True, fd_plants=True)),
    "dense-17x65": ("17 x 65: not square, a second row block of one wave and a second trip of one lane; entries at float32("
                    "pos_radius), float32(safe_radius) and one ulp to either side; feats_dist 0, 1e-6, 2",
                    dict(seed=45, na=17, nb=65, thresholds=True, fd_plants=True, grad_out=0.75)),
    "dense-64x16": ("64 x 16: rows a multiple of CL_ROWS, the column pass sweeps 64 rows in one full trip",
                    dict(seed=46, na=64, nb=16, thresholds=True, fd_plants=True)),
    "dense-443x3": ("443 x 3: the column pass has 443 entries per wave (7 trips, the last short); rows with a negative and no "
                    "positive", dict(seed=47, na=443, nb=3, thresholds=True, fd_plants=True, expect=dict(neg_no_pos=True))),
    "dense-64x16-rows-only": ("row 0 selected, no column selected: out4[3] = 0, loss NaN, the row part of the gradient finite",
                              dict(seed=48, na=64, nb=16, mode="rows-only", expect=dict(loss_nan=True, rows_only=True))),
}


# ------------------------------------------------------------------------------------------- select and overlap labels
def build_select(name, fact, seed, n_corr, n_src, n_tgt, mode="mixed"):
    """src point j is the pre-image of tgt point j % n_tgt plus an offset whose length cycles through thr -+ k 1e-4
    (k = 1, 2, 3: either side of float32(pos_radius - 0.001), at a margin above the distance bound of ~2e-5), 0.05 and 0.5."""
    rng = np.random.default_rng(seed)
    thr = O.f32r(SELECT_THRESH)
    tgt = rng.uniform(-8, 8, (n_tgt, 3)).astype(F32)
    j = np.arange(n_src)
    kk = 1 + (j // 8) % 3
    length = np.choose(j % 8, [thr - 1e-4 * kk, thr + 1e-4 * kk, 0.05, 0.5, thr - 1e-4 * kk, thr + 2e-4 * kk, 0.15, 0.3])
    Rinv = np.linalg.inv(O.f64(ROT))
    src = ((O.f64(tgt)[j % n_tgt] + length[:, None] * _dirs(rng, n_src) - O.f64(TRANS)) @ Rinv.T).astype(F32)
    if mode == "all":                                          # every point of both clouds labelled
        assert n_src == n_tgt and n_corr >= n_src
        s = np.concatenate([np.arange(n_src), rng.integers(0, n_src, n_corr - n_src)])
        corr = np.stack([s, s], 1)[rng.permutation(n_corr)]
    elif mode == "allbad":                                     # no point labelled: both ends of every row out of range
        corr = np.stack([rng.choice([-1, -9, n_src, n_src + 3], n_corr), rng.choice([-2, n_tgt, n_tgt + 70000], n_corr)], 1)
    else:
        s = rng.integers(0, n_src, n_corr)
        corr = np.stack([s, s % n_tgt], 1)
        if n_corr >= 16:
            cross = rng.choice(n_corr, n_corr // 8, replace=False)                   # unrelated pairs, far apart
            corr[cross, 1] = rng.integers(0, n_tgt, len(cross))
            dup = rng.choice(n_corr, n_corr // 8, replace=False)                     # duplicate correspondences
            corr[dup] = corr[(dup * 7 + 3) % n_corr]
            bad = rng.choice(n_corr, 10, replace=False)
            corr[bad[:5], 0] = [-1, n_src, -2 ** 40, n_src + 5, 2 ** 35]
            corr[bad[5:], 1] = [-1, n_tgt, -3, n_tgt + 1, 2 ** 33]
    return dict(name=name, fact=fact, kind="select", corr=corr.astype(np.int64).reshape(-1, 2), src_pcd=src, tgt_pcd=tgt, rot=ROT,
                trans=TRANS, thresh=SELECT_THRESH, n_src=n_src, n_tgt=n_tgt)


_SELECT = {
    "sel-n0": ("n_corr = 0: no launch of k_labels_set, both lists empty, count 0", dict(seed=61, n_corr=0, n_src=5, n_tgt=7)),
    "sel-n1": ("n_corr = 1, n_src = 1, n_tgt = 70 001: thread 0 alone has a chunk; the tgt compaction walks 69 per thread",
               dict(seed=62, n_corr=1, n_src=1, n_tgt=70001)),
    "sel-n1023": ("n_corr = 1023: one row per thread, thread 1023 idle", dict(seed=63, n_corr=1023, n_src=300, n_tgt=211)),
    "sel-n1024": ("n_corr = 1024: one row per thread, all 16 waves full", dict(seed=64, n_corr=1024, n_src=300, n_tgt=211)),
    "sel-n1025": ("n_corr = 1025: two rows per thread, thread 512 has one, threads 513.. none", dict(seed=65, n_corr=1025, n_src=300, n_tgt=211)),
    "sel-n5000": ("n_corr = 5000, n_src = 70 000, n_tgt = 1: five rows per thread, threads 1000.. idle; the one tgt point labelled",
                  dict(seed=66, n_corr=5000, n_src=70000, n_tgt=1)),
    "sel-all": ("every point of both clouds labelled: the lists are 0 .. n - 1, counts equal the lengths",
                dict(seed=67, n_corr=2500, n_src=1100, n_tgt=1100, mode="all")),
    "sel-allbad": ("every row out of range at both ends: no point labelled, nothing selected", dict(seed=68, n_corr=40, n_src=9, n_tgt=6, mode="allbad")),
}


# ------------------------------------------------------------------------------------------------------------- arg-max
def build_argmax(name, fact, seed, na, nb, na_dev=None, nb_dev=None, b_positive=False, neg_rows=(), row_ties=(), col_ties=(),
                 last_col_row=None, beyond=None):
    """index lists of length na / nb that permute and skip rows of [na + 7, 32] / [nb + 5, 32] matrices; device counts na_dev
    / nb_dev.  row_ties (r, c1, c2): list columns c1 and c2 hold bitwise identical rows and row r's maximum is on them."""
    rng = np.random.default_rng(seed)
    a = _unit(rng.standard_normal((na + 7, D))).astype(F32)
    b = _unit(rng.standard_normal((nb + 5, D))).astype(F32)
    a_idx = rng.permutation(na + 7)[:na].astype(np.int32)
    b_idx = rng.permutation(nb + 5)[:nb].astype(np.int32)
    na_dev, nb_dev = na if na_dev is None else na_dev, nb if nb_dev is None else nb_dev
    nbe = min(nb, nb_dev)
    if b_positive:
        b = np.abs(b)
    for r in neg_rows:
        a[a_idx[r]] = -np.abs(a[a_idx[r]])
    for r, c1, c2 in row_ties:
        b[b_idx[c2]] = b[b_idx[c1]]
        a[a_idx[r]] = (2 * b[b_idx[c1]] + 0.05 * rng.standard_normal(D)).astype(F32)
    for c, r1, r2 in col_ties:
        noise = 0.05 * rng.standard_normal(D)
        if b_positive:                                      # keep every b row positive: the negative rows stay negative
            a[a_idx[r1]], noise = np.abs(a[a_idx[r1]]), np.abs(noise)
        a[a_idx[r2]] = a[a_idx[r1]]
        b[b_idx[c]] = (2 * a[a_idx[r1]] + noise).astype(F32)
    if last_col_row is not None:
        a[a_idx[last_col_row]] = (2 * b[b_idx[nbe - 1]]).astype(F32)
    if beyond is not None:                                  # (row, column >= nb_dev): a winner that must not be seen
        a[a_idx[beyond[0]]] = (3 * b[b_idx[beyond[1]]]).astype(F32)
    return dict(name=name, fact=fact, kind="argmax", a=a, b=b, a_idx=a_idx, b_idx=b_idx, na_dev=na_dev, nb_dev=nb_dev,
                neg_rows=tuple(neg_rows), row_ties=tuple(row_ties), col_ties=tuple(col_ties), last_col_row=last_col_row,
                b_positive=b_positive)


_ARGMAX = {
    "am-1x1": ("1 x 1: one row, one column, 63 padded columns and 63 padded rows", dict(seed=81, na=1, nb=1)),
    "am-1x65-neg": ("1 x 65, every score negative: the 63 zero-padded columns of the second block (and, in the column pass, 63 "
                    "padded rows) score 0 > every true score; na_dev above the list length",
                    dict(seed=82, na=1, nb=65, na_dev=5, b_positive=True, neg_rows=(0,))),
    "am-63x64": ("63 x 64: one full column block; na_dev = 60 below the list length: rows 60 .. 62 stay untouched",
                 dict(seed=83, na=63, nb=64, na_dev=60, last_col_row=7)),
    "am-64x63": ("64 x 63: a full row block against a short column block; nb_dev above the list length; a row's maximum on the "
                 "last valid column 62", dict(seed=84, na=64, nb=63, nb_dev=70, last_col_row=5)),
    "am-65x129": ("65 x 129: a second row block of one row, three column blocks; exact ties on two lanes of one 16-column tile (3, "
                  "9), of two tiles of a block (20, 50) and of two blocks (10, 100), settled by the closing shuffle; ties on ONE lane, "
                  "in two tiles of a block (5, 21) and in two blocks (7, 71), settled by the running strict > alone; column ties "
                  "across row blocks on two lanes (rows 2, 64) and on one lane in two tiles (rows 1, 17); maximum on column 128",
                  dict(seed=85, na=65, nb=129, row_ties=((11, 3, 9), (12, 20, 50), (13, 10, 100), (14, 5, 21), (15, 7, 71)),
                       col_ties=((77, 2, 64), (78, 1, 17)), last_col_row=30)),
    "am-65x129-short": ("65 x 129 with nb_dev = 100: columns 100 .. 128 are not there, though row 6 would prefer column 110; "
                        "col_arg[100:] untouched", dict(seed=86, na=65, nb=129, nb_dev=100, beyond=(6, 110), last_col_row=9)),
    "am-130x17-neg": ("130 x 17: three row blocks, a 17-column block with 47 padded columns; every b row is positive and rows 0 .. 9 "
                      "are negative, so all their scores are negative; a tie in column 4 between rows 20 and 84: one lane of the "
                      "column pass (20 & 15 == 84 & 15) in the first and the second row block",
                      dict(seed=87, na=130, nb=17, b_positive=True, neg_rows=tuple(range(10)), col_ties=((4, 20, 84),))),
}


# ------------------------------------------------------------------------------------------------------------ saliency
def build_saliency(name, fact, seed, n_src, n_tgt, n_pairs):
    """n_pairs one-to-one correspondences; partner k is 0.3 -+ 2e-4 (either side of float32(matchability_radius)), 0.1 or
    0.6 away, and is the mutual arg-max of its point by construction (features 0.2 apart, everything else ~ sqrt 2)."""
    rng = np.random.default_rng(seed)
    s, t = rng.permutation(n_src)[:n_pairs], rng.permutation(n_tgt)[:n_pairs]
    src = rng.uniform(-8, 8, (n_src, 3)).astype(F32)
    tgt = rng.uniform(-8, 8, (n_tgt, 3)).astype(F32)
    r = O.f32r(KITTI["matchability_radius"])
    length = np.choose(np.arange(n_pairs) % 4, [r - 2e-4, r + 2e-4, 0.1, 0.6])
    tgt[t] = _partner(src[s], length[:, None] * _dirs(rng, n_pairs)).astype(F32)
    sf, tf = _unit(rng.standard_normal((n_src, D))), _unit(rng.standard_normal((n_tgt, D)))
    tf[t] = _unit(sf[s] + 0.2 * _unit(rng.standard_normal((n_pairs, D))))
    return dict(name=name, fact=fact, kind="saliency", corr=np.stack([s, t], 1).astype(np.int64), src_pcd=src, tgt_pcd=tgt,
                src_feats=sf.astype(F32), tgt_feats=tf.astype(F32), rot=ROT, trans=TRANS, n_src=n_src, n_tgt=n_tgt,
                scores=rng.uniform(0.01, 0.99, n_src + n_tgt).astype(F32), radius=KITTI["matchability_radius"])


_SALIENCY = {
    "sal-40": ("40 pairs in clouds of 100 and 77: one block; counts (40, 40) below the vector lengths, the tail of every output "
               "untouched", dict(seed=101, n_src=100, n_tgt=77, n_pairs=40)),
    "sal-290": ("290 pairs in clouds of 400 and 300: 580 entries, three blocks, the switch from the src list to the tgt list "
                "inside block 1", dict(seed=102, n_src=400, n_tgt=300, n_pairs=290)),
}


# ---------------------------------------------------------------------------------------------------------------- BCE
BCE_SPECIAL = np.array([0.0, 1.0, 0.5, 2.0 ** -149, 1.0 - 2.0 ** -24, np.nextafter(F32(0.5), F32(1))], dtype=F32)


def build_bce(name, fact, seed, n, gt_mode):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.01, 0.99, n).astype(F32)
    gt = {"ones": np.ones(n), "zeros": np.zeros(n), "single": np.zeros(n), "mixed": (rng.uniform(size=n) < 0.3) * 1.0}[gt_mode]
    if n >= 8:
        pred[:6] = BCE_SPECIAL
        if gt_mode == "mixed":
            gt[:6] = [1, 0, 1, 0, 1, 0]
    if gt_mode == "single" and n:
        gt[n - 1] = 1.0                                         # the one positive is the last entry
    return dict(name=name, fact=fact, kind="bce", n=n, pred=pred, gt=gt.astype(F32), grad_out=float(F32(0.75)),
                scatter_pos=rng.permutation(n + 9)[:n].astype(np.int32))


_BCE = {
    "bce-n0": ("n = 0: one block that sums nothing; 0 / 0 = NaN loss, zero precision / recall, no backward launch", dict(seed=120, n=0, gt_mode="zeros")),
    "bce-n1": ("n = 1, the one label positive: w_positive = 0, the loss is 0", dict(seed=121, n=1, gt_mode="single")),
    "bce-n255": ("n = 255: one short block; predictions 0, 1, 0.5, 2^-149, 1 - 2^-24, nextafter(0.5, 1)", dict(seed=122, n=255, gt_mode="mixed")),
    "bce-n256": ("n = 256: one full block; gt all ones: w_negative = 1", dict(seed=123, n=256, gt_mode="ones")),
    "bce-n257": ("n = 257: a second block of one thread; gt all zeros: w_negative = 0, NaN-free", dict(seed=124, n=257, gt_mode="zeros")),
    "bce-n65536": ("n = 65 536 = 256 blocks of 256: the last size without a second grid-stride trip", dict(seed=125, n=65536, gt_mode="mixed")),
    "bce-n65537": ("n = 65 537: block 0, thread 0 takes a second trip, and the only positive label is that entry",
                   dict(seed=126, n=65537, gt_mode="single")),
    "bce-n70001": ("n = 70 001: 4465 entries in the second trip, the last block short", dict(seed=127, n=70001, gt_mode="mixed")),
}


def bce_n_devs(n):
    """the device counts each BCE case runs with: absent, 0, 1, n - 1, n, n + 5, -3"""
    return [None, 0, 1, n - 1, n, n + 5, -3]


# ------------------------------------------------------------------------------------------------------------ registry
_BUILDERS = (("anchors", _ANCHORS, build_anchors), ("dense", _DENSE, build_dense), ("select", _SELECT, build_select),
             ("argmax", _ARGMAX, build_argmax), ("saliency", _SALIENCY, build_saliency), ("bce", _BCE, build_bce))
NAMES = {kind: list(reg) for kind, reg, _ in _BUILDERS}
ALL = [n for kind in NAMES for n in NAMES[kind]]
FACTS = {n: reg[n][0] for _, reg, _ in _BUILDERS for n in reg}


@functools.lru_cache(maxsize=None)
def get(name):
    for _, reg, fn in _BUILDERS:
        if name in reg:
            fact, kw = reg[name]
            return fn(name, fact, **kw)
    raise KeyError(name)


# -------------------------------------------------------------------------------------- oracle chains, computed once
@functools.lru_cache(maxsize=None)
def anchors_oracle(name):
    """select -> gather -> forward -> backward -> scatter on the case, all from the oracle"""
    c = get(name)
    sel = O.circle_select(c["corr"], c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], c["thresh"])
    g = O.circle_gather(c["corr"], sel["filt"], sel["count"], c["choice"], c["src_pcd"], c["tgt_pcd"], c["src_feats"],
                        c["tgt_feats"], c["rot"], c["trans"])
    fw = O.anchors_forward(c["q"], g)
    bw = O.circle_backward(c["q"], fw, c["grad_out"], g["a_feats"], g["b_feats"])
    d_src = O.scatter_bounded(bw["d_a"], bw["d_a_bound"], g["a_row"], len(c["src_pcd"]))
    d_tgt = O.scatter_bounded(bw["d_b"], bw["d_b_bound"], g["b_row"], len(c["tgt_pcd"]))
    return dict(sel=sel, g=g, fw=fw, bw=bw, d_src=d_src, d_tgt=d_tgt)


@functools.lru_cache(maxsize=None)
def dense_oracle(name):
    c = get(name)
    fw = O.circle_forward(c["q"], c["cd"], c["fd"])
    return dict(fw=fw, bw=O.circle_backward(c["q"], fw, c["grad_out"]))


@functools.lru_cache(maxsize=None)
def select_oracle(name):
    c = get(name)
    return dict(lab=O.overlap_labels(c["corr"], c["n_src"], c["n_tgt"]),
                sel=O.circle_select(c["corr"], c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], c["thresh"]))


@functools.lru_cache(maxsize=None)
def argmax_oracle(name):
    c = get(name)
    return O.gathered_argmax(c["a"], c["a_idx"], c["na_dev"], c["b"], c["b_idx"], c["nb_dev"])


@functools.lru_cache(maxsize=None)
def saliency_oracle(name):
    c = get(name)
    lab = O.overlap_labels(c["corr"], c["n_src"], c["n_tgt"])
    am = O.gathered_argmax(c["src_feats"], lab["src_idx"], lab["counts"][0], c["tgt_feats"], lab["tgt_idx"], lab["counts"][1])
    sal = O.saliency_labels(c["src_pcd"], c["tgt_pcd"], c["rot"], c["trans"], lab["src_idx"], lab["tgt_idx"], lab["counts"],
                            am["row_arg"], am["col_arg"], c["scores"], c["radius"])
    return dict(lab=lab, am=am, sal=sal)


# ------------------------------------------------------------------------------------------------------------ verdicts
# One judgement per family, shared by the host float32 run (CPU test) and the kernels (GPU test): `got` holds plain NumPy
# arrays, buffers with their sentinel tails.  -> dict of worst |got - oracle| / bound per output; an exact output that
# differs, a NaN out of place or a touched sentinel gives inf.
INF = float("inf")


def _exact(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return 0.0 if got.shape == ref.shape and np.array_equal(got.astype(np.float64), ref.astype(np.float64)) else INF


def _tail(buf, n, sentinel):
    return 0.0 if (np.asarray(buf)[n:] == sentinel).all() else INF


def judge_records(st, nn, S, n, sent_f, sent_i):
    """records [n + pad, 8] and arg-min of one side against the oracle's side S"""
    st = np.asarray(st)
    v = {"flags": _exact(st[:n][:, [3, 4, 5, 7]], S["st"][:, [3, 4, 5, 7]]), "rec_tail": _tail(st, n, sent_f)}
    for k, col in (("lse_pos", 0), ("lse_neg", 1), ("loss", 2), ("sigmoid", 6)):
        v[k] = O.worst_ratio(st[:n, col], S["st"][:, col], S["bound"][:, col])[0]
    if nn is not None:
        v["nn"] = _exact(np.asarray(nn)[:n], S["nn"])
        v["nn_tail"] = _tail(nn, n, sent_i)
    return v


def judge_anchors(name, got, sent_f, sent_i):
    c, r = get(name), anchors_oracle(name)
    sel, g, fw, bw = r["sel"], r["g"], r["fw"], r["bw"]
    P, cnt = c["P"], sel["count"]
    v = {"count": _exact(got["count"], cnt), "filt": _exact(np.asarray(got["filt"])[:cnt], sel["filt"]),
         "filt_tail": _tail(got["filt"], cnt, sent_i), "a_row": _exact(got["a_row"], g["a_row"]), "b_row": _exact(got["b_row"], g["b_row"]),
         "b_pts": _exact(got["b_pts"], g["b_pts"]), "a_feats": _exact(got["a_feats"], g["a_feats"]),
         "b_feats": _exact(got["b_feats"], g["b_feats"]),
         "a_pts": O.worst_ratio(got["a_pts"], g["a_pts"], g["a_pts_bound"])[0]}
    v.update({"A_" + k: x for k, x in judge_records(got["st_a"], got["nn"], fw["A"], P, sent_f, sent_i).items()})
    v.update({"B_" + k: x for k, x in judge_records(got["st_b"], None, fw["B"], P, sent_f, sent_i).items()})
    v["out4"] = max(O.worst_ratio(got["out4"][:2], fw["out4"][:2], fw["out4_bound"][:2])[0], _exact(got["out4"][2:], fw["out4"][2:]))
    for k in ("d_a", "d_b"):
        v[k] = O.worst_ratio(got[k], bw[k], bw[k + "_bound"])[0]
        v[k + "_absent"] = 0.0 if (np.asarray(got[k])[~g["present"]] == 0).all() else INF
    for k in ("d_src", "d_tgt"):
        ref, bound, touched = r[k]
        v[k] = O.worst_ratio(got[k], ref, bound)[0]
        v[k + "_untouched"] = 0.0 if (np.asarray(got[k])[~touched] == 0).all() else INF
    return v


def judge_dense(name, got, sent_f, sent_i):
    c, r = get(name), dense_oracle(name)
    fw, bw = r["fw"], r["bw"]
    v = {"A_" + k: x for k, x in judge_records(got["st_a"], got["nn"], fw["A"], c["na"], sent_f, sent_i).items()}
    v.update({"B_" + k: x for k, x in judge_records(got["st_b"], None, fw["B"], c["nb"], sent_f, sent_i).items()})
    v["out4"] = max(O.worst_ratio(got["out4"][:2], fw["out4"][:2], fw["out4_bound"][:2])[0], _exact(got["out4"][2:], fw["out4"][2:]))
    v["d_fd"] = O.worst_ratio(got["d_fd"], bw["d_fd"], bw["d_fd_bound"])[0]
    return v


def judge_select(name, got, sent_i):
    r = select_oracle(name)
    lab, sel = r["lab"], r["sel"]
    ns, nt = lab["counts"][0], lab["counts"][1]
    return {"gt": _exact(got["gt"], lab["gt"]), "counts": _exact(got["counts"], lab["counts"]),
            "src_idx": _exact(np.asarray(got["src_idx"])[:ns], lab["src_idx"]), "tgt_idx": _exact(np.asarray(got["tgt_idx"])[:nt], lab["tgt_idx"]),
            "src_tail": _tail(got["src_idx"], ns, sent_i), "tgt_tail": _tail(got["tgt_idx"], nt, sent_i),
            "count": _exact(got["count"], sel["count"]), "filt": _exact(np.asarray(got["filt"])[:sel["count"]], sel["filt"]),
            "filt_tail": _tail(got["filt"], sel["count"], sent_i)}


def judge_argmax(name, got, sent_i):
    r = argmax_oracle(name)
    return {"row_arg": _exact(np.asarray(got["row_arg"])[:r["na"]], r["row_arg"]), "col_arg": _exact(np.asarray(got["col_arg"])[:r["nb"]], r["col_arg"]),
            "row_tail": _tail(got["row_arg"], r["na"], sent_i), "col_tail": _tail(got["col_arg"], r["nb"], sent_i)}


def judge_saliency(name, got, sent_f, sent_i):
    s = saliency_oracle(name)["sal"]
    n = s["n"]
    return {"labels": _exact(np.asarray(got["labels"])[:n], s["labels"]), "sel": _exact(np.asarray(got["sel"])[:n], s["sel"]),
            "pos": _exact(np.asarray(got["pos"])[:n], s["pos"]), "dist": O.worst_ratio(np.asarray(got["dist"])[:n], s["dist"], s["dist_bound"])[0],
            "labels_tail": _tail(got["labels"], n, sent_f), "sel_tail": _tail(got["sel"], n, sent_f), "pos_tail": _tail(got["pos"], n, sent_i),
            "dist_tail": _tail(got["dist"], n, sent_f)}


def judge_bce(name, n_dev, got_out8, got_d=None, scatter=False, sent_f=None):
    """forward out8 and, when given, the backward's vector (length n, or n + 9 through scatter_pos) against the oracle"""
    c = get(name)
    ref, bound = O.weighted_bce(c["pred"], c["gt"], n_dev)
    v = {"out8": O.worst_ratio(got_out8, ref, bound)[0]}
    if got_d is not None:
        d, bd = O.weighted_bce_backward(c["pred"], c["gt"], c["grad_out"], n_dev)
        n = len(d)
        at = c["scatter_pos"][:n] if scatter else np.arange(n)
        got_d = np.asarray(got_d)
        v["d"] = O.worst_ratio(got_d[at], d, bd)[0]
        rest = np.ones(len(got_d), bool)
        rest[at] = False
        v["d_tail"] = 0.0 if (got_d[rest] == sent_f).all() else INF
    return v


def worst(v):
    k = max(v, key=lambda k: v[k])
    return k, v[k]

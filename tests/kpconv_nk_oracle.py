"""Float64 NumPy statement of the rigid KPConv with ANY kernel-point count (apr_kpconv_weighted_nk,
apr_kpconv_dfeat_contrib_nk; apr_amd/csrc/kpconv_nk.hip), every influence and both aggregations, with per-element error
bounds for a float32 evaluation, a plain float32 evaluation of the same statement and its one-rule mutants.  numpy only.

The contract is tests/kpconv_oracle.py's with kp [K, 3], K = kp.shape[0], and wf[q, k * cin + c] for k < K; the modes are
tests/kpconv_modes_oracle.py's on a rigid layer: mode = (influence, closest), influence 0 constant (w = 1), 1 linear
(w = max(0, 1 - d / extent)), 2 gaussian (w = exp(-d2 / (2 (0.3 extent)^2 + 1e-9)), not clipped); closest keeps w for
k = argmin_k d2 alone, the lowest k on an exact tie.  Every real neighbour takes part, padding (outside 0 .. ns - 1) adds
nothing and is not counted, num = max(1, #{real, feature sum > 0}).

What is reused and what is restated: `geometry`, `weighted` and `bound_weighted` of kpconv_oracle are general in K and serve
(linear, sum) as they are (tests/test_kpconv_nk_oracle_cpu.py holds the statements below to them); `contrib`, `d_W`,
`bound_contrib` and `bound_dx` reshape by its constant KP = 15 and are restated here with K from kp.shape[0], and so are the
gaussian / closest terms of kpconv_modes_oracle (whose geometry is 15-point too).  The bound derivations -- the docstrings
of those two modules -- count roundings per term and per sum; no step of them depends on K: A = (n + 3) / 2 with n the terms
that exist, the influence's own error per term (linear eps32 (B_W geo + w / 2); constant 0; gaussian w expm1(da) + E_EXP
eps32 w + 2^-125), the rows' sum (n_r - 1) u.
"""
import numpy as np

import kpconv_modes_oracle as MO
import kpconv_oracle as O

EPS32, B_W, M_EDGE, SECOND_ORDER, U = O.EPS32, O.B_W, O.M_EDGE, O.SECOND_ORDER, O.EPS32 / 2.0
E_EXP, ABS_EXP = MO.E_EXP, MO.ABS_EXP
CONSTANT, LINEAR, GAUSSIAN = 0, 1, 2
MODES = MO.MODES
DEFAULT = (LINEAR, 0)
mode_name = MO.mode_name
gauss_den = MO.gauss_den
compare_rows = O.compare_rows
F32 = np.float32
MUTANTS = ("tiles_swapped", "rows_ge16_dropped", "stride_15cin", "tie_high")


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def geometry(q, s, nbr, kp, extent, mode):
    """-> dict: real, idx [nq, H], D [nq, H, 3] (centred neighbour), diff [nq, H, K, 3], d2, d [nq, H, K] (arbitrary for
    padding), cl [nq, H] closest kernel point, keep [nq, H, K] (real and, with closest, the one-hot), w [nq, K, H]"""
    inf, closest = mode
    q, s, kp = _f64(q, s, kp)
    K = len(kp)
    real = O.real_mask(nbr, len(s))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    D = s[idx] - q[:, None, :]
    diff = D[:, :, None, :] - kp[None, None, :, :]
    d2 = (diff ** 2).sum(-1)
    d = np.sqrt(d2)
    cl = np.argmin(d2, axis=-1)
    keep = np.broadcast_to(real[:, :, None], d2.shape).copy()
    if closest:
        keep &= np.arange(K)[None, None, :] == cl[:, :, None]
    if inf == CONSTANT:
        w = np.ones_like(d2)
    elif inf == LINEAR:
        w = np.maximum(0.0, 1.0 - d / float(extent))
    else:
        w = np.exp(-d2 / gauss_den(extent))
    return dict(real=real, idx=idx, D=D, diff=diff, d2=d2, d=d, cl=cl, keep=keep, w=(w * keep).transpose(0, 2, 1), mode=mode, K=K)


def weighted(q, s, nbr, x, kp, extent, mode=DEFAULT):
    """-> wf [nq, K cin], num [nq], geometry"""
    x, = _f64(x)
    g = geometry(q, s, nbr, kp, extent, mode)
    num, _ = O.neighbour_count(nbr, x)
    xg = x[g["idx"]] * g["real"][:, :, None]
    wf = np.einsum("qkh,qhc->qkc", g["w"], xg) / num[:, None, None]
    return wf.reshape(len(wf), -1), num, g


def forward(q, s, nbr, x, kp, extent, W, mode=DEFAULT):
    W, = _f64(W)
    return weighted(q, s, nbr, x, kp, extent, mode)[0] @ W.reshape(-1, W.shape[-1])


def contrib(q, s, nbr, x, kp, extent, dwf, mode=DEFAULT):
    """dwf [nq, K cin] -> [nq * H, cin]; the rows of padding neighbours are 0"""
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, kp, extent, mode)
    num, _ = O.neighbour_count(nbr, x)
    gg = dwf.reshape(nq, g["K"], -1) / num[:, None, None]
    return np.einsum("qkh,qkc->qhc", g["w"], gg).reshape(nq * H, -1)


def d_x_from_dwf(q, s, nbr, x, kp, extent, dwf, mode=DEFAULT):
    return O.scatter_rows(contrib(q, s, nbr, x, kp, extent, dwf, mode), nbr, len(np.asarray(s)))


def d_x(q, s, nbr, x, kp, extent, W, d_out, mode=DEFAULT):
    W, d_out = _f64(W, d_out)
    return d_x_from_dwf(q, s, nbr, x, kp, extent, d_out @ W.reshape(-1, W.shape[-1]).T, mode)


def d_W(q, s, nbr, x, kp, extent, d_out, mode=DEFAULT):
    d_out, = _f64(d_out)
    wf = weighted(q, s, nbr, x, kp, extent, mode)[0]
    return (wf.T @ d_out).reshape(len(np.asarray(kp)), -1, d_out.shape[1])


# ----------------------------------------------------------------------------------------------------------- margins
def edge_margin(q, s, nbr, kp, extent):
    """min over the real (q, h, k) of |d / extent - 1|: how far every neighbour stays from the edge of every ball"""
    g = geometry(q, s, nbr, kp, extent, DEFAULT)
    r = np.abs(g["d"] / float(extent) - 1.0)[g["real"]]
    return float(r.min()) if r.size else np.inf


def closest_margin(q, s, nbr, kp, extent, exempt=()):
    """min over the real (q, h) outside `exempt` of (second smallest d2 - smallest d2) / extent^2 (inf for K = 1)"""
    g = geometry(q, s, nbr, kp, extent, DEFAULT)
    if g["K"] < 2:
        return np.inf
    two = np.sort(g["d2"], axis=-1)[:, :, :2]
    gap = (two[:, :, 1] - two[:, :, 0]) / float(extent) ** 2
    ok = g["real"].copy()
    for row, h in exempt:
        ok[row, h] = False
    return float(gap[ok].min()) if ok.any() else np.inf


# ------------------------------------------------------------------------------------------------------------ bounds
def _influence_error(g, kp, extent):
    """-> (w [nq, H, K], e_sum: the absolute error of a float32 influence where the term exists, without the eps32 w / 2
    that the sums' factor A already holds (linear), lives: the terms that may be non-zero in float32)"""
    inf, _ = g["mode"]
    keep = g["keep"]
    w = g["w"].transpose(0, 2, 1)
    if inf == CONSTANT:
        return w, np.zeros_like(w), keep
    if inf == LINEAR:
        kp, = _f64(kp)
        lives = keep & (g["d"] < float(extent) * (1.0 + M_EDGE))
        geo = (np.linalg.norm(g["D"], axis=-1)[:, :, None] + np.linalg.norm(kp, axis=-1)[None, None, :]) / float(extent)
        return w, EPS32 * B_W * geo * lives, lives
    den = gauss_den(extent)
    e, D = np.abs(g["diff"]), np.abs(g["D"])[:, :, None, :]
    b_d2 = U * (2.0 * (e * (e + D)).sum(-1) + 3.0 * g["d2"])
    da = np.where(keep, b_d2 / den + 4.0 * U * g["d2"] / den, 0.0)
    e_w = ((w * np.expm1(da) + E_EXP * EPS32 * w) * SECOND_ORDER + ABS_EXP) * keep
    return w, e_w, keep


def bound_weighted(q, s, nbr, x, kp, extent, mode=DEFAULT):
    """per-element bound [nq, K cin] of |fp32 wf - wf|"""
    x, = _f64(x)
    g = geometry(q, s, nbr, kp, extent, mode)
    w, e_w, lives = _influence_error(g, kp, extent)
    num, _ = O.neighbour_count(nbr, x)
    ax = np.abs(x[g["idx"]]) * g["real"][:, :, None]
    a = (lives.sum(1) + 3.0) / 2.0                                                  # [nq, K]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qhc->qkc", w, ax)
    edge = np.einsum("qhk,qhc->qkc", e_w, ax)
    b = SECOND_ORDER * (rel + edge) / num[:, None, None]
    return b.reshape(len(b), -1)


def bound_contrib(q, s, nbr, x, kp, extent, dwf, mode=DEFAULT):
    """per-element bound [nq * H, cin] of the contribution rows (0 for padding rows)"""
    dwf, = _f64(dwf)
    nq, H = np.asarray(nbr).shape
    g = geometry(q, s, nbr, kp, extent, mode)
    w, e_w, lives = _influence_error(g, kp, extent)
    num, _ = O.neighbour_count(nbr, x)
    ag = np.abs(dwf.reshape(nq, g["K"], -1))
    a = (lives.sum(2) + 3.0) / 2.0                                                  # [nq, H]
    rel = EPS32 * a[:, :, None] * np.einsum("qhk,qkc->qhc", w, ag)
    edge = np.einsum("qhk,qkc->qhc", e_w, ag)
    return (SECOND_ORDER * (rel + edge) / num[:, None, None]).reshape(nq * H, -1)


def bound_dx(q, s, nbr, x, kp, extent, dwf, mode=DEFAULT):
    """per-element bound [ns, cin] of d_x summed from fp32 contribution rows in any order"""
    ns = len(np.asarray(s))
    rows = np.abs(contrib(q, s, nbr, x, kp, extent, dwf, mode))
    bc = bound_contrib(q, s, nbr, x, kp, extent, dwf, mode)
    flat = np.asarray(nbr, np.int64).reshape(-1)
    n_rows = np.bincount(flat[(flat >= 0) & (flat < ns)], minlength=ns).astype(np.float64)
    summed = O.scatter_rows(rows + bc, nbr, ns)
    return O.scatter_rows(bc, nbr, ns) + 0.5 * EPS32 * np.maximum(n_rows - 1.0, 0.0)[:, None] * summed


# ------------------------------------------------------------------------- a plain float32 evaluation and its mutants
def eval32(q, s, nbr, x, kp, extent, dwf, mode=DEFAULT, mutant=None):
    """The statement with every operation in float32 (NumPy, no kernel's order) -> (wf [nq, K cin], contrib [nq * H, cin],
    the rows of padding neighbours 0).  mutant: one rule changed --
      tiles_swapped      kernel point k trades places with k +- 16 where both exist (the two MFMA tiles mixed up)
      rows_ge16_dropped  kernel points 16 .. K - 1 never stored / never summed
      stride_15cin       the rows of wf and dwf addressed as q * 15 cin instead of q * K cin
      tie_high           an exact tie for the closest kernel point goes to the HIGHER index"""
    inf, closest = mode
    q, s, kp, x, dwf = (np.asarray(a, F32) for a in (q, s, kp, x, dwf))
    nq, H = np.asarray(nbr).shape
    K, cin = len(kp), x.shape[1]
    real = O.real_mask(nbr, len(s))
    idx = np.where(real, np.asarray(nbr, np.int64), 0)
    D = s[idx] - q[:, None, :]
    e = D[:, :, None, :] - kp[None, None, :, :]
    d2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]
    assert d2.dtype == F32
    if inf == CONSTANT:
        w = np.ones_like(d2)
    elif inf == LINEAR:
        w = np.maximum(F32(1) - np.sqrt(d2) * (F32(1) / F32(extent)), F32(0))
    else:
        w = np.exp(-d2 / F32(gauss_den(extent)))
    keep = np.broadcast_to(real[:, :, None], d2.shape).copy()
    if closest:
        cl = (K - 1 - np.argmin(d2[:, :, ::-1], axis=-1)) if mutant == "tie_high" else np.argmin(d2, axis=-1)
        keep &= np.arange(K)[None, None, :] == cl[:, :, None]
    w = (w * keep).astype(F32)                                                       # [nq, H, K]
    cnt = (real & (x.astype(np.float64).sum(1)[idx] > 0)).sum(1)
    inv = (F32(1) / np.maximum(cnt, 1).astype(F32)).astype(F32)
    xg = (x[idx] * real[:, :, None]).astype(F32)
    wf = (np.einsum("qhk,qhc->qkc", w, xg) * inv[:, None, None]).astype(F32)         # [nq, K, cin]
    g3 = dwf.reshape(nq, K, cin)
    if mutant == "stride_15cin":
        flat = np.zeros(nq * max(K, 15) * cin + K * cin, F32)
        src = flat.copy()
        src[:nq * K * cin] = dwf.reshape(-1)
        g3 = np.stack([src[r * 15 * cin:r * 15 * cin + K * cin] for r in range(nq)]).reshape(nq, K, cin)
        for r in range(nq):      # (later rows overwrite earlier ones where the strides overlap, as the stores would)
            flat[r * 15 * cin:r * 15 * cin + K * cin] = wf[r].reshape(-1)
        wf = flat[:nq * K * cin].reshape(nq, K, cin).copy()
    wk = w
    if mutant == "tiles_swapped":
        perm = np.arange(K)
        for k in range(K):
            if k < 16 and k + 16 < K:
                perm[k], perm[k + 16] = k + 16, k
        wf = wf[:, perm]
        wk = w[:, :, perm]
    if mutant == "rows_ge16_dropped":
        wf = wf.copy()
        wf[:, 16:] = 0
        wk = w.copy()
        wk[:, :, 16:] = 0
    gg = (g3 * inv[:, None, None]).astype(F32)
    rows = np.einsum("qhk,qkc->qhc", wk, gg).astype(F32)
    return wf.reshape(nq, K * cin), rows.reshape(nq * H, cin)

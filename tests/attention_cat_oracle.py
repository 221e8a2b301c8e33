"""Float64 NumPy statement of the geometric cross attention ('cross_cat', apr_amd/csrc/attention_cat.hip), forward and
backward, with per-element error bounds for a float32 evaluation.  numpy only, no torch; the softmax statements and their
bounds are tests/attention_oracle.py's, imported unchanged.

Contract, as the kernels state it
---------------------------------
q [n, dim * H], k, v [m, dim * H] in the interleaved channel layout d * H + h, c0 [n, 3], c1 [m, 3].  Per head h and query i,
with P_ij = softmax_j(<q_i, k_j>_h / sqrt(dim))   (the scale uses dim, not dim + 3):
    feat[d] = sum_j P_ij v[j, d, h]     soft[a] = sum_j P_ij c1[j, a]     aug1 = soft - c0[i]     aug2 = ||aug1||_2
    y[i, e * H + h], e in [0, dim + 7):   e < dim: feat;  dim .. dim+2: soft;  dim+3 .. dim+5: aug1;  dim+6: aug2.
Backward, g the gradient of y split the same way, coordinates without gradient:
    g_soft = g[soft] + g[aug1] + g[aug2] * aug1 / aug2   (the last term 0 where aug2 == 0, as torch's norm has it)
    dV = P^T g_feat,   dP_ij = <g_feat_i, v_j> + <g_soft_i, c1_j>,   D_i = sum_j P_ij dP_ij,   dS = P o (dP - D),
    dq = dS k / sqrt(dim),   dk = dS^T q / sqrt(dim).

Error bounds (u = 2^-24, the conventions of attention_oracle.py's docstring)
---------------------------------------------------------------------------
feat, soft   softmax-weighted sums: attention_oracle.softmax_sum's bound with v, respectively c1, as the value rows.  The
             coordinate columns of the MFMA kernel go through the same rescale and merge steps as the value columns; their
             products with the probabilities (one fused step per key) and the two additions over a query's four lanes stay
             inside the count S of that bound, which allows 32 merged partials where the kernel merges 4.
aug1         one more rounding, of the subtraction:   b(aug1) = b(soft) + u (|aug1| + b(soft)).
             b(soft) is of the order u S max|c1| whatever aug1 is, so this bound is ABSOLUTE: it does not shrink with aug1.
aug2         the norm is 1-Lipschitz in its argument:  | ||aug1'|| - ||aug1|| | <= ||b(aug1)||_2.  Three products and two
             additions (all terms >= 0, so the relative errors do not amplify: 3 u on the sum of squares, 1.5 u after the
             root) and the square root itself (2 u: not assumed correctly rounded):
             b(aug2) = ||b(aug1)||_2 + 4 u (aug2 + ||b(aug1)||_2) + 2^-126.
Backward: attention_oracle.mha_train's propagation, to first order in the float64 quantities, with
    r = aug1 / aug2 read from the stored float32 y:   |r' - r| <= (b(aug1) + |r| b(aug2)) / (aug2 - b(aug2)) + 2 u |r|
             (<= 2 ||b(aug1)||_2 / aug2 to first order; asserted: b(aug2) < aug2 / 4 wherever aug2 > 0).  Where aug2 == 0 the
             oracle's term is 0 and a float32 evaluation that does not reach exactly 0 may hold any unit vector: b(r) = 1
             there.  (The planted zero rows have m = 1, where dS = 0 whatever g_soft is: their dq, dk bounds stay small.)
    b(g_soft) = |g[aug2]| b(r) + 3 u (|g[soft]| + |g[aug1]| + |g[aug2] r|)
    b(dP_j)  = (dim + 3) u (sum_d |g_feat_d| |v_jd| + sum_a |g_soft_a| |c1_ja|) + sum_a b(g_soft_a) |c1_ja|
    dV, D, dS, dq, dk as in mha_train with these dP and b(dP).
All times 1 + 2^-10 for the second-order terms.
"""
import numpy as np

import attention_oracle as O

U, TINY, SECOND_ORDER = O.U, O.TINY, O.SECOND_ORDER


def split(y, dim, H):
    """y [n, (dim + 7) * H] -> feat [H, n, dim], soft [H, n, 3], aug1 [H, n, 3], aug2 [H, n]"""
    yh = O.heads_of(y, H)
    return yh[:, :, :dim], yh[:, :, dim:dim + 3], yh[:, :, dim + 3:dim + 6], yh[:, :, dim + 6]


def _head_forward(Q, K, V, C0, C1, scale):
    feat, b_feat, P = O.softmax_sum(Q, K, V, scale)
    soft, b_soft, _ = O.softmax_sum(Q, K, C1, scale)
    aug1 = soft - C0
    b_aug1 = (b_soft + U * (np.abs(aug1) + b_soft)) * SECOND_ORDER
    aug2 = np.sqrt((aug1 ** 2).sum(1))
    nb = np.sqrt((b_aug1 ** 2).sum(1))
    b_aug2 = (nb + 4 * U * (aug2 + nb) + TINY) * SECOND_ORDER
    y = np.concatenate([feat, soft, aug1, aug2[:, None]], 1)
    b = np.concatenate([b_feat, b_soft, b_aug1, b_aug2[:, None]], 1)
    return y, b, P


def forward(q, k, v, c0, c1, H):
    """-> y [n, (dim + 7) * H], bound (same shape), P [H, n, m]"""
    qh, kh, vh = (O.heads_of(np.asarray(t, np.float64), H) for t in (q, k, v))
    c0, c1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    scale = 1.0 / np.sqrt(qh.shape[2])
    res = [_head_forward(qh[h], kh[h], vh[h], c0, c1, scale) for h in range(H)]
    return O.interleave(np.stack([r[0] for r in res])), O.interleave(np.stack([r[1] for r in res])), np.stack([r[2] for r in res])


def train(q, k, v, c0, c1, dy, H):
    """-> dict of (value, bound) for y, dq, dk, dv (interleaved layouts) and P [H, n, m]"""
    qh, kh, vh = (O.heads_of(np.asarray(t, np.float64), H) for t in (q, k, v))
    c0, c1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    n, m, dim = qh.shape[1], kh.shape[1], qh.shape[2]
    gh = O.heads_of(np.asarray(dy, np.float64), H)           # [H, n, dim + 7]
    scale = 1.0 / np.sqrt(dim)
    aC = np.abs(c1)
    val = {key: [] for key in ("y", "P", "dq", "dk", "dv")}
    bnd = {key: [] for key in val}
    for h in range(H):
        Q, K, V = qh[h], kh[h], vh[h]
        G, g_s, g_a1, g_a2 = gh[h][:, :dim], gh[h][:, dim:dim + 3], gh[h][:, dim + 3:dim + 6], gh[h][:, dim + 6]
        y, by, P = _head_forward(Q, K, V, c0, c1, scale)
        _, _, _, eps = O.softmax_core(Q, K, scale)
        aug1, aug2 = y[:, dim + 3:dim + 6], y[:, dim + 6]
        b_aug1, b_aug2 = by[:, dim + 3:dim + 6], by[:, dim + 6]
        pos = aug2 > 0
        assert (b_aug2[pos] < aug2[pos] / 4).all(), "the first-order bound of aug1 / aug2 needs b(aug2) well below aug2"
        safe = np.where(pos, aug2, 1.0)
        r = np.where(pos[:, None], aug1 / safe[:, None], 0.0)
        b_r = np.where(pos[:, None], (b_aug1 + np.abs(r) * b_aug2[:, None]) / (safe - np.where(pos, b_aug2, 0.0))[:, None]
                       + 2 * U * np.abs(r), 1.0)
        gs = g_s + g_a1 + g_a2[:, None] * r
        b_gs = np.abs(g_a2)[:, None] * b_r + 3 * U * (np.abs(g_s) + np.abs(g_a1) + np.abs(g_a2[:, None] * r))
        aV, aG, aQ, aK = np.abs(V), np.abs(G), np.abs(Q), np.abs(K)
        dP_ = P * (eps + (P * eps).sum(1, keepdims=True) + (m + 3) * U) + 2 * TINY
        dV = P.T @ G
        dV_ = dP_.T @ aG + (n + 1) * U * (P.T @ aG)
        dPm = G @ V.T + gs @ c1.T
        ddP_ = (dim + 3) * U * (aG @ aV.T + np.abs(gs) @ aC.T) + b_gs @ aC.T
        D = (P * dPm).sum(1, keepdims=True)
        dD_ = (dP_ * np.abs(dPm) + P * ddP_).sum(1, keepdims=True) + (m + 1) * U * (P * np.abs(dPm)).sum(1, keepdims=True)
        dS = P * (dPm - D)
        ddS_ = dP_ * np.abs(dPm - D) + P * (ddP_ + dD_ + 2 * U * np.abs(dPm - D)) + TINY
        dQ = scale * (dS @ K)
        dQ_ = scale * (ddS_ @ aK + (m + 4) * U * (np.abs(dS) @ aK)) + TINY
        dK = scale * (dS.T @ Q)
        dK_ = scale * (ddS_.T @ aQ + (n + 4) * U * (np.abs(dS).T @ aQ)) + TINY
        for key, x, b in (("y", y, by), ("P", P, dP_ * SECOND_ORDER), ("dq", dQ, dQ_ * SECOND_ORDER), ("dk", dK, dK_ * SECOND_ORDER),
                          ("dv", dV, (dV_ + TINY) * SECOND_ORDER)):
            val[key].append(x)
            bnd[key].append(b)
    out = {"P": (np.stack(val["P"]), np.stack(bnd["P"]))}
    for key in ("y", "dq", "dk", "dv"):
        out[key] = (O.interleave(np.stack(val[key])), O.interleave(np.stack(bnd[key])))
    return out

"""Named inputs for the geometric cross attention ('cross_cat', apr_amd/csrc/attention_cat.hip), each with the edge it exists
for (tests/test_attention_cat_oracle_cpu.py confirms the planted facts from the oracle's own float64 values).  numpy only.

q, k, v and the designated rows are tests/attention_cases.build_softmax's (4 heads, interleaved channels): a designated row
(i, h) has a query whose scores are known in closed form.  On top of them:
* coordinates c0 [n, 3], c1 [m, 3]: multiples of 1 / 8 within +-80 (metres at KITTI's coarsest level), redrawn until
  aug2 = ||sum_j P_ij c1_j - c0_i|| >= 0.5 for every (i, h) -- except where a case plants a zero;
* one key (m = 1, every P = 1): soft == c1[0] exactly; the case sets c0[0] = c1[0], so aug1 and aug2 of query 0 are exactly
  0 in every head and the aug2 term of every gradient is 0 (`zero_rows`);
* `dominant` rows (score gaps of 112): soft == c1[m - 1];
* `tie2` cases copy key m - 1 into key m - 2 in every head: the `dominant` row of such a case (renamed `tie2`) sees an exact
  two-key tie 112 above everything else, soft is the midpoint of c1[m - 2] and c1[m - 1].
The last key (both tied keys of a `tie2` case) has z = 40, so the rows it dominates have a soft that is far from 0 in a known
column (a norm that takes one column too many is seen there).  dy [n, (dim + 7) * 4] is standard normal.

Kernel constants the shapes are built around: k_mha_cat_mfma owns 16 queries per workgroup (n = 15, 16, 17, 33: a short
block, a full one, a second block with one query, three blocks) and walks 16-key tiles with 4 waves (m = 15, 16, 17: the key
tile; 63, 64, 65: the 4-wave sweep and its first tail; 130: two sweeps and a tail); the training kernels take any dim.
"""
import numpy as np

import attention_cases as K
import attention_oracle as O

F32 = np.float32
H = 4
MIN_AUG2 = 0.5
PLANTED_Z = 40.0


def _grid_coords(rng, rows):
    return (np.rint(rng.uniform(-80, 80, (rows, 3)) * 8) / 8).astype(F32)


def build(name, fact, seed, n, m, dim, tie2=False):
    c = K.build_softmax(name, fact, seed, n, m, dim, H, family="cat")
    rng = np.random.default_rng(seed + 1000)
    k = c["k"].reshape(m, dim, H).copy()
    rows = [dict(r) for r in c["rows"]]
    if tie2:
        assert m >= 2
        k[m - 2] = k[m - 1]
        for r in rows:
            if r["kind"] == "dominant":
                r["kind"] = "tie2"
    c["k"] = np.ascontiguousarray(k.reshape(m, dim * H))
    c0, c1 = _grid_coords(rng, n), _grid_coords(rng, m)
    c1[max(m - 2, 0) if tie2 else m - 1:, 2] = PLANTED_Z
    qh, kh = O.heads_of(c["q"], H), O.heads_of(c["k"], H)
    scale = 1.0 / np.sqrt(dim)
    soft = np.stack([O.softmax_core(qh[h], kh[h], scale)[2] @ c1.astype(np.float64) for h in range(H)])      # [H, n, 3]
    for _ in range(50):
        near = (np.linalg.norm(soft - c0[None].astype(np.float64), axis=2) < MIN_AUG2).any(0)
        if not near.any():
            break
        c0[near] = _grid_coords(rng, int(near.sum()))
    else:
        raise AssertionError("could not draw coordinates with aug2 >= 0.5")
    zero_rows = []
    if m == 1:
        c0[0] = c1[0]
        zero_rows = [0]
    dy = rng.standard_normal((n, (dim + 7) * H)).astype(F32)
    c.update(c0=c0, c1=c1, dy=dy, rows=rows, zero_rows=zero_rows, tie2=tie2, H=H)
    return c


# name: (edge, seed, n, m, dim, tie2)
_CASES = {
    "cat-n1-m1":     ("one query, one key: P = 1, the planted zero; three waves see no tile", 301, 1, 1, 64, False),
    "cat-n17-m1":    ("one key, n = 17: a second block with one query; query 0 holds the planted zero", 302, 17, 1, 64, False),
    "cat-n15-m15":   ("a short query block, a short key tile", 303, 15, 15, 64, False),
    "cat-n16-m16":   ("exactly one query block and one key tile; two-key tie", 304, 16, 16, 64, True),
    "cat-n17-m17":   ("a last tile with one key, a last block with one query", 305, 17, 17, 64, False),
    "cat-n33-m63":   ("three query blocks; four tiles, one per wave, the last short", 306, 33, 63, 64, True),
    "cat-n16-m64":   ("four full tiles", 307, 16, 64, 64, False),
    "cat-n15-m65":   ("wave 0 takes a second tile with a single key: one rescale, one prefetch", 308, 15, 65, 64, True),
    "cat-n33-m130":  ("nine tiles: two sweeps and a tail of two keys", 309, 33, 130, 64, False),
    "cat-d1-n16-m16":   ("training kernels, dim 1: one channel per head", 310, 16, 16, 1, True),
    "cat-d1-n17-m65":   ("training kernels, dim 1; m = 65", 311, 17, 65, 1, False),
    "cat-d16-n15-m1":   ("training kernels, dim 16; one key, the planted zero", 312, 15, 1, 16, False),
    "cat-d16-n33-m130": ("training kernels, dim 16; n = 33, m = 130; two-key tie", 313, 33, 130, 16, True),
    "cat-d16-n1-m63":   ("training kernels, dim 16; one query, m = 63", 314, 1, 63, 16, False),
    "cat-d1-n33-m15":   ("training kernels, dim 1; m = 15, m = 17 and m = 64 below", 315, 33, 15, 1, False),
    "cat-d16-n16-m17":  ("training kernels, dim 16; m = 17", 316, 16, 17, 16, False),
    "cat-d16-n15-m64":  ("training kernels, dim 16; m = 64", 317, 15, 64, 16, True),
}
CASES = {name: build(name, s[0], *s[1:]) for name, s in _CASES.items()}
MFMA = {name: c for name, c in CASES.items() if c["dim"] == 64}

# dim 64 unless stated; `off`: q misaligned by that many floats
REFUSED = {
    "hm-dim32": dict(fn="headmajor", n=5, m=9, dim=32), "hm-misaligned": dict(fn="headmajor", n=5, m=9, dim=64, off=1),
    "hm-ldy": dict(fn="headmajor", n=5, m=9, dim=64, ldy=(64 + 7) * 4 - 1),
    "train-dim1025": dict(fn="train", n=2, m=3, dim=1025), "train-ldy": dict(fn="train", n=5, m=9, dim=16, ldy=(16 + 7) * 4 - 1),
}

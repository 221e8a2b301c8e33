"""Print the library's workspace sizes over a fixed list of arguments as one JSON table.

    python scripts/dump_scratch_sizes.py > table.json

Run on a build of the parent commit, the output is tests/golden/scratch_sizes_parent.json: tests/test_scratch_sizes_cpu.py
holds the current build against it.  The table maps a function name to a list of [arguments, bytes]; the two descriptor
sizes are tabulated over the row counts of one small descriptor each, apr_match_pose_batch_scratch_bytes under
apr_match_pose_set_lanes(1) and (3) (left at 1).  Host code only: no GPU is needed.
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# around the 256-byte edges of 1-, 4-, 8-, 16- and 32-byte elements, then cloud sizes
COUNTS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 28000, 140000]
FEW = [1, 65, 257, 28000, 140000]
MAX_ITER = [1, 1000, 1 << 20, (1 << 20) + 1, 4000000]


def _pairs():
    """(a, b): both counts together, then each against a fixed 257"""
    return [(n, n) for n in COUNTS] + [(n, 257) for n in COUNTS] + [(257, n) for n in COUNTS]


def argument_lists():
    one = [(n,) for n in COUNTS]
    geo_iter = [m for m in MAX_ITER if m <= 1 << 20]
    return {
        "apr_map_scratch_bytes": one,
        "apr_grid_subsample_scratch_bytes": one,
        "apr_voxel_down_sample_scratch_bytes": one,
        "apr_crop_scratch_bytes": one,
        "apr_irls_scratch_bytes": one,
        "apr_valid_pair_scratch_bytes": one,
        "apr_pairlist3_bytes": one,
        "apr_radius_scratch_bytes": _pairs(),
        "apr_nn3_scratch_bytes": _pairs(),
        "apr_reverse_table_scratch_bytes": [(n, h, ns) for n in COUNTS for h, ns in ((1, 257), (33, 28000))],
        "apr_icp_scratch_bytes": [(a, b, nb) for a, b in _pairs() for nb in (1, 3)],
        "apr_information_scratch_bytes": [(a, b, nb) for a, b in _pairs() for nb in (1, 3)],
        "apr_ransac_scratch_bytes": [(n, m) for n in COUNTS for m in MAX_ITER],
        "apr_ransac_geometric_scratch_bytes": [(n, n1, m) for n in COUNTS for n1 in (257, 28000) for m in geo_iter],
        "apr_ransac_pairs_geometric_scratch_bytes":
            [(1000, n1, n, m, v) for n in COUNTS for n1 in (257, 28000) for m, v in ((1000, 1000), (1 << 16, 500), (1, 1))],
        "apr_feature_nn_fast_scratch_bytes":
            [(a, b, c) for c in (32, 64, 128) for a, b in _pairs() + [(a, b) for a in FEW for b in FEW]],
        "apr_voxel_pyramid_scratch_bytes": [(n, s) for n in COUNTS for s in (1, 2, 12)],
        "apr_bn_stats_scratch_bytes": [(n, c) for n in COUNTS for c in (32, 256)],
        "apr_norm_backward_scratch_bytes": [(n, c) for n in COUNTS for c in (32, 256)],
        "apr_spconv_wgrad_scratch_bytes": [(n, 27, 64, 64) for n in COUNTS],
        "apr_dense_gemm_bf3_norm_scratch_bytes": [(n, 64, s) for n in COUNTS for s in (1, 3)],
        "apr_pairlist_bytes": [(n, k) for n in COUNTS for k in (1, 27)],
        "apr_spconv_os_pairs_bytes": [(n, 27, r) for n in COUNTS for r in (64, 128)],
        "apr_weighted_bce_scratch_bytes": [()],
    }


BATCH = [(b, n, n1, c, m) for b in (1, 3, 6) for n, n1 in ((1, 1), (257, 300), (28000, 28000), (140000, 28000))
         for c in (32, 33) for m in MAX_ITER]


def gcn_desc():
    from apr_amd import _lib
    d = _lib.GcnDesc()
    d.n_layers, d.c = 2, 256
    d.layer[0].kind, d.layer[0].k = 0, 10
    d.layer[1].kind, d.layer[1].heads = 1, 4
    for L in (d.layer[0], d.layer[1]):      # non-NULL stand-ins: only sized, never read
        L.w1 = L.w2 = L.w3 = L.wq = L.wk = L.wv = L.wm = 1
    return d


def kp_desc(n_in, n_out):
    from apr_amd import _lib
    d = _lib.KpResnetDesc()
    d.n_in, d.n_out, d.in_dim, d.mid, d.out_dim, d.strided = n_in, n_out, 128, 64, 256, int(n_in != n_out)
    d.H, d.n_kp, d.nseg = 32, 15, 2
    d.w_unary1 = d.w_shortcut = 1           # in_dim != mid, in_dim != out_dim
    return d


def table(lib):
    out = {}
    for name, args in argument_lists().items():
        out[name] = [[list(a), int(getattr(lib, name)(*a))] for a in args]
    g = gcn_desc()
    out["apr_gcn_scratch_bytes"] = [[[a, b], int(lib.apr_gcn_scratch_bytes(C.byref(g), a, b))] for a, b in _pairs()]
    out["apr_kp_resnet_scratch_bytes"] = [
        [[a, b], int(lib.apr_kp_resnet_scratch_bytes(C.byref(kp_desc(a, b))))] for a, b in _pairs()]
    for lanes in (3, 1):                    # left at 1
        assert lib.apr_match_pose_set_lanes(lanes) == 0
        out[f"apr_match_pose_batch_scratch_bytes@lanes={lanes}"] = [
            [list(a), int(lib.apr_match_pose_batch_scratch_bytes(*a))] for a in BATCH]
    return out


if __name__ == "__main__":
    from apr_amd import _lib
    json.dump(table(_lib.load()), sys.stdout, separators=(",", ":"), sort_keys=True)
    print()

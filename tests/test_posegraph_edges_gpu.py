"""apr_posegraph_optimize held to tests/posegraph_oracle.py step by step at its edges: every named graph of
tests/posegraph_cases.py (tests/test_posegraph_cases_cpu.py holds the facts they claim and shows that each rule of the
optimiser, once broken, is rejected at this very bar) with statuses, iteration counts and kept flags exact and every other
output within posegraph_cases.BAR; graphs of status 1 to 4 between graphs that optimise, with what DESIGN section 19.2 says
is and is not written; the transform stride; and the open3d-shaped entry."""
import functools

import numpy as np
import pytest
import torch

from tests import posegraph_cases as C
from tests import posegraph_oracle as PG

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7


def _graph_of(name):
    c = C.cases()[name]
    ne = len(c["edges"])
    return dict(n=c["n"], rows=[(e.s, e.t, int(e.uncertain)) for e in c["edges"]],
                T=np.stack([e.T for e in c["edges"]]) if ne else np.zeros((0, 4, 4)),
                info=np.stack([e.info for e in c["edges"]]) if ne else np.zeros((0, 6, 6)), init=c["init"])


def _malformed(name):
    m = C.MALFORMED[name]
    ne = len(m["rows"])
    return dict(n=m["n"], rows=m["rows"], T=np.tile(np.eye(4), (ne, 1, 1)), info=np.tile(100.0 * np.eye(6), (ne, 1, 1)),
                init=np.tile(np.eye(4), (m["n"], 1, 1)))


def _launch(dev, graphs, options=C.DEFAULTS, with_init=False, t_form="4x4"):
    """One apr_posegraph_optimize call on tensors allocated here and pre-filled with a sentinel (ops.posegraph_optimize's own
    argument order; its layout class refuses the malformed graphs this file needs).  `t_form`: the transforms as [ne,4,4],
    as 20-double records the way apr_icp_batch leaves them, or as rows of 12 doubles.
    -> per graph dict(poses [n,4,4], confidence, kept, iterations, status), all numpy."""
    from apr_amd import ops
    node_off = np.concatenate([[0], np.cumsum([g["n"] for g in graphs])]).astype(np.int32)
    edge_off = np.concatenate([[0], np.cumsum([len(g["rows"]) for g in graphs])]).astype(np.int32)
    rows = np.array([r for g in graphs for r in g["rows"]], dtype=np.int32).reshape(-1, 3)
    T = np.concatenate([g["T"] for g in graphs]).reshape(-1, 16)
    if t_form == "record":
        T = np.concatenate([T, np.full((len(T), 4), np.nan)], 1)
    elif t_form == "rows12":
        T = T[:, :12]
    info = np.concatenate([g["info"] for g in graphs]).reshape(-1, 36)
    nn, ne, ng = int(node_off[-1]), int(edge_off[-1]), len(graphs)
    assert len(rows) == ne and len(T) == ne and ne >= 1

    def gpu(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_no, d_eo, d_rows, d_T, d_info = gpu(node_off), gpu(edge_off), gpu(rows), gpu(T), gpu(info)
    d_init = gpu(np.concatenate([g["init"] for g in graphs]).reshape(nn, 16)) if with_init else None
    poses = torch.full((nn, 4, 4), SENTINEL, dtype=torch.float64, device=dev)
    conf = torch.full((ne,), SENTINEL, dtype=torch.float64, device=dev)
    kept = torch.full((ne,), ISENTINEL, dtype=torch.int32, device=dev)
    iters = torch.full((ng, 2), ISENTINEL, dtype=torch.int32, device=dev)
    status = torch.full((ng,), ISENTINEL, dtype=torch.int32, device=dev)
    ops.check(ops._lib_().apr_posegraph_optimize(
        ops.ptr(d_no), ops.ptr(d_eo), ng, ops.ptr(d_rows), ops.ptr(d_T), int(T.shape[1]), ops.ptr(d_info), ops.ptr(d_init),
        float(options["mcd"]), float(options["edge_prune_threshold"]), float(options["preference_loop_closure"]),
        ops.ptr(poses), ops.ptr(conf), ops.ptr(kept), ops.ptr(iters), ops.ptr(status), ops.stream()))
    torch.cuda.synchronize()
    poses, conf, kept, iters, status = [x.cpu().numpy() for x in (poses, conf, kept, iters, status)]
    return [dict(poses=poses[node_off[g]:node_off[g + 1]], confidence=conf[edge_off[g]:edge_off[g + 1]],
                 kept=kept[edge_off[g]:edge_off[g + 1]], iterations=iters[g], status=status[g]) for g in range(ng)]


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("poses", "confidence", "kept", "iterations", "status"))


def _as_result(out):
    return C.result_of(out["poses"], out["confidence"], out["kept"], out["iterations"], out["status"])


def _launch_groups():
    """Options are per call, and so is the choice between initial poses handed in and the chain built by the kernel."""
    out = []
    for options, names in C.option_groups():
        for with_init in (False, True):
            part = [n for n in names if (C.cases()[n]["init"] is not None) == with_init and len(C.cases()[n]["edges"])]
            single = [n for n in names if not len(C.cases()[n]["edges"]) and (C.cases()[n]["init"] is not None) == with_init]
            if part:
                out.append((options, with_init, part[:1] + single + part[1:]))      # the edgeless graph sits inside the batch
    return out


def test_every_case_in_batched_launches_against_the_oracle(dev):
    worst, seen = {}, set()
    for options, with_init, names in _launch_groups():
        graphs = [_graph_of(n) for n in names]
        batch = _launch(dev, graphs, options, with_init)
        again = _launch(dev, graphs, options, with_init)
        for name, g, out, out2 in zip(names, graphs, batch, again):
            want = C.oracle(name)
            exact, dc, dp = C.difference(_as_result(out), want)
            print(f"{name}: status {out['status']}, iterations {tuple(int(v) for v in out['iterations'])}, kept {int((out['kept'] != 0).sum())}"
                  f" of {len(out['kept'])}; mismatch {exact}; confidence {dc:.2e}, relative poses {dp:.2e}")
            worst[name] = max(dc, dp)
            seen.add(name)
        for name, g, out, out2 in zip(names, graphs, batch, again):
            C.compare(_as_result(out), C.oracle(name), C.BAR)
            assert np.isfinite(out["poses"]).all(), name
            assert set(np.unique(out["kept"])) <= {0, 1}, name             # written, not the sentinel read as "kept"
            assert _same_bits(out, out2), f"{name}: run to run"
            if len(g["rows"]):
                assert _same_bits(out, _launch(dev, [g], options, with_init)[0]), f"{name}: alone"
    assert seen == set(C.cases())
    top = max(worst.values())
    print(f"worst difference over all cases {top:.2e}; BAR {C.BAR:.0e} = {C.BAR / max(top, 1e-300):.0f} x")
    # the edgeless graph: the identity, or the pose handed in, bit for bit
    for with_init, name in ((False, "status_1_single_node"), (True, "status_1_single_node_init")):
        g = _graph_of(name)
        out = _launch(dev, [_graph_of("odd_sizes_3") if not with_init else _graph_of("no_chain_with_init"), g], C.DEFAULTS, with_init)[1]
        assert out["status"] == 1 and tuple(out["iterations"]) == (0, 0)
        assert np.array_equal(out["poses"][0], g["init"][0] if with_init else np.eye(4))


@functools.lru_cache(maxsize=None)
def _zero_information():
    edges = PG.synthetic_graph(4, 30)[0]
    return dict(n=4, rows=[(e.s, e.t, int(e.uncertain)) for e in edges], T=np.stack([e.T for e in edges]),
                info=np.zeros((len(edges), 6, 6)), init=None), np.stack(PG.odometry_chain(4, edges))


def test_graphs_of_status_1_to_4_between_graphs_that_optimise(dev):
    """What DESIGN section 19.2 says is and is not written, and neighbours that do not notice."""
    a, b = _graph_of("odd_sizes_3"), _graph_of("odd_sizes_5")
    clean = _launch(dev, [a, b])
    for k, name in ((0, "odd_sizes_3"), (1, "odd_sizes_5")):
        C.compare(_as_result(clean[k]), C.oracle(name), C.BAR)

    def middle(g):
        out = _launch(dev, [a, g, b])
        assert _same_bits(out[0], clean[0]) and _same_bits(out[2], clean[1])
        return out[1]

    # status 1: the initial poses, confidence 1, kept 1, iterations (0, 0)
    zero, chain = _zero_information()
    out = middle(zero)
    assert out["status"] == 1 and tuple(out["iterations"]) == (0, 0)
    assert (out["confidence"] == 1.0).all() and (out["kept"] == 1).all()
    assert np.abs(out["poses"] - chain).max() <= 1e-12
    out = middle(_graph_of("status_1_single_node"))
    assert out["status"] == 1 and tuple(out["iterations"]) == (0, 0) and np.array_equal(out["poses"][0], np.eye(4))
    # status 2: first-pass poses, first-pass confidences and flags, iterations (k, 0)
    out, want = middle(_graph_of("status_2")), C.oracle("status_2")
    assert out["status"] == 2 and tuple(out["iterations"]) == (want["iterations"][0], 0) and want["iterations"][0] > 0
    C.compare(_as_result(out), want, C.BAR)
    assert (out["kept"] != 0).sum() == 2 and set(np.unique(out["kept"])) <= {0, 1}
    # status 3: the poses of the last accepted step, everything finite
    for name in ("status_3", "status_3_after_a_step", "status_3_mid_pass", "general_lambda_asymmetric"):
        if name not in C.cases():
            continue
        out, want = middle(_graph_of(name)), C.oracle(name)
        assert out["status"] == 3
        C.compare(_as_result(out), want, C.BAR)
        assert np.isfinite(out["poses"]).all() and np.isfinite(out["confidence"]).all() and set(np.unique(out["kept"])) <= {0, 1}
    chain = np.stack(PG.odometry_chain(3, C.cases()["status_3"]["edges"]))
    assert np.abs(middle(_graph_of("status_3"))["poses"] - chain).max() <= 1e-12
    # status 4: nothing of the graph is touched beyond its status and iterations = (0, 0)
    for name in C.MALFORMED:
        out = middle(_malformed(name))
        assert out["status"] == 4 and tuple(out["iterations"]) == (0, 0), name
        assert (out["poses"] == SENTINEL).all() and (out["confidence"] == SENTINEL).all() and (out["kept"] == ISENTINEL).all(), name
    # with initial poses the chain is not needed: the same rows optimise
    g = _malformed("missing_chain_edge")
    out = _launch(dev, [_graph_of("no_chain_with_init"), g, _graph_of("sparse_shuffled_6_init")], with_init=True)[1]
    assert out["status"] == 0 and (out["poses"] != SENTINEL).all()


def test_transform_stride(dev):
    """T as [ne, 4, 4], as 20-double ICP records (the four doubles behind the matrix are NaN here) and as rows of 12."""
    for options, with_init, names in _launch_groups()[:2]:
        graphs = [_graph_of(n) for n in names]
        ref = _launch(dev, graphs, options, with_init, "4x4")
        for form in ("record", "rows12"):
            for name, x, y in zip(names, ref, _launch(dev, graphs, options, with_init, form)):
                assert _same_bits(x, y), (name, form)


@pytest.mark.parametrize("name", ["sparse_shuffled_6_init", "status_2"])
def test_registration_global_optimization_agrees_with_the_raw_call(dev, name):
    from apr_amd.fcgf import registration as R
    c, g = C.cases()[name], dict(_graph_of(name))
    if g["init"] is None:
        g["init"] = np.stack(PG.odometry_chain(c["n"], c["edges"]))
    raw = _launch(dev, [g], c["options"], True)[0]
    pg = R.PoseGraph()
    pg.nodes = [R.PoseGraphNode(p) for p in g["init"]]
    pg.edges = [R.PoseGraphEdge(e.s, e.t, e.T, e.info, uncertain=e.uncertain) for e in c["edges"]]
    res = R.global_optimization(pg, R.GlobalOptimizationLevenbergMarquardt(), R.GlobalOptimizationConvergenceCriteria(),
                                R.GlobalOptimizationOption(max_correspondence_distance=c["options"]["mcd"],
                                                           edge_prune_threshold=c["options"]["edge_prune_threshold"],
                                                           preference_loop_closure=c["options"]["preference_loop_closure"],
                                                           reference_node=0))
    assert res == dict(iterations=tuple(int(v) for v in raw["iterations"]), status=int(raw["status"]))
    assert res["status"] == c["facts"]["status"]
    assert np.array_equal(np.stack([nd.pose for nd in pg.nodes]), raw["poses"])
    kept = raw["kept"] != 0
    assert [(e.source_node_id, e.target_node_id) for e in pg.edges] == [(e.s, e.t) for e, k in zip(c["edges"], kept) if k]
    assert [e.confidence for e in pg.edges] == [float(x) for x, k in zip(raw["confidence"], kept) if k]
    C.compare(C.result_of(raw["poses"], raw["confidence"], raw["kept"], raw["iterations"], raw["status"]),
              PG.global_optimization(c["n"], c["edges"], c["options"]["mcd"], g["init"]), C.BAR)

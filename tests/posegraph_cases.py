"""Named pose graphs for the optimiser of csrc/posegraph.hip, each with the facts it exists for, and the one comparator the
CPU and the GPU tests share.  tests/test_posegraph_cases_cpu.py asserts every fact from the oracle's result and trace, so a
case that stops hitting its edge fails there and not on the GPU.  numpy only.

A case is dict(n, edges [PG.Edge], init [n,4,4] or None, options, facts).  `options` are the keyword arguments of
PG.global_optimization after `edges` (mcd, edge_prune_threshold, preference_loop_closure); cases with equal options share
one launch on the GPU.  Seeds that a fact depends on were searched on the CPU once and are fixed here.

Facts (all optional but status): status, iterations (first, second pass), kept (number of edges kept), rejected (rejected
steps, both passes), reject_then_accept, consecutive_rejections, unclamped_scale, second_pass_longer, several_pruned,
unsymmetric, accepted_in_the_failing_pass,
denominator_matters_early (the + 1e-3 of rho's denominator moves a scale factor before the last step of a pass), scrambled,
accepted_before_failure, alternate_vec (the place where vec takes its sy < 1e-6 branch), layout_refuses_without_init."""
import functools
import math

import numpy as np

from tests import icp_oracle as O
from tests import posegraph_oracle as PG

# 1000 x the worst difference of the kernel from the oracle measured on the MI355X over every case below, rounded up to a
# power of ten (DESIGN section 19.2 has the per-case figures).  The mutant test of the CPU suite runs at the same constant.
BAR = 1e-9

DEFAULTS = dict(mcd=PG.MCD_FINE, edge_prune_threshold=PG.PRUNE, preference_loop_closure=PG.PREFERENCE)


# ---- the comparator ----
def result_of(poses, confidence, kept, iterations, status):
    return dict(poses=[np.asarray(p, dtype=np.float64) for p in poses], confidence=np.asarray(confidence, dtype=np.float64),
                kept=np.asarray(kept) != 0, iterations=tuple(int(i) for i in iterations), status=int(status))


def difference(got, want):
    """-> (the first exact mismatch as text or None, worst confidence difference, worst entry difference of any P_0^-1 P_i
    divided by max(1, |t_i|)).  Entry by entry: an angle taken through arccos cannot resolve rotations below 2e-6 degrees."""
    for key in ("status", "iterations"):
        if tuple(np.atleast_1d(got[key])) != tuple(np.atleast_1d(want[key])):
            return f"{key}: {got[key]} != {want[key]}", math.inf, math.inf
    if not np.array_equal(np.asarray(got["kept"]) != 0, np.asarray(want["kept"]) != 0):
        return f"kept: {np.asarray(got['kept']).astype(int)} != {np.asarray(want['kept']).astype(int)}", math.inf, math.inf
    dc = float(np.abs(np.asarray(got["confidence"]) - np.asarray(want["confidence"])).max()) if len(want["confidence"]) else 0.0
    dp = 0.0
    for a, b in zip(PG.relative_poses(list(got["poses"])), PG.relative_poses(list(want["poses"]))):
        d = float(np.abs(a - b).max()) / max(1.0, float(np.linalg.norm(b[:3, 3])))
        dp = max(dp, d if np.isfinite(d) else math.inf)
    return None, (dc if np.isfinite(dc) else math.inf), dp


def compare(got, want, bar):
    """Status, both iteration counts and the kept flags equal; max |confidence difference| <= bar; every entry of every
    P_0^-1 P_i within bar * max(1, |t_i|).  -> the worst of the two differences; AssertionError otherwise."""
    exact, dc, dp = difference(got, want)
    assert exact is None, exact
    assert dc <= bar, f"confidence differs by {dc:.3e} > {bar:.1e}"
    assert dp <= bar, f"a relative pose differs by {dp:.3e} x max(1, |t|) > {bar:.1e}"
    return max(dc, dp)


# ---- builders ----
def _case(n, edges, init=None, facts=None, **options):
    return dict(n=n, edges=list(edges), init=None if init is None else np.stack(init), options={**DEFAULTS, **options},
                facts=dict(facts or {}))


def far_start(n, seed, **facts):
    """The odometry chain of synthetic_graph(n, 20 + n), every node moved by 2 m and 35 degrees of its own."""
    edges = PG.synthetic_graph(n, 20 + n)[0]
    init = [O.perturbation(2.0, 35.0, seed * 10 + i) @ p for i, p in enumerate(PG.odometry_chain(n, edges))]
    return _case(n, edges, init, facts)


# There is no lm_cap case.  Leaving the inner loop through count > 20 takes 21 rejections in a row; they multiply lambda by
# 2^(1 + 2 + ... + 21) = 2^231, delta = (H + lambda I)^-1 b shrinks by as much, and the criterion
# ||delta|| < 1e-6 (||x|| + 1e-6) ends the pass first: the longest inner loop of any case below runs 7 solves.
# A CPU search over the chains of synthetic_graph(n, 20 + n), n = 3, 4, 5, thrown 5 m .. 1000 km and 60 .. 179 degrees off,
# 24 seeds each (864 graphs), found no pass that reaches its 21st solve.
LM_CAP = None


def near_minimum(n, **facts):
    """n = 3, 5, 7 near the minimum like the n = 4, 6, 8 of the batch test; the loop edge (0, n - 1) planted for n >= 5."""
    return _case(n, PG.synthetic_graph(n, 10 + n, planted=True)[0], None, facts)


def sparse_shuffled(n, with_init, **facts):
    """The chain and three loop closures of synthetic_graph(n, 40 + n, planted=False) in a fixed random order."""
    full = PG.synthetic_graph(n, 40 + n, planted=False)[0]
    want = {(j, j + 1) for j in range(n - 1)} | {(0, 2), (1, n - 2), (0, n - 1)}
    edges = [e for e in full if (e.s, e.t) in want]
    order = np.random.default_rng(SHUFFLE_SEED[n]).permutation(len(edges))
    edges = [edges[i] for i in order]
    return _case(n, edges, PG.odometry_chain(n, edges) if with_init else None, facts)


SHUFFLE_SEED = {6: 0, 8: 2}       # the first seeds whose order passes chain_order_is_scrambled


def chain_order_is_scrambled(edges):
    """The first edge is no chain edge, and no chain edge (j, j + 1) is directly followed by (j + 1, j + 2)."""
    pairs = [(e.s, e.t) for e in edges]
    if pairs[0][1] == pairs[0][0] + 1:
        return False
    return not any(a[1] == a[0] + 1 and b == (a[1], a[1] + 1) for a, b in zip(pairs, pairs[1:]))


def no_chain_with_init(**facts):
    """n = 4, edges (0, 2), (0, 3), (1, 3), all uncertain; the start is the chain of the complete graph they came from."""
    full = PG.synthetic_graph(4, 33, planted=False)[0]
    edges = [PG.Edge(e.s, e.t, e.T, e.info, True) for e in full if (e.s, e.t) in ((0, 2), (0, 3), (1, 3))]
    return _case(4, edges, PG.odometry_chain(4, full), facts)


def isolated_after_prune(**facts):
    """n = 4: chain (0, 1), (1, 2) and the loop (0, 2); node 3 hangs by (0, 3) and (1, 3) alone, both uncertain and planted
    wrong in different directions, so both are pruned and the second pass holds node 3 by the damping alone."""
    full = PG.synthetic_graph(4, 34, planted=False)[0]
    edges = []
    for e in full:
        if (e.s, e.t) == (2, 3):
            continue
        T = O.perturbation(5.0, 40.0, 50 + e.s) @ e.T if e.t == 3 else e.T
        edges.append(PG.Edge(e.s, e.t, T, e.info, e.uncertain or e.t == 3))
    return _case(4, edges, PG.odometry_chain(4, full), facts)


GIMBAL_R = PG.mat((0.3, math.pi / 2, 0.0, 1.0, 2.0, 3.0))


def gimbal_node(**facts):
    """init = R chain with hypot(R00, R10) = 6e-17: vec(P_0) takes its other branch when x is first formed."""
    edges = PG.synthetic_graph(4, 14)[0]
    return _case(4, edges, [GIMBAL_R @ p for p in PG.odometry_chain(4, edges)], facts)


GIMBAL_EDGE_ALPHA = 3.0


def gimbal_edge(**facts):
    """The loop edge (0, 2) is off by exactly 90 degrees of pitch (and 3 radians of roll) from P_t^-1 P_s at the start: its
    error vec(T^-1 P_t^-1 P_s) = vec(mat(3, pi/2, 0, ...)) takes the other branch at the first evaluation.  Any step leaves
    the branch, and beyond it alpha - gamma = 3 splits between the two angles as the step's direction decides, so the yaw
    row and column of this edge's Lambda are scaled by 0.1: the residual then falls for nearly every split, steps are
    accepted, and an alternate branch that hands back another vector changes the run."""
    edges = PG.synthetic_graph(4, 14, planted=False)[0]
    P = PG.odometry_chain(4, edges)
    Z = PG.mat((GIMBAL_EDGE_ALPHA, math.pi / 2, 0.0, 0.3, -0.2, 0.1))
    D = np.diag([1.0, 1.0, 0.1, 1.0, 1.0, 1.0])
    out = []
    for e in edges:
        if (e.s, e.t) == (0, 2):
            out.append(PG.Edge(e.s, e.t, np.linalg.inv(P[e.t]) @ P[e.s] @ np.linalg.inv(Z), D @ e.info @ D, e.uncertain))
        else:
            out.append(e)
    return _case(4, out, P, facts)


def weak_information(**facts):
    """far_start_5 with every Lambda scaled by 1e-4 (clouds of a point or two): cur - new and delta (lambda delta + b) come
    down to the order of the 1e-3 in rho's denominator while the run is still far from its end, so the term decides scale
    factors that later steps build on."""
    c = far_start(5, 1)
    return _case(5, [PG.Edge(e.s, e.t, e.T, e.info * 1e-4, e.uncertain) for e in c["edges"]], c["init"], facts)


def _general_lambda_edges(graph_seed, rng):
    edges = []
    for e in PG.synthetic_graph(4, graph_seed)[0]:
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        L = Q @ np.diag(10.0 ** rng.uniform(0.0, 4.0, size=6)) @ Q.T
        edges.append(PG.Edge(e.s, e.t, e.T, (L + L.T) / 2, e.uncertain))
    return edges


def _with_skew(edges, relative, seed, only=None):
    """Every Lambda (or that of edge `only`) plus a skew matrix of largest entry relative * max |Lambda|: e^T Lambda e is
    unchanged, Lambda e and Js^T Lambda Js are not, and Lambda^T gives another b and another H."""
    rng, out = np.random.default_rng(seed), []
    for e in edges:
        S = rng.normal(size=(6, 6))
        S = S - S.T
        k = relative if only is None or (e.s, e.t) == only else 0.0
        out.append(PG.Edge(e.s, e.t, e.T, e.info + k * np.abs(e.info).max() * S / np.abs(S).max(), e.uncertain))
    return out


def general_lambda(skew=None, only=None, skew_seed=62, **facts):
    """n = 4, Lambda_e = Q diag(10^U[0, 4]) Q^T: Lambda(3,3) != Lambda(5,5) and no sum G^T G shape.  `skew` (relative to
    max |Lambda|) makes Lambda unsymmetric.  The lower triangle of H + lambda I, which is all the factorisation reads, then
    loses the gauge null space that the damping alone holds up, by about skew * |H|:
      3e-8 stays below the damping to the end: status 0, and Lambda read transposed moves P_0^-1 P_i by 4e-9, above BAR;
      2e-5 on edge (0, 1) alone passes one solve and fails the second, after an accepted step of the same pass: status 3
        with the poses, confidences and flags of that step;
      a largest entry of 5 (absolute) fails the first solve: status 3 with everything as it came in."""
    edges = _general_lambda_edges(35, np.random.default_rng(61))
    if skew == "gross":
        rng, out = np.random.default_rng(61), []
        for e in _general_lambda_edges(35, rng):               # the draws that follow the six Lambdas of this stream
            S = rng.normal(size=(6, 6))
            out.append(PG.Edge(e.s, e.t, e.T, e.info + 5.0 * (S - S.T) / np.abs(S - S.T).max(), e.uncertain))
        edges = out
    elif skew is not None:
        edges = _with_skew(edges, skew, skew_seed, only)
    return _case(4, edges, None, facts)


def transposed(case):
    """The same case with every Lambda transposed: what a kernel reading info[6 j + i] for Lambda(i, j) would optimise."""
    return {**case, "edges": [PG.Edge(e.s, e.t, e.T, e.info.T, e.uncertain) for e in case["edges"]]}


def second_pass_mu(**facts):
    """n = 4, general Lambda, every node 0.5 m and 8 degrees off, and the Lambda of the planted edge (0, 3) scaled by 100:
    the edge is pruned, so mu of the second pass (mean Lambda(5,5) over the kept edges) is a fraction of the first's; two
    uncertain edges stay, and the second pass accepts two steps, so the confidences it recomputes from mu shape a later
    step.  A second pass of 2 iterations cannot show mu: the confidences of its one accepted step are used by no solve
    whose step is taken."""
    edges = _general_lambda_edges(24, np.random.default_rng(102))
    edges = [PG.Edge(e.s, e.t, e.T, e.info * (100.0 if (e.s, e.t) == (0, 3) else 1.0), e.uncertain) for e in edges]
    init = [O.perturbation(0.5, 8.0, 20 + i) @ p for i, p in enumerate(PG.odometry_chain(4, edges))]
    return _case(4, edges, init, facts)


def options_case(facts, **options):
    """The planted n = 6 graph of the batch test under other options."""
    return _case(6, PG.synthetic_graph(6, 16, planted=True)[0], None, facts, **options)


def single_node(with_init, **facts):
    return _case(1, [], [O.perturbation(0.7, 20.0, 3)] if with_init else None, facts)


def _status_graph():
    return PG.synthetic_graph(3, 31, planted=False)[0]


def status_2(**facts):
    """The chain edges carry no weight in Lambda(5,5) and the loop edge is pruned: mu = 0 for the second pass."""
    edges = []
    for e in _status_graph():
        L, T = e.info.copy(), e.T
        if e.t == e.s + 1:
            L[5, :] = 0.0
            L[:, 5] = 0.0
        else:
            T = O.perturbation(1.5, 12.0, 5) @ T
        edges.append(PG.Edge(e.s, e.t, T, L, e.uncertain))
    return _case(3, edges, None, facts)


def status_3_first_solve(**facts):
    L = np.diag([-1e6, -1e6, -1e6, 1.0, 1.0, 1.0])
    return _case(3, [PG.Edge(e.s, e.t, e.T, L, e.uncertain) for e in _status_graph()], None, facts)


STATUS_3_LATE_SCALE = 475000.0  # searched over 2e5 .. 5e5 in steps of 5e3: below, no solve fails; above, the first one does


def status_3_after_a_step(**facts):
    """Lambda positive definite on the chain edges, indefinite on the loop edge only, scaled so that the oracle accepts at
    least one step before a solve fails."""
    L = np.diag([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]) * STATUS_3_LATE_SCALE
    edges = [PG.Edge(e.s, e.t, e.T, L if e.uncertain else e.info, e.uncertain) for e in _status_graph()]
    return _case(3, edges, None, facts)


# ---- malformed graphs: raw (n, [(source, target, uncertain)]) rows; the kernel answers status 4 before it reads through an
# index, ops.PoseGraphLayout refuses them on the host.  `chain`: refused only where the chain is needed (init = NULL) ----
MALFORMED = {
    "source_not_below_target": dict(n=3, rows=[(0, 1, 0), (2, 1, 0), (0, 2, 1)], chain=False),
    "source_equals_target": dict(n=3, rows=[(0, 1, 0), (1, 1, 0), (0, 2, 1)], chain=False),
    "target_beyond_n": dict(n=3, rows=[(0, 1, 0), (1, 3, 0), (0, 2, 1)], chain=False),
    "negative_index": dict(n=3, rows=[(0, 1, 0), (-1, 2, 0), (0, 2, 1)], chain=False),
    "nine_nodes": dict(n=9, rows=[(j, j + 1, 0) for j in range(8)], chain=False),
    "missing_chain_edge": dict(n=3, rows=[(0, 1, 0), (0, 2, 1)], chain=True),
}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Built once."""
    c = {}
    c["far_start_3"] = far_start(3, 1, status=0, iterations=(13, 1), rejected=6, reject_then_accept=True,
                                 consecutive_rejections=True)
    c["far_start_5"] = far_start(5, 1, status=0, iterations=(5, 12), rejected=20, kept=4, second_pass_longer=True,
                                 several_pruned=True, reject_then_accept=True, consecutive_rejections=True)
    c["far_start_7"] = far_start(7, 2, status=0, unclamped_scale=True)
    c["far_start_8"] = far_start(8, 2, status=0, unclamped_scale=True)
    for n in (3, 5, 7):
        c[f"odd_sizes_{n}"] = near_minimum(n, status=0, kept=n * (n - 1) // 2 - (n >= 5))
    for n in (6, 8):
        c[f"sparse_shuffled_{n}"] = sparse_shuffled(n, False, status=0, scrambled=True, kept=n + 2)
        c[f"sparse_shuffled_{n}_init"] = sparse_shuffled(n, True, status=0, scrambled=True, kept=n + 2)
    c["no_chain_with_init"] = no_chain_with_init(status=0, layout_refuses_without_init=True)
    c["isolated_after_prune"] = isolated_after_prune(status=0, kept=3)
    c["gimbal_node"] = gimbal_node(status=0, iterations=(5, 1), alternate_vec="node 0 at the start")
    c["gimbal_edge"] = gimbal_edge(status=0, iterations=(7, 1), kept=5, rejected=0, alternate_vec="edge (0, 2) at the start")
    c["weak_information"] = weak_information(status=0, iterations=(5, 11), denominator_matters_early=True)
    c["general_lambda"] = general_lambda(status=0, iterations=(7, 2), kept=5)
    c["general_lambda_skewed"] = general_lambda(3e-8, status=0, iterations=(7, 2), kept=5, unsymmetric=True)
    c["general_lambda_asymmetric"] = general_lambda("gross", status=3, iterations=(1, 0), kept=6, unsymmetric=True)
    c["status_3_mid_pass"] = general_lambda(2e-5, (0, 1), 68, status=3, iterations=(2, 0), kept=3, unsymmetric=True,
                                            accepted_in_the_failing_pass=True)
    c["second_pass_mu"] = second_pass_mu(status=0, iterations=(8, 3), kept=5, second_pass_longer=True)
    c["options_prune_0"] = options_case(dict(status=0, iterations=(5, 1), kept=15), edge_prune_threshold=0.0)
    c["options_prune_1"] = options_case(dict(status=0, iterations=(5, 2), kept=5), edge_prune_threshold=1.0)
    c["options_preference_0.1"] = options_case(dict(status=0, iterations=(6, 1), kept=14), preference_loop_closure=0.1)
    c["options_preference_10"] = options_case(dict(status=0, iterations=(5, 2), kept=14), preference_loop_closure=10.0)
    c["options_mcd_0.03"] = options_case(dict(status=0, iterations=(6, 1), kept=14), mcd=0.03)
    c["options_mcd_0.5"] = options_case(dict(status=0, iterations=(5, 2), kept=14), mcd=0.5)
    c["status_1_single_node"] = single_node(False, status=1, iterations=(0, 0))
    c["status_1_single_node_init"] = single_node(True, status=1, iterations=(0, 0))
    c["status_2"] = status_2(status=2, iterations=(4, 0), kept=2)
    c["status_3"] = status_3_first_solve(status=3, iterations=(1, 0), kept=3)
    if STATUS_3_LATE_SCALE is not None:
        c["status_3_after_a_step"] = status_3_after_a_step(status=3, iterations=(1, 1), accepted_before_failure=True)
    return c


@functools.lru_cache(maxsize=None)
def oracle(name):
    c = cases()[name]
    o = c["options"]
    return PG.global_optimization(c["n"], c["edges"], o["mcd"], c["init"], o["edge_prune_threshold"],
                                  o["preference_loop_closure"])


def option_groups():
    """Cases that share options share a launch: -> [(options, [names])], the default group first."""
    groups = {}
    for name, c in cases().items():
        groups.setdefault(tuple(sorted(c["options"].items())), []).append(name)
    return [(dict(k), v) for k, v in groups.items()]


# ---- what a trace shows ----
def _scale(rho):
    return 1.0 - (2.0 * rho - 1.0) ** 3


def trace_facts(res):
    """The facts of a result's trace: rejected steps, reject-then-accept, consecutive rejections, unclamped scale factors,
    steps where the +1e-3 of rho's denominator moves the clamped factor by more than 1e-3 relative, inner loops left
    through count > 20, failed solves and the accepted steps before the first of them."""
    f = dict(rejected=0, reject_then_accept=False, consecutive_rejections=False, unclamped_scale=False,
             denominator_matters=False, lm_cap=False, failed=False, accepted_before_failure=0, accepted_in_the_failing_pass=0)
    for tr in res["trace"]["passes"]:
        prev = None
        for s in tr["steps"]:
            if s["failed"]:
                f["failed"] = True
                f["accepted_in_the_failing_pass"] = sum(1 for x in tr["steps"] if x["accepted"])
                continue
            if s["rho"] is None:
                prev = None
                continue
            if not s["accepted"]:
                f["rejected"] += 1
                f["consecutive_rejections"] |= prev is False and s["count"] > 0
                f["lm_cap"] |= s["count"] == PG.MAX_ITERATION_LM
            else:
                if not f["failed"]:
                    f["accepted_before_failure"] += 1
                f["reject_then_accept"] |= prev is False and s["count"] > 0
                k = _scale(s["rho"])
                f["unclamped_scale"] |= 1.0 / 3.0 < k < 2.0 / 3.0
                clamp = lambda v: max(1.0 / 3.0, min(v, 2.0 / 3.0))
                k0 = clamp(_scale((s["cur"] - s["new"]) / s["den"]))
                f["denominator_matters"] |= abs(clamp(k) - k0) > 1e-3 * clamp(k)
            prev = s["accepted"]
    return f


def smallest_margin(res):
    """The smallest relative gap |lhs - rhs| / max(|lhs|, |rhs|) over every recorded comparison (|rho| itself against 0),
    and the comparison that has it.  The prune comparisons are held by bands of their own (prune_is_clear)."""
    worst, where = math.inf, None
    for p, tr in enumerate(res["trace"]["passes"]):
        for name, it, count, lhs, rhs in tr["decisions"]:
            gap = abs(lhs) if name == "rho" else abs(lhs - rhs) / max(abs(lhs), abs(rhs))
            if gap < worst:
                worst, where = gap, (p, name, it, count, lhs, rhs)
    return worst, where


def prune_is_clear(res):
    """Kept flags are compared exactly.  For a threshold inside (0, 1): the band rule of
    test_planted_cases_keep_clear_of_the_prune_threshold, no confidence within 0.1 of it.  Threshold 0: `c < 0` is false
    for every c >= 0, whatever its rounding.  Threshold 1: c = (mu / (mu + r))^2 is 1 only for r = 0; every confidence must
    be below 1 by 1e-6 relative, the margin of every other comparison."""
    for c, thr in res["trace"]["prune"]:
        if thr <= 0.0:
            ok = c >= 0.0
        elif thr >= 1.0:
            ok = c <= 1.0 - 1e-6
        else:
            ok = abs(c - thr) > 0.1
        if not ok:
            return False
    return True

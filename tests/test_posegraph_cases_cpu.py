"""The named graphs of tests/posegraph_cases.py held to the facts they claim, without a GPU: every fact is read from the
oracle's result and trace; every comparison the contract makes clears its threshold by 1e-6 relative, so that the GPU test
may compare statuses, iteration counts and kept flags exactly; and every rule of the optimiser, broken in a copy of the
oracle's text, is rejected by posegraph_cases.compare at the committed bar on at least one case."""
import functools
import os
import types

import numpy as np
import pytest

from tests import posegraph_cases as C
from tests import posegraph_oracle as PG

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-6


def test_the_oracle_returns_what_it_returned_before_the_trace():
    """Poses, confidences, flags, iterations and statuses of PG.graph_batch(), bit for bit, against values recorded before
    the trace, the status-3 rule and the options were added (tests/golden/posegraph_oracle_before.npz)."""
    g = np.load(os.path.join(HERE, "golden", "posegraph_oracle_before.npz"))
    for i, (n, (edges, _, _)) in enumerate(zip(PG.GRAPH_SIZES, PG.graph_batch())):
        r = PG.global_optimization(n, edges, PG.MCD_FINE)
        assert np.array_equal(np.stack(r["poses"]), g[f"poses_{i}"]) and np.array_equal(r["confidence"], g[f"confidence_{i}"])
        assert np.array_equal(r["kept"], g[f"kept_{i}"]) and r["iterations"] == tuple(g[f"iterations_{i}"])
        assert r["status"] == int(g[f"status_{i}"])
        P, conf, it = PG.optimize_once(PG.odometry_chain(n, edges), edges, [1.0] * len(edges), PG.MCD_FINE)
        assert it == r["iterations"][0] and np.array_equal(np.where([e.uncertain for e in edges], conf, 1.0), r["confidence"])


@pytest.mark.parametrize("name", list(C.cases()))
def test_case_claims_hold_and_every_decision_is_clear(name):
    c, res = C.cases()[name], C.oracle(name)
    claims, seen = c["facts"], C.trace_facts(res)
    margin, where = C.smallest_margin(res)
    print(f"{name}: n = {c['n']}, {len(c['edges'])} edges, status {res['status']}, iterations {res['iterations']}, kept "
          f"{int(res['kept'].sum())}, rejected {seen['rejected']}, smallest decision margin {margin:.2e} at {where}; claims {claims}")
    assert all(np.isfinite(p).all() for p in res["poses"]) and np.isfinite(res["confidence"]).all()
    assert res["status"] == claims["status"]
    if "iterations" in claims:
        assert res["iterations"] == claims["iterations"]
    if "kept" in claims:
        assert int(res["kept"].sum()) == claims["kept"]
    for key in ("rejected", "reject_then_accept", "consecutive_rejections", "unclamped_scale"):
        if key in claims:
            assert seen[key] == claims[key], key
    if claims.get("second_pass_longer"):
        assert res["iterations"][1] > 1
    if claims.get("several_pruned"):
        assert (~res["kept"]).sum() > 1
    if claims.get("accepted_in_the_failing_pass"):            # poses, confidences and flags of a step of that very pass
        assert seen["failed"] and seen["accepted_in_the_failing_pass"] >= 1 and not res["kept"].all()
    if claims.get("unsymmetric"):
        assert all(not np.array_equal(e.info, e.info.T) for e in c["edges"] if np.abs(e.info - e.info.T).max() > 0)
        assert any(not np.array_equal(e.info, e.info.T) for e in c["edges"])
    if claims.get("accepted_before_failure"):
        assert seen["failed"] and seen["accepted_before_failure"] >= 1
    if claims.get("denominator_matters_early"):               # a step that is not the last of its pass
        late = [s for tr in res["trace"]["passes"] for s in tr["steps"][:-1] if s["accepted"] and
                abs(s["den"]) < 1.0 and abs(1e-3 / (s["den"] + 1e-3)) > 1e-3]
        assert late and seen["denominator_matters"]
    if claims.get("scrambled"):
        assert C.chain_order_is_scrambled(c["edges"])
        assert len(c["edges"]) < c["n"] * (c["n"] - 1) // 2
    # the margins: a condition on the inputs, met by the oracle alone
    assert margin >= MARGIN, where
    assert C.prune_is_clear(res), res["trace"]["prune"]
    for tr in res["trace"]["passes"]:
        for s in tr["steps"]:
            if s["failed"]:                                     # status 3: clearly not positive definite
                lo, hi = s["eigenvalues"]
                assert lo <= -MARGIN * hi, (lo, hi)
    if res["status"] == 3:
        assert seen["failed"]


def test_the_far_starts_cover_every_rule_of_the_damping():
    """Among far_start_*: a rejection followed by an acceptance (ni reset), two rejections in a row (ni doubled), a scale
    factor strictly inside (1/3, 2/3), a step where the +1e-3 of rho's denominator moves the factor by more than 1e-3, a
    second pass of more than one iteration, more than one pruned edge."""
    seen = {n: C.trace_facts(C.oracle(n)) for n in C.cases() if n.startswith("far_start")}
    for key in ("reject_then_accept", "consecutive_rejections", "unclamped_scale", "denominator_matters"):
        print(key, [n for n, f in seen.items() if f[key]])
        assert any(f[key] for f in seen.values()), key
    assert any(C.oracle(n)["iterations"][1] > 1 for n in seen) and any((~C.oracle(n)["kept"]).sum() > 1 for n in seen)
    assert sorted(C.cases()[n]["n"] for n in seen) == [3, 5, 7, 8]


def test_vec_takes_its_other_branch_where_the_gimbal_cases_say():
    c = C.cases()["gimbal_node"]
    assert np.hypot(c["init"][0][0, 0], c["init"][0][1, 0]) < 1e-12 < 1e-6
    c = C.cases()["gimbal_edge"]
    hits = []
    for e in c["edges"]:
        Z = e.Ti @ np.linalg.inv(c["init"][e.t]) @ c["init"][e.s]
        hits.append(np.hypot(Z[0, 0], Z[1, 0]) < 1e-6)
        if hits[-1]:
            assert np.hypot(Z[0, 0], Z[1, 0]) < 1e-12 and abs(PG.vec(Z)[0] - C.GIMBAL_EDGE_ALPHA) < 1e-12      # alpha is not what gamma is
    assert hits == [(e.s, e.t) == (0, 2) for e in c["edges"]]


def test_general_lambda_is_general():
    for e in C.cases()["general_lambda"]["edges"]:
        assert np.array_equal(e.info, e.info.T) and np.linalg.eigvalsh(e.info).min() > 0.9
        assert abs(e.info[3, 3] - e.info[5, 5]) > 1e-2 * abs(e.info[5, 5]) and np.abs(e.info[3:, 3:] - e.info[5, 5] * np.eye(3)).max() > 1.0
    for e in C.cases()["general_lambda_asymmetric"]["edges"]:
        assert np.abs(e.info - e.info.T).max() > 1.0
    for e, f in zip(C.cases()["general_lambda_skewed"]["edges"], C.cases()["general_lambda"]["edges"]):
        assert np.array_equal((e.info + e.info.T) / 2, f.info) or np.abs((e.info + e.info.T) / 2 - f.info).max() < 1e-11
        assert 1e-8 * np.abs(f.info).max() < np.abs(e.info - e.info.T).max() < 1e-7 * np.abs(f.info).max()
    kept = C.oracle("second_pass_mu")["kept"]
    l55 = np.array([e.info[5, 5] for e in C.cases()["second_pass_mu"]["edges"]])
    assert (~kept).sum() == 1 and l55[kept].mean() < 0.5 * l55.mean()          # mu of the second pass is another number
    assert sum(1 for e, k in zip(C.cases()["second_pass_mu"]["edges"], kept) if k and e.uncertain) >= 2


def test_lambda_read_transposed_is_rejected_by_the_skewed_case_alone():
    """A kernel that read info[6 j + i] for Lambda(i, j) computes the oracle's answer to the transposed matrices.  On every
    symmetric case that is the same answer; general_lambda_skewed tells the two apart at BAR."""
    killers = []
    for name, c in C.cases().items():
        t, o = C.transposed(c), c["options"]
        got = PG.global_optimization(t["n"], t["edges"], o["mcd"], t["init"], o["edge_prune_threshold"], o["preference_loop_closure"])
        exact, dc, dp = C.difference(got, C.oracle(name))
        if exact is not None or max(dc, dp) > C.BAR:
            killers.append(name)
            print(f"Lambda transposed: rejected by {name} ({exact}, confidence {dc:.2e}, relative poses {dp:.2e})")
        elif not c["facts"].get("unsymmetric"):
            assert max(dc, dp) <= 1e-3 * C.BAR, name               # symmetric up to the rounding of its builder
    assert "general_lambda_skewed" in killers
    assert C.oracle("general_lambda_skewed")["status"] == 0


def test_the_host_layout_refuses_what_the_kernel_calls_status_4():
    from apr_amd import _lib, ops
    for name, m in C.MALFORMED.items():
        with pytest.raises(_lib.AprHipError, match="posegraph"):
            ops.PoseGraphLayout([(m["n"], m["rows"])], need_chain=True)
        if not m["chain"]:
            with pytest.raises(_lib.AprHipError, match="posegraph"):
                ops.PoseGraphLayout([(m["n"], m["rows"])], need_chain=False)
    c = C.cases()["no_chain_with_init"]
    assert all(e.uncertain for e in c["edges"]) and not any(e.t == e.s + 1 for e in c["edges"]) and c["init"] is not None
    with pytest.raises(_lib.AprHipError, match="odometry chain"):
        ops.PoseGraphLayout([(c["n"], [(e.s, e.t, e.uncertain) for e in c["edges"]])], need_chain=True)


def test_compare_accepts_the_oracle_and_rejects_what_lies_beyond_the_bar():
    want = C.oracle("far_start_5")
    assert C.compare(want, want, C.BAR) == 0.0
    for key, bad in (("status", 3), ("iterations", (5, 11)), ("kept", ~want["kept"])):
        with pytest.raises(AssertionError):
            C.compare({**want, key: bad}, want, C.BAR)
    conf = want["confidence"].copy()
    conf[2] += 3 * C.BAR
    with pytest.raises(AssertionError):
        C.compare({**want, "confidence": conf}, want, C.BAR)
    # a rotation of 3 bar radians: far below what an arccos of the trace resolves, and rejected entry by entry
    poses = [p.copy() for p in want["poses"]]
    poses[3] = poses[3] @ PG.mat((3 * C.BAR, 0, 0, 0, 0, 0))
    with pytest.raises(AssertionError):
        C.compare({**want, "poses": poses}, want, C.BAR)
    poses[3] = want["poses"][3] @ PG.mat((0.1 * C.BAR, 0, 0, 0, 0, 0))
    C.compare({**want, "poses": poses}, want, C.BAR)
    # a common left factor (the gauge) does not count
    G = PG.mat((0.2, -0.1, 0.3, 1.0, 2.0, 3.0))
    assert C.compare({**want, "poses": [G @ p for p in want["poses"]]}, want, C.BAR) < 1e-13


# ---- mutants: one rule each, broken in a copy of the oracle's text ----
MUTANTS = {
    "jacobian rotation columns x 0.7": ("    return Js\n", "    Js[:, :3] *= 0.7\n    return Js\n"),
    "jacobian lever-arm block zeroed": ("    return Js\n", "    Js[3:, :3] = 0.0\n    return Js\n"),
    "lambda0 = 1e-3 max diag H": ("lam, ni = 1e-5 * H.diagonal().max(), 2.0", "lam, ni = 1e-3 * H.diagonal().max(), 2.0"),
    "scale clamp [2/3, 1]": ("max(1.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0))",
                             "max(2.0 / 3.0, min(1.0 - (2.0 * rho - 1.0) ** 3, 1.0))"),
    "second pass restarts from confidences 1": ("[c for c, k in zip(conf1, kept) if k], mu2", "[1.0 for c, k in zip(conf1, kept) if k], mu2"),
    "H_st x 0.9": ("H[s, t] += l * Js.T @ e.info @ Jt", "H[s, t] += 0.9 * l * Js.T @ e.info @ Jt\n"
                   "        H[t, s] += -0.1 * l * Jt.T @ e.info @ Js"),
    "rho without + 1e-3": ("rho = (cur - new) / (den + 1e-3)", "rho = (cur - new) / den"),
    "mu from Lambda(3,3)": ("e.info[5, 5] for e in edges", "e.info[3, 3] for e in edges"),
    "ni not reset on acceptance": ("                    ni = 2.0\n", ""),
    "ni not doubled": ("ni *= 2.0", "ni *= 1.0"),
    "confidences from the errors before the step": ("for e, er, l in zip(edges, errs_n, conf)]", "for e, er, l in zip(edges, errs, conf)]"),
    "confidences not squared": ("(mu / (mu + float(er @ e.info @ er))) ** 2 if", "(mu / (mu + float(er @ e.info @ er))) if"),
    "residual without mu (sqrt(l) - 1)^2": ("tot += l * r + mu * (math.sqrt(l) - 1.0) ** 2 if e.uncertain else r",
                                            "tot += l * r if e.uncertain else r"),
    "mu not recomputed for the second pass": ("mu2 = _mu(sub, mcd, preference_loop_closure)", "mu2 = _mu(edges, mcd, preference_loop_closure)"),
    "b_t with the wrong sign": ("b[t] -= l * Jt.T @ e.info @ er", "b[t] += l * Jt.T @ e.info @ er"),
    "alternate vec branch returns gamma for alpha": (
        "a, b, g = math.atan2(-M[1, 2], M[1, 1]), math.atan2(-M[2, 0], sy), 0.0",
        "a, b, g = 0.0, math.atan2(-M[2, 0], sy), math.atan2(-M[1, 2], M[1, 1])"),
}
# `stop |= count > 20` turned into `>=` needs a pass that runs its 21st inner solve.  posegraph_cases explains why no finite
# graph has one (LM_CAP); without such a case the two rules are the same function of every input the suite can build.
LM_CAP_MUTANT = ("stop = stop or count > MAX_ITERATION_LM", "stop = stop or count >= MAX_ITERATION_LM")


@functools.lru_cache(maxsize=None)
def _source():
    with open(os.path.join(HERE, "posegraph_oracle.py")) as f:
        return f.read()


def _mutated(old, new):
    text = _source()
    assert text.count(old) == 1, f"{old!r} must occur exactly once in the oracle"
    mod = types.ModuleType("posegraph_oracle_mutant")
    exec(compile(text.replace(old, new), "posegraph_oracle_mutant", "exec"), mod.__dict__)
    return mod


def _killed_by(mod):
    """The cases whose final outputs compare rejects, in the order of posegraph_cases.cases()."""
    killers = []
    for name, c in C.cases().items():
        o = c["options"]
        try:
            with np.errstate(all="ignore"):
                got = mod.global_optimization(c["n"], c["edges"], o["mcd"], c["init"], o["edge_prune_threshold"],
                                              o["preference_loop_closure"])
            C.compare(got, C.oracle(name), C.BAR)
        except (AssertionError, np.linalg.LinAlgError, ValueError, ZeroDivisionError, FloatingPointError):
            killers.append(name)
    return killers


def test_the_unmutated_copy_is_the_oracle():
    mod = _mutated("MAX_ITERATION, MAX_ITERATION_LM, MIN = 100, 20, 1e-6", "MAX_ITERATION, MAX_ITERATION_LM, MIN = 100, 20, 1e-6 ")
    assert _killed_by(mod) == []


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_is_rejected_by_a_named_case(mutant):
    killers = _killed_by(_mutated(*MUTANTS[mutant]))
    print(f"{mutant}: rejected by {killers}")
    assert killers, f"{mutant} survives every case at BAR = {C.BAR:.0e}"


def test_the_count_mutant_is_held_by_lm_cap_or_is_unreachable():
    killers = _killed_by(_mutated(*LM_CAP_MUTANT))
    print(f"count >= 20: rejected by {killers}")
    if "lm_cap" in C.cases():
        assert killers
    else:
        assert C.LM_CAP is None and killers == []       # no inner loop of any case reaches its 21st solve
        longest = max(s["count"] for n in C.cases() for tr in C.oracle(n)["trace"]["passes"] for s in tr["steps"])
        print(f"the longest inner loop of any case runs {longest + 1} solves")
        assert longest < PG.MAX_ITERATION_LM - 1

"""Workspace sizes against the commit before the arena walks (tests/golden/scratch_sizes_parent.json, the output of
scripts/dump_scratch_sizes.py on a build of that commit)."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(lib):
    spec = importlib.util.spec_from_file_location("dump_scratch_sizes", os.path.join(ROOT, "scripts", "dump_scratch_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "scratch_sizes_parent.json")) as f:
        parent = json.load(f)
    return parent, mod.table(lib)


def test_no_size_grew_by_more_than_the_base_rounding(tables):
    """An arena walk rounds its base up to 256 and says so in bytes(); some of the hand-summed formulas it replaces had no
    allowance for that.  So a size may exceed the parent's by those 256 bytes and by nothing else; where the parent
    refused (0), so does the walk.  Smaller is allowed: the lower bound is the walk itself (test_scratch_guard_gpu.py)."""
    parent, new = tables
    assert set(parent) == set(new)
    bad = []
    for name in sorted(parent):
        assert [a for a, _ in parent[name]] == [a for a, _ in new[name]], name
        for (args, was), (_, now) in zip(parent[name], new[name]):
            if now > was + 256 or (was == 0) != (now == 0):
                bad.append((name, args, was, now))
    assert not bad, bad[:20]


def test_nn_scratch_size_stays_monotone(tables):
    """as tests/test_library_cpu.py::test_nn_scratch_size_is_monotone, over the tabulated counts"""
    _, new = tables
    size = {tuple(a): v for a, v in new["apr_feature_nn_fast_scratch_bytes"]}
    for (n0, n1, c), v in size.items():
        for (m0, m1, d), w in size.items():
            if d == c and m0 >= n0 and m1 >= n1:
                assert w >= v, ((n0, n1, c), v, (m0, m1, d), w)
    batch = {tuple(a): v for a, v in new["apr_match_pose_batch_scratch_bytes@lanes=1"]}
    for (b, n0, n1, c, m), v in batch.items():
        if c == 32:
            assert v > size.get((n0, n1, c), 0)

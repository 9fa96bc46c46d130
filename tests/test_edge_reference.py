r"""The C oracle against the REFERENCE on the tree edge-case families.  Every GPU test over tree_threshold_cases,
tree_split_cases, tree_storage_cases and tree_abi_cases asserts libbbhip.so == oracle; here the oracle's replay of the same
cases - through the raw case configuration, the very replay those GPU tests compare against - is held against what the
reference's own BitBirch computed for them (tests/golden/edges.npz, written by tests/golden/make_golden_edges.py; the cases
and the observables are edge_reference_cases.py's).  A misreading of the reference that the oracle and the kernels share -
`>` for `>=` in an accept, the last of equal maxima, a lost majority tie - fails here; DESIGN.md, "Oracle against reference
on the edge-case families", has the mutations of oracle/bb_oracle.c that were tried and the tests that caught them.

When a case fails, `python tests/golden/make_golden_edges.py --explain CASE` (where the reference is) prints the first
element, leaf or walk row that differs: the digests kept in the fixture cannot.

Measured: the whole file 298 tests in 2.4 min alone; in the whole suite the 24 000-row oracle replays are shared with
test_tree_threshold_cases.py through tree_threshold_cases.replay_named's cache."""
from __future__ import annotations

import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import edge_reference_cases as E
from _refimport import reference_available
from oracle_engine import OracleEngine

LADDER = [cid for cid, (group, _) in E.RECORDED.items() if group == "ladder"]
# regenerated where the reference is: a ladder case on the edge, a tie case, a majority tie, the reset, a corner shape
REGENERATED = ["thr/5_9-bf50-crit0-+0ulp-pure-grouped", "thr/tie-50-0-0.5", "split/camps-bf127-tie", "storage/reset", "abi/corner-bf2-F8192"]


def test_representation():
    r"""What of the four families the fixture holds, what it leaves out and why: every group that puts a decision of the
    reference's on an edge keeps at least one recorded case, and nothing is left out for a reason but the three that the
    reference's public class cannot express."""
    recorded = set(E.fixture())
    assert recorded == set(E.RECORDED), (sorted(set(E.RECORDED) - recorded)[:5], sorted(recorded - set(E.RECORDED))[:5])
    groups = Counter(group for group, _ in E.RECORDED.values())
    families = Counter(cid.split("/")[0] for cid in E.RECORDED)
    print("recorded cases by family:", dict(families))
    print("recorded cases by group:", dict(groups))
    for cid, _, reason, detail in E.LEFT_OUT:
        print(f"left out: {cid}: {reason} ({detail})")
    assert all(groups[g] >= 1 for g in E.REQUIRED_GROUPS), {g: groups[g] for g in E.REQUIRED_GROUPS}
    assert {reason for _, _, reason, _ in E.LEFT_OUT} <= set(E.REASONS)
    assert not {cid for cid, _, _, _ in E.LEFT_OUT} & set(E.RECORDED)
    assert set(REGENERATED) <= set(E.RECORDED)


def test_the_lists_are_what_the_rule_says():
    r"""Mechanically, with a recording engine factory: every recorded case has only operations the reference has and the
    configuration the host's own BitBirch hands to an engine; every left-out case that can be built fails that rule for the
    reason written next to it."""
    for cid in E.RECORDED:
        c, ops = E.build(cid)
        assert E.why_not(c, ops) is None, (cid, E.why_not(c, ops))
    for cid, src, reason, _ in E.LEFT_OUT:
        if src is not None:
            assert E.why_not(*E.build_source(src)) == reason, (cid, E.why_not(*E.build_source(src)), reason)


def test_table_reads():
    r"""The rule's own helper: a table counts as equal to another when both read the same for every cluster size."""
    assert (E.table_reads((), 4) == 0).all() and (E.table_reads(np.zeros(1001), 4) == E.table_reads((), 4)).all()
    assert E.table_reads((0.0, 0.0, 0.1), 1).tolist() == [0.0, 0.0] and E.table_reads((0.0, 0.0, 0.1), 3).tolist() == [0.0, 0.0, 0.1, 0.0]
    c = dict(E.T.cfg(50, 0.5, 64, E.T.TOL_LEGACY, 1e-16, ()))
    assert E.host_config(c)["tol"] == 1e-16 and E.host_config(dict(c, crit=E.T.DIAMETER))["tol"] == 0.0


def test_a_planted_difference_is_noticed_and_located():
    r"""The comparison's own tools: one n_samples and one linear-sum entry changed fail the digests, and first_difference
    (what `--explain` prints) names the row."""
    cid = "split/camps-bf3-tie"
    obs = E.oracle_observables(cid)
    assert E.first_difference(obs, obs) == [] and E.against_fixture(cid, obs) == []
    counts, cols, vals = obs["ls"]
    bad = dict(obs, ns=obs["ns"].copy(), ls=(counts, cols, vals.copy()))
    bad["ns"][2] += 1
    bad["ls"][2][int(counts[:3].sum())] += 1  # the first non-zero entry of leaf 3
    lines = E.first_difference(bad, obs)
    assert any(ln.startswith("ns:") and "first at 2:" in ln for ln in lines) and any(ln.startswith("ls: first at row 3,") for ln in lines), lines
    failed = E.against_fixture(cid, bad)
    assert any(f.startswith("ns_sha") for f in failed) and any(f.startswith("ls_sha") for f in failed), failed


@pytest.mark.parametrize("cid", list(E.RECORDED))
def test_oracle_equals_reference(cid):
    r"""The input rows are the ones the reference saw, and the oracle's replay through the raw case configuration equals the
    reference in every recorded observable: cluster count after every fit call, assignments, unsorted member order,
    centroids, n_samples and linear sums of the leaves, and the pre-order walk - per node depth, leaf flag, length and
    chain position, per row n_samples, centroid and (where the family's replay keeps them) linear sum."""
    c, ops = E.build(cid)
    want = E.fixture()[cid]
    assert E.input_digest(ops) == bytes(want["input_sha"]).hex(), "the case's rows are not the ones the fixture was made from"
    obs = E.oracle_observables(cid)
    assert {"assign", "members", "ns", "cents", "ls", "walk_nodes", "walk_n", "walk_cent"} <= set(obs)
    bad = E.against_fixture(cid, obs)
    assert not bad, f"{cid}: the oracle differs from the reference in " + "; ".join(bad)


@pytest.mark.parametrize("cid", LADDER)
def test_host_route_equals_reference(cid):
    r"""The ladder cases through bblean_amd.BitBirch(merge_criterion=name, tolerance=t, _engine_factory=OracleEngine): the
    host's translation of a criterion into a code, a tolerance and a table is part of what is pinned."""
    c, ops = E.build(cid)
    from bblean_amd import BitBirch

    tree, obs = E.public_observables(lambda **kw: BitBirch(_engine_factory=OracleEngine, **kw), c, ops)
    tree._engine.close()
    bad = E.against_fixture(cid, obs)
    assert not bad, f"{cid}: BitBirch on the oracle differs from the reference in " + "; ".join(bad)


@pytest.mark.reference
@pytest.mark.skipif(not reference_available(), reason="the reference is not on this machine")
def test_fixture_is_current():
    r"""Where the reference is: a handful of cases regenerated by the generator (in a process of its own: importing the
    reference puts stand-ins for its missing dependencies into sys.modules) equal the committed fixture."""
    gen = Path(__file__).resolve().parent / "golden" / "make_golden_edges.py"
    run = subprocess.run([sys.executable, str(gen), "--check"] + REGENERATED, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]

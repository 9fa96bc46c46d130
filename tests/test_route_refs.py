r"""route_refs.py held against the oracle and against the conditions its cases are named for (no GPU).

The reference is a NumPy descent over the oracle's walk; what it must reproduce is the oracle's own insertion: rebuild the
tree, insert the query alone - it merges iff the reference says accept, and then into the leaf the reference names.  And a
case that does not meet its condition (a tied search, both merge outcomes, a tier, the depth) fails here, so that the GPU
comparison in test_hip_route.py never passes on a case that has gone empty."""
from __future__ import annotations

import numpy as np
import pytest

import route_refs as R
import tree_abi_cases as T
import tree_threshold_cases as TH


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_is_the_oracles_insertion(name):
    r"""For every query of every case: the oracle, rebuilt, inserts that row alone.  Its merge counter rises iff the reference
    accepts, and its out_leaf is then the reference's leaf.  (A refused row is appended under a new id.)"""
    c, ops, q = R.CASES[name]()
    want = R.expected(name)
    eng = R.build_oracle(c, ops)
    known = set(eng.export_leaves()[0].tolist())
    eng.close()
    for e in range(q.shape[0]):
        merged, leaf = R.insert_alone(c, ops, q[e])
        assert merged == bool(want["accept"][e]), (name, e, merged, want["accept"][e])
        if merged:
            assert leaf == want["leaf"][e], (name, e, leaf, want["leaf"][e])
        else:
            assert leaf not in known, (name, e, leaf)
        assert int(want["leaf"][e]) in known, (name, e)
        assert want["inter"][e] <= want["union"][e] or want["union"][e] == 0


def test_depth_case_reaches_four_levels_with_both_outcomes():
    want = R.expected("depth")
    assert want["tree_depth"] == 4 and (want["depth"] == 4).all(), (want["tree_depth"], set(want["depth"].tolist()))
    assert len(want["accept"]) == 150 and 20 <= int(want["accept"].sum()) <= 130, int(want["accept"].sum())


def test_width_cases_meet_their_node_lengths():
    r"""Every (width, bf) corner builds; the never-merge trees at bf 1023 are one leaf root of more than 512 rows; leaf roots of
    1, 4, 5 and bf rows exist; trees of several levels at bf 2, 3, 50 and 254."""
    for F in R.WIDTHS:
        assert R.expected(f"width_{F}_bf1023")["node_lens"] == [600]
        assert not R.expected(f"width_{F}_bf1023")["accept"].any()
        for bf in (2, 3):
            assert R.expected(f"width_{F}_bf{bf}")["tree_depth"] >= 3
        if F > 8:
            for bf in (50, 254):
                assert R.expected(f"width_{F}_bf{bf}")["tree_depth"] >= 2, (F, bf)
    for n in R.LENGTHS:
        assert R.expected(f"length_{n}")["node_lens"] == [n] and set(R.expected(f"length_{n}")["lens"]) == {n}
    assert R.LENGTHS[-1] == R.length_case(R.LENGTHS[-1])[0]["bf"]
    assert 254 in R.expected("width_8192_bf254")["node_lens"]  # a full node of bf rows at bf 254, too


def test_tie_cases_tie():
    zero = R.expected("ties_zero")
    c, ops, q = R.CASES["ties_zero"]()
    assert not q[0].any() and zero["inter"][0] == 0 and zero["depth"][0] >= 2
    eng = R.build_oracle(c, ops)
    walk = eng.walk()
    eng.close()
    assert (walk["pop"] == 0).any(), "no all-zero centroid row in the tree"
    # the all-zero query goes down row 0 of every node: its leaf is the first row of the first leaf in pre-order
    first_leaf = int(np.argmax(walk["nodes"][:, 1] != 0))
    assert first_leaf == zero["depth"][0] - 1
    assert zero["leaf"][0] == walk["id"][int(np.concatenate([[0], np.cumsum(walk["nodes"][:, 2])])[first_leaf])]
    # (its union with an all-zero centroid would be 0: allowed)
    dups = R.expected("ties_dups")
    assert (dups["ties"] > 0).all(), "duplicated centroids must tie"
    assert (dups["inter"][:12] == dups["union"][:12]).all(), "a query equal to a centroid has similarity 1"
    halves = R.expected("ties_halves")
    assert halves["ties_differ"][0] == 1 and (halves["inter"][0], halves["union"][0]) == (1, 2), "1/2 against 2/4: the lower row, 1/2, wins"
    assert R.expected("ties_blocks")["ties_differ"].sum() >= 1
    assert sum(int(R.expected(n)["ties"].sum()) for n in R.CASES) >= 100


@pytest.mark.parametrize("crit,F,bf", R.CRIT_SHAPES, ids=lambda v: str(v))
def test_criterion_cases_decide_both_ways_and_on_the_threshold(crit, F, bf):
    name = f"crit_{crit}_{F}_bf{bf}"
    want = R.expected(name)
    acc = int(want["accept"].sum())
    if crit == "never":
        assert acc == 0
        return
    assert 0 < acc < len(want["accept"]), (name, acc)
    # on the threshold: one ulp more and fewer rows are accepted (the family members' decisions are equalities)
    c, ops, q = R.CASES[name]()
    eng = R.build_oracle(c, ops)
    walk = eng.walk()
    eng.close()
    if crit == "tol_radius":  # (its edge is the second comparison: the table entry old_n = 2 reads, less one ulp of the values compared)
        tab = np.array(c["table"])
        v3 = TH.criterion_value(R.RADIUS, 3, R.CRIT_C, R.CRIT_P)
        tab[2] -= TH.ulps(v3, 1) - v3
        above = R.route(walk, dict(c, table=tab), q)
    else:
        above = R.route(walk, dict(c, thr=TH.ulps(c["thr"], 1)), q)
    assert int(above["accept"].sum()) < acc, (name, acc, int(above["accept"].sum()))
    assert (above["leaf"] == want["leaf"]).all()
    if crit in ("tol_diameter", "tol_radius"):
        reached = walk["n"][np.isin(walk["id"], want["leaf"])]
        assert (reached >= len(c["table"])).any(), "no decision reads beyond the tolerance table"


def test_tier_case_reaches_every_tier():
    want = R.expected("tiers")
    assert sorted(set(want["tier"].tolist())) == [0, 1, 2, 3], sorted(set(want["tier"].tolist()))
    for t in range(4):
        assert len(set(want["accept"][want["tier"] == t].tolist())) >= 1
    assert 0 < int(want["accept"].sum()) < len(want["accept"])


def test_storage_cases_have_nodes_to_seal():
    r"""Sealing needs nodes shorter than bf + 1 rows, on more than one level."""
    for name in ("depth", "storage_wide"):
        want = R.expected(name)
        c = R.CASES[name]()[0]
        assert want["tree_depth"] >= 2 and want["node_lens"][0] + 4 <= c["bf"] + 1 or c["bf"] == 5, (name, want["node_lens"])
        assert 0 < int(want["accept"].sum()) < len(want["accept"])


def test_ref_engine_is_consistent_with_the_cases():
    r"""RefEngine (the engine of test_route_api.py) gives the cases' expected answers."""
    c, ops, q = R.CASES["tiers"]()
    eng = R.RefEngine(c["bf"], c["thr"], c["crit"], c["tol"], c["table"], c["F"])
    for op in ops:
        T.apply_op(eng, op)
    leaf, acc, inter, union = eng.route_packed(q)
    want = R.expected("tiers")
    assert (leaf == want["leaf"]).all() and (acc == want["accept"]).all() and (inter == want["inter"]).all() and (union == want["union"]).all()
    eng.close()

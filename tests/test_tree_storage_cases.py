r"""The cases of tree_storage_cases.py against the conditions that make them worth running, on the C oracle and its storage
model alone (no GPU): a case whose rows stop reaching a sealed node tests nothing.  test_hip_tree_storage.py runs the same
cases on the GPU.

bbo_tree_storage and bbo_tree_thaw_counts (oracle/bb_oracle.h) say what the model holds after every operation - used blocks,
compactions, cold and full nodes of the last one, thaws, and what each thaw met; every case names the values it exists for,
operation by operation.  The model only observes: a replay with every compaction and reload taken out gives the same tree."""
from __future__ import annotations

import numpy as np
import pytest

import tree_abi_cases as T
import tree_image_format as IMG
import tree_storage_cases as SC
from oracle_engine import THAW_COUNTS

NAMED = [n for n in THAW_COUNTS if not n.startswith("_")]


@pytest.mark.parametrize("name", list(SC.CASES))
def test_case_meets_its_conditions(name):
    c, ops, checks = SC.build(name)
    snaps = SC.replay(name)
    print(name, [op[0] for op in ops], snaps[-1]["storage"], {k: v for k, v in snaps[-1]["thaw"].items() if v})
    assert checks and not SC.unmet(snaps, checks), (name, SC.unmet(snaps, checks))
    full = SC.node_blocks(c["bf"] + 1)
    for i, snap in enumerate(snaps):
        IMG.check_walk(snap["walk"], f"{name}, oracle, after operation {i}")
        st = snap["storage"]
        assert st["live"] == max(len(snap["walk"]["nodes"]), 1) and st["sealed_now"] < st["live"]
        if st["pools"]:  # no node takes more than full capacity, the holes only add
            assert st["used_blocks"] >= st["live"] - st["sealed_now"] and st["used_blocks"] >= full
    # the last operation brings every node back to full capacity
    assert ops[-1] == ("compact", 0) and snaps[-1]["storage"]["used_blocks"] == snaps[-1]["storage"]["live"] * full


@pytest.mark.parametrize("name", ["seal_all-bf8-F64", "thaw_then_split", "seal_rule", "tiers-w4", "reset", "reload-thaw_links-merge"])
def test_the_model_only_observes(name):
    r"""The same operations without the compactions and reloads: every leaf, counter and row of the walk is the same."""
    c, ops, _ = SC.build(name)
    with_model = SC.replay(name)[-1]
    plain = SC.replay_ops(c, [op for op in ops if op[0] not in ("compact", "reload")])[-1]
    T.same(plain, with_model)
    IMG.same_walk(plain["walk"], with_model["walk"], "without the storage operations against with them")
    assert plain["storage"]["thaws"] == 0 and plain["storage"]["sealed_now"] == 0


def test_worked_example():
    r"""bf 8 (9 rows a node: 3 blocks), by hand.  Nine rows split the root: 3 nodes, 9 blocks.  The first compaction records,
    the second seals the two leaves (5 and 4 rows: 2 blocks and 1) - 3 + 2 + 1 = 6 blocks.  A row for the leaf of 4: its thaw
    leaves a hole of 1 block and takes 3 - 9 blocks.  compact(1): the thawed leaf has no record and stays full, the other
    stays sealed, the hole goes - 3 + 3 + 2 = 8."""
    c, ops, _ = SC.build("length-bf8-F64-L4")
    snaps = SC.replay("length-bf8-F64-L4")
    assert [op[0] for op in ops] == ["packed", "compact", "compact", "packed", "packed", "compact"]
    used = [s["storage"]["used_blocks"] for s in snaps]
    assert sorted(snaps[0]["walk"]["nodes"][1:, 2].tolist()) == [4, 5]
    assert used[:4] == [9, 9, 6, 9], used
    assert [snaps[i]["storage"]["thaws"] for i in range(5)] == [0, 0, 0, 1, 1]
    eng = T.make_oracle(c)
    for op in ops[:4]:
        T.apply_op(eng, op)
    eng.compact(1)
    st = eng.storage()
    eng.close()
    assert (st["used_blocks"], st["cold"], st["full"], st["sealed_now"]) == (8, 1, 2, 1), st


@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.kernel_id)
def test_kernel_case_meets_its_conditions(case):
    r"""The second tail - after two compactions or a reload - thaws a sealed leaf-parent, sealed leaves under a leaf-parent an
    earlier element thawed, a leaf without a spare row, and splits a leaf it thawed.  Behind the prefix the root is a zero
    level; the grouped rows keep every level informative (the multi-level instance's shape) and reach every leaf-parent."""
    bf, how, kind = case
    gained = SC.second_tail(case)
    snaps = SC.replay_kernel(*case)
    at = SC.second_fit(case)
    print(SC.kernel_id(case), {k: v for k, v in gained.items() if v})
    assert not [k for k in SC.KERNEL_CONDITIONS if gained[k] <= 0], gained
    walk = snaps[at - 1]["walk"]
    root_pops = walk["pop"][:walk["nodes"][0, 2]]
    if kind == "prefix":
        assert len(snaps[0]["out_leaf"][0]) == SC.PF.N_PREFIX and snaps[-1]["depth"] >= 3
        assert bf != 50 or (root_pops == 0).all(), "at bf 50 the root over the prefix is a zero level"
    else:
        assert len(snaps[0]["out_leaf"][0]) == SC.GROUPED_FIRST > 8192 and snaps[at - 1]["depth"] == snaps[-1]["depth"] == 3
        assert (root_pops > 0).all(), "every tracking row of the root is informative: no zero level"
        n_parents = int(((walk["nodes"][:, 0] == 2) & (walk["nodes"][:, 1] == 0)).sum())
        assert gained["leaf_parent"] >= n_parents - 3 >= 5, (gained["leaf_parent"], n_parents)  # (most leaf-parents are sealed and reached)
    before = snaps[at - 1]["storage"]
    assert before["sealed_now"] > 0 and before["thaws"] == 0
    assert before["sealed_now"] < before["live"] - 1, "leaves whose length rounds up to full capacity are cold, not sealed"
    IMG.check_walk(snaps[-1]["walk"], f"{SC.kernel_id(case)}, oracle")


def test_multi_tree_meets_its_conditions():
    r"""The one call's rows thaw leaves and leaf-parents of the sealed and of the reloaded tree and nothing of the fresh one."""
    replays = SC.replay_multi_tree()
    for name, c, before, rows in SC.multi_tree():
        snaps = replays[name]
        gained = {k[1:]: v for k, v in SC.numbers(snaps, len(snaps) - 1).items() if k.startswith("+")}
        print(name, {k: v for k, v in gained.items() if v})
        if name == "fresh":
            assert not before and gained["thaws"] == 0 and snaps[-1]["depth"] >= 3
        else:
            assert snaps[len(before) - 1]["storage"]["sealed_now"] > 0
            assert gained["leaf_parent"] > 0 and gained["leaf_under_thawed_parent"] > 0 and gained["thawed_leaf_splits"] > 0, gained
        assert snaps[len(before) - 1 if before else 0]["storage"]["runs"] == (2 if name == "sealed" else 0)
        IMG.check_walk(snaps[-1]["walk"], f"multi_tree {name}, oracle")


def test_every_thaw_counter_has_a_case():
    met = {n: [] for n in NAMED}
    for name in SC.CASES:
        counts = SC.replay(name)[-1]["thaw"]
        for n in NAMED:
            if counts[n]:
                met[n].append(name)
    assert not [n for n, cases in met.items() if not cases], met


def test_reload_and_two_compactions_leave_the_same_capacities():
    r"""Every node but the root at its rounded length either way; only the handle's compaction counters differ."""
    a = SC.replay("thaw_then_split")
    b = SC.replay("reload-thaw_then_split")
    sa, sb = a[2]["storage"], b[1]["storage"]
    assert (sa["used_blocks"], sa["sealed_now"], sa["live"]) == (sb["used_blocks"], sb["sealed_now"], sb["live"])
    assert (sa["runs"], sb["runs"]) == (2, 0)
    assert a[-1]["storage"]["thaws"] == b[-1]["storage"]["thaws"] == 2
    assert np.array_equal(a[-1]["walk"]["nodes"], b[-1]["walk"]["nodes"])

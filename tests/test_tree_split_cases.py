r"""The cases of tree_split_cases.py against the conditions that make them worth running, on the C oracle alone (no GPU): a case
whose split stops sitting on its edge tests nothing.  test_hip_tree_splits.py runs the same cases on the GPU.

bbo_tree_split_counts (oracle/bb_oracle.h) says how many splits of a replay met each condition; every case names the ones it
exists for - True: some split met it, False: none did (the "one row away" twins) - and the fit call they are counted over.
Every condition of the list is met by some case of the complete engine (test_every_condition_has_a_case), and by some tail
of every insertion kernel where the kernels' shapes can reach it.  The exceptions: at bf 50 and 254 a node has m = 51 or 255 rows, both odd, so a majority tie
(2 * count == m) and n1 == n2 cannot occur there; the tails are fingerprints, whose BitFeatures stay far below 65 536 members;
a tail in a tree of its own splits no internal node, and behind the prefix no tail splits the root.

The oracle's walk (bbo_tree_walk) is held against its leaf export, and the invariant checker of tree_image_format.py against
the walk of every case and against walks with one planted fault each."""
from __future__ import annotations

import numpy as np
import pytest

import tree_abi_cases as T
import tree_image_format as IMG
import tree_split_cases as S
from oracle_engine import SPLIT_COUNTS

NAMED = [n for n in SPLIT_COUNTS if not n.startswith("_")]


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_meets_its_conditions(name):
    snaps, counts = S.replay(name)
    scope, conditions = S.CASES[name][2]
    print(name, scope, {k: v for k, v in S.scoped(counts, scope).items() if v})
    assert not S.unmet(counts, scope, conditions), (name, scope, S.scoped(counts, scope))
    assert snaps[-1]["stats"][4] == counts[-1]["splits"] > 0
    for i, snap in enumerate(snaps):
        IMG.check_walk(snap["walk"], f"{name}, oracle, after fit {i}")


@pytest.mark.parametrize("prefixed", [False, True], ids=["alone", "behind-the-prefix"])
@pytest.mark.parametrize("case", S.KERNEL_CASES, ids=S.kernel_id)
def test_kernel_tail_meets_its_conditions(case, prefixed):
    r"""The tails of the three insertion kernels, alone (steady-state kernel, complete engine) and behind the prefix (pipelined
    kernel): the conditions hold over the splits of the TAIL's fit calls."""
    name, bf = case
    snaps, counts = S.replay_kernel(name, bf, prefixed)
    tail = S.kernel_tail_counts(name, bf, prefixed)
    print(S.kernel_id(case), prefixed, {k: v for k, v in tail.items() if v})
    bad = {k: tail[k] for k, want in S.KERNEL_CONDITIONS[name].items() if (tail[k] > 0) != want}
    assert not bad, bad
    if not prefixed:
        for k in S.ALONE_CONDITIONS.get(name, {}):  # (in more splits than the root's own: in a leaf split under a parent with room)
            assert tail[k] > (tail["root"] if k != "fp1_last_row" else 0) and tail["root"] == 1, (k, tail)
    assert tail["splits"] - tail["internal"] >= 2, "leaf splits in the tail"
    assert tail["majority_tie"] == 0 and tail["n1_eq_n2"] == 0, "m = 51 and 255 are odd"
    if prefixed:
        assert len(snaps[0]["out_leaf"][0]) == S.PF.N_PREFIX
    IMG.check_walk(snaps[-1]["walk"], f"{S.kernel_id(case)}, oracle")


def test_every_condition_has_a_case():
    r"""Every counter of bbo_tree_split_counts is non-zero in some in-process case, and in some tail of the three kernels unless
    the kernels' shapes rule it out."""
    met = {n: [] for n in NAMED}
    for name in S.CASES:
        counts = S.replay(name)[1][-1]
        for n in NAMED:
            if counts[n]:
                met[n].append(name)
    assert not [n for n, cases in met.items() if not cases], met
    for prefixed in (False, True):  # (alone: the steady-state kernel and the complete engine; behind the prefix: the pipelined kernel)
        tails = {n: 0 for n in NAMED}
        for name, bf in S.KERNEL_CASES:
            counts = S.kernel_tail_counts(name, bf, prefixed)
            for n in NAMED:
                tails[n] += counts[n]
        # The exceptions, all of them: m = 51 and 255 are odd - no majority tie, no n1 == n2.  Fingerprint tails stay far below
        # 65 536 members a BitFeature (the in-process tier cases have them).  A tail alone builds a root over leaves and nothing
        # deeper, so no internal node splits there; behind the prefix the root never splits in a tail.  (The steady-state and
        # pipelined kernels hand the split of an internal node or of the root to the complete engine anyway.)
        never = {"majority_tie", "n1_eq_n2", "small_over_65535"} | ({"root"} if prefixed else {"internal"})
        assert {n for n, v in tails.items() if not v} <= never, (prefixed, tails)
        assert tails["majority_tie"] == 0 and tails["n1_eq_n2"] == 0


@pytest.mark.parametrize("name", ["camps-bf3-tie", "second-bf127-s17-le", "tier-u32-leaf", "natural-bf5", "lopsided-bf50", "peel-bf254"])
def test_walk_and_export_agree(name):
    r"""The leaves of bbo_tree_walk, put in chain order, are bbo_tree_export_leaves; the walk's node and row counts match the
    counters."""
    for snap in S.replay(name)[0]:
        leaves = IMG.walk_leaves(snap["walk"])
        for key in ("ids", "ns", "cents", "ls"):
            assert leaves[key].shape == snap[key].shape and (leaves[key] == snap[key]).all(), key
        nodes = snap["walk"]["nodes"]
        assert len(nodes) == snap["stats"][5] and nodes[:, 0].max() >= snap["stats"][6]  # (the counter: the deepest descent so far)
        assert nodes[0, 0] == 1 and (nodes[0, 1] == 1) == (len(nodes) == 1)
        assert snap["walk"]["n"].shape[0] == nodes[:, 2].sum()


def test_walk_of_an_empty_tree():
    eng = T.make_oracle(S.never(5, 64))
    w = eng.walk()
    eng.close()
    assert w["nodes"].shape == (0, 4) and w["ls"].shape == (0, 64)
    IMG.check_walk(w, "empty")


def _planted(walk, what):
    w = {k: v.copy() for k, v in walk.items()}
    nodes = w["nodes"]
    start = np.concatenate([[0], np.cumsum(nodes[:, 2])])
    inner = int(np.flatnonzero(nodes[:, 1] == 0)[-1])  # an internal node: its row 0
    r = int(start[inner])
    if what == "sum":
        w["ls"][r, int(np.argmax(w["ls"][r]))] -= 1
    elif what == "n":
        w["n"][r] += 1
    elif what == "centroid":
        w["cent"][r, 0] ^= 0x80
    elif what == "popcount":
        w["pop"][r] += 1
    elif what == "chain":
        leaf = int(np.flatnonzero(nodes[:, 1] == 1)[0])
        nodes[leaf, 3] = nodes[int(np.flatnonzero(nodes[:, 1] == 1)[1]), 3]
    elif what == "id":
        w["id"][r] = 7
    return w


@pytest.mark.parametrize("what", ["sum", "n", "centroid", "popcount", "chain", "id"])
def test_invariant_checker_names_a_planted_fault(what):
    r"""One entry of a valid walk changed: a tracking row's linear sum off by one in one column (what a wrong by-difference
    sum leaves behind), its n_samples, its centroid, its popcount, two leaves on one chain position, a tracking row with an
    id."""
    walk = S.replay("lopsided-bf50")[0][-1]["walk"]
    assert IMG.walk_faults(walk) == []
    faults = IMG.walk_faults(_planted(walk, what))
    assert faults, what
    word = {"sum": "linear sum", "n": "n_samples", "centroid": "centroid", "popcount": "popcount", "chain": "chain", "id": "id"}[what]
    assert any(word in f for f in faults), faults
    with pytest.raises(AssertionError, match="differs"):
        IMG.same_walk(_planted(walk, what), walk)


def test_hand_built_image_walks():
    r"""Image.walk on the hand-built three-node image of tree_image_format.synthetic_image: an internal root over two leaves of
    two one-member rows each (their sums are their centroid rows), chain positions 0 and 1, tracking sums from cf32."""
    w = IMG.Image(bytearray(IMG.synthetic_image())).walk()
    assert w["nodes"].tolist() == [[1, 0, 2, -1], [2, 1, 2, 0], [2, 1, 2, 1]]
    assert w["n"].tolist() == [2, 2, 1, 1, 1, 1] and w["id"].tolist() == [IMG.NONE, IMG.NONE, 0, 1, 2, 3]
    assert (w["ls"][:2] == 1).all(), "the cf32 section of the hand-built image is all ones"
    assert w["ls"][2:].sum(axis=1).tolist() == [1, 1, 1, 1] and w["pop"][2:].tolist() == [1, 1, 1, 1]
    leaves = IMG.walk_leaves(w)
    assert leaves["ids"].tolist() == [0, 1, 2, 3]

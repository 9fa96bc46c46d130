r"""The cases of tree_threshold_cases.py against the conditions that make them worth running, on the C oracle alone (no GPU):
a case that stops deciding on the edge, or stops tying, tests nothing.  test_hip_tree_thresholds.py runs the same cases on the
GPU.  The oracle's bbo_tree_edge_counts says [merge decisions, those with a comparison of two equal float64 values, best-row
searches with a tied maximum > 0, those tied between different (inter, union) pairs]; the floors below are what the cases
reach (the measured value stands next to each), never under 300.

(a) on-edge cases decide >= 1000 merges (the floor of the case) on equal values, the grouped ones a quarter of all decisions
(b) one ulp (and more) above q no pure family case merges at all; the mixed ones still merge >= 1000 times
(c) the rows a case needs for the pipelined kernel to take the majority, declared here, counted on the GPU
(d) tie cases: >= 1000 searches tied between different (inter, union) pairs, trees of >= 3 levels at bf 50, and
    bbo_tree_tie_depths counts such ties at the internal levels as well as in the leaf nodes
(e) tier case: >= 40 on-edge merges with new_n > 255
(f) tolerance-legacy: the merge counts at tolerances 0.0, 1e-16 and 1e-15 differ pairwise (rounding alone tells them apart)
(g) radius criteria: the merge counts at the recurring value and one ulp above it differ
(h) tolerance-radius tables: the second comparison decides on equal values, the tree differs from the empty table's and from a
    read one entry up or down, clusters grow beyond tol_len"""
from __future__ import annotations

import numpy as np
import pytest

import tree_abi_cases as T
import tree_threshold_cases as H

MERGES, DEPTH = 2, 6  # indices into the seven counters


def merges(snap):
    return int(snap["stats"][MERGES])


def test_ulps_steps_through_adjacent_doubles():
    for x in (0.5, 1 / 3, 0.75, float.fromhex("0x1.fffffffffffffp-2")):
        assert H.ulps(x, 0) == x
        assert H.ulps(x, 1) == np.nextafter(x, 2.0) and H.ulps(x, -1) == np.nextafter(x, 0.0)
        assert H.ulps(H.ulps(x, 1000), -1000) == x


def test_ladder_stands_inside_on_the_edge_of_and_outside_the_band():
    r"""The pipelined kernel forms the quotient only within a relative 2^-48 of the threshold: 16 - 32 ulps for q in
    [0.25, 1).  8 is inside for every fraction, 24 inside or outside depending on it, 40 and 1000 outside."""
    inexact = 0
    for name, (c, p) in H.FRACTIONS.items():
        q = H.q_of(c, p)
        band = q * 2.0**-48 / (H.ulps(q, 1) - q)
        assert 0.25 <= q < 1 and 16 <= band <= 32, name
        inexact += q * (c + 2 * p) != c or (c + 2 * p) & (c + 2 * p - 1) != 0
    assert inexact >= 4 and H.q_of(*H.FRACTIONS["1/2"]) == 0.5
    assert set(H.LADDER) == {0, 1, -1, 8, -8, 24, -24, 40, -40, 1000, -1000}
    full = [fr for fr, _ in H.LADDER_PLAN]
    assert len([fr for fr in full if fr != "1/2"]) >= 3 and "1/2" in full
    bands = {fr: H.q_of(*H.FRACTIONS[fr]) * 2.0**-48 / (H.ulps(H.q_of(*H.FRACTIONS[fr]), 1) - H.q_of(*H.FRACTIONS[fr])) for fr in full}
    assert any(b < 24 for b in bands.values()) and any(b > 24 for b in bands.values()), "24 ulps falls on both sides of the edge"


def test_family_members_share_a_core_and_nothing_else():
    c, p, m = 12, 8, 20
    bits = np.unpackbits(H.families(3, 5, m, c, p, "grouped"), axis=1).astype(bool)
    for f in range(5):
        fam = bits[f * m:(f + 1) * m]
        assert (fam.sum(axis=1) == c + p).all()
        assert int(fam.all(axis=0).sum()) == c and int(fam.any(axis=0).sum()) == c + m * p
        # iSIM of any n members is c / (c + 2 p), from the oracle's own function
        lib = H.oracle_lib()
        for n in (2, 3, 7, m):
            ls = np.ascontiguousarray(fam[:n].sum(axis=0), dtype=np.uint64)
            assert lib.bbo_isim_from_sum(ls.ctypes.data, ls.size, n) == H.q_of(c, p)
    for order in H.ORDERS:
        rows = H.families(3, 5, m, c, p, order)
        assert sorted(r.tobytes() for r in rows) == sorted(r.tobytes() for r in np.packbits(bits, axis=1)), order
    inter = np.unpackbits(H.families(3, 5, m, c, p, "interleaved"), axis=1).astype(bool)
    assert (inter[:5] == bits[::m]).all(), "member 0 of every family first"


def test_block_rows_are_unions_of_whole_blocks():
    bits = np.unpackbits(H.tie_rows()[:2000], axis=1).reshape(2000, 32, 64)
    assert ((bits.sum(axis=2) == 0) | (bits.sum(axis=2) == 64)).all()
    per_row = bits.any(axis=2).sum(axis=1)
    assert per_row.min() >= 2 and per_row.max() <= 6 and len(set(per_row.tolist())) >= 4


# ---------------------------------------------------------------------------------------------------------------------
# (a), (b), (c): the threshold ladders
# ---------------------------------------------------------------------------------------------------------------------

# floor of edge_counts()[1] at the offset 0, by (kind, order); measured: grouped 22 761 - 22 796 (bf 50 / 254, every fraction),
# shuffled 1 431 (7/11, bf 50), interleaved 1 505 (1/3, bf 254), mixed 10 841 - 11 150
EDGE_FLOOR = {("pure", "grouped"): 22000, ("pure", "shuffled"): 1400, ("pure", "interleaved"): 1500, ("mixed", "grouped"): 10000}


@pytest.mark.parametrize("case", H.LADDER_CASES, ids=H.ladder_id)
def test_ladder_cases(case):
    fr, bf, crit, off, kind, order = case
    snap = H.replay_named("ladder", *case)
    decided, equal = snap["edge"][:2]
    n = sum(o.size for o in snap["out_leaf"])
    assert len(snap["out_leaf"]) == 3, "three fit_packed calls"
    # (c) 24 000 rows: the steady-state kernel's first stretch of 8 192 leaves the pipelined kernel the majority
    assert n >= 24000 and n - 8192 > n // 2
    assert decided >= n - 1000
    at_q = H.replay_named("ladder", fr, bf, crit, 0, kind, order)
    if off == 0:
        assert equal >= EDGE_FLOOR[(kind, order)], equal  # (a)
        if order == "grouped" and kind == "pure":
            assert equal * 4 >= decided
    elif crit == H.DIAMETER or (off > 0 and kind == "pure"):
        assert equal == 0, "off the edge by construction: nothing else in these rows sits within 1000 ulps of q"
    elif off < 0:
        # tolerance-diameter under q: new_dc >= old_dc - 0.0 still compares equal values (measured: grouped 21 563 / 21 595,
        # shuffled 335, mixed 16 212 / 16 848)
        assert equal >= (21000 if order == "grouped" and kind == "pure" else 300), equal
    if off > 0:  # (b)
        if kind == "pure":
            assert merges(snap) == 0
        else:
            assert 1000 <= merges(snap) < merges(at_q) - 1000
            assert int(snap["ns"].max()) > 255, "a duplicate run crossed the tier promotion"
        assert snap["stats"][4] > 0, "splits"
    if off < 0:
        assert merges(snap) == merges(at_q) and (snap["out_leaf"][-1] == at_q["out_leaf"][-1]).all()


@pytest.mark.parametrize("case", [("7/11", 50, H.DIAMETER, 0, "pure", "shuffled"), ("1/3", 254, H.DIAMETER, 0, "pure", "interleaved"),
                                  ("5/9", 50, H.DIAMETER, 0, "mixed", "grouped"), ("1/3", 50, H.DIAMETER, 0, "pure", "grouped")], ids=H.ladder_id)
def test_rows_behind_the_first_stretch_decide_on_the_edge(case):
    r"""(c) What the pipelined kernel gets - the rows after the steady-state kernel's first 8 192 - holds >= 1 000 on-edge
    decisions in every order (measured: 1 007, 1 077, 7 382, 14 988)."""
    c, ops = H.build("ladder", *case)
    rows = np.concatenate([op[1] for op in ops])
    eng = T.make_oracle(c)
    eng.fit_packed(rows[:8192])
    before = eng.edge_counts()[1]
    eng.fit_packed(rows[8192:])
    after = eng.edge_counts()[1]
    eng.close()
    assert after - before >= 1000, (before, after)
    assert after == H.replay_named("ladder", *case)["edge"][1]


@pytest.mark.parametrize("case", H.TOL_DIAMETER_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tolerance_tables_land_on_under_and_over(case):
    r"""`five`: clusters stop at four members (nT = 4 = tol_len - 1 reads -u: one ulp over); `four`: they grow on (nT >= 4 =
    tol_len reads 0.0: on the edge).  Both differ from the empty table's tree or equal it as the entries say."""
    fr, bf, name = case
    snap = H.replay_named("tol", *case)
    empty = H.replay_named("ladder", fr, bf, H.TOL_DIAMETER, 0, "pure", "grouped") if (fr, bf) in [("3/7", 50), ("5/9", 254)] else None
    q = H.q_of(*H.FRACTIONS[fr])
    tab = H.tol_tables(q)[name]
    assert q - tab[3] == H.ulps(q, -1) and q + tab[3] == H.ulps(q, 1) and tab[2] == 0.0, "entries of one ulp of q"
    assert snap["edge"][1] >= 20000  # measured: five 20 613 / 22 484, four 22 766 / 22 796
    if name == "five":
        assert len(tab) == 5 and int(snap["ns"].max()) == 4
        assert merges(snap) >= 4000  # measured 4 505 / 4 010
    else:
        assert len(tab) == 4 and int(snap["ns"].max()) == H.PIPE_M
        assert merges(snap) >= 22000
    if empty is not None:
        assert (merges(snap) == merges(empty)) == (name == "four")


# ---------------------------------------------------------------------------------------------------------------------
# (e) tier promotion on the edge
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bf,crit", H.TIER_CASES)
def test_tier_case_crosses_255_on_the_edge(bf, crit):
    rows, start = H.tier_rows()
    assert rows.shape[0] == (H.PIPE_K - 1) * H.PIPE_M + H.TIER_BIG and start > 8192, "behind the steady-state kernel's first stretch"
    snap = H.replay_named("tier", bf, crit)
    above = H.replay_named("tier", bf, crit, 1)
    assert merges(above) == 0, "every merge at q is decided on the edge"
    assert snap["edge"][1] >= 22000  # measured 23 064 / 23 095
    beyond = int(np.maximum(snap["ns"].astype(np.int64) - 255, 0).sum())  # single rows merge: one merge per member beyond 255
    assert beyond >= 40, beyond  # measured 65
    assert int(snap["ns"].max()) == H.TIER_BIG


# ---------------------------------------------------------------------------------------------------------------------
# (f) tolerance-legacy
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("bf", [50, 254])
def test_tolerance_legacy_counts_depend_on_rounding_alone(bf):
    count = {tol: merges(H.replay_named("legacy", bf, tol)) for tol in H.LEGACY_TOLERANCES}
    # measured: bf 50: 5 583 / 5 583 / 4 680 / 11 382, bf 254: 5 958 / 5 958 / 4 453 / 11 398
    assert len({count[0.0], count[1e-16], count[1e-15]}) == 3, count
    assert count[1e-17] == count[0.0], "1e-17 is under half an ulp of q"
    for tol in H.LEGACY_TOLERANCES:
        assert H.replay_named("legacy", bf, tol)["edge"][1] >= 10000, tol  # measured 10 339 - 11 398


# ---------------------------------------------------------------------------------------------------------------------
# (g) radius criteria
# ---------------------------------------------------------------------------------------------------------------------


def test_radius_values_recur_in_every_family():
    assert H.criterion_value(H.RADIUS, 2).hex() == "0x1.9999999999998p-1", "0.8 less two ulps: itself a rounding product"
    assert H.criterion_value(H.RADIUS, 3).hex() == "0x1.7777777777777p-1"
    lib = H.oracle_lib()
    bits = np.unpackbits(H.radius_rows()[:3 * H.RADIUS_M], axis=1).astype(np.uint64)
    for step in H.RADIUS_STEPS:
        for f in range(3):
            ls = np.ascontiguousarray(bits[f * H.RADIUS_M:f * H.RADIUS_M + step].sum(axis=0))
            assert lib.bbo_isim_radius_compl_from_sum(ls.ctypes.data, ls.size, step) == H.criterion_value(H.RADIUS, step)
    values = [H.criterion_value(H.RADIUS, s) for s in range(2, 21)]
    assert values == sorted(values, reverse=True) and len(set(values)) == len(values)


@pytest.mark.parametrize("case", [c for c in H.RADIUS_CASES if c[3] == 0], ids=lambda c: "-".join(map(str, c)))
def test_radius_counts_move_with_one_ulp(case):
    bf, crit, step, _, tab = case
    at, above, below = (H.replay_named("radius", bf, crit, step, off, tab) for off in (0, 1, -1))
    assert merges(at) != merges(above), (merges(at), merges(above))
    assert merges(below) == merges(at) and above["edge"][1] == 0 and below["edge"][1] == 0
    # measured at the step to 2: 3 581 / 3 547 (bf 5 / 17); to 3: 593 / 463; to 5: 461 / 451; to 9: 399 / 372
    assert at["edge"][1] >= (3000 if step == 2 else 350), at["edge"]


@pytest.mark.parametrize("case", H.RADIUS_WIDE, ids=lambda c: "-".join(map(str, c)))
def test_wide_radius_cases(case):
    snap = H.replay_named("radius", *case, "empty", True)
    assert snap["edge"][1] >= 3000 and snap["cents"].shape[1] == H.F // 8  # measured 3 645 / 3 403 at 400 families


@pytest.mark.parametrize("bf,tab", H.TOLRAD_CASES + H.TOLRAD_WIDE)
def test_tolerance_radius_tables_decide_the_second_comparison_on_the_edge(bf, tab):
    r"""The table is read, not uniform, and crossed: the tree differs from the empty table's and from what a read one entry up
    or down gives; every comparison of equal values is the second one (no family reaches the threshold's nine members);
    duplicate runs grow beyond tol_len on table reads of 0.0."""
    wide = (bf, tab) in H.TOLRAD_WIDE
    snap = H.replay_named("tolrad", bf, tab, wide)
    table = H.tolrad_tables()[tab]
    v = [H.criterion_value(H.RADIUS, n) for n in range(10)]
    assert v[2] - table[2] == v[3] and v[4] - table[4] == v[5], "on the edge"
    assert v[3] - table[3] == H.ulps(v[4], -1), "one ulp under"
    if tab == "six":
        assert v[5] - table[5] == H.ulps(v[6], 1), "one ulp over"
    assert len(set(table[2:])) == len(table) - 2, "no two entries alike"
    ns = snap["ns"].astype(np.int64)
    runs = H.RADIUS_K // H.TOLRAD_DUP_EVERY
    # families stop at five members: nT = tol_len - 1 refused one ulp over (six), nT = tol_len reads 0.0 (five); only the
    # duplicate runs (one of them may lose a row to a split) grow on, across tol_len
    assert not ((ns > 5) & (ns < H.TOLRAD_DUP_RUN - 2)).any() and (ns == 5).sum() >= 400
    assert (ns >= H.TOLRAD_DUP_RUN - 2).sum() >= runs - 2 and int(ns.max()) == H.TOLRAD_DUP_RUN > len(table)
    # measured: six 1 337 / 1 285 (bf 5 / 17), 1 213 wide; five 1 377 / 1 325
    assert snap["edge"][1] >= 1200, snap["edge"]
    assert merges(snap) >= 2400  # measured 2 837 / 2 733 / 2 432
    others = [H.replay_named("tolrad", bf, "none", wide)] + [H.replay_named("tolrad", bf, tab, wide, shift) for shift in (1, -1)]
    for other in others:
        assert merges(other) != merges(snap) and other["ns"].tolist() != snap["ns"].tolist()
    # `five` counts the duplicates' 1 >= 1 - 0.0 at nT = 5 = tol_len on top of what `six` counts
    if tab == "five" and not wide:
        assert snap["edge"][1] == H.replay_named("tolrad", bf, "six")["edge"][1] + runs


# ---------------------------------------------------------------------------------------------------------------------
# (d) ties
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", H.TIE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_tie_cases_tie_between_different_pairs(case):
    bf = case[0]
    snap = H.replay_named("tie", *case)
    assert snap["edge"][3] >= 1000, snap["edge"]  # measured 1 077 / 1 426 / 1 169
    assert snap["edge"][2] >= 10000 and snap["edge"][1] >= 4000  # measured 13 735 - 15 917 and 4 234 - 4 906: few rationals
    assert snap["stats"][DEPTH] >= (3 if bf == 50 else 2), "internal levels route as well"
    # ties between different pairs by the depth of the node searched; measured [2, 103, 972], [14, 1 412], [0, 68, 1 101]
    depth = int(snap["stats"][DEPTH])
    internal, leaves = sum(snap["tie_depths"][:depth - 1]), sum(snap["tie_depths"][depth - 1:])
    assert internal + leaves == snap["edge"][3] and leaves >= 900
    assert internal >= (60 if bf == 50 else 10), snap["tie_depths"]
    assert snap["stats"][MERGES] > 5000 and snap["stats"][4] > 50
    assert sum(o.size for o in snap["out_leaf"]) == H.TIE_N == 24000


# ---------------------------------------------------------------------------------------------------------------------
# buffers, the multi-tree launch, the pool-stop case
# ---------------------------------------------------------------------------------------------------------------------


def test_chunk_features_are_what_a_tree_of_the_chunk_holds():
    rng = np.random.default_rng(5)
    bits = H._family_bits(rng, 20, H.BUF_C, H.BUF_P, H.F)
    feats = H.chunk_features(bits, H.BUF_CHUNKS)
    lo = 0
    for row, size in zip(feats, H.BUF_CHUNKS):
        snap = T.replay(T.cfg(50, H.q_of(H.BUF_C, H.BUF_P), H.F), [("packed", np.packbits(bits[lo:lo + size], axis=1))])
        assert snap["leaf_count"] == 1 and (T.snapshot_rows(snap)[0] == row).all()
        lo += size


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("crit,bf", H.BUF_CASES)
def test_buffer_cases_decide_on_the_edge_with_several_members(crit, bf, width):
    c, ops = H.build("buffers", crit, bf, width)
    tab = np.concatenate([op[1] for op in ops])
    assert tab.dtype == T.W[width] and len(ops) == 2
    n_col = tab[:, -1].astype(np.int64)
    assert {1, 3, 4, 5, 7} <= set(n_col.tolist())
    snap = H.replay_named("buffers", crit, bf, width)
    radius = crit in (H.RADIUS, H.TOL_RADIUS)
    # measured: diameter 1 592 / 1 600, tolerance-diameter 1 599 / 1 607, tolerance-legacy 1 578 / 1 570, radius 319,
    # tolerance-radius 660 (both comparisons of the step to 13 and the second one of the step to 8)
    assert snap["edge"][1] >= (300 if radius else 1500), snap["edge"]
    assert merges(snap) >= (600 if radius else 1100)  # measured: radius 736, tolerance-radius 673
    if crit == H.TOL_RADIUS:
        assert snap["edge"][1] >= 600 and len(c["table"]) == 9 and (snap["ns"] == 13).sum() >= 300, "7 + 1 + 5 members: nT = 7 and 8 read"
    if width == 4 and not radius:
        assert (n_col == H.BUF_BIG // 2).sum() == 2 * (400 // H.BUF_BIG_EVERY), "buffers wider than uint8"
        assert (snap["ns"] == H.BUF_BIG).sum() >= 4, "300 + 300 merged on the edge"


def test_multi_and_pool_stop_cases_are_on_the_edge():
    assert len({c[0] for c in H.MULTI_CASES}) == 3 and {c[1] for c in H.MULTI_CASES} == {254}
    for case in H.MULTI_CASES + [H.TINY_CASE]:
        assert H.replay_named("ladder", *case)["edge"][1] >= 10000
    assert H.replay_named("ladder", *H.TINY_CASE)["stats"][4] > 100, "splits: nodes and slots run out again and again"


def test_compact_and_expand_are_inverse():
    snap = T.replay(T.cfg(5, 0.5, 64), [("packed", T.rows_near(1, 200, 64))])
    back = H.expand(H.compact(snap))
    T.same(back, snap)
    assert back["ls"].dtype == np.uint64 and back["ls"].shape == snap["ls"].shape

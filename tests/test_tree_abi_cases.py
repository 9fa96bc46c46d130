r"""The cases of tree_abi_cases.py against the conditions that make them worth running, on the C oracle alone (no GPU): a
case that does not reach what it is named for tests nothing.  test_hip_tree_abi_edges.py runs the same cases on the GPU."""
from __future__ import annotations

import numpy as np
import pytest

import tree_abi_cases as T


def leaves_of(snap):
    return dict(zip(snap["ids"].tolist(), snap["ns"].tolist()))


@pytest.mark.parametrize("name", list(T.RUN_TABLES))
def test_run_tables_hold_maximal_singleton_runs_of_the_stated_lengths(name):
    tab = T.run_table(name)
    assert tab.dtype == np.uint8 and tab.shape[1] == T.RUN_F + 1
    assert T.singleton_runs(tab[:, T.RUN_F]) == T.RUN_LENGTHS[name]
    singles = tab[tab[:, T.RUN_F] == 1]
    assert singles[:, :T.RUN_F].max(initial=0) <= 1
    assert (tab[:, :T.RUN_F] <= tab[:, T.RUN_F:]).all(), "ls[j] <= n_samples"
    if name != "one_run":
        st = T.replay(T.RUN_CFG, [("buffers", tab)])["stats"]
        assert st[2] > 0 and st[3] > 0 and st[4] > 0, "merges, appends and splits all happen"


def test_run_lengths_straddle_the_splitter_threshold():
    assert T.RUN_LENGTHS["mixed"] == [1023, 1024, 1025, 2100]
    assert T.RUN_TABLES["starts_long"][0] == ("s", 1500) and T.RUN_TABLES["ends_long"][-1] == ("s", 1300)
    assert T.RUN_LENGTHS["one_run"] == [1100] and T.RUN_LENGTHS["no_singleton"] == []
    assert T.RUN_TABLES["rewind"][:4] == [("m", 6), ("s", 1023), ("m", 1), ("s", 1030)]
    # slabs of 64 KB cut the long runs, slabs of 16 KB hold no run of 1024
    assert (64 << 10) // (T.RUN_F + 1) == 1008 and (16 << 10) // (T.RUN_F + 1) < 1024


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_tier_tables_cross_the_tier_boundaries(width):
    tab, pairs = T.tier_table(width)
    n_col = tab[:, T.TIER_F].astype(np.uint64)
    assert tab.dtype == T.W[width] and (n_col == 1).sum() > 50
    assert (tab[:, :T.TIER_F] <= tab[:, T.TIER_F:]).all()
    for special in (255, 256, 65535, 65536):
        assert (special in n_col.tolist()) == (special <= T.TIER_MAX_N[width])
    snap = T.replay(T.TIER_CFG, [("buffers", tab)])
    out, ns = snap["out_leaf"][0], leaves_of(snap)
    assert snap["stats"][2] > 0
    assert len(pairs) == (1 if width == 1 else 2)
    for a, b, n in pairs:
        assert out[a] == out[b], "the pair merged"
        assert ns[int(out[a])] >= 2 * n
    # 200 + 200 crosses 255 at every width; width 1 is no tier case beyond that: its n_samples column ends at 255 and
    # no pair of its rows reaches 65536 - the tier cases proper are the widths 2, 4 and 8
    assert any(256 <= n <= 65535 for n in ns.values())
    if width > 1:
        assert any(n >= 65536 for n in ns.values())


def test_pool_table_needs_more_uint8_slots_than_a_first_call_reserves():
    tab = T.pool_table()
    assert tab.dtype == np.uint64 and int(tab[:, 64].max()) <= 255 and int(tab[:, 64].min()) >= 2
    assert T.replay(T.POOL_CFG, [("buffers", tab)])["stats"][3] > 1500  # appended buffers; a first call reserves 1025 slots


def test_range_table_has_one_row_beyond_the_engine_limit():
    bad, good = T.range_tables()
    assert bad.dtype == np.uint64 and bad.shape == (11, 65) and int(bad[10, 64]) == 1 << 32 and int(bad[:10, 64].max()) < 256
    assert T.replay(T.RANGE_CFG, [("buffers", good)])["leaf_count"] > 1


@pytest.mark.parametrize("width", [1, 4])
def test_switch_tables(width):
    tab = T.switch_table(width)
    assert T.singleton_runs(tab[:, T.SWITCH_F]) == [1500, 500] and tab.shape[0] == 3000
    for bf in (50, 254):
        st = T.replay(T.switch_cfg(bf), [("buffers", tab)])["stats"]
        assert st[2] > 0 and st[3] > bf and st[4] > 0, (bf, st.tolist())


@pytest.mark.parametrize("extra", T.STRIDE_EXTRA)
def test_strided_views_end_with_their_allocation_and_span_the_slabs(extra):
    per = (T.STRIDE_SLAB_KB << 10) // (8 + extra)
    for slabs in (1, 2, 3):
        rows = T.stride_rows(extra, slabs)
        n = rows.shape[0]
        assert -(-n // per) == slabs and (slabs == 1 or n % per == 1)
        base, view = T.strided_view(rows, 8 + extra)
        assert base.nbytes == (n - 1) * (8 + extra) + 8 and (np.ascontiguousarray(view) == rows).all()
        assert T.replay(T.STRIDE_CFG, [("packed", rows)])["stats"][4] > 0


def test_misaligned_layouts():
    assert [(off | stride) % 16 == 0 for off, stride in T.MISALIGNED] == [False, False, True, False, False]
    assert all(stride >= 256 for _, stride in T.MISALIGNED)
    assert T.replay(T.MISALIGNED_CFG, [("packed", T.misaligned_rows())])["stats"][4] > 0


@pytest.mark.parametrize("bf,F", T.CORNERS)
def test_corner_trees_stay_within_the_engine_depth(bf, F):
    c, rows = T.corner_case(bf, F)
    snap = T.replay(c, [("packed", rows)])
    assert int(snap["stats"][6]) + 2 < 256
    assert snap["stats"][2] > 0 and snap["leaf_count"] > 1
    if bf == 2:
        assert snap["stats"][4] > 0 and snap["stats"][6] >= 3, "root splits"


def test_threshold_extremes():
    rows = T.threshold_rows()
    zero = T.replay(T.THRESHOLD_CASES[0.0], [("packed", rows)])
    one = T.replay(T.THRESHOLD_CASES[1.0], [("packed", rows)])
    assert zero["leaf_count"] == 1 and int(zero["ns"][0]) == rows.shape[0]
    seen, repeats = set(), 0
    for r in rows:
        repeats += r.tobytes() in seen
        seen.add(r.tobytes())
    assert 50 <= one["stats"][2] <= repeats and one["stats"][4] > 0, "only exact repeats merge at threshold 1.0"


def test_tolerance_table_matters_beyond_its_length():
    rows = T.tol_rows()
    snaps = {name: T.replay(c, [("packed", rows)]) for name, c in T.tol_cases().items()}
    for name, snap in snaps.items():
        assert int(snap["ns"].max()) > len(T.TOL_TABLE), name
    for crit in ("tol_diameter", "tol_radius"):
        assert snaps[crit]["ns"].tolist() != snaps[crit + "_null"]["ns"].tolist(), "the table changes the tree"


@pytest.mark.parametrize("which", ["packed", "buffers"])
def test_mixed_launch_trees_all_split(which):
    trees = T.mixed_packed() if which == "packed" else T.mixed_buffers()
    assert len({(c["bf"], c["F"]) for c, _, _ in trees.values()}) >= 4
    assert T.RADIUS in {c["crit"] for c, _, _ in trees.values()}
    if which == "buffers":
        assert {t.dtype.itemsize for _, _, t in trees.values() if t is not None} == {1, 2, 4, 8}
    for name, (c, before, data) in trees.items():
        if data is None:
            continue
        snap = T.replay(c, before + [(which, data)])
        assert snap["stats"][4] > 0, name


def test_gather_tree_holds_singletons_and_every_tier():
    snap = T.replay(T.GATHER_CFG, T.gather_ops())
    ns = snap["ns"]
    assert (ns == 1).any() and ((ns > 1) & (ns < 256)).any() and ((ns >= 256) & (ns < 65536)).any() and (ns >= 65536).any()
    assert snap["stats"][6] >= 2 and snap["leaf_count"] > 2 * T.GATHER_CFG["bf"], "at least three leaf nodes"
    # the narrow widths truncate: some linear sum does not fit them
    assert int(snap["ls"].max()) > 65535
    for pos in T.position_sets(snap["leaf_count"]).values():
        assert pos.min() >= 0 and pos.max() < snap["leaf_count"]


def test_chunk_tree_tells_the_second_launch_from_the_first():
    snap = T.replay(T.CHUNK_CFG, T.chunk_ops())
    k, bf = snap["leaf_count"], T.CHUNK_CFG["bf"]
    shift = (1 << 22) % k  # a second launch that read the first launch's nodes would be off by this many leaves
    assert bf < shift < k - bf, "further than a leaf node is long: another node"
    assert (snap["ns"] == 1).any() and (snap["ns"] == 2).any()
    assert len({r.tobytes() for r in T.snapshot_rows(snap)}) == k, "every leaf differs"


def test_refused_set_merge_cases_tell_old_settings_from_new():
    a, b = T.merge_rows(0), T.merge_rows(1)
    crit, tol, tab, thr = T.MERGE_NEW
    old = T.replay(T.MERGE_CFG, [("packed", a), ("packed", b)])
    new = T.replay(T.MERGE_CFG, [("packed", a), ("set_merge", crit, tol, tab, thr, T.MERGE_CFG["bf"]), ("packed", b)])
    assert old["stats"][6] >= 3, "several levels"
    assert old["out_leaf"][1].tolist() != new["out_leaf"][1].tolist() and old["ns"].tolist() != new["ns"].tolist()
    # each single setting on its own is visible as well: a partial application could not hide
    c = T.MERGE_CFG
    for op in [("set_merge", crit, c["tol"], c["table"], c["thr"], c["bf"]), ("set_merge", c["crit"], c["tol"], c["table"], thr, c["bf"]),
               ("set_merge", c["crit"], c["tol"], (), c["thr"], c["bf"])]:
        part = T.replay(T.MERGE_CFG, [("packed", a), op, ("packed", b)])
        assert part["out_leaf"][1].tolist() != old["out_leaf"][1].tolist(), op[1:5]
    # a branching factor change on the reset tree is visible too
    at7 = T.replay(T.MERGE_CFG, [("packed", a), ("reset",), ("set_merge", c["crit"], c["tol"], c["table"], c["thr"], 7), ("packed", b)])
    at4 = T.replay(T.MERGE_CFG, [("packed", a), ("reset",), ("packed", b)])
    assert at7["stats"].tolist() != at4["stats"].tolist()

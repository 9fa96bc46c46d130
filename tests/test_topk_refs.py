r"""The top-k reference against the order itself, and the case tables against what they are named for (no GPU)."""
from __future__ import annotations

import numpy as np
import pytest

import kernel_refs as R
import topk_refs as T


def ranges_of(nq, nc, k, fast=True):
    per, nsplit = T.topk_ranges(nq, nc, k, fast)
    return per, nsplit, [(s * per, min(nc, (s + 1) * per)) for s in range(nsplit)]


@pytest.mark.parametrize("nb,nq,nc,k", [(8, 40, 65, 64), (16, 40, 90, 12), (16, 3, 700, 64)])
def test_exact_topk_is_the_rational_order_small(nb, nq, nc, k):
    r"""Tie-heavy rows (8 and 16 bytes at density 1/2): the stable float64 argsort is the cross-multiplying order."""
    q, c = R.assign_inputs(nb, nq, nc)
    inter, union = T.counts(q, c)
    want = T.exact_topk(q, c, k)
    ties = sum(len(np.unique(row)) < len(row) for row in want[3])
    assert ties > 0
    assert (want[0] == T.python_topk(q, c, k)).all()
    ex = want[0][:, 0]
    assert (T.exact_topk(q, c, k, ex)[0] == T.python_topk(q, c, k, ex)).all()
    r = np.arange(nq)[:, None]
    assert (want[1] == inter[r, want[0]]).all() and (want[2] == union[r, want[0]]).all()


def test_exact_topk_is_the_rational_order_beyond_2048_bits():
    r"""65 600-bit rows: products pass 2^32, c[7] == c[5]; float64 ties are still the rational ties."""
    q, c = R.assign_wide_inputs(8200)
    nc = len(c)
    inter, union = T.counts(q, c)
    assert int(inter.max()) * int(union.max()) >= 1 << 32 and int(union.max()) < 1 << 26
    want = T.exact_topk(q, c, nc)
    assert (want[0] == T.python_topk(q, c, nc)).all()
    pos5, pos7 = (int(np.flatnonzero(want[0][2] == m)[0]) for m in (5, 7))
    assert (pos5, pos7) == (0, 1) and want[3][2][0] == want[3][2][1]
    ex = np.arange(len(q))
    assert (T.exact_topk(q, c, nc - 1, ex)[0] == T.python_topk(q, c, nc - 1, ex)).all()


def test_distinct_fractions_divide_to_distinct_doubles():
    r"""The bound the order argument rests on, at its edge: neighbours a / b and c / d with b, d < 2^26 differ by at least
    1 / (b d) > 2^-52, more than the spacing of doubles below 1."""
    b, d = (1 << 26) - 1, (1 << 26) - 2
    a = b - 1
    c = (a * d) // b  # the largest c with c / d <= a / b; the two differ
    assert a * d != c * b and np.float64(a) / np.float64(b) != np.float64(c) / np.float64(d)
    assert (np.float64(a) / np.float64(b) > np.float64(c) / np.float64(d)) == (a * d > c * b)


def test_split_case_has_several_ranges_and_a_straddling_tie():
    nb, nq, nc, k = T.SPLIT_CASE
    per, nsplit, rng = ranges_of(nq, nc, k)
    assert nsplit > 2 and per >= k
    q, c = T.assign_case(nb, nq, nc)
    want = T.exact_topk(q, c, k)
    owner = want[0] // per
    assert all(len(np.unique(o)) > 1 for o in owner)  # every query's answer comes from more than one range


def test_tiled_case_ties_straddle_range_boundaries():
    nb, nq, nc, k = T.TILED_CASE
    per, nsplit, _ = ranges_of(nq, nc, k)
    assert nsplit > 1 and per % 5 != 0  # a period of the tiling is cut by a boundary
    q, c = T.tiled_inputs()
    want = T.exact_topk(q, c, k)
    for i in range(nq):
        d = want[3][i]
        groups = [want[0][i][d == v] for v in np.unique(d)]
        assert all((np.diff(g) > 0).all() for g in groups)            # inside a tie group the index alone decides
        assert any(len(np.unique(g // per)) > 1 for g in groups)      # a tie group with members in different ranges


def test_short_range_case_has_a_range_shorter_than_k():
    nb, nq, nc, k = T.SHORT_RANGE_CASE
    per, nsplit, rng = ranges_of(nq, nc, k)
    assert nsplit > 1 and any(b - a < k for a, b in rng) and k <= nc


def test_nested_case_is_the_worst_and_the_best_of_the_list():
    _, nc, k = T.NESTED_CASE
    q, c = T.nested_inputs(False)
    inter, union = T.counts(q, c)
    assert (np.diff(inter[0] / union[0]) > 0).all()  # every row beats all before it
    assert (T.exact_topk(q, c, k)[0][0] == np.arange(nc - 1, nc - 1 - k, -1)).all()
    q, c = T.nested_inputs(True)
    assert (T.exact_topk(q, c, k)[0][0] == np.arange(k)).all()


def test_zero_case_orders_empty_unions_first():
    nb, nq, nc, k = T.ZERO_CASE
    q, c = T.zero_inputs()
    want = T.exact_topk(q, c, k)
    z = len(T.ZERO_ROWS)
    assert (want[0][:, :z] == np.array(T.ZERO_ROWS)).all() and (want[2][:, :z] == 0).all() and (want[3][:, :z] == 0).all()
    rest = [m for m in range(nc) if m not in T.ZERO_ROWS][: k - z]
    assert (want[0][:, z:] == np.array(rest)).all() and (want[3][:, z:] == 1.0).all()


def test_exclude_cases_hit_what_they_name():
    nb, nq, nc, k = T.EXCLUDE_SHAPE
    q, c, cases = T.exclude_inputs()
    plain = T.exact_topk(q, c, k)
    assert (cases["best row"] == plain[0][:, 0]).all()
    assert (T.exact_topk(q, c, k, cases["best row"])[0][:, 0] == T.exact_topk(q, c, k + 1)[0][:, 1]).all()
    for name in ("-1", "nc"):
        assert (T.exact_topk(q, c, k, cases[name])[0] == plain[0]).all()
    tie = cases["inside a tie group"]
    assert (tie >= 0).sum() >= nq // 2
    got = T.exact_topk(q, c, k, tie)[0]
    for i in np.flatnonzero(tie >= 0):
        assert tie[i] in plain[0][i] and tie[i] not in got[i]


def test_self_case_duplicates_are_each_others_first_neighbour():
    c = T.self_inputs()
    want = T.exact_topk(c, c, 5, np.arange(len(c)))
    for a, b in ((7, 30), (8, 50)):
        assert want[0][a, 0] == b and want[0][b, 0] == a and want[3][a, 0] == 0.0 and want[3][b, 0] == 0.0
    assert (want[0] != np.arange(len(c))[:, None]).all()


def test_fast_cases_cover_every_width_and_block_size():
    assert sorted({nb for nb, *_ in T.FAST_CASES}) == list(R.ASSIGN_FAST_WIDTHS)
    assert {T.topk_block(k) for *_, k in T.FAST_CASES} == {256, 64} and T.topk_block(T.OUTPUT_CASES[1][3]) == 64
    assert T.topk_block(T.LAYOUT_SHAPE[2]) == 128
    assert T.topk_ranges(513, 700, 64, True)[1] > 1 and T.topk_ranges(513, 700, 1, True)[1] > 1

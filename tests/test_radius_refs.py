r"""The radius-search reference against the semantics themselves, the table of smallest passing intersections against the
comparison it replaces, and the case tables against what they are named for (no GPU)."""
from __future__ import annotations

import numpy as np
import pytest

import kernel_refs as R
import radius_refs as X
import topk_refs as T

NBITS = 2048


@pytest.fixture(scope="module")
def all_pairs():
    r"""d[u, i] = fl((u - i) / u) for every 0 <= i <= u <= 2048 (0.0 at u = 0), +inf above the diagonal."""
    u = np.arange(NBITS + 1, dtype=np.float64)[:, None]
    i = np.arange(NBITS + 1, dtype=np.float64)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (u - i) / u
    d[0, 0] = 0.0
    d[i > u] = np.inf
    return d


def table_radii(d: np.ndarray) -> list[float]:
    r"""64 realised distances spread over every (i, u) (1 / 3, 2 / 3, 1 / 2 and the extremes among them), the float64
    neighbours of each on both sides, and the special radii."""
    rng = np.random.default_rng(45)
    us = rng.integers(1, NBITS + 1, 57)
    vals = [d[u, rng.integers(0, u + 1)] for u in us]
    vals += [d[3, 2], d[3, 1], d[2, 1], d[NBITS, NBITS - 1], d[NBITS, 1], d[2047, 1023], d[240, 160]]
    out = []
    for v in vals:
        out += [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]
    return out + [-0.0, 0.0, 1.0, -1e-300, 1 + 1e-9]


def test_imin_table_is_the_comparison(all_pairs):
    r"""i >= imin[u]  <=>  fl((u - i) / u) <= r, on every (i, u) with u <= 2048, at 197 radii."""
    i = np.arange(NBITS + 1)[None, :]
    u = np.arange(NBITS + 1)[:, None]
    valid = i <= u
    radii = table_radii(all_pairs)
    assert len(radii) == 197
    for r in radii:
        tab = X.imin_table(r, NBITS)
        assert tab.shape == (NBITS + 1,) and (tab >= 0).all() and (tab <= np.arange(NBITS + 1) + 1).all()
        want = all_pairs <= np.float64(r)
        got = (i >= tab[:, None]) & valid
        assert (got == want).all(), r


def test_imin_table_is_a_prefix_of_the_wider_table():
    r"""imin[u] does not depend on the row width: the 64-bit table is the start of the 2048-bit one."""
    for r in (0.3, 1 / 3, 0.0, -1.0, 1.0):
        assert (X.imin_table(r, 64) == X.imin_table(r, NBITS)[:65]).all()


def test_imin_table_special_radii():
    u = np.arange(NBITS + 1)
    assert (X.imin_table(-1.0, NBITS) == u + 1).all() and (X.imin_table(-1e-300, NBITS) == u + 1).all()
    assert (X.imin_table(1.0, NBITS) == 0).all() and (X.imin_table(float("inf"), NBITS) == 0).all()
    assert (X.imin_table(0.0, NBITS) == u).all() and (X.imin_table(-0.0, NBITS) == u).all()  # i == u, and the empty union
    assert (X.imin_table(float("-inf"), NBITS) == u + 1).all()


@pytest.mark.parametrize("nb,nq,nc", [(8, 20, 65), (16, 20, 90), (32, 9, 70), (100, 7, 30)])
def test_exact_radius_is_the_python_loop(nb, nq, nc):
    q, c = R.assign_inputs(nb, nq, nc)
    d = R.exact(q, c)[3]
    ex = (np.arange(nq) * 7) % nc
    for r in (-1.0, 0.0, 1.0, X.median_radius(nb, nq, nc), float(np.unique(d)[1])):
        for exclude in (None, ex):
            off, idx, inter, union, dist = X.exact_radius(q, c, r, exclude)
            want = X.python_radius(q, c, r, exclude)
            assert off[0] == 0 and off[-1] == len(idx) == sum(len(w) for w in want)
            assert [idx[off[a]:off[a + 1]].tolist() for a in range(nq)] == want
            ai, au = T.counts(q, c)
            rows = np.repeat(np.arange(nq), np.diff(off))
            assert (inter == ai[rows, idx]).all() and (union == au[rows, idx]).all()
            assert (R.bits(dist) == R.bits(d[rows, idx])).all()


def test_fixed_radii_mean_what_they_say():
    nb, nq, nc = 64, 257, 63
    q, c = X.assign_case(nb, nq, nc)
    assert X.exact_radius(q, c, -1.0)[0][-1] == 0
    assert X.exact_radius(q, c, 1.0)[0][-1] == nq * nc
    assert X.exact_radius(q, c, 1.0, np.arange(nq) % nc)[0][-1] == nq * (nc - 1)
    off, idx, inter, union, dist = X.exact_radius(q, c, 0.0)
    assert len(idx) > 0 and (union == 0).all()  # the all-zero query against the all-zero row, nothing else
    off, idx, inter, union, dist = X.exact_radius(q, c, X.median_radius(nb, nq, nc))
    assert 0.4 < len(idx) / (nq * nc) < 0.6


@pytest.mark.parametrize("nb", [32, 100])
@pytest.mark.parametrize("all_ones", [False, True])
def test_boundary_case_has_pairs_at_the_radius_and_just_above(nb, all_ones):
    q, c, n_set = X.boundary_inputs(nb, all_ones)
    assert q.shape == (1, nb) and c.shape == (241, nb)
    inter, union = T.counts(q, c)
    assert (union[0] == n_set).all() and (inter[0] == np.arange(241)).all()
    if all_ones and nb == 32:
        assert n_set == nb * 8  # u = nbits: the table's last entry
    d = R.exact(q, c)[3][0]
    realised = np.unique(d)
    values = X.boundary_values(n_set)
    assert len(values) == 10 and (1 / 3 in values) == (not all_ones)
    for v in values:
        lo, at, hi = X.boundary_radii(v)
        assert lo < at < hi and (d == at).sum() == 1  # a pair at the radius, bit for bit
        above = realised[realised > at]
        n_at = int(X.exact_radius(q, c, at)[0][-1])
        assert n_at == int(X.exact_radius(q, c, hi)[0][-1]) == int(X.exact_radius(q, c, lo)[0][-1]) + 1  # steps at v
        if len(above):  # ... and a pair at the next larger realised distance, which stays out
            nxt = int(np.flatnonzero(d == above[0])[0])
            assert nxt not in X.exact_radius(q, c, hi)[1]


def test_split_case_has_several_ranges_with_hits_on_both_sides_of_every_edge():
    nb, nq, nc = X.SPLIT_CASE
    per, nsplit = X.radius_ranges(nq, nc, True)
    assert nsplit > 2 and per % 5 != 0  # a period of the tiling is cut by an edge
    assert X.radius_ranges(nq, nc, False)[1] > 2
    q, c = X.split_inputs()
    r = X.split_radius()
    off, idx, *_ = X.exact_radius(q, c, r)
    assert (R.exact(q, c)[3] == r).any()
    hits = idx[off[0]:off[1]]
    assert 0 < len(hits) < nc
    for s in range(1, nsplit):
        edge = s * per
        assert ((hits >= edge - 5) & (hits < edge)).any() and ((hits >= edge) & (hits < edge + 5)).any()


def test_radius_ranges_is_the_assign_rule():
    r"""The same split as top-k's at workgroups of 256 lanes (k <= 8)."""
    for nq, nc in ((3, 700), (513, 700), (1, 1), (300, 130), (5000, 100000)):
        for fast in (True, False):
            assert X.radius_ranges(nq, nc, fast) == T.topk_ranges(nq, nc, 1, fast)


def test_exclude_cases_hit_what_they_name():
    q, c, cases, r = X.exclude_inputs()
    nq, nc = len(q), len(c)
    plain = X.exact_radius(q, c, r)
    per_query = lambda t: [t[1][t[0][a]:t[0][a + 1]].tolist() for a in range(nq)]  # noqa: E731
    base = per_query(plain)
    for name in ("-1", "nc"):
        assert per_query(X.exact_radius(q, c, r, cases[name])) == base
    removed = 0
    for name in ("best row", "inside a tie group"):
        got = per_query(X.exact_radius(q, c, r, cases[name]))
        for a in range(nq):
            e = int(cases[name][a])
            assert got[a] == [m for m in base[a] if m != e]
            removed += len(got[a]) < len(base[a])
    assert removed >= nq  # the excluded rows really were hits, in most queries


def test_self_case_keeps_the_duplicate_and_drops_the_row_itself():
    c = T.self_inputs()
    off, idx, inter, union, dist = X.exact_radius(c, c, 0.0, np.arange(len(c)))
    pairs = {(a, int(m)) for a in range(len(c)) for m in idx[off[a]:off[a + 1]]}
    assert pairs == {(7, 30), (30, 7), (8, 50), (50, 8)} and (dist == 0.0).all()


def test_cases_cover_every_width():
    assert [nb for nb, *_ in X.GENERIC_CASES if nb in R.ASSIGN_FAST_WIDTHS] == []
    assert X.GENERIC_CASES[1][0] * 8 > 2048 * 32
    assert all(nb in R.ASSIGN_FAST_WIDTHS for nb in (X.SPLIT_CASE[0], X.CAPACITY_CASE[0], X.EXCLUDE_SHAPE[0]))
    assert int(X.exact_radius(*X.assign_case(*X.CAPACITY_CASE), X.median_radius(*X.CAPACITY_CASE))[0][-1]) > 7

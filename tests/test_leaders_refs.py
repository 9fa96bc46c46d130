r"""CPU: the two references of the leader-clustering tests against each other (the sequential sphere exclusion and the
round / cover / tail / assignment formulation the device runs, with the tail forced after 0, 1 and 3 rounds and left to the
rounds alone), the defining properties on the adjacency matrix, and every named case of tests/leaders_refs.py against the
condition it is named for."""
from __future__ import annotations

import numpy as np
import pytest

import components_refs as C
import leaders_refs as L

NAMES = [name for name, _, _, _ in L.all_cases()]
VARIANTS = [(weighted, ties_high) for weighted in (False, True) for ties_high in (False, True)]


def test_case_names_are_unique():
    assert len(set(NAMES)) == len(NAMES) > 200
    assert {name for name, _, _ in C.all_cases()} <= set(NAMES)


def same(a, b):
    return (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2] and (a[3] == b[3]).all()


@pytest.mark.parametrize("name", NAMES)
def test_rounds_give_the_sequential_result(name):
    rows, r, w = L.case(name)
    adj = L.case_adjacency(name)
    for weighted, ties_high in VARIANTS:
        want = L.expected(name, weighted, ties_high)
        wv = L.weights_of(len(rows), w if weighted else None)
        for cap in (None, 0, 1, 3):
            got = L.rounds_of(adj, wv, ties_high, cap=cap)
            assert same(got, want), (name, weighted, ties_high, cap)
        got = L.rounds_of(adj, wv, ties_high, rule=True)
        assert same(got, want), (name, weighted, ties_high, "rule")


@pytest.mark.parametrize("name", NAMES)
def test_defining_properties(name):
    rows, r, w = L.case(name)
    n = len(rows)
    adj = L.case_adjacency(name)
    d = C.R.exact(rows, rows)[3]
    for weighted, ties_high in VARIANTS:
        centre, label, count, dens = L.expected(name, weighted, ties_high)
        wv = L.weights_of(n, w if weighted else None)
        assert centre.dtype == label.dtype == np.int32 and dens.dtype == np.uint64
        # density is the matrix product (exact: object integers)
        prod = adj.astype(object) @ np.array([int(x) for x in wv], object) + np.array([int(x) for x in wv], object)
        assert [int(x) for x in dens] == [int(x) for x in np.atleast_1d(prod)]
        order = L.priority_order(dens, ties_high)
        rank = np.empty(n, np.int64)
        rank[order] = np.arange(n)  # smaller = higher priority
        is_c = centre == np.arange(n)
        cs = np.flatnonzero(is_c)
        assert not adj[np.ix_(cs, cs)].any()  # no two centres are adjacent
        for v in range(n):
            nb = np.flatnonzero(adj[v])
            higher_centres = [u for u in nb if is_c[u] and rank[u] < rank[v]]
            assert is_c[v] == (not higher_centres), (name, v)  # a centre iff no higher-priority neighbour is one
            if not is_c[v]:
                cn = [u for u in nb if is_c[u]]
                assert centre[v] == min(cn, key=lambda u: rank[u])  # the highest-priority neighbouring centre
                assert d[v, centre[v]] <= np.float64(r)  # within the radius of it
        assert count == len(cs) and (label[cs] == np.arange(count)).all() and (label == label[centre]).all()


def test_monotone_path_needs_many_rounds():
    rows, r, _ = L.case(L.MONOTONE)
    assert len(rows) == 513
    *_, rounds = L.leaders_by_rounds(rows, r)
    assert rounds >= 200
    trace = {}
    *_, rounds = L.leaders_by_rounds(rows, r, rule=True, trace=trace)
    assert rounds <= 4 and trace["steps"] > 400  # the built-in rule steps


@pytest.mark.parametrize("radius", C.BLOCK_RADII[1:4])
def test_block_model_needs_few_rounds(radius):
    rows = C.block_rows()
    for weighted, ties_high in VARIANTS:
        w = L.case(f"block {radius}")[2] if weighted else None
        *_, rounds = L.leaders_by_rounds(rows, radius, w, ties_high)
        assert rounds <= 5
        trace = {}
        *_, ruled = L.leaders_by_rounds(rows, radius, w, ties_high, rule=True, trace=trace)
        assert ruled == rounds and trace["steps"] == 0  # the built-in rule never steps here


def test_late_better_centre():
    rows, r, _ = L.case(L.LATE)
    trace = {}
    centre, label, count, dens, rounds = L.leaders_by_rounds(rows, r, trace=trace)
    assert [int(dens[v]) for v in (L.LATE_Y, L.LATE_X, L.LATE_C, L.LATE_M, L.LATE_B)] == [7, 6, 5, 3, 4]
    pos = trace["pos"]
    first = int(trace["aidx"][trace["first_cover"][int(pos[L.LATE_M])]])
    assert first == L.LATE_B and centre[L.LATE_M] == L.LATE_C and centre[L.LATE_C] == L.LATE_C and rounds >= 3
    assert centre[L.LATE_X] == L.LATE_Y and centre[L.LATE_B] == L.LATE_B


def test_member_next_to_a_lower_priority_centre():
    rows, r, _ = L.case(L.LOWER)
    centre, _, _, dens = L.expected(L.LOWER, False, False)
    assert centre[1] == 0 and centre[2] == 2 and dens[1] > dens[2]
    assert L.case_adjacency(L.LOWER)[1, 2]


def test_the_flips_flip():
    plain = L.expected(L.WEIGHTS_FLIP, False, False)
    heavy = L.expected(L.WEIGHTS_FLIP, True, False)
    assert plain[0].tolist() == [1, 1, 1, 1, 4] and heavy[0].tolist() == [0, 0, 2, 3, 0]
    low = L.expected(L.TIES_FLIP, False, False)
    high = L.expected(L.TIES_FLIP, False, True)
    k = C.BRIDGE_COPIES
    assert (low[0] == np.repeat([0, k], k)).all() and (high[0] == np.repeat([k - 1, 2 * k - 1], k)).all()
    assert low[2] == high[2] == 2 and (low[1] == high[1]).all()


def test_zero_weights():
    r"""Rows of weight 0 that have neighbours: the density cannot say who has a neighbour."""
    rows, r, w = L.case(L.ZERO_WEIGHTS)
    adj = L.case_adjacency(L.ZERO_WEIGHTS)
    dens = L.expected(L.ZERO_WEIGHTS, True, False)[3]
    assert ((dens == 0) & adj.any(1)).any()
    dens = L.expected(L.ALL_ZERO_WEIGHTS, True, False)[3]
    assert (dens == 0).all() and L.case_adjacency(L.ALL_ZERO_WEIGHTS).any()
    assert L.expected(L.ALL_ZERO_WEIGHTS, True, False)[2] < 257


def test_graph_rows():
    rows = L.graph_rows([(0, 1), (1, 2)], 4, 2)
    d = C.R.exact(rows, rows)[3]
    assert (L.adjacency(rows, L.GRAPH_R) == np.array([[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 0]], bool)).all()
    assert d[0, 2] == 1.0 and d[0, 3] == 1.0 and d[0, 1] < 1.0


def test_degenerate_radii():
    rows, _, _ = L.case("degenerate r = -0.0")
    n = len(rows)
    none = L.exact_leaders(rows, -1e-300)
    assert (none[0] == np.arange(n)).all() and none[2] == n and (none[3] == 1).all()
    one = L.exact_leaders(rows, 1.0, ties_high=True)
    assert (one[0] == n - 1).all() and one[2] == 1 and (one[3] == n).all()
    assert L.exact_leaders(rows, 1.0)[0].tolist() == [0] * n
    assert same(L.exact_leaders(rows, -0.0), L.exact_leaders(rows, 0.0)) and L.exact_leaders(rows, 0.0)[2] == 3
    assert L.exact_leaders(rows[:0], 0.3)[2] == 0

r"""CPU: the reference of the connected-components tests against scipy, and every case of tests/components_refs.py against
the condition it is named for."""
from __future__ import annotations

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import components_refs as C
import kernel_refs as R
import radius_refs as X

CASES = {name: (rows, r) for name, rows, r in C.all_cases()}


def test_case_names_are_unique():
    assert len(CASES) == sum(1 for _ in C.all_cases()) > 150


@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_scipy_s(name):
    r"""The same count and the same label array as connected_components on the dense d <= r; roots are the minima."""
    rows, r = CASES[name]
    roots, labels, count = C.expected(name)
    n, want = connected_components(csr_matrix(C.linked(rows, r)), directed=False)
    assert count == n and labels.dtype == roots.dtype == np.int32 and (labels == want).all()
    for lab in range(count):
        members = np.flatnonzero(labels == lab)
        assert (roots[members] == members[0]).all()
    firsts = np.unique(roots)
    assert len(firsts) == count and (labels[firsts] == np.arange(count)).all()


@pytest.mark.parametrize("order", C.CHAIN_ORDERS)
def test_chain(order):
    rows = C.chain_rows(order)
    assert rows.shape == (C.CHAIN_N, C.CHAIN_NB)
    d = R.exact(rows, rows)[3]
    np.fill_diagonal(d, 9.0)
    near = np.sort(np.unique(d))[:2]
    assert near[0] == 0.4 == C.CHAIN_D and near[1] == 2 / 3  # the next distance up
    assert ((d == 0.4).sum(1) == 2).sum() == C.CHAIN_N - 2 and ((d == 0.4).sum(1) == 1).sum() == 2
    for r, count in C.CHAIN_RADII.items():
        assert C.expected(f"chain {order} {r!r}")[2] == count
    assert list(C.CHAIN_RADII.values()) == [1, 1, 513]


@pytest.mark.parametrize("hub", C.STAR_HUBS)
def test_star(hub):
    rows = C.star_rows(hub)
    assert rows.shape == (C.STAR_LEAVES + 1, C.STAR_NB)
    d = R.exact(rows, rows)[3]
    leaves = np.delete(np.arange(len(rows)), hub)
    assert (R.bits(d[hub, leaves]) == R.bits(np.float64(C.STAR_R))).all()  # 2044 / 2046 and 1022 / 1023: one double
    ll = d[np.ix_(leaves, leaves)]
    assert (ll[~np.eye(len(leaves), dtype=bool)] == 1.0).all()
    assert C.expected(f"star hub {hub} {C.STAR_R!r}")[2] == 1
    assert C.expected(f"star hub {hub} {C.below(C.STAR_R)!r}")[2] == C.STAR_LEAVES + 1


def test_bridge():
    for at in C.BRIDGE_AT:
        rows = C.bridge_rows(at)
        assert len(rows) == 2 * C.BRIDGE_COPIES + 1 and np.unpackbits(rows[at]).sum() == 200
        assert C.expected(f"bridge C at {at}")[2] == 1
    roots, labels, count = C.expected("bridge C at None")
    assert count == 2 and (roots == np.repeat([0, C.BRIDGE_COPIES], C.BRIDGE_COPIES)).all()
    assert C.BRIDGE_AT == (0, 255, 256, 600)


def test_block_model():
    r"""The recorded counts, and at least three radii with a count strictly between the centres and the rows."""
    assert C.block_rows().shape == (C.BLOCK_N, C.BLOCK_NB)
    counts = tuple(C.expected(f"block {r}")[2] for r in C.BLOCK_RADII)
    assert counts == C.BLOCK_COUNTS
    assert sum(C.BLOCK_CENTRES < k < C.BLOCK_N for k in counts) >= 3
    assert C.BLOCK_RADII == (0.1, 0.13, 0.14, 0.15, 0.2)


@pytest.mark.parametrize("nb", C.BOUNDARY_WIDTHS)
@pytest.mark.parametrize("all_ones", [False, True])
def test_boundaries(nb, all_ones):
    tables = C.boundary_tables(nb, all_ones)
    assert len(tables) == X.BOUNDARY_VALUES == 10
    if not all_ones:
        assert any(v == float(np.float64(1) / np.float64(3)) for v, _ in tables)
    for v, rows in tables:
        assert rows.shape == (3, nb)
        assert R.bits(R.exact(rows[2:], rows[:1])[3])[0, 0] == R.bits(np.float64(v)).reshape(-1)[0]
        counts = tuple(C.expected(f"boundary {nb} {all_ones} {r!r}")[2] for r in X.boundary_radii(v))
        assert counts == C.BOUNDARY_COUNTS


@pytest.mark.parametrize("name", list(C.DEGENERATE))
def test_degenerate(name):
    rows, r, count = C.DEGENERATE[name]
    assert C.expected(f"degenerate {name}")[2] == count


def test_degenerate_covers_the_list():
    sizes = {len(rows) for rows, _, _ in C.DEGENERATE.values()}
    radii = {int(R.bits(np.float64(r)).reshape(-1)[0]) for _, r, _ in C.DEGENERATE.values()}
    assert {1, 2} <= sizes
    for r in (0.0, -0.0, -1e-300, 1 + 1e-9, 1.0, C.below(1.0)):
        assert int(R.bits(np.float64(r)).reshape(-1)[0]) in radii


@pytest.mark.parametrize("nb", C.FAST_WIDTHS + C.GENERIC_WIDTHS)
def test_widths(nb):
    r"""Neither trivial at the middle radius: some rows tied, some alone."""
    rows = C.width_rows(nb)
    assert rows.shape == (C.WIDTH_N, nb) and not rows[77].any() and (rows[201] == rows[5]).all()
    radii = C.width_radii(nb)
    counts = [C.expected(f"width {nb} {r!r}")[2] for r in radii]
    assert counts[-1] == 1 and counts[0] < C.WIDTH_N
    assert 1 < counts[-2] < C.WIDTH_N  # (the median radius; 0 at one byte, where it is 0)
    assert C.FAST_WIDTHS == (8, 16, 32, 64, 128, 256) and C.GENERIC_WIDTHS == (1, 3, 24, 100, 257, 1024, 8192)

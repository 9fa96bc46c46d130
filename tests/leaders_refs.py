r"""Reference and cases of the leader-clustering tests (bblean_amd/csrc/bb_leaders.hip).  TEST INFRASTRUCTURE.
test_hip_leaders_edges.py / test_hip_leaders.py (GPU) compare the library with `exact_leaders`, the sequential sphere
exclusion; test_leaders_refs.py (CPU) holds it against `leaders_by_rounds`, the round / cover / tail / assignment
formulation that the device runs, checks the defining properties on the adjacency matrix and that every named case meets
the condition it is named for.  The distances are kernel_refs.exact's (integers until the one float64 division); nothing
here has a tolerance."""
from __future__ import annotations

import functools
import zlib

import numpy as np

import components_refs as C

UNDECIDED, CENTRE, MEMBER = 0, 1, 2


def adjacency(rows: np.ndarray, r: float) -> np.ndarray:
    r"""The n x n boolean neighbour matrix: d <= r off the diagonal."""
    adj = C.linked(rows, r).copy() if len(rows) else np.zeros((0, 0), bool)
    np.fill_diagonal(adj, False)
    return adj


def weights_of(n: int, weights) -> np.ndarray:
    return np.ones(n, np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)


def density_of(adj: np.ndarray, w: np.ndarray) -> np.ndarray:
    r"""w[a] + the weights of a's neighbours, exact (Python integers)."""
    wl = [int(x) for x in w]
    return np.array([wl[a] + sum(wl[b] for b in np.flatnonzero(adj[a])) for a in range(len(wl))], np.uint64).reshape(len(wl))


def priority_order(dens: np.ndarray, ties_high: bool) -> np.ndarray:
    r"""The rows, highest priority first: density descending, then the lower (ties_high: the higher) row."""
    n = len(dens)
    return np.array(sorted(range(n), key=lambda v: (-int(dens[v]), -v if ties_high else v)), np.int64).reshape(n)


def labels_of(centre: np.ndarray):
    n = len(centre)
    is_c = centre == np.arange(n)
    rank = np.cumsum(is_c) - is_c
    return rank[centre].astype(np.int32), int(is_c.sum())


def leaders_of(adj: np.ndarray, w: np.ndarray, ties_high: bool = False):
    r"""The sequential procedure on an adjacency matrix: walk the rows in priority order; a row not yet taken becomes a
    centre and takes all of its neighbours that are not yet taken.  -> (centre int32, label int32, count, density uint64)"""
    n = len(adj)
    dens = density_of(adj, w)
    centre = np.full(n, -1, np.int32)
    for v in priority_order(dens, ties_high).tolist():
        if centre[v] >= 0:
            continue
        centre[v] = v
        centre[adj[v] & (centre < 0)] = v
    label, count = labels_of(centre)
    return centre, label, count, dens


def exact_leaders(rows: np.ndarray, r: float, weights=None, ties_high: bool = False):
    n = len(rows)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.zeros(0, np.uint64)
    return leaders_of(adjacency(rows, r), weights_of(n, weights), ties_high)


def rounds_of(adj: np.ndarray, w: np.ndarray, ties_high: bool = False, cap=None, rule: bool = False, trace=None):
    r"""The formulation of the device.  The rows with a neighbour, in priority order, are the positions; a round is a cover
    pass (undecided rows next to a centre of the round before become members) and a block pass (a still-undecided row with
    a still-undecided neighbour at a smaller position is blocked; the others become centres).  `cap`: the tail starts
    after that many rounds (None: never, unless `rule`, the library's built-in rule: two consecutive rounds that together
    decided less than 1 / 64 of the rows undecided before them).  The tail: one more cover pass, then the remaining
    positions one by one.  The assignment is a pass of its own.  -> (centre, label, count, density, rounds run).
    `trace`: a dict that receives "first_cover" (position -> the first centre position that covered it), "pos" (row ->
    position), "steps" (rows that entered the tail)."""
    n = len(adj)
    dens = density_of(adj, w)
    centre = np.arange(n, dtype=np.int32)
    order = priority_order(dens, ties_high)
    aidx = order[adj.any(1)[order]]
    na = len(aidx)
    A = adj[np.ix_(aidx, aidx)]
    state = np.zeros(na, np.int8)
    U = np.arange(na)
    newc = np.zeros(0, np.int64)
    first_cover: dict[int, int] = {}

    def cover():
        if len(newc) and len(U):
            hit = A[np.ix_(U, newc)]
            got = hit.any(1)
            for p, k in zip(U[got].tolist(), hit[got].argmax(1).tolist()):
                first_cover.setdefault(p, int(newc[k]))
            state[U[got]] = MEMBER

    rounds, before_last = 0, -1
    while len(U):
        if cap is not None and rounds >= cap:
            break
        nu = len(U)
        cover()
        und = U[state[U] == UNDECIDED]
        blocked = np.tril(A[np.ix_(und, und)], -1).any(1)
        newc = und[~blocked]
        state[newc] = CENTRE
        U = und[blocked]
        assert len(U) < nu, "a round decided nothing"  # (the first undecided row is never blocked)
        rounds += 1
        slow = before_last >= 0 and (before_last - len(U)) * 64 < before_last
        before_last = nu
        if cap is None and rule and slow:
            break
    steps = len(U)
    if len(U):
        cover()
        for v in U.tolist():
            if state[v] != UNDECIDED:
                continue
            state[v] = CENTRE
            later = U[U > v]
            state[later[A[v, later] & (state[later] == UNDECIDED)]] = MEMBER
    cpos = np.flatnonzero(state == CENTRE)
    mpos = np.flatnonzero(state == MEMBER)
    assert len(cpos) + len(mpos) == na
    if len(mpos):
        hit = A[np.ix_(mpos, cpos)]
        assert hit.any(1).all()
        centre[aidx[mpos]] = aidx[cpos[hit.argmax(1)]]
    if trace is not None:
        pos = np.full(n, -1, np.int64)
        pos[aidx] = np.arange(na)
        trace.update(first_cover=first_cover, pos=pos, steps=steps, aidx=aidx)
    label, count = labels_of(centre)
    return centre, label, count, dens, rounds


def leaders_by_rounds(rows: np.ndarray, r: float, weights=None, ties_high: bool = False, cap=None, rule: bool = False, trace=None):
    n = len(rows)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0, np.zeros(0, np.uint64), 0
    return rounds_of(adjacency(rows, r), weights_of(n, weights), ties_high, cap, rule, trace)


# ---------------------------------------------------------------------------------------------------------------------
# any small graph as rows: vertex v has the private bit v (without it two empty rows would be at distance 0), edge e a
# private bit n + e that its two ends share.  Adjacent rows are below 1, all others at exactly 1: GRAPH_R gives the graph.
# ---------------------------------------------------------------------------------------------------------------------
GRAPH_R = C.below(1.0)


def graph_rows(edges, n: int, nb: int) -> np.ndarray:
    edges = list(edges)
    assert n + len(edges) <= nb * 8 and all(0 <= a < n and 0 <= b < n and a != b for a, b in edges)
    sets = [[v] for v in range(n)]
    for e, (a, b) in enumerate(edges):
        sets[a].append(n + e)
        sets[b].append(n + e)
    return C.bit_rows(sets, nb)


def _with_leaves(path_edges, n_path: int, leaves):
    r"""`leaves[v]` pendant vertices on path vertex v, numbered after the path."""
    edges = list(path_edges)
    nxt = n_path
    for v, k in enumerate(leaves):
        for _ in range(k):
            edges.append((v, nxt))
            nxt += 1
    return edges, nxt


# late better centre: the path y - x - c - m - b (vertices 0 .. 4) with 5, 3, 2, 0, 2 leaves: densities 7, 6, 5, 3, 4, so
# y > x > c > b > m.  Round 1 makes y and b centres, round 2 covers x and m (m under b), round 3 makes c a centre, and m
# belongs to c.
LATE_Y, LATE_X, LATE_C, LATE_M, LATE_B = range(5)


def late_rows() -> np.ndarray:
    edges, n = _with_leaves([(0, 1), (1, 2), (2, 3), (3, 4)], 5, (5, 3, 2, 0, 2))
    return graph_rows(edges, n, 8)


# member next to a lower-priority centre: c1 (3 leaves) - v - c2.  c1 takes v; c2, whose only neighbour is a member, is a
# centre of lower priority than v.
def lower_rows() -> np.ndarray:
    edges, n = _with_leaves([(0, 1), (1, 2)], 3, (3, 0, 0))
    return graph_rows(edges, n, 3)


# weights flip the centre: b (1) is next to a, c, d; a (0) also to e (4).  Unweighted b leads a, c and d and e is alone;
# with 100 molecules in e, a leads b and e.
def flip_rows() -> np.ndarray:
    return graph_rows([(0, 1), (1, 2), (1, 3), (0, 4)], 5, 16)


FLIP_WEIGHTS = np.array([1, 1, 1, 1, 100], np.uint32)

SMALL_BLOCK_NS = (1, 2, 63, 64, 65, 255, 256, 257, 513)
SMALL_BLOCK_R = 0.15


@functools.lru_cache(maxsize=None)
def small_block_rows(n: int) -> np.ndarray:
    r"""n rows of 32 bytes around 6 random centres, every bit flipped with probability 0.04."""
    rng = np.random.default_rng([6006, n])
    centres = rng.integers(0, 2, (6, 256), dtype=np.uint8)
    flip = (rng.random((n, 256)) < 0.04).astype(np.uint8)
    return np.packbits(centres[rng.integers(0, 6, n)] ^ flip, axis=1)


def case_weights(name: str, n: int) -> np.ndarray:
    r"""The weights of a case's weighted variant: small values (ties stay common), zeros and the largest uint32."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return rng.choice(np.array([0, 1, 1, 2, 3, 7, 2 ** 32 - 1], np.uint32), n)


MONOTONE = "monotone path"
LATE = "late better centre"
LOWER = "member next to a lower-priority centre"
WEIGHTS_FLIP = "weights flip the centre"
TIES_FLIP = "ties flip the centre"
ZERO_WEIGHTS = "zero weights on rows with neighbours"
ALL_ZERO_WEIGHTS = "all weights zero"


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for name, rows, r in C.all_cases():
        out.append((name, rows, r, case_weights(name, len(rows))))
    for n in SMALL_BLOCK_NS:
        name = f"small block {n}"
        out.append((name, small_block_rows(n), SMALL_BLOCK_R, case_weights(name, n)))
    chain = C.chain_rows("ascending")
    out.append((MONOTONE, chain, C.CHAIN_D, case_weights(MONOTONE, len(chain))))
    out.append((LATE, late_rows(), GRAPH_R, case_weights(LATE, len(late_rows()))))
    out.append((LOWER, lower_rows(), GRAPH_R, case_weights(LOWER, len(lower_rows()))))
    out.append((WEIGHTS_FLIP, flip_rows(), GRAPH_R, FLIP_WEIGHTS))
    bridge = C.bridge_rows(None)
    out.append((TIES_FLIP, bridge, C.BRIDGE_R, case_weights(TIES_FLIP, len(bridge))))
    zw = np.ones(len(chain), np.uint32)
    zw[::3] = 0
    zw[100:140] = 0
    out.append((ZERO_WEIGHTS, C.chain_rows("permuted"), C.CHAIN_D, zw))
    out.append((ALL_ZERO_WEIGHTS, small_block_rows(257), SMALL_BLOCK_R, np.zeros(257, np.uint32)))
    same = np.ascontiguousarray(np.repeat(C.bit_rows([range(3, 40)], 16), 70, axis=0))
    out.append(("all rows identical", same, 0.0, case_weights("all rows identical", 70)))
    out.append(("all-zero rows", np.zeros((70, 24), np.uint8), 0.0, case_weights("all-zero rows", 70)))
    for _, rows, _, w in out:
        rows.flags.writeable = False
        w.flags.writeable = False
    return tuple(out)


def all_cases():
    r"""Every (name, rows, radius, weights) of this file; a case runs with its weights and without."""
    return iter(_cases())


@functools.lru_cache(maxsize=None)
def case(name: str):
    for nm, rows, r, w in _cases():
        if nm == name:
            return rows, r, w
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_adjacency(name: str) -> np.ndarray:
    rows, r, _ = case(name)
    adj = adjacency(rows, r)
    adj.flags.writeable = False
    return adj


@functools.lru_cache(maxsize=None)
def expected(name: str, weighted: bool, ties_high: bool):
    r"""exact_leaders of a case, computed once and shared (read-only)."""
    rows, r, w = case(name)
    out = leaders_of(case_adjacency(name), weights_of(len(rows), w if weighted else None), ties_high)
    for a in (out[0], out[1], out[3]):
        a.flags.writeable = False
    return out

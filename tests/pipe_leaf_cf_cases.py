r"""Inputs of tests/test_hip_pipe_leaf_cf.py: tails behind the prefix of tests/pipe_forward_cases.py (which hands the tree to the
pipelined kernel) that take the branches of the leaf engine's cluster-feature path (bb_tree_pipe.inc, pipe_leaf).

The leaf engine picks the best row of the leaf from the helper wave's pre-compare (rows that changed since are compared again),
gets the row's uint8 cluster features from its LDS cache of eight entries or from HBM, and merges with the majority vote taken
four bytes at a time (bb_pipe_bytes.h).  All cases: 2048 bits, branching factor 50, diameter criterion,
threshold pipe_forward_cases.THR, 9 692 + at most 3 000 rows.  TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import functools

import numpy as np

from pipe_forward_cases import F, _pack


def _disjoint(rng, *sizes):
    idx = rng.permutation(F)
    out, at = [], 0
    for s in sizes:
        out.append(idx[at:at + s]); at += s
    return out


def _row(*index_sets) -> np.ndarray:
    r = np.zeros(F, bool)
    for s in index_sets:
        r[s] = True
    return r


@functools.lru_cache(maxsize=None)
def stale_best_row() -> np.ndarray:
    r"""Groups over a core c of 400 bits.  First, for every group: a = c + s1 (300 bits), a2 = a with three bits toggled
    (merges: A is a pair with a uint8 row of its own) and b = c + s2 (300 other bits; Tanimoto 0.4 with a, and {a, a2, b} is
    below the threshold as a set: a BitFeature of its own).  By the time the second part comes, A's cluster features have left
    the leaf engine's LDS cache (eight entries).  Then for every group y = b + t (100 fresh bits; 700 / 800 with b: merges,
    the pair's centroid is b | y) directly followed by z = c + t + 40 bits of s1: 440 / 800 = 0.55 with A, 400 / 840 = 0.476
    with b as it was, 500 / 840 = 0.595 with b | y.  A pre-compare of z that ran before y's merge was written has A ahead;
    the compare behind the merge must end at B (whose cluster features are in the LDS cache).  Last, for every group a3 = a
    with three bits toggled: it merges into A, whose cluster features come from HBM."""
    rng = np.random.default_rng(41)
    groups = 110
    first, second, third = [], [], []
    for _ in range(groups):
        c, s1, s2, t = _disjoint(rng, 400, 300, 300, 100)
        a = _row(c, s1)
        a2, a3 = a.copy(), a.copy()
        a2[rng.integers(0, F, 3)] ^= True
        a3[rng.integers(0, F, 3)] ^= True
        first += [a, a2, _row(c, s2)]
        second += [_row(c, s2, t), _row(c, t, s1[:40])]
        third.append(a3)
    return _pack(np.array(first + second + third))


@functools.lru_cache(maxsize=None)
def lazy_singleton() -> np.ndarray:
    r"""Triples (x, x', x''): x unlike everything before it (appended: a singleton without a uint8 row, SLOT_LAZY8), x' and x''
    near-duplicates (four bits toggled each).  x' makes the singleton a pair - its first uint8 row, spread to bytes only now -
    in the job before x'', whose pre-compare may have seen the singleton: the row record changes under it."""
    rng = np.random.default_rng(42)
    m = 250
    x = rng.random((m, F)) < 0.3
    out = np.repeat(x[:, None, :], 3, axis=1)
    for i in range(m):
        out[i, 1, rng.integers(0, F, 4)] ^= True
        out[i, 2, rng.integers(0, F, 4)] ^= True
    return _pack(out.reshape(3 * m, F))


@functools.lru_cache(maxsize=None)
def tier_change() -> np.ndarray:
    r"""300 exact copies of one row: the BitFeature crosses 255 -> 256 members, leaves the uint8 tier (its entry of the LDS cache
    is invalidated) while every job in flight goes to it.  Then pairs of near-duplicates of fresh rows alternating with more copies:
    uint8 rows, the LDS cache and the wide tier in turns."""
    rng = np.random.default_rng(43)
    d = rng.random(F) < 0.3
    rows = [d] * 300
    for _ in range(40):
        e = rng.random(F) < 0.3
        e2 = e.copy()
        e2[rng.integers(0, F, 4)] ^= True
        rows += [e, d, e2, d]
    return _pack(np.array(rows))


@functools.lru_cache(maxsize=None)
def vote_boundaries() -> np.ndarray:
    r"""One BitFeature of 260 rows whose vote counts sit ON the threshold at every size.  600 bits are set in every row; for
    every c in 0 .. 129 one more bit (anywhere in the row) is set in the rows 0 .. c - 1 only.  After the row that makes the
    BitFeature n strong (n = 2, 3, 4, ... 127, 128, ... 254, 255, then the wide tier) the bits of c have min(c, n) votes against
    the threshold ceil(n / 2): c = ceil(n / 2) is exactly on it (in), c = ceil(n / 2) - 1 one below (out) - for even and odd n.
    Rows differ in at most 130 of >= 600 bits (Tanimoto >= 0.82): every one merges, and no row of the prefix comes near them."""
    rng = np.random.default_rng(44)
    sets = _disjoint(rng, 600, *([1] * 130))
    rows = [_row(sets[0], *[sets[1 + c] for c in range(130) if c > i]) for i in range(260)]
    return _pack(np.array(rows))


@functools.lru_cache(maxsize=None)
def full_leaf() -> np.ndarray:
    r"""100 rows over a common core (300 bits + 300 of their own: Tanimoto 0.33 with each other, every one appended, the core keeps
    them on one path), each followed by a near-duplicate of the row before it (merges).  Whenever their leaf is full, the next
    job on it is a duplicate that merges - decided on a full leaf - and the one after it a row that is appended and splits it,
    both with pre-compares of the jobs behind them outstanding."""
    rng = np.random.default_rng(45)
    core, = _disjoint(rng, 300)
    rest = np.setdiff1d(np.arange(F), core)
    rows, prev = [], None
    for _ in range(100):
        o = _row(core, rng.permutation(rest)[:300])
        rows.append(o)
        if prev is not None:
            dup = prev.copy()
            dup[rng.integers(0, F, 3)] ^= True
            rows.append(dup)
        prev = o
    return _pack(np.array(rows))


CASES = {"stale_best_row": stale_best_row, "lazy_singleton": lazy_singleton, "tier_change": tier_change, "vote_boundaries": vote_boundaries,
         "full_leaf": full_leaf}

r"""Inputs of tests/test_hip_pipe_forward.py: a prefix that hands the tree to the pipelined kernel, and crafted tails.

The pipelined kernel's router FORWARDS the intersection of the tracking row it has just committed with the next element
(bb_tree_pipe.inc, pipe_fwd), and its leaf engine numbers the versions of the rows it merges into or appends by itself.
Every tail here makes consecutive elements meet the row the element before them changed, at the leaf-parent and in the
leaf, in a way the random workloads of tests/test_hip_pipe_fuzz.py only do by chance.  All cases: 2048 bits, branching
factor 50, diameter criterion, threshold THR.  TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import functools

import numpy as np

F = 2048
THR = 0.65
KW = dict(branching_factor=50, threshold=THR, merge_criterion="diameter")
N_PREFIX = 8192 + 1500  # the first 8 192 elements of a tree go through the steady-state kernel


def _pack(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.packbits(bits, axis=1))


@functools.lru_cache(maxsize=None)
def prefix() -> np.ndarray:
    r"""make_fake_fingerprints-like rows (popcount ~ N(750, 400), uniform positions; test_hip_pipe_fuzz's kind 4): at this
    threshold nearly every one stays a BitFeature of its own, the root's tracking rows are all-zero majorities, the
    leaf-parents' are not - the shape the single-level instance of the pipelined kernel takes."""
    rng = np.random.default_rng(20260)
    dens = np.clip(rng.normal(750 / F, 400 / F, (N_PREFIX, 1)), 1 / F, 1 - 1 / F)
    out = _pack(rng.random((N_PREFIX, F)) < dens)
    out.setflags(write=False)
    return out


def _noisy(rng, proto: np.ndarray, m: int, flip: float, support: np.ndarray | None = None) -> np.ndarray:
    t = rng.random((m, F)) < flip
    if support is not None:
        t &= support
    return proto[None, :] ^ t


@functools.lru_cache(maxsize=None)
def merge_chain() -> np.ndarray:
    r"""Noisy copies (1 % of the bits toggled) of two prototypes that share half their bits: copies of one prototype merge
    (Tanimoto ~ 0.9), the two BitFeatures never do (~ 0.33) but sit in one leaf.  A stretch of each, then strictly
    alternating (the row just changed is the SECOND best row of the next element), then stretches of 2 - 5 (it is the best
    one).  Both BitFeatures grow 1 -> 2 -> 3 (lazy uint8 slot, OR centroid, first majority vote) -> about 45."""
    rng = np.random.default_rng(31)
    p = rng.random(F) < 0.3
    q = p.copy()
    on = np.nonzero(p)[0]
    q[rng.permutation(on)[: on.size // 2]] = False
    off = np.nonzero(~p)[0]
    q[rng.permutation(off)[: on.size // 2]] = True
    which = [0] * 8 + [1] * 8 + [0, 1] * 12
    while len(which) < 90:
        which += [len(which) % 2] * int(rng.integers(2, 6))
    protos = np.stack([p, q])
    bits = protos[np.array(which)] ^ (rng.random((len(which), F)) < 0.01)
    return _pack(bits)


@functools.lru_cache(maxsize=None)
def append_then_match() -> np.ndarray:
    r"""Pairs (x, x'): x is unlike everything before it (a fresh random row: appended), x' is x with four bits toggled
    (Tanimoto > 0.98 with x, ~ 0.2 with every other row: it merges with x and only with x).  The row appended by one job
    decides the next one; the leaves the pairs land in fill up and split on the way."""
    rng = np.random.default_rng(32)
    m = 300
    x = rng.random((m, F)) < 0.3
    x2 = x.copy()
    for i in range(m):
        x2[i, rng.integers(0, F, 4)] ^= True
    return _pack(np.stack([x, x2], axis=1).reshape(2 * m, F))


@functools.lru_cache(maxsize=None)
def ties(older_first: bool) -> np.ndarray:
    r"""Groups (a, b, y, z) over a common core c of 400 bits: a = c + s1, b = c + s2 (150 bits each, disjoint: Tanimoto 0.57,
    two BitFeatures), y = b exactly (merges into b: the row is rewritten with the centroid it had) and z = c, equally similar
    to a and to the just-changed b (400 / 550).  np.argmax keeps the first index: older_first - a was appended before b and
    takes z; otherwise b was, and the row just rewritten takes it."""
    rng = np.random.default_rng(33 + int(older_first))
    rows = []
    for _ in range(120):
        idx = rng.permutation(F)
        c = np.zeros(F, bool); c[idx[:400]] = True
        a = c.copy(); a[idx[400:550]] = True
        b = c.copy(); b[idx[550:700]] = True
        rows += [a, b, b, c] if older_first else [b, a, b, c]
    return _pack(np.array(rows))


@functools.lru_cache(maxsize=None)
def other_leaf_next() -> np.ndarray:
    r"""Two families on disjoint halves of the bits (a dense prototype each, 1 % of its half toggled per row): a stretch of
    each pulls a tracking row of its own towards the family, then they alternate strictly - consecutive jobs never share a
    leaf, and the tracking row the router has just committed is never the one the next element goes to."""
    rng = np.random.default_rng(34)
    lo = np.arange(F) < F // 2
    pa = (rng.random(F) < 0.5) & lo
    pb = (rng.random(F) < 0.5) & ~lo
    fa = _noisy(rng, pa, 340, 0.01, lo)
    fb = _noisy(rng, pb, 340, 0.01, ~lo)
    order = [0] * 90 + [1] * 90 + [0, 1] * 250
    ia = ib = 0
    rows = []
    for w in order:
        if w == 0:
            rows.append(fa[ia]); ia += 1
        else:
            rows.append(fb[ib]); ib += 1
    return _pack(np.array(rows))


@functools.lru_cache(maxsize=None)
def split_then_duplicates() -> np.ndarray:
    r"""64 rows over a common core (300 bits + 300 of their own: Tanimoto 0.33 with each other, every one appended, the core
    keeps them on one path down the tree: their leaf overflows and splits, more than once), then a near-duplicate of each
    (three bits toggled: merges with its original where the splits have left it on the duplicate's path, is appended where not)."""
    rng = np.random.default_rng(35)
    core = np.zeros(F, bool)
    core[rng.permutation(F)[:300]] = True
    rest = np.nonzero(~core)[0]
    orig = np.repeat(core[None, :], 64, axis=0)
    for i in range(64):
        orig[i, rng.permutation(rest)[:300]] = True
    dup = orig.copy()
    for i in range(64):
        dup[i, rng.integers(0, F, 3)] ^= True
    return _pack(np.concatenate([orig, dup[rng.permutation(64)]]))


def with_prefix(tail: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([prefix(), tail]))

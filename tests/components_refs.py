r"""Reference and cases of the connected-components tests (bblean_amd/csrc/bb_components.hip).  TEST INFRASTRUCTURE.
test_hip_components_edges.py / test_hip_components.py (GPU) compare the library with `exact_components`;
test_components_refs.py (CPU) holds `exact_components` against scipy.sparse.csgraph.connected_components and checks that
every case meets the condition it is named for.  The distances are kernel_refs.exact's (integers until the one float64
division); nothing here has a tolerance."""
from __future__ import annotations

import functools

import numpy as np

import kernel_refs as R
import radius_refs as X


def linked(rows: np.ndarray, r: float) -> np.ndarray:
    r"""The n x n boolean matrix d <= r of a table against itself (the diagonal is True where r >= 0)."""
    return R.exact(rows, rows)[3] <= np.float64(r)


def components_of(adj: np.ndarray):
    r"""(roots int32, labels int32, count) of a symmetric boolean adjacency matrix: a plain union-find, the larger root
    under the smaller; roots[v] = the smallest row of v's component, labels[v] = the rank of that root among the roots."""
    n = len(adj)
    parent = list(range(n))

    def find(v: int) -> int:
        while parent[v] != v:
            v = parent[v]
        return v

    a, b = np.nonzero(np.triu(adj, 1))
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    roots = np.array([find(v) for v in range(n)], np.int32).reshape(n)
    is_root = roots == np.arange(n)
    rank = np.cumsum(is_root) - is_root
    return roots, rank[roots].astype(np.int32), int(is_root.sum())


def exact_components(rows: np.ndarray, r: float):
    return components_of(linked(rows, r)) if len(rows) else (np.zeros(0, np.int32), np.zeros(0, np.int32), 0)


def below(v: float) -> float:
    return float(np.nextafter(v, -np.inf))


def above(v: float) -> float:
    return float(np.nextafter(v, np.inf))


def bit_rows(sets, nb: int) -> np.ndarray:
    r"""Packed rows of nb bytes from an iterable of bit-index iterables."""
    sets = list(sets)
    b = np.zeros((len(sets), nb * 8), np.uint8)
    for k, s in enumerate(sets):
        b[k, list(s)] = 1
    return np.packbits(b, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# chain: row k has bits [2k, 2k + 8).  Neighbours share 6 of 10 bits: d = 0.4; two apart 4 of 12: d = 2 / 3.
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_N = 513
CHAIN_NB = 256
CHAIN_ORDERS = ("ascending", "descending", "permuted")
CHAIN_D = 4 / 10
CHAIN_RADII = {0.5: 1, CHAIN_D: 1, below(CHAIN_D): CHAIN_N}  # radius -> components


@functools.lru_cache(maxsize=None)
def chain_rows(order: str) -> np.ndarray:
    rows = bit_rows((range(2 * k, 2 * k + 8) for k in range(CHAIN_N)), CHAIN_NB)
    if order == "descending":
        rows = rows[::-1]
    elif order == "permuted":
        rows = rows[np.random.default_rng(513).permutation(CHAIN_N)]
    return np.ascontiguousarray(rows)


# ---------------------------------------------------------------------------------------------------------------------
# star: 1023 disjoint leaves of 2 bits and a hub that is their union.  Hub-leaf: i = 2, u = 2046, d = 2044 / 2046, the
# same rational as 1022 / 1023, so the same double; leaf-leaf: d = 1.
# ---------------------------------------------------------------------------------------------------------------------
STAR_LEAVES = 1023
STAR_NB = 256
STAR_HUBS = (0, 511, 1023)
STAR_R = 1022 / 1023
STAR_RADII = {STAR_R: 1, below(STAR_R): STAR_LEAVES + 1}


@functools.lru_cache(maxsize=None)
def star_rows(hub: int) -> np.ndarray:
    sets = [range(2 * k, 2 * k + 2) for k in range(STAR_LEAVES)]
    sets.insert(hub, range(2 * STAR_LEAVES))
    return bit_rows(sets, STAR_NB)


# ---------------------------------------------------------------------------------------------------------------------
# bridge: 300 copies of A = bits [0, 100), 300 of B = bits [100, 200), d(A, B) = 1; C = bits [0, 200) is at 0.5 of both.
# ---------------------------------------------------------------------------------------------------------------------
BRIDGE_COPIES = 300
BRIDGE_NB = 32
BRIDGE_AT = (0, 255, 256, 2 * BRIDGE_COPIES)  # where C stands; None = no C
BRIDGE_R = 0.5


@functools.lru_cache(maxsize=None)
def bridge_rows(at) -> np.ndarray:
    sets = [range(0, 100)] * BRIDGE_COPIES + [range(100, 200)] * BRIDGE_COPIES
    if at is not None:
        sets.insert(at, range(0, 200))
    return bit_rows(sets, BRIDGE_NB)


# ---------------------------------------------------------------------------------------------------------------------
# block model: 1500 rows, each one of 40 random centres with every bit flipped with probability 0.04
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_CENTRES = 40
BLOCK_N = 1500
BLOCK_NB = 256
BLOCK_RADII = (0.1, 0.13, 0.14, 0.15, 0.2)
BLOCK_COUNTS = (1500, 587, 129, 45, 40)  # exact_components' counts, recorded; test_components_refs.py holds them


@functools.lru_cache(maxsize=None)
def block_rows() -> np.ndarray:
    rng = np.random.default_rng(4004)
    centres = rng.integers(0, 2, (BLOCK_CENTRES, BLOCK_NB * 8), dtype=np.uint8)
    which = rng.integers(0, BLOCK_CENTRES, BLOCK_N)
    flip = (rng.random((BLOCK_N, BLOCK_NB * 8)) < 0.04).astype(np.uint8)
    return np.packbits(centres[which] ^ flip, axis=1)


@functools.lru_cache(maxsize=None)
def block_linked_at(r: float):
    return exact_components(block_rows(), r)


# ---------------------------------------------------------------------------------------------------------------------
# boundaries: radius_refs' query and ten of its nested subsets, one table of three rows per realised distance v =
# (n_set - m) / n_set: [subset m, an all-zero row, the query].  The zero row is at distance 1 of both, so the table has 3
# components one ulp below v and 2 at v and one ulp above.
# ---------------------------------------------------------------------------------------------------------------------
BOUNDARY_WIDTHS = (32, 100)  # the table of k_cc_pairs, the division of k_cc_pairs_generic
BOUNDARY_COUNTS = (3, 2, 2)  # one ulp below, at, one ulp above


@functools.lru_cache(maxsize=None)
def boundary_tables(nb: int, all_ones: bool):
    r"""[(v, rows)] for the ten values of radius_refs.boundary_values."""
    q, c, n_set = X.boundary_inputs(nb, all_ones)
    d = R.exact(q, c)[3][0]
    out = []
    for v in X.boundary_values(n_set):
        m = int(np.flatnonzero(d == v)[0])
        out.append((v, np.ascontiguousarray(np.concatenate([c[m:m + 1], np.zeros((1, nb), np.uint8), q]))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# degenerate tables and radii: name -> (rows, radius, components)
# ---------------------------------------------------------------------------------------------------------------------
def _degenerate():
    one = bit_rows([range(0, 9)], 16)
    pair = bit_rows([range(0, 8), range(4, 12)], 16)  # i = 4, u = 12: d = 2 / 3
    zeros = bit_rows([[], range(0, 5), [], range(0, 5), range(0, 4), [], range(64, 70)], 16)
    dup = bit_rows([range(0, 40), range(1, 41), range(0, 40), range(1, 41), range(0, 40), range(2, 42)], 32)
    return {
        "n = 1": (one, 0.3, 1),
        "n = 1, radius < 0": (one, -1.0, 1),
        "n = 2, linked": (pair, 2 / 3, 1),
        "n = 2, not linked": (pair, below(2 / 3), 2),
        "zero rows, r = 0": (zeros, 0.0, 4),           # {0, 2, 5}, {1, 3}, {4}, {6}
        "zero rows, r just below 1": (zeros, below(1.0), 3),  # the zero rows, the rows inside bits [0, 5), {6}
        "zero rows, r = 1": (zeros, 1.0, 1),
        "duplicates, r = 0": (dup, 0.0, 3),
        "r = -0.0": (dup, -0.0, 3),
        "r = -1e-300": (dup, -1e-300, 6),
        "r = 1 + 1e-9": (dup, 1 + 1e-9, 1),
    }


DEGENERATE = _degenerate()

# ---------------------------------------------------------------------------------------------------------------------
# widths: the six k_cc_pairs is instantiated for, and seven for k_cc_pairs_generic; about 300 rows each
# ---------------------------------------------------------------------------------------------------------------------
FAST_WIDTHS = (8, 16, 32, 64, 128, 256)
GENERIC_WIDTHS = (1, 3, 24, 100, 257, 1024, 8192)
WIDTH_N = 300


@functools.lru_cache(maxsize=None)
def width_rows(nb: int) -> np.ndarray:
    r"""100 distinct rows (densities 0.1 .. 0.5; up to 3 bytes: random bytes), each followed by two copies with a few bits
    flipped, shuffled; an all-zero row at 77 and a duplicate of row 5 at 201."""
    rng = np.random.default_rng([77, nb])
    base = rng.integers(0, 256, (WIDTH_N // 3, nb), dtype=np.uint8) if nb <= 3 else R.density_rows(rng, WIDTH_N // 3, nb, 0.1, 0.5)
    bits = np.unpackbits(np.repeat(base, 3, axis=0), axis=1)
    flips = rng.random(bits.shape) < min(0.25, 2.0 / (nb * 8))
    flips[::3] = False
    rows = np.packbits(bits ^ flips, axis=1)[rng.permutation(WIDTH_N)]
    rows[77] = 0
    rows[201] = rows[5]
    return np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def width_radii(nb: int) -> tuple[float, ...]:
    r"""0, 1 and the median of the rows' nearest-neighbour distances (a realised value: about half of the rows have a
    partner at it)."""
    d = R.exact(width_rows(nb), width_rows(nb))[3].copy()
    np.fill_diagonal(d, np.inf)
    return tuple(dict.fromkeys((0.0, float(np.sort(d.min(1))[WIDTH_N // 2]), 1.0)))  # (1 byte: the median is 0)


def all_cases():
    r"""Every (name, rows, radius) of this file, for the tests that walk all of them."""
    for order in CHAIN_ORDERS:
        for r in CHAIN_RADII:
            yield f"chain {order} {r!r}", chain_rows(order), r
    for hub in STAR_HUBS:
        for r in STAR_RADII:
            yield f"star hub {hub} {r!r}", star_rows(hub), r
    for at in BRIDGE_AT + (None,):
        yield f"bridge C at {at}", bridge_rows(at), BRIDGE_R
    for r in BLOCK_RADII:
        yield f"block {r}", block_rows(), r
    for nb in BOUNDARY_WIDTHS:
        for all_ones in (False, True):
            for v, rows in boundary_tables(nb, all_ones):
                for r in X.boundary_radii(v):
                    yield f"boundary {nb} {all_ones} {r!r}", rows, r
    for name, (rows, r, _) in DEGENERATE.items():
        yield f"degenerate {name}", rows, r
    for nb in FAST_WIDTHS + GENERIC_WIDTHS:
        for r in width_radii(nb):
            yield f"width {nb} {r!r}", width_rows(nb), r


@functools.lru_cache(maxsize=None)
def expected(name: str):
    r"""exact_components of a case of all_cases(), computed once and shared (read-only)."""
    for nm, rows, r in all_cases():
        if nm == name:
            out = exact_components(rows, r)
            out[0].flags.writeable = out[1].flags.writeable = False
            return out
    raise KeyError(name)

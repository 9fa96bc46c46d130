r"""Reference, case tables and builders of the radius-search tests (bblean_amd/csrc/bb_radius.hip).  TEST INFRASTRUCTURE.
test_hip_radius_edges.py / test_hip_radius.py (GPU) compare the library with `exact_radius`; test_radius_refs.py (CPU)
holds `exact_radius` against a pure-Python loop, `imin_table` against the comparison it replaces, and checks that every case
meets the condition it is named for.  Integers only until the one float64 division; nothing here has a tolerance."""
from __future__ import annotations

import functools

import numpy as np

import kernel_refs as R
import topk_refs as T

CUS = T.CUS  # compute units of an MI355X: the split-dependent case is derived for it (and re-derived on the device)


def exact_radius(q: np.ndarray, c: np.ndarray, r: float, exclude=None):
    r"""(offsets int64 (nq + 1,), idx int32, inter uint32, union uint32, dist float64): per query the columns of
    `kernel_refs.exact`'s float64 distance matrix with d <= r, the excluded column out, in ascending index."""
    d = R.exact(q, c)[3]
    inter, union = T.counts(q, c)
    hit = d <= np.float64(r)
    if exclude is not None:
        ex = np.asarray(exclude)
        inside = (ex >= 0) & (ex < len(c))
        hit[np.flatnonzero(inside), ex[inside]] = False
    rows, cols = np.nonzero(hit)  # row-major: ascending query, then ascending column
    offsets = np.zeros(len(q) + 1, np.int64)
    np.cumsum(hit.sum(1), out=offsets[1:])
    return (offsets, cols.astype(np.int32), inter[rows, cols].astype(np.uint32), union[rows, cols].astype(np.uint32),
            d[rows, cols])


def python_radius(q: np.ndarray, c: np.ndarray, r: float, exclude=None) -> list[list[int]]:
    r"""The semantics in Python numbers: d = float(u - i) / float(u), 0.0 where u == 0; a hit iff d <= r."""
    inter, union = T.counts(q, c)
    out = []
    for a in range(len(q)):
        skip = -1 if exclude is None else int(exclude[a])
        hits = []
        for m in range(len(c)):
            i, u = int(inter[a, m]), int(union[a, m])
            d = 0.0 if u == 0 else float(u - i) / float(u)
            if d <= float(r) and m != skip:
                hits.append(m)
        out.append(hits)
    return out


def imin_table(r: float, nbits: int) -> np.ndarray:
    r"""k_radius_table restated: imin[u] = the smallest i in 0 .. u with fl((u - i) / u) <= r (0.0 for u == 0), u + 1 where
    there is none - by the same bisection on the monotone predicate."""
    r = np.float64(r)
    u = np.arange(nbits + 1, dtype=np.int64)
    uf = np.maximum(u, 1).astype(np.float64)

    def passes(i: np.ndarray) -> np.ndarray:
        return np.where(u == 0, 0.0, (u - i).astype(np.float64) / uf) <= r

    some = passes(u)  # i = u is the smallest distance of the union
    lo, hi = np.zeros_like(u), np.where(some, u, u + 1)
    while (lo < hi).any():  # every u at once; a u without a passing i has lo = 0, hi = u + 1 and must not move
        mid = (lo + hi) >> 1
        ok = passes(np.minimum(mid, u))
        live = (lo < hi) & some
        hi = np.where(live & ok, mid, hi)
        lo = np.where(live & ~ok, mid + 1, np.where(some, lo, hi))
    return hi


def radius_ranges(nq: int, nc: int, fast: bool, cus: int = CUS) -> tuple[int, int]:
    r"""(rows per range, number of ranges) of bbh_jt_radius: bbh_jt_assign's rule with query tiles of 256 (a wave per
    query and four to a workgroup in the generic kernel)."""
    qblocks = (nq + 255) // 256 if fast else (nq + 3) // 4
    want = min((4 * cus + qblocks - 1) // qblocks, (nc + 63) // 64, 65535)
    per = (nc + want - 1) // want
    return per, (nc + per - 1) // per


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------

FIXED_RADII = (-1.0, 0.0, 1.0)                  # nothing; identical rows and empty unions; everything
GENERIC_CASES = [(100, 70, 70), (8200, 6, 40)]  # (nb, nq, nc): an odd width; 65 600 bits, beyond any table
LAYOUT_SHAPE = R.ASSIGN_ALIGN_SHAPE             # (nq, nc) of the pointer-offset and stride cases
SPLIT_CASE = (32, 3, 700)                       # several ranges: five distinct rows tiled to 700
BOUNDARY_BITS = 240                             # set bits of the first boundary query (of 256)
BOUNDARY_VALUES = 10                            # realised distances probed per boundary case
EXCLUDE_SHAPE = T.EXCLUDE_SHAPE[:3]
CAPACITY_CASE = (32, 70, 90)
OUTPUT_CASES = [(256, 200, 150), (16, 300, 70), (100, 70, 70)]


@functools.lru_cache(maxsize=None)
def assign_case(nb: int, nq: int, nc: int):
    return R.assign_inputs(nb, nq, nc)


@functools.lru_cache(maxsize=None)
def median_radius(nb: int, nq: int, nc: int) -> float:
    r"""The median of the case's reference distances (a realised value: the lower of the two middle ones)."""
    q, c = assign_case(nb, nq, nc)
    d = np.sort(R.exact(q, c)[3], axis=None)
    return float(d[(len(d) - 1) // 2])


def boundary_inputs(nb: int, all_ones: bool):
    r"""One query against 241 rows that are its nested subsets (row m keeps the query's first m set bits), in the first
    32 bytes of nb-byte rows.  all_ones = False: 240 set bits, u = 240, d = (240 - m) / 240 takes every multiple of 1 / 240.
    all_ones = True: the 256 bits all set, rows 0 .. 240 of the nest, u = 256 = nbits where nb = 32: dyadic distances."""
    n_set = 256 if all_ones else BOUNDARY_BITS
    qbits = np.zeros(nb * 8, np.uint8)
    setpos = np.arange(256) if all_ones else np.flatnonzero(np.arange(256) % 16 != 5)  # 240 of the 256
    assert len(setpos) == n_set
    qbits[setpos] = 1
    cbits = np.zeros((BOUNDARY_BITS + 1, nb * 8), np.uint8)
    for m in range(BOUNDARY_BITS + 1):
        cbits[m, setpos[:m]] = 1
    return np.packbits(qbits)[None, :], np.packbits(cbits, axis=1), n_set


def boundary_values(n_set: int) -> list[float]:
    r"""Ten realised distances (n_set - m) / n_set, 1 / 3 (m = 2 / 3 n_set where that is whole) among them, else the
    nearest below."""
    ms = sorted({(2 * n_set) // 3, 1, 7, n_set // 2, 100, 113, 171, 200, 239, 240})
    assert len(ms) == BOUNDARY_VALUES
    return [float(np.float64(n_set - m) / np.float64(n_set)) for m in ms]


def boundary_radii(v: float) -> tuple[float, float, float]:
    return float(np.nextafter(v, -np.inf)), v, float(np.nextafter(v, np.inf))


def split_inputs():
    r"""Five distinct rows tiled to 700, as topk_refs.tiled_inputs: every realised distance recurs every five rows, so a
    radius at a realised distance has hits on both sides of every range edge."""
    nb, nq, nc = SPLIT_CASE
    rng = np.random.default_rng([44, nb])
    base = R.density_rows(rng, 5, nb, 0.2, 0.6)
    c = np.ascontiguousarray(np.tile(base, (nc // 5, 1)))
    q = R.density_rows(rng, nq, nb, 0.2, 0.6)
    return q, c


def split_radius() -> float:
    r"""The third smallest of the first query's five realised distances."""
    q, c = split_inputs()
    return float(np.sort(np.unique(R.exact(q, c)[3][0]))[2])


def exclude_inputs():
    r"""topk_refs.exclude_inputs with a radius that keeps its 12 best of most queries: the median of the 12th distances."""
    q, c, cases = T.exclude_inputs()
    kth = T.exact_topk(q, c, T.EXCLUDE_SHAPE[3])[3][:, -1]
    return q, c, cases, float(np.sort(kth)[len(kth) // 2])

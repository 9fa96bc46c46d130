r"""Reference, case tables and builders of the top-k tests (bblean_amd/csrc/bb_topk.hip).  TEST INFRASTRUCTURE.
test_hip_topk_edges.py / test_hip_topk.py (GPU) compare the library with `exact_topk`; test_topk_refs.py (CPU) holds
`exact_topk` against a pure-Python sort with the cross-multiplying comparator and checks that every case meets the condition
it is named for.  Integers only until the one float64 division; nothing here has a tolerance."""
from __future__ import annotations

import functools

import numpy as np

import kernel_refs as R

TOPK_MAX = 64  # BBH_TOPK_MAX (include/bbhip.h)
CUS = 256      # compute units of an MI355X: the split-dependent cases are derived for it (and re-derived on the device)


def counts(q: np.ndarray, c: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    r"""Exact (intersection, union) of every pair, int64: kernel_refs.exact's integers."""
    qb = np.unpackbits(q, axis=1).astype(np.float32)  # 0/1 sums <= 2^24: exact in float32
    cb = np.unpackbits(c, axis=1).astype(np.float32)
    inter = (qb @ cb.T).astype(np.int64)
    union = qb.sum(1).astype(np.int64)[:, None] + cb.sum(1).astype(np.int64)[None, :] - inter
    return inter, union


def exact_topk(q: np.ndarray, c: np.ndarray, k: int, exclude=None):
    r"""(idx int32 (nq, k), inter uint32, union uint32, dist float64): the stable argsort of the float64 distances
    `kernel_refs.exact` gives, the excluded column at +inf.  Two different fractions with u < 2^26 are at least 2^-52 apart,
    so they divide to different doubles and equal ones to the same: float64 ties are the rational ties."""
    d = R.exact(q, c)[3].copy()
    inter, union = counts(q, c)
    assert int(union.max(initial=0)) < 1 << 26
    if exclude is not None:
        ex = np.asarray(exclude)
        hit = (ex >= 0) & (ex < len(c))
        d[np.flatnonzero(hit), ex[hit]] = np.inf
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    assert np.isfinite(np.take_along_axis(d, idx, 1)).all()
    return (idx.astype(np.int32), np.take_along_axis(inter, idx, 1).astype(np.uint32),
            np.take_along_axis(union, idx, 1).astype(np.uint32), np.take_along_axis(d, idx, 1))


def python_topk(q: np.ndarray, c: np.ndarray, k: int, exclude=None) -> np.ndarray:
    r"""The order of DESIGN 5a / 5e in Python integers: n = i + (u == 0); a before b iff n_a u_b > n_b u_a, or equal and
    index_a < index_b."""
    inter, union = counts(q, c)

    def cmp(a, b):
        l, r = a[0] * b[1], b[0] * a[1]
        return -1 if l > r or (l == r and a[2] < b[2]) else 1

    out = np.empty((len(q), k), np.int32)
    for i in range(len(q)):
        skip = -1 if exclude is None else int(exclude[i])
        cand = [(int(inter[i, m]) + (union[i, m] == 0), int(union[i, m]), m) for m in range(len(c)) if m != skip]
        cand.sort(key=functools.cmp_to_key(cmp))
        out[i] = [t[2] for t in cand[:k]]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the builder's range split (bbh_jt_topk), restated
# ---------------------------------------------------------------------------------------------------------------------


def topk_block(k: int) -> int:
    r"""Lanes (queries) of a k_topk_bcnt workgroup."""
    return 256 if k <= 8 else 128 if k <= 24 else 64


def topk_ranges(nq: int, nc: int, k: int, fast: bool, cus: int = CUS) -> tuple[int, int]:
    r"""(rows per range, number of ranges): bbh_jt_assign's rule; twice the ranges for workgroups of 128 lanes."""
    t = topk_block(k)
    qblocks = (nq + t - 1) // t if fast else (nq + 3) // 4
    fill = 4 * cus * (2 if fast and t == 128 else 1)  # workgroups of 128 lanes count as halves
    want = min((fill + qblocks - 1) // qblocks, (nc + 63) // 64, 65535)
    per = (nc + want - 1) // want
    return per, (nc + per - 1) // per


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------

FAST_SHAPES = [(1, 1, 1), (255, 65, 64), (256, 64, 64), (257, 63, 63), (513, 700, 1), (513, 700, 7), (513, 700, 64)]
FAST_CASES = [(nb, nq, nc, k) for nb in R.ASSIGN_FAST_WIDTHS for nq, nc, k in FAST_SHAPES]
GENERIC_WIDTH_CASE = (100, 70, 70, 9)        # (nb, nq, nc, k)
LAYOUT_SHAPE = R.ASSIGN_ALIGN_SHAPE + (20,)  # (nq, nc, k) of the pointer-offset and stride cases
SPLIT_CASE = (32, 3, 700, 64)                # several ranges
SHORT_RANGE_CASE = (32, 1, 130, 64)          # a range shorter than k
TILED_CASE = (32, 5, 700, 64)                # five distinct rows tiled: every place decided by the index, across ranges
NESTED_CASE = (32, 200, 64)                  # (nb, nc, k): all-ones query against nested rows
ZERO_CASE = (16, 4, 90, 20)                  # all-zero queries, several all-zero rows
ZERO_ROWS = (3, 17, 64, 89)
EXCLUDE_SHAPE = (16, 40, 90, 12)             # (nb, nq, nc, k)
OUTPUT_CASES = [(256, 200, 150, 10), (16, 300, 70, 33), (100, 70, 70, 9)]


@functools.lru_cache(maxsize=None)
def assign_case(nb: int, nq: int, nc: int):
    return R.assign_inputs(nb, nq, nc)


def tiled_inputs():
    nb, nq, nc, _ = TILED_CASE
    rng = np.random.default_rng([41, nb])
    base = R.density_rows(rng, 5, nb, 0.2, 0.6)
    c = np.ascontiguousarray(np.tile(base, (nc // 5, 1)))
    q = R.density_rows(rng, nq, nb, 0.2, 0.6)
    return q, c


def nested_inputs(reverse: bool):
    r"""Row m has its first m + 1 bits set; against the all-ones query i / u = (m + 1) / 256 ascends with m, so every row
    enters at the head of the list; reversed, nothing enters after the first k."""
    nb, nc, _ = NESTED_CASE
    bits = (np.arange(nb * 8)[None, :] <= np.arange(nc)[:, None]).astype(np.uint8)
    c = np.packbits(bits, axis=1)
    if reverse:
        c = np.ascontiguousarray(c[::-1])
    return np.full((1, nb), 0xFF, np.uint8), c


def zero_inputs():
    nb, nq, nc, _ = ZERO_CASE
    rng = np.random.default_rng([42, nb])
    c = rng.integers(1, 256, (nc, nb), dtype=np.uint8)
    c[list(ZERO_ROWS)] = 0
    return np.zeros((nq, nb), np.uint8), c


def exclude_inputs():
    r"""(q, c, {name: exclude}).  16-byte rows at density 1/2: tie groups are common."""
    nb, nq, nc, k = EXCLUDE_SHAPE
    q, c = assign_case(nb, nq, nc)
    best = exact_topk(q, c, k)
    inter, union = counts(q, c)
    in_tie = np.full(nq, -1, np.int64)
    for i in range(nq):  # the second member of the first tie group among the k best, where there is one
        for j in range(1, k):
            a, b = best[0][i, j - 1], best[0][i, j]
            if inter[i, a] * union[i, b] == inter[i, b] * union[i, a]:
                in_tie[i] = b
                break
    return q, c, {
        "best row": best[0][:, 0].astype(np.int64),
        "-1": np.full(nq, -1, np.int64),
        "nc": np.full(nq, nc, np.int64),
        "inside a tie group": in_tie,
    }


def self_inputs():
    r"""A table against itself; rows 7 and 30 are equal, and so are 8 and 50."""
    rng = np.random.default_rng(43)
    c = R.density_rows(rng, 60, 32, 0.1, 0.4)
    c[30] = c[7]
    c[50] = c[8]
    return c

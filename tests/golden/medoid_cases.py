r"""The inputs of tests/golden/medoids.npz and a NumPy restatement of the arithmetic `bbh_compl_isim_segments`
implements (data and test code only; shared by the generator, which runs the reference, and the tests, which run
this package - both rebuild the rows from the seeds with their own `make_fake_fingerprints`, which give the same
arrays bit for bit).

Three groups of sets:
  tree   the clusters of a fitted tree (the generator stores offsets and members, the rows come from TREE)
  hand   hand-made sets over HAND_ROWS: sizes 1, 2, 3, all-zero rows, one row repeated, constructed ties
  big    one set of BIG["draws"] rows drawn with repetition from BIG["distinct"] distinct rows (counters past
         uint16, 17 bit planes); equal rows have equal values, so the golden keeps one value per distinct row
"""
from __future__ import annotations

import numpy as np

TREE = dict(n=20000, seed=7, bf=50, thr=0.3)
HAND = dict(n=64, seed=11, zero_rows=4)  # the rows array is n fake rows followed by zero_rows all-zero rows
BIG = dict(distinct=3000, seed=13, draws=70000, draw_seed=17)

# hand-made sets as lists of row numbers of the hand rows (64 .. 67 are the all-zero rows)
HAND_SETS = [
    [0],
    [1, 2],
    [3, 4, 5],
    [64, 65, 66, 67],            # all-zero rows: every value is 1.0
    [6, 6, 6, 6, 6],             # one row repeated
    [8, 8, 7, 7, 9],             # [a, a, b, b, c]: the minimum is shared by the two a, position 0 wins
    [10, 11, 11, 10, 12, 12],
    [13, 13, 13, 14],
    [15, 16, 15, 16],
    [17, 18, 19, 18, 17, 19, 20],
    [64, 21, 65, 21],            # zero rows among others
    [22, 23, 24, 25, 26, 27, 28, 29, 30],
    [31, 32, 33, 31],
    [1, 2, 64],
    list(range(34, 64)) + list(range(34, 64)),
]


def tree_rows(make_fake_fingerprints) -> np.ndarray:  # type: ignore[no-untyped-def]
    return np.array(make_fake_fingerprints(TREE["n"], seed=TREE["seed"]), dtype=np.uint8)


def hand_rows(make_fake_fingerprints) -> np.ndarray:  # type: ignore[no-untyped-def]
    x = np.array(make_fake_fingerprints(HAND["n"], seed=HAND["seed"]), dtype=np.uint8)
    return np.concatenate([x, np.zeros((HAND["zero_rows"], x.shape[1]), np.uint8)])


def hand_index() -> tuple[np.ndarray, np.ndarray]:
    r"""(offsets, members) of HAND_SETS."""
    sizes = np.array([len(s) for s in HAND_SETS], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    members = np.array([r for s in HAND_SETS for r in s], dtype=np.int64)
    return offsets, members


def big_rows(make_fake_fingerprints) -> tuple[np.ndarray, np.ndarray]:  # type: ignore[no-untyped-def]
    r"""(distinct rows, draw): the set is distinct[draw]."""
    x = np.array(make_fake_fingerprints(BIG["distinct"], seed=BIG["seed"]), dtype=np.uint8)
    x[np.arange(len(x)) % 50 != 0, :8] = 0xFF  # 64 columns that nearly every row sets: their counts pass 2^16
    draw = np.random.default_rng(BIG["draw_seed"]).integers(0, BIG["distinct"], BIG["draws"]).astype(np.int64)
    return x, draw


# -------------------------------------------------------------------------------------------------------------
# NumPy restatement.  For a set of m >= 3 packed rows x_r with column sums ls: S = sum ls, Q = sum ls^2,
#   p_r = popcount(x_r), d_r = sum_b 2^b popcount(x_r & P_b) with the bit planes P_b of ls (packed like the rows),
#   s_r = S - p_r, q_r = Q - 2 d_r + p_r, value = a / ((a + (m - 1) s_r) - q_r) with a = (q_r - s_r) / 2.0,
# everything before the last line in exact uint64.
# -------------------------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)


def _popcount_rows(a: np.ndarray) -> np.ndarray:
    return _POP8[a].sum(axis=-1, dtype=np.uint64)


def compl_isim_set(rows: np.ndarray, n_features: int | None = None) -> np.ndarray:
    r"""Complementary iSIM of every row of one set of packed uint8 rows; NaN for sets of fewer than 3 rows."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    m = len(rows)
    if m < 3:
        return np.full(m, np.nan)
    nb = rows.shape[1] if n_features is None else n_features // 8
    rows = rows[:, :nb]
    ls = np.zeros(nb * 8, dtype=np.uint64)
    for lo in range(0, m, 4096):  # column sums without unpacking everything at once
        ls += np.unpackbits(rows[lo:lo + 4096], axis=1).sum(axis=0, dtype=np.uint64)
    S = ls.sum(dtype=np.uint64)
    Q = np.dot(ls, ls)
    p = _popcount_rows(rows)
    d = np.zeros(m, dtype=np.uint64)
    for b in range(int(m).bit_length()):
        plane = np.packbits(((ls >> np.uint64(b)) & np.uint64(1)).astype(np.uint8))
        d += _popcount_rows(rows & plane) << np.uint64(b)
    s = S - p
    q = Q - np.uint64(2) * d + p
    n = np.uint64(m - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (q - s).astype(np.float64) / 2.0
        val = a / ((a + (n * s).astype(np.float64)) - q.astype(np.float64))
    return np.where(s == 0, 1.0, val)


def compl_isim_segments(rows: np.ndarray, offsets: np.ndarray, members: np.ndarray | None = None,
                        n_features: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    r"""(medoid position per set, values in set order) - what `jt_compl_isim_segments` must return, exactly."""
    k = len(offsets) - 1
    med = np.zeros(k, dtype=np.int64)
    out = np.empty(int(offsets[-1]), dtype=np.float64)
    for g in range(k):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        sel = rows[lo:hi] if members is None else rows[members[lo:hi]]
        v = compl_isim_set(sel, n_features)
        out[lo:hi] = v
        med[g] = 0 if hi - lo < 3 else int(np.argmin(v))
    return med, out


# -------------------------------------------------------------------------------------------------------------
# Weighted form and the edge cases of tests/test_hip_medoid_edges.py.  The values of a set depend only on its
# multiset of rows, so a set of millions of rows is (a few distinct rows, how often each occurs) here and a
# `members` array over the distinct rows on the GPU.
# -------------------------------------------------------------------------------------------------------------
def compl_isim_weighted(distinct: np.ndarray, counts: np.ndarray, n_features: int | None = None) -> np.ndarray:
    r"""Complementary iSIM of every distinct row of the set that holds distinct[i] counts[i] times (one value per
    distinct row, whatever its count); NaN for sets of fewer than 3 rows.  Exact uint64 up to the last line."""
    distinct = np.ascontiguousarray(distinct, dtype=np.uint8)
    counts = np.asarray(counts, dtype=np.uint64)
    m = int(counts.sum())
    if m < 3:
        return np.full(len(distinct), np.nan)
    nb = distinct.shape[1] if n_features is None else n_features // 8
    rows = distinct[:, :nb]
    ls = counts @ np.unpackbits(rows, axis=1).astype(np.uint64)
    assert ls.dtype == np.uint64 and nb * 8 * m * m < 1 << 63
    S = ls.sum(dtype=np.uint64)
    Q = np.dot(ls, ls)
    p = _popcount_rows(rows)
    d = np.zeros(len(rows), dtype=np.uint64)
    for b in range(m.bit_length()):
        plane = np.packbits(((ls >> np.uint64(b)) & np.uint64(1)).astype(np.uint8))
        d += _popcount_rows(rows & plane) << np.uint64(b)
    s = S - p
    q = Q - np.uint64(2) * d + p
    n = np.uint64(m - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (q - s).astype(np.float64) / 2.0
        val = a / ((a + (n * s).astype(np.float64)) - q.astype(np.float64))
    return np.where(s == 0, 1.0, val)


def weighted_medoid(values: np.ndarray, members: np.ndarray) -> int:
    r"""First position in `members` of any distinct row that attains the minimum over the rows that occur."""
    present = np.zeros(len(values), dtype=bool)
    present[members] = True
    attains = present & (values == values[present].min())
    return int(np.argmax(attains[members]))


def column_sums(distinct: np.ndarray, counts: np.ndarray) -> np.ndarray:
    return np.asarray(counts, dtype=np.uint64) @ np.unpackbits(distinct, axis=1).astype(np.uint64)


SMALL_MAX = 2047      # bb_medoid.hip: the largest set the one-wave kernel takes
CHUNK = 256           # rows per wave of the large path
MAX_WORDS_REG = 128   # rows of more words go to k_seg_rows_wide
PLANE_STEPS = (16, 20, 24, 32)  # the NP instances of k_seg_rows
SHARED_BIT = 0x80     # byte 0: the column every non-zero distinct row sets


def instance_of(m: int, nbytes: int) -> tuple[str, int, int]:
    r"""(kernel, words per lane, planes) the launch code of bbh_compl_isim_segments picks for a set of m rows."""
    words = (nbytes + 3) // 4
    if m <= SMALL_MAX and words <= MAX_WORDS_REG:
        return "small", 1 if words <= 64 else 2, 11
    if words > MAX_WORDS_REG:
        return "wide", 0, int(m).bit_length()
    return "rows", 1 if words <= 64 else 2, next(s for s in PLANE_STEPS if int(m).bit_length() <= s)


def plane_distinct(nbytes: int) -> np.ndarray:
    r"""48 distinct rows: 0 the all-zero row, 1 the all-ones row, the rest random at densities 0.05 .. 0.9 with the
    shared column set."""
    rng = np.random.default_rng([41, nbytes])
    dens = rng.uniform(0.05, 0.9, (48, 1))
    x = np.packbits(rng.random((48, nbytes * 8)) < dens, axis=1)
    x[:, 0] |= SHARED_BIT
    x[0] = 0
    x[1] = 0xFF
    assert len(np.unique(x, axis=0)) == 48
    return x


# (m, nbytes, with the zero row): every plane instance at 8-byte rows, the two-word and the wide kernel at two sizes.
# The 2^24 set runs once, without the zero row: only then a column count (= m) has bit 24, the third plane group.
PLANE_MS = (65535, 65536, (1 << 20) - 1, 1 << 20, 1 << 24)
PLANE_EXPECT = {65535: 16, 65536: 20, (1 << 20) - 1: 20, 1 << 20: 24, 1 << 24: 32}
PLANE_CASES = [(m, 8, z) for m in PLANE_MS[:4] for z in (True, False)] + [(1 << 24, 8, False)] + \
              [(m, nb, z) for nb in (260, 512, 516) for m in (65536, 1 << 20) for z in (True, False)]
FULL_CHUNK = 100  # besides chunk 0, the chunk that holds only rows with the shared column


def plane_members(m: int, nbytes: int, with_zero: bool) -> np.ndarray:
    r"""`members` of one set of m rows over plane_distinct(nbytes); rows 0 .. 255 and chunk FULL_CHUNK never hold the
    zero row, so the shared column's count in those chunks is exactly 256."""
    rng = np.random.default_rng([42, m, nbytes, int(with_zero)])
    mem = rng.integers(0 if with_zero else 1, 48, m).astype(np.int64)
    for lo in (0, FULL_CHUNK * CHUNK):
        part = mem[lo:lo + CHUNK]
        part[part == 0] = 1 + lo // CHUNK % 47
    return mem


# argmin: 2^17 rows = 512 partials, two turns of the 256-thread scan.  First copy of the minimal row at ...
ARGMIN_M = 1 << 17
ARGMIN_FIRST = (0, 255, 256 * 255 + 17, 256 * 256, 256 * 300 + 37, ARGMIN_M - 1)
ARGMIN_LATER_CHUNKS = (1, 7, 70, 130, 250, 300, 511)  # chunks after the first copy's that hold another copy


def argmin_case(first: int) -> tuple[np.ndarray, np.ndarray, int]:
    r"""(distinct rows, members, minimal distinct row): the minimal row's first copy is at `first`, further copies
    sit in later chunks (other waves, other threads, the other turn of the scan); at m - 1 it is the only copy."""
    m = ARGMIN_M
    distinct = plane_distinct(8)[1:]
    rng = np.random.default_rng([43, first])
    counts = np.bincount(np.random.default_rng(44).integers(0, len(distinct), m), minlength=len(distinct))
    r0 = int(np.argmin(compl_isim_weighted(distinct, counts)))
    later = [first // CHUNK * CHUNK + c * CHUNK + int(rng.integers(0, CHUNK)) for c in ARGMIN_LATER_CHUNKS]
    later = sorted({p for p in later if first < p < m})
    heavy = int(np.argmax(np.where(np.arange(len(counts)) == r0, 0, counts)))
    counts[heavy] += counts[r0] - 1 - len(later)
    counts[r0] = 1 + len(later)
    others = np.repeat(np.arange(len(distinct)), np.where(np.arange(len(counts)) == r0, 0, counts))
    rng.shuffle(others)
    mem = np.empty(m, dtype=np.int64)
    at = np.zeros(m, dtype=bool)
    at[[first] + later] = True
    mem[at] = r0
    mem[~at] = others
    return distinct, mem, r0


# contiguous rows at the word-count boundaries: (nbytes, n_features)
WORD_CASES = [(260, 2080), (260, 2072), (260, 2056), (512, 4096), (516, 4128)]
WORD_MS = (40, 2047, 2048, 5000)


def word_rows(nbytes: int, m: int) -> np.ndarray:
    r"""m rows drawn from 300 distinct ones (ties), every byte of the row random: bits past n_features are set."""
    rng = np.random.default_rng([45, nbytes, m])
    distinct = np.packbits(rng.random((300, nbytes * 8)) < rng.uniform(0.1, 0.8, (300, 1)), axis=1)
    distinct[:, -4:] |= rng.integers(1, 256, (300, 4), dtype=np.uint8)
    distinct[0] = 0
    return distinct[rng.integers(0, 300, m)]


MANY_SIZES = (2048, 3, 1, 6000, 40, 2, 3000, 2047, 4500, 2049, 700, 5999, 1, 2500)  # seven large sets, first and last large


def many_sets() -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    r"""(rows, offsets, members) of MANY_SIZES over 500 distinct 64-byte rows."""
    rng = np.random.default_rng(46)
    rows = np.packbits(rng.random((500, 512)) < rng.uniform(0.05, 0.6, (500, 1)), axis=1)
    offsets = np.concatenate([[0], np.cumsum(MANY_SIZES)]).astype(np.int64)
    return rows, offsets, rng.integers(0, 500, int(offsets[-1])).astype(np.int64)

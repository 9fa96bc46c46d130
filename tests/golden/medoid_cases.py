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

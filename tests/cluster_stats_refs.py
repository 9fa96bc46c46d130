r"""Data and NumPy references of the cluster statistics kernels (bblean_amd/csrc/bb_cluster_stats.hip), shared by
test_cluster_stats_refs.py (CPU: the references against the C oracle) and test_hip_cluster_stats_edges.py (GPU: the kernels
against the references).  Everything is exact: integer counts, then the float64 operations of the contract in
include/bbhip.h, each rounded once."""
from __future__ import annotations

import functools
import re
from pathlib import Path

import numpy as np

import kernel_refs as R

REPO = Path(__file__).resolve().parents[1]
SMALL_MAX = 2047  # bb_segments.h
CHUNK = 256
DBI_TILE = int(re.search(r"#define\s+BBH_DBI_TILE\s+(\d+)", (REPO / "include" / "bbhip.h").read_text()).group(1))

# set sizes of the mixed call: the one-wave kernel's first sizes and the wave width, the border of the two paths, the
# chunk edges of the large path (9 chunks of 256, and one row more), and one set whose counts need 17 planes
MIX_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 2304, 2305, 70_001)
MIX_NB = 64
WIDTHS = (1, 3, 4, 252, 256, 260, 512, 516, 1024)
WIDTH_SIZES = (1, 2, 5, 70, 2100)
TIE_MS = (2, 6, 7, 64, 65, 2048, 2049)  # even and odd, one-wave and large path
DBI_KS = (1, 2, 3, DBI_TILE - 1, DBI_TILE, DBI_TILE + 1, 3 * DBI_TILE + 5)
DBI_WIDTHS = (1, 3, 256, 260, 516)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------


def ref_cluster_stats(rows: np.ndarray, off: np.ndarray, mem: np.ndarray | None = None, nf: int | None = None,
                      centrals: np.ndarray | None = None):
    r"""(centroids [k, nf / 8] uint8, isim [k], dist [off[-1]], sums [k, nf] uint64) of the sets rows[mem[off[g]:off[g + 1]]]:
    column sums by unpacking, centroid_from_sum and the iSIM formula on them, 1 - arr-vec similarity to the central."""
    nf = rows.shape[1] * 8 if nf is None else nf
    nb, k = nf // 8, len(off) - 1
    cents, isim = np.zeros((k, nb), np.uint8), np.zeros(k)
    dist, sums = np.zeros(int(off[-1])), np.zeros((k, nf), np.uint64)
    for g in range(k):
        b, e = int(off[g]), int(off[g + 1])
        sub = np.ascontiguousarray((rows[mem[b:e]] if mem is not None else rows[b:e])[:, :nb])
        m = e - b
        ls = R.ref_add_rows_packed(sub, nf)
        sums[g] = ls
        cents[g] = R.ref_centroid(ls, m, True)
        s1, s2 = int(ls.sum(dtype=np.uint64)), int((ls * ls).sum(dtype=np.uint64))  # (nothing wraps at these sizes)
        assert s2 < 1 << 63
        isim[g] = R.isim_from_ints(s1, s2, m) if m >= 2 else np.nan
        central = cents[g] if centrals is None else np.ascontiguousarray(centrals[g, :nb])
        dist[b:e] = 1.0 - R.ref_arr_vec(sub, central)[0]
    return cents, isim, dist, sums


def ref_worst_ratios(cents: np.ndarray, scatter: np.ndarray):
    r"""(worst [k] float64, flags [2]): for every i the maximum over j != i of (scatter[i] + scatter[j]) / (1.0 - sim_ij),
    from 0.0, a NaN candidate skipped; flags = ordered pairs that divided a non-zero / a zero numerator by zero."""
    k = len(cents)
    b = np.unpackbits(cents, axis=1).astype(np.float32)  # 0/1 sums <= 2^24: exact in float32
    inter = (b @ b.T).astype(np.int64)
    p = b.sum(1).astype(np.int64)
    union = p[:, None] + p[None, :] - inter
    den = 1.0 - inter.astype(np.float64) / np.maximum(union.astype(np.float64), 1.0)
    num = scatter[:, None] + scatter[None, :]
    with np.errstate(all="ignore"):
        cand = num / den
    off_diag = ~np.eye(k, dtype=bool)
    worst = np.zeros(k)
    for i in range(k):
        for x in cand[i][off_diag[i]].tolist():
            worst[i] = max(worst[i], x)  # (Python's max keeps its first argument against a NaN)
    flags = np.array([((den == 0) & (num != 0) & off_diag).sum(), ((den == 0) & (num == 0) & off_diag).sum()], np.uint32)
    return worst, flags


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------


def offsets_of(sizes) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def mix_case():
    r"""(rows, off, mem, reference): MIX_SIZES over a pool of 3000 rows of 64 bytes, members unordered and with repeats;
    the last set draws its 70 001 members from 48 rows that all share one column."""
    rng = np.random.default_rng(11)
    rows = R.density_rows(rng, 3000, MIX_NB, 0.05, 0.6)
    rows[:48, 0] |= 0x10
    mem = [rng.integers(0, 3000, m) for m in MIX_SIZES[:-1]] + [rng.integers(0, 48, MIX_SIZES[-1])]
    mem = np.concatenate(mem).astype(np.int64)
    off = offsets_of(MIX_SIZES)
    ref = ref_cluster_stats(rows, off, mem)
    assert int(ref[3][-1].max()) == MIX_SIZES[-1] >= 1 << 16  # 17 planes
    return rows, off, mem, ref


@functools.lru_cache(maxsize=None)
def small_mix():
    r"""A quick call with both paths: sets of 1, 2, 3, 40 and 2100 rows of 16 bytes, contiguous."""
    rng = np.random.default_rng(12)
    off = offsets_of((1, 2, 3, 40, 2100, 7))
    rows = R.density_rows(rng, int(off[-1]), 16, 0.1, 0.7)
    return rows, off, ref_cluster_stats(rows, off)


@functools.lru_cache(maxsize=None)
def width_case(nb: int, padded: bool):
    r"""(buffer, nbytes, stride, nf, off, reference).  padded: rows of nb + 3 bytes, nb + 5 apart, n_features = nb * 8 and
    garbage in every byte behind them."""
    rng = np.random.default_rng(100 + nb)
    off = offsets_of(WIDTH_SIZES)
    n = int(off[-1])
    rows = R.density_rows(rng, n, nb, 0.05, 0.8)
    ref = ref_cluster_stats(rows, off)
    if not padded:
        return rows, nb, nb, nb * 8, off, ref
    buf = rng.integers(1, 256, (n, nb + 5), dtype=np.uint8)
    buf[:, :nb] = rows
    return buf, nb + 3, nb + 5, nb * 8, off, ref


def tie_rows(m: int) -> tuple[np.ndarray, np.ndarray]:
    r"""m rows of 8 bytes whose 64 column counts cycle through the counts next to the majority threshold:
    m/2 (set) and m/2 - 1 (clear) for even m, (m + 1)/2 (set) and (m - 1)/2 (clear) for odd m, and 0, 1, m - 1, m."""
    near = [m // 2, m // 2 - 1] if m % 2 == 0 else [(m + 1) // 2, (m - 1) // 2]
    counts = np.array([max(c, 0) for c in (near + [0, 1, m - 1, m, near[0] + 1])] * 10)[:64]
    bits = (np.arange(m)[:, None] < counts[None, :]).astype(np.uint8)
    rng = np.random.default_rng(m)
    for c in range(64):  # every column's set rows at their own places
        bits[:, c] = bits[rng.permutation(m), c]
    return np.packbits(bits, axis=1), counts


def dbi_case(k: int, nb: int, seed: int = 0):
    rng = np.random.default_rng(1000 * k + nb + seed)
    cents = R.density_rows(rng, k, nb, 0.05, 0.7)
    scatter = rng.random(k)
    return cents, scatter

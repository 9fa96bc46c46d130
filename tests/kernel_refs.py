r"""Case lists, seeded inputs and plain NumPy references of the stateless kernels (bblean_amd/csrc/bb_kernels.hip).
TEST INFRASTRUCTURE.  test_hip_cabi_edges.py (GPU) compares the C ABI with these; test_kernel_refs.py (CPU) compares these
with the C oracle on the same case lists, so a wrong reference shows without a GPU.  Integers only until the single float64
formula at the end of each reference; nothing here has a tolerance."""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)

# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------


def mixed_rows(rng: np.random.Generator, n: int, nb: int) -> np.ndarray:
    r"""Dense (1/2), sparse (1/8), all-zero and all-one rows; with n >= 4 every kind occurs."""
    arr = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    kind = rng.integers(0, 4, n)
    kind[: min(n, 4)] = np.arange(4)[: min(n, 4)]
    rng.shuffle(kind)
    sparse = kind == 1
    arr[sparse] &= rng.integers(0, 256, (int(sparse.sum()), nb), dtype=np.uint8)
    arr[sparse] &= rng.integers(0, 256, (int(sparse.sum()), nb), dtype=np.uint8)
    arr[kind == 2] = 0
    arr[kind == 3] = 0xFF
    return arr


def probe_vecs(rng: np.random.Generator, nb: int) -> list[np.ndarray]:
    r"""A dense vector, the all-zero one (empty union with a zero row: sim 0 / 1) and the all-one one (maximum counts)."""
    return [rng.integers(0, 256, nb, dtype=np.uint8), np.zeros(nb, np.uint8), np.full(nb, 0xFF, np.uint8)]


# arr-vec / popcount: every LPR of the fast kernel (16 -> 1, 32 -> 2, 48/64 -> 4, 80..128 -> 8, 144..256 -> 16), chunk counts
# that are no power of two, and n around the 64-row tile
ARR_VEC_WIDTHS = (16, 32, 48, 64, 80, 96, 112, 128, 144, 240, 256)
ARR_VEC_NS = (1, 63, 64, 65, 130)
ARR_VEC_FAST = [(n, nb) for nb in ARR_VEC_WIDTHS for n in ARR_VEC_NS]
# the generic kernel: a 16-aligned width above 256, and the second turn of its grid-stride loop (2048 blocks x 4 waves)
ARR_VEC_GENERIC = [(70, 272), (8200, 100)]
ARR_VEC_CASES = ARR_VEC_FAST + ARR_VEC_GENERIC


def arr_vec_inputs(n: int, nb: int) -> tuple[np.ndarray, list[np.ndarray]]:
    rng = np.random.default_rng([11, n, nb])
    return mixed_rows(rng, n, nb), probe_vecs(rng, nb)


# strided views: name -> (columns of the base array, view of it); every view is 130 rows
STRIDE_ROWS = 130
STRIDE_LAYOUTS = {
    "cols_0_128_of_256": (256, 1, lambda t: t[:, :128]),        # stride 256, fast
    "every_other_row": (256, 2, lambda t: t[::2]),              # stride 512, fast
    "cols_16_144_of_256": (256, 1, lambda t: t[:, 16:144]),     # aligned offset, fast
    "cols_3_131_of_256": (256, 1, lambda t: t[:, 3:131]),       # misaligned data pointer, generic
    "cols_0_256_of_259": (259, 1, lambda t: t[:, :256]),        # stride no multiple of 16, generic
    "cols_44_300_of_300": (300, 1, lambda t: t[:, 44:]),        # the last row ends where the buffer ends
}


def stride_base(name: str) -> np.ndarray:
    cols, every, _ = STRIDE_LAYOUTS[name]
    rng = np.random.default_rng([12, cols, every])
    return mixed_rows(rng, STRIDE_ROWS * every, cols)


def best_match_overflow_inputs() -> tuple[np.ndarray, np.ndarray]:
    r"""65 536-bit rows: query all ones, centroid 0 all ones but one bit, centroid 1 all ones.  65536 * 65536 is 2^32: a
    32-bit cross-multiplication wraps to 0 and keeps index 0; the answer is index 1 (sim 1.0 against 0.99998474)."""
    q = np.full((1, 8192), 0xFF, np.uint8)
    c = np.full((2, 8192), 0xFF, np.uint8)
    c[0, 4000] = 0xFE
    return q, c


def best_match_wide_inputs() -> tuple[np.ndarray, np.ndarray]:
    r"""131 072-bit rows at density 0.8: inter ~ 84 000, union ~ 126 000, products ~ 2^33.  c[4] = c[2], and q[1] is a subset
    of c[2], so that pair of equal rows is q[1]'s maximum and the first of them has to win."""
    rng = np.random.default_rng(13)
    nb = 16384
    q = np.packbits(rng.random((3, nb * 8)) < 0.8, axis=1)
    c = np.packbits(rng.random((9, nb * 8)) < 0.8, axis=1)
    c[4] = c[2]
    q[1] = c[2] & np.packbits(rng.random(nb * 8) < 0.9)
    return q, c


def best_match_inputs(nq: int, nc: int, nb: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng([14, nq, nc, nb, seed])
    return mixed_rows(rng, nq, nb), mixed_rows(rng, nc, nb)


# most dissimilar: the 256-thread argmin block with exactly one, just over one, and many rows per thread; a generic width
MOST_DISSIMILAR_CASES = [(256, 256, 2048), (257, 256, 2048), (1000, 256, 2048), (5000, 256, 2048), (700, 100, 800),
                         (300, 256, 2024)]


def most_dissimilar_inputs(n: int, nb: int, nf: int) -> np.ndarray:
    rng = np.random.default_rng([15, n, nb, nf])
    # rows of density 1/4, 1/2 and 3/4 over the full width: bits past n_features are set too
    a, b = (rng.integers(0, 256, (n, nb), dtype=np.uint8) for _ in range(2))
    kind = rng.integers(0, 3, (n, 1))
    return np.where(kind == 0, a & b, np.where(kind == 1, a, a | b)).astype(np.uint8)


def most_dissimilar_tie_inputs(second_pass: bool) -> np.ndarray:
    r"""600 rows of 2048 bits whose minimum is attained by two identical rows, at 45 and 300 (threads 45 and 44 of the
    argmin block), in the first pass (similarity to the centroid) or in the second (similarity to the first pick).
    Bits 0..1023 (A): every ordinary row has ~70 % of them, so the centroid is about all of A.  Bits 1024..2047 (B): an
    ordinary row has exactly one.  First pass: rows 45 and 300 are all of B and nothing of A - similarity 0 to the centroid,
    everything else is above 0.  Second pass: row 10 is that all-of-B row (the only 0 of the first pass), rows 45 and 300
    are one ordinary row with its B bit removed - the only rows that share nothing with row 10."""
    rng = np.random.default_rng([16, int(second_pass)])
    n = 600
    bits = np.zeros((n, 2048), np.uint8)
    bits[:, :1024] = rng.random((n, 1024)) < 0.7
    bits[np.arange(n), 1024 + rng.integers(0, 1024, n)] = 1
    only_b = np.zeros(2048, np.uint8)
    only_b[1024:] = 1
    if second_pass:
        bits[10] = only_b
        bits[45, 1024:] = 0
        bits[300] = bits[45]
    else:
        bits[45] = only_b
        bits[300] = only_b
    return np.packbits(bits, axis=1)


# add_rows: one, two (n / 256 row splits joined by atomics), a ragged last split, many, and the 1024-split cap
ADD_ROWS_NS = (511, 512, 513, 1025, 70_000)
ADD_ROWS_UNPACKED_COLS = 300  # no multiple of the 64-thread block
ADD_ROWS_PACKED_CASES = [(n, 256, 2048) for n in ADD_ROWS_NS] + [(262_400, 32, 256), (600, 256, 2024), (600, 8, 8)]


def add_rows_packed_inputs(n: int, nb: int, nf: int) -> np.ndarray:
    rng = np.random.default_rng([17, n, nb, nf])
    return rng.integers(0, 256, (n, nb), dtype=np.uint8)  # (bits past n_features are set and must not be counted)


def add_rows_unpacked_inputs(n: int) -> np.ndarray:
    rng = np.random.default_rng([18, n])
    return rng.integers(0, 256, (n, ADD_ROWS_UNPACKED_COLS), dtype=np.uint8)  # byte values are summed, not bits


UNPACK_CASES = [(4100, 256, 2048), (37, 256, 2024)]  # (4100 x 256 bytes: 1 049 600 threads' worth against a 1 048 576 grid)
PACK_FEATURES = (1, 7, 9, 2047)

# centroid / iSIM from sums
LS_WIDTHS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
CENTROID_SAMPLES = (0, 1, 2, 3, 254, 255)
CENTROID_FEATURES = (1, 5, 8, 13, 2048)


def centroid_sums(n_samples: int, nf: int) -> np.ndarray:
    r"""uint64 sums that fit one byte.  n >= 2: 0, n and the values around n / 2 (n/2 - 1, n/2, n/2 + 1 for even n, the floor
    and the ceiling for odd n), each of them in the first columns and at random after that.  n <= 1 (the cast): 0, 1, 2, 255."""
    rng = np.random.default_rng([19, n_samples, nf])
    if n_samples <= 1:
        vals = [1, 0, 2, 255]
    elif n_samples % 2 == 0:
        h = n_samples // 2
        vals = [h, h - 1, h + 1, 0, n_samples]
    else:
        vals = [n_samples // 2, n_samples // 2 + 1, 0, n_samples]
    vals = np.array(vals, dtype=np.uint64)
    ls = vals[rng.integers(0, len(vals), nf)]
    ls[: min(nf, len(vals))] = vals[: min(nf, len(vals))]
    return ls


def isim_sums(nf: int) -> np.ndarray:
    rng = np.random.default_rng([20, nf])
    return rng.integers(0, 256, nf).astype(np.uint64)


def isim_wrap_sums() -> tuple[np.ndarray, int]:
    r"""64 entries near 2^32: each square is near 2^64, their sum wraps mod 2^64 many times over."""
    rng = np.random.default_rng(21)
    ls = ((1 << 32) + rng.integers(-1000, 1000, 64)).astype(np.uint64)
    return ls, 3_000_000_019


# pair min gap
PAIR_GAP_CASES = [(k, f) for k in (0, 1, 2, 3, 5) for f in (8, 100, 2048)] + [(300, 100)]


def pair_gap_inputs(k: int, f: int) -> tuple[np.ndarray, np.ndarray]:
    r"""Column sums of k clusters of 2..400 rows with their own bit densities (sums <= sizes, as real clusters have).  (2, 8):
    two all-zero clusters, iSIM 1.0 by definition, gap exactly 0."""
    rng = np.random.default_rng([22, k, f])
    sizes = rng.integers(2, 400, k).astype(np.uint64)
    p = rng.uniform(0.05, 0.6, (k, 1)) * rng.uniform(0.2, 1.0, (1, f))
    sums = rng.binomial(sizes.astype(np.int64)[:, None], p).astype(np.uint64).reshape(k, f)
    if (k, f) == (2, 8):
        sums[:] = 0
    return np.ascontiguousarray(sums), sizes


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------


def ref_popcount(arr: np.ndarray) -> np.ndarray:
    return POP8[arr].sum(axis=1, dtype=np.uint32)


def ref_arr_vec(arr: np.ndarray, vec: np.ndarray, card: np.ndarray | None = None):
    r"""(sim float64, inter uint32, union uint32); union = card + |vec| - inter in uint32, sim = inter / max(union, 1)."""
    inter = POP8[arr & vec[None, :]].sum(axis=1, dtype=np.uint32)
    c = ref_popcount(arr) if card is None else card.astype(np.uint32)
    union = ((c.astype(np.int64) + int(POP8[vec].sum()) - inter.astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
    sim = inter.astype(np.float64) / np.maximum(union.astype(np.float64), 1.0)
    return sim, inter, union


def ref_best_match(q: np.ndarray, c: np.ndarray):
    r"""(idx int32, inter, union, sims nq x nc): the first index of the maximum similarity (np.argmax)."""
    nq, nc = len(q), len(c)
    sims = np.empty((nq, nc))
    idx, inter, union = np.empty(nq, np.int32), np.empty(nq, np.uint32), np.empty(nq, np.uint32)
    card = ref_popcount(c)
    for i in range(nq):
        s, ii, uu = ref_arr_vec(c, q[i], card)
        sims[i] = s
        j = int(np.argmax(s))
        idx[i], inter[i], union[i] = j, ii[j], uu[j]
    return idx, inter, union, sims


def ref_unpack(arr: np.ndarray, nf: int) -> np.ndarray:
    return np.unpackbits(arr, axis=1)[:, :nf]


def ref_pack(un: np.ndarray) -> np.ndarray:
    return np.packbits(un != 0, axis=-1)


def ref_add_rows_packed(arr: np.ndarray, nf: int, chunk: int = 4096) -> np.ndarray:
    out = np.zeros(nf, dtype=np.uint64)
    for i in range(0, len(arr), chunk):
        out += np.unpackbits(arr[i:i + chunk, : nf // 8], axis=1).sum(0, dtype=np.uint64)
    return out


def ref_add_rows_unpacked(arr: np.ndarray) -> np.ndarray:
    return arr.sum(0, dtype=np.uint64)


def ref_centroid(ls: np.ndarray, n_samples: int, pack: bool) -> np.ndarray:
    c = ls.astype(np.uint8) if n_samples <= 1 else (ls >= n_samples * 0.5).astype(np.uint8)
    return np.packbits(c) if pack else c  # (packbits: any non-zero is a set bit)


def isim_from_ints(s1: int, s2: int, n: int) -> float:
    r"""The float64 formula on uint64 moments: every integer step mod 2^64, each conversion to float64 rounds to nearest
    (Python's int -> float does), then a / ((a + n s1) - s2) in that order."""
    if s1 == 0:
        return 1.0
    with np.errstate(all="ignore"):
        a = np.float64(float((s2 - s1) & M64)) / np.float64(2.0)
        return float(a / ((a + np.float64(float((n * s1) & M64))) - np.float64(float(s2))))


def ref_isim_from_sum(ls: np.ndarray, n_objects: int) -> float:
    if n_objects < 2:
        return float("nan")
    v = ls.astype(np.uint64)
    s1 = int(v.sum(dtype=np.uint64))       # NumPy's uint64 sums and products wrap mod 2^64
    s2 = int((v * v).sum(dtype=np.uint64))
    return isim_from_ints(s1, s2, n_objects & M64)


def ref_isim_rows(col_sums: np.ndarray, n: int) -> float:
    r"""On exact Python integers (nothing wraps at these sizes)."""
    if n < 2:
        return float("nan")
    s1 = sum(int(x) for x in col_sums)
    s2 = sum(int(x) * int(x) for x in col_sums)
    assert s2 < 1 << 64 and n * s1 < 1 << 64
    return isim_from_ints(s1, s2, n)


def ref_pair_min_gap(sums: np.ndarray, sizes: np.ndarray) -> float:
    best = 1.0
    for i in range(len(sums) - 1):
        for j in range(i + 1, len(sums)):
            x = sums[i] + sums[j]
            best = min(best, 1.0 - isim_from_ints(int(x.sum()), int((x * x).sum()), int(sizes[i]) + int(sizes[j])))
    return best


def ref_most_dissimilar(Y: np.ndarray, nf: int):
    r"""(idx1, idx2, sims1, sims2): centroid of the first n_features bits, the row least similar to it (first minimum), the
    row least similar to that one; cardinalities and similarities over the whole packed width."""
    n, nb = Y.shape
    cen = np.zeros(nb, np.uint8)
    cen[: (nf + 7) // 8] = ref_centroid(ref_add_rows_packed(Y, nf), n, True)
    card = ref_popcount(Y)
    i1 = int(np.argmin(ref_arr_vec(Y, cen, card)[0]))
    s1 = ref_arr_vec(Y, Y[i1], card)[0]
    i2 = int(np.argmin(s1))
    return i1, i2, s1, ref_arr_vec(Y, Y[i2], card)[0]


def bits(x: np.ndarray) -> np.ndarray:
    r"""float64 -> its uint64 bit patterns (comparisons are on these: -0.0 != 0.0, NaN == the same NaN)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# assignment (bblean_amd/csrc/bb_assign.hip): reference, case lists and builders of test_hip_assign_edges.py
# ---------------------------------------------------------------------------------------------------------------------


def exact(q: np.ndarray, c: np.ndarray):
    r"""(first argmin, its intersection, its union, the distance matrix) from exact integer counts."""
    qb = np.unpackbits(q, axis=1).astype(np.float32)  # 0/1 sums <= 2^24: exact in float32
    cb = np.unpackbits(c, axis=1).astype(np.float32)
    inter = (qb @ cb.T).astype(np.int64)
    union = qb.sum(1).astype(np.int64)[:, None] + cb.sum(1).astype(np.int64)[None, :] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(union == 0, 0.0, (union - inter).astype(np.float64) / union.astype(np.float64))
    idx = np.argmin(d, axis=1)  # equal fractions divide to the same double: float64 ties are the rational ties
    r = np.arange(q.shape[0])
    return idx.astype(np.int32), inter[r, idx].astype(np.uint32), union[r, idx].astype(np.uint32), d


def density_rows(rng: np.random.Generator, n: int, nb: int, lo: float, hi: float) -> np.ndarray:
    r"""n packed rows, each at its own bit density from [lo, hi]."""
    return np.packbits(rng.random((n, nb * 8)) < rng.uniform(lo, hi, (n, 1)), axis=1)


# the widths k_assign_bcnt / k_jaccard_dist are instantiated for (bb_assign.hip: W32 = nbytes / 4)
ASSIGN_FAST_WIDTHS = (8, 16, 32, 64, 128, 256)
ASSIGN_SHAPES = ((1, 1), (255, 65), (256, 64), (257, 63), (513, 700))
ASSIGN_WIDTH_CASES = [(nb, nq, nc) for nb in ASSIGN_FAST_WIDTHS for nq, nc in ASSIGN_SHAPES]
ASSIGN_DISPATCH_CASES = [(256, 63, 64), (256, 64, 63), (256, 64, 64)]  # use_mfma needs nq >= 64 and nc >= 64


def assign_inputs(nb: int, nq: int, nc: int) -> tuple[np.ndarray, np.ndarray]:
    r"""Rows of up to 16 bytes at density 1/2 (exact ties are common), wider ones at 0.05 .. 0.3; an all-zero query and an
    all-zero centroid where there is room; at 8, 64 and 256 bytes (1, 1) is the all-zero query against the all-zero centroid."""
    rng = np.random.default_rng([31, nb, nq, nc])
    if nb <= 16:
        q, c = (rng.integers(0, 256, (n, nb), dtype=np.uint8) for n in (nq, nc))
    else:
        q, c = density_rows(rng, nq, nb, 0.05, 0.3), density_rows(rng, nc, nb, 0.05, 0.3)
    if nq > 2:
        q[nq // 2] = 0
    if nc > 3:
        c[nc // 3] = 0
    if (nq, nc) == (1, 1) and nb in (8, 64, 256):
        q[:], c[:] = 0, 0
    return q, c


# device layouts of the alignment cases: name -> (query base offset, centroid base offset, q_stride - nbytes or None for 2 x)
ASSIGN_LAYOUTS = {
    "q+4": (4, 0, 0), "c+4": (0, 4, 0), "both+4": (4, 4, 0), "q+1": (1, 0, 0), "both+1": (1, 1, 0),
    "stride+4": (0, 0, 4), "stride+1": (0, 0, 1), "stride x2": (0, 0, None),
}
ASSIGN_ALIGN_SHAPE = (300, 130)  # both >= 64: the aligned 256-byte call goes to the matrix cores on its own


def layout_stride(name: str, nb: int) -> int:
    extra = ASSIGN_LAYOUTS[name][2]
    return 2 * nb if extra is None else nb + extra


def strided_buffer(rows: np.ndarray, off: int, stride: int) -> np.ndarray:
    r"""A flat buffer of 0xFF with rows[i] at off + i * stride that ends with the last row's last byte."""
    n, nb = rows.shape
    flat = np.full(off + (n - 1) * stride + nb, 0xFF, np.uint8)
    np.lib.stride_tricks.as_strided(flat[off:], (n, nb), (stride, 1))[:] = rows
    return flat


# distance matrix: several queries per grid range (k_jaccard_dist's inner loop), as bbh_jt_dist_matrix cuts them
DIST_RANGE_CASES = [(16, 5000, 300), (16, 4097, 257), (16, 5003, 300)]
DIST_GRID_Z_CASE = (3, 65535 + 70, 3)  # generic kernel, the second turn of blockIdx.z


def dist_queries_per_range(nq: int, nc: int, cus: int) -> int:
    cblocks = (nc + 255) // 256
    want = min((4 * cus + cblocks - 1) // cblocks, nq, 65535)
    return (nq + want - 1) // want


ASSIGN_WIDE_WIDTHS = (8192, 8200)
ASSIGN_WIDE_SHAPE = (6, 40)


def assign_wide_inputs(nb: int) -> tuple[np.ndarray, np.ndarray]:
    r"""65 536-bit rows and a little more, dense: n * u passes 2^32.  q[0] / c[0], c[1] are best_match_overflow_inputs (all
    ones against all ones but one bit, then all ones: index 1); c[7] = c[5] is q[2]'s nearest, the first of the two wins."""
    rng = np.random.default_rng([32, nb])
    nq, nc = ASSIGN_WIDE_SHAPE
    q, c = density_rows(rng, nq, nb, 0.7, 0.95), density_rows(rng, nc, nb, 0.7, 0.95)
    oq, oc = best_match_overflow_inputs()
    q[0], c[:2] = 0xFF, 0xFF
    q[0, :8192], c[:2, :8192] = oq[0], oc
    c[7] = c[5]
    q[2] = c[5] & density_rows(rng, 1, nb, 0.9, 0.9)[0]
    q[5] = 0xFF
    c[20] = 0
    return q, c


def first_argmin_int32(inter: np.ndarray, union: np.ndarray) -> int:
    r"""k_assign_generic's scan with the cross-multiplication wrapped to a signed 32-bit integer."""
    def wrap(v):
        v &= 0xFFFFFFFF
        return v - (1 << 32) if v >= 1 << 31 else v
    bn, bu, best = -1, 1, 0
    for m in range(len(inter)):
        u = int(union[m])
        n = int(inter[m]) + (u == 0)
        if wrap(n * bu) > wrap(bn * u):
            bn, bu, best = n, u, m
    return best


# matrix cores at their limits: 256-byte rows, nc so that padded rows sit in every lane group and in a whole wave half
MFMA_LIMIT_NCS = (1, 65, 129)
MFMA_LIMIT_NQ = 130


def mfma_limit_inputs(nc: int) -> tuple[np.ndarray, np.ndarray]:
    r"""All-ones, all-zero and dense (0.5, 0.9) rows on both sides."""
    rng = np.random.default_rng([33, nc])

    def side(n):
        x = np.concatenate([density_rows(rng, n - n // 2, 256, 0.5, 0.5), density_rows(rng, n // 2, 256, 0.9, 0.9)])
        rng.shuffle(x)
        x[0] = 0xFF
        if n > 2:
            x[n // 2] = 0
            x[n - 1] = 0xFF
        return x
    return side(MFMA_LIMIT_NQ), side(nc)


ONE_HOT_WIDTHS = (32, 64, 128, 256)


def one_hot_inputs(nb: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    r"""(queries = the nb * 8 one-hot rows, centroids = the same rows permuted + one all-ones row, position of query j's
    own centroid).  A kernel that takes the two operands through different orders of the bits pairs a query with the wrong one-hot
    centroid: intersection 0 where (1, 1) is expected."""
    n = nb * 8
    q = np.packbits(np.eye(n, dtype=np.uint8), axis=1)
    perm = np.random.default_rng([34, nb]).permutation(n)
    c = np.concatenate([q[perm], np.full((1, nb), 0xFF, np.uint8)])
    where = np.empty(n, np.int32)
    where[perm] = np.arange(n, dtype=np.int32)
    return q, c, where


ASSIGN_OUTPUT_CASES = [(256, 200, 150), (16, 300, 70), (100, 70, 70)]  # matrix cores, popcount, generic

r"""The NumPy references of tests/kernel_refs.py against the C oracle, on the case lists test_hip_cabi_edges.py uses on the GPU.
No GPU needed: a reference that is wrong fails here, before it can be blamed on a kernel."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kernel_refs as R
import medoid_cases as mc
from oracle_engine import oracle_lib


def o_popcount(arr):
    out = np.empty(len(arr), np.uint32)
    oracle_lib().bbo_popcount_rows(arr.ctypes.data, arr.shape[0], arr.shape[1], out.ctypes.data)
    return out


def o_arr_vec(arr, vec, card=None):
    n, nb = arr.shape
    s, i, u = np.empty(n), np.empty(n, np.uint32), np.empty(n, np.uint32)
    oracle_lib().bbo_jt_arr_vec(arr.ctypes.data, n, nb, vec.ctypes.data, card.ctypes.data if card is not None else None,
                                s.ctypes.data, i.ctypes.data, u.ctypes.data)
    return s, i, u


def same_arr_vec(got, want):
    return (R.bits(got[0]) == R.bits(want[0])).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all()


@pytest.mark.parametrize("n,nb", R.ARR_VEC_CASES)
def test_ref_arr_vec_and_popcount(n, nb):
    arr, vecs = R.arr_vec_inputs(n, nb)
    assert (R.ref_popcount(arr) == o_popcount(arr)).all()
    fake = (R.ref_popcount(arr) * 3 + 7).astype(np.uint32)
    for vec in vecs:
        assert same_arr_vec(R.ref_arr_vec(arr, vec), o_arr_vec(arr, vec))
        assert same_arr_vec(R.ref_arr_vec(arr, vec, fake), o_arr_vec(arr, vec, fake))
    if n >= 4:  # the mix is what the case list promises: empty unions and the maximum counts occur
        pc = R.ref_popcount(arr)
        assert (pc == 0).any() and (pc == nb * 8).any()
        assert R.ref_arr_vec(arr, vecs[1])[2].min() == 0 and R.ref_arr_vec(arr, vecs[2])[1].max() == nb * 8


@pytest.mark.parametrize("name", list(R.STRIDE_LAYOUTS))
def test_ref_strided_views(name):
    base = R.stride_base(name)
    view = R.STRIDE_LAYOUTS[name][2](base)
    assert view.shape[0] == R.STRIDE_ROWS and not view.flags.c_contiguous
    arr = np.ascontiguousarray(view)
    vec = arr[5].copy()
    assert (R.ref_popcount(view) == o_popcount(arr)).all()
    assert same_arr_vec(R.ref_arr_vec(view, vec), o_arr_vec(arr, vec))
    if name == "cols_44_300_of_300":  # the view's last byte is the buffer's last byte
        assert view[-1, -1:].ctypes.data + 1 == base.ctypes.data + base.nbytes


def emulated_u32_first_argmax(inter, union):
    r"""The first-argmax loop with the cross-multiplication in 32 bits, as k_best_match_generic had it."""
    best, bi, bu = 0, 0, 1
    for m in range(len(inter)):
        i, u = int(inter[m]), max(int(union[m]), 1)
        if m == 0 or (i * bu) & 0xFFFFFFFF > (bi * u) & 0xFFFFFFFF:
            best, bi, bu = m, i, u
    return best


def test_ref_best_match_wide_rows():
    r"""The two wide-row cases: reference = argmax of the oracle's similarities; and why 32-bit products fail on them."""
    q, c = R.best_match_overflow_inputs()
    idx, inter, union, sims = R.ref_best_match(q, c)
    s, i, u = o_arr_vec(c, q[0])
    assert (R.bits(sims[0]) == R.bits(s)).all() and s.tolist() == [65535 / 65536, 1.0]
    assert int(np.argmax(s)) == 1 and (idx[0], inter[0], union[0]) == (1, 65536, 65536)
    assert emulated_u32_first_argmax(i, u) == 0  # 65536 * 65536 wraps to 0: index 0 is kept

    q, c = R.best_match_wide_inputs()
    idx, inter, union, sims = R.ref_best_match(q, c)
    wrong = 0
    for k in range(len(q)):
        s, i, u = o_arr_vec(c, q[k])
        j = int(np.argmax(s))
        assert (R.bits(sims[k]) == R.bits(s)).all() and (idx[k], inter[k], union[k]) == (j, i[j], u[j])
        assert int(i.max()) * int(u.max()) >= 1 << 32
        wrong += emulated_u32_first_argmax(i, u) != j
    assert idx[1] == 2 and sims[1, 2] == sims[1, 4]  # the tie, first index
    assert wrong > 0


@pytest.mark.parametrize("nq,nc,nb,seed", [(5, 7, 256, 0), (257, 1, 256, 1)])
def test_ref_best_match(nq, nc, nb, seed):
    q, c = R.best_match_inputs(nq, nc, nb, seed)
    idx, inter, union, sims = R.ref_best_match(q, c)
    for k in range(nq):
        s, i, u = o_arr_vec(c, q[k])
        j = int(np.argmax(s))
        assert (R.bits(sims[k]) == R.bits(s)).all() and (idx[k], inter[k], union[k]) == (j, i[j], u[j])


def o_most_dissimilar(Y, nf):
    n, nb = Y.shape
    i1, i2 = C.c_int64(-1), C.c_int64(-1)
    s1, s2 = np.empty(n), np.empty(n)
    oracle_lib().bbo_most_dissimilar(Y.ctypes.data, n, nb, nf, C.byref(i1), C.byref(i2), s1.ctypes.data, s2.ctypes.data)
    return i1.value, i2.value, s1, s2


def same_most_dissimilar(got, want):
    return got[:2] == want[:2] and (R.bits(got[2]) == R.bits(want[2])).all() and (R.bits(got[3]) == R.bits(want[3])).all()


@pytest.mark.parametrize("n,nb,nf", R.MOST_DISSIMILAR_CASES)
def test_ref_most_dissimilar(n, nb, nf):
    Y = R.most_dissimilar_inputs(n, nb, nf)
    assert same_most_dissimilar(R.ref_most_dissimilar(Y, nf), o_most_dissimilar(Y, nf))
    if nf < nb * 8:
        assert R.ref_popcount(Y[:, nf // 8:]).any()  # bits past n_features are set


@pytest.mark.parametrize("second_pass", [False, True])
def test_ref_most_dissimilar_ties(second_pass):
    Y = R.most_dissimilar_tie_inputs(second_pass)
    got = R.ref_most_dissimilar(Y, 2048)
    assert same_most_dissimilar(got, o_most_dissimilar(Y, 2048))
    assert (Y[45] == Y[300]).all()
    if second_pass:
        assert got[:2] == (10, 45) and np.flatnonzero(got[2] == got[2].min()).tolist() == [45, 300]
    else:
        cen = R.ref_centroid(R.ref_add_rows_packed(Y, 2048), len(Y), True)
        sc = R.ref_arr_vec(Y, cen)[0]
        assert got[0] == 45 and np.flatnonzero(sc == sc.min()).tolist() == [45, 300]


@pytest.mark.parametrize("n,nb,nf", R.ADD_ROWS_PACKED_CASES)
def test_ref_add_rows_packed(n, nb, nf):
    arr = R.add_rows_packed_inputs(n, nb, nf)
    got = R.ref_add_rows_packed(arr, nf)
    want = np.zeros(nf, np.uint64)
    part = np.empty(nf, np.uint64)
    for i in range(0, n, 8192):  # the oracle adds unpacked rows: unpack with it, a chunk at a time
        chunk = np.ascontiguousarray(arr[i:i + 8192])
        un = np.empty((len(chunk), nf), np.uint8)
        oracle_lib().bbo_unpack(chunk.ctypes.data, len(chunk), nb, nf, un.ctypes.data)
        oracle_lib().bbo_add_rows(un.ctypes.data, len(chunk), nf, part.ctypes.data)
        want += part
    assert (got == want).all()
    assert R.bits(np.float64(R.ref_isim_rows(got, n))) == R.bits(np.float64(oracle_lib().bbo_isim_from_sum(got.ctypes.data, nf, n)))


@pytest.mark.parametrize("n", R.ADD_ROWS_NS)
def test_ref_add_rows_unpacked(n):
    arr = R.add_rows_unpacked_inputs(n)
    want = np.empty(arr.shape[1], np.uint64)
    oracle_lib().bbo_add_rows(arr.ctypes.data, n, arr.shape[1], want.ctypes.data)
    got = R.ref_add_rows_unpacked(arr)
    assert (got == want).all()
    assert R.bits(np.float64(R.ref_isim_rows(got, n))) == R.bits(np.float64(oracle_lib().bbo_isim_from_sum(got.ctypes.data, arr.shape[1], n)))


@pytest.mark.parametrize("n,nb,nf", R.UNPACK_CASES)
def test_ref_unpack(n, nb, nf):
    arr = R.add_rows_packed_inputs(n, nb, nf)
    want = np.empty((n, nf), np.uint8)
    oracle_lib().bbo_unpack(arr.ctypes.data, n, nb, nf, want.ctypes.data)
    assert (R.ref_unpack(arr, nf) == want).all()


@pytest.mark.parametrize("n_samples", R.CENTROID_SAMPLES)
@pytest.mark.parametrize("nf", R.CENTROID_FEATURES)
def test_ref_centroid(n_samples, nf):
    ls = R.centroid_sums(n_samples, nf)
    assert int(ls.max()) <= 255
    if n_samples >= 2 and nf >= 5:  # the values around n / 2 are there, on both sides
        assert (2 * ls.astype(np.int64) == n_samples).any() or n_samples % 2
        assert (2 * ls.astype(np.int64) < n_samples).any() and (2 * ls.astype(np.int64) > n_samples).any()
    for pack in (0, 1):
        want = np.full((nf + 7) // 8 if pack else nf, 0xAA, np.uint8)
        oracle_lib().bbo_centroid_from_sum(ls.ctypes.data, nf, n_samples, pack, want.ctypes.data)
        assert (R.ref_centroid(ls, n_samples, bool(pack)) == want).all()


def test_ref_centroid_uint8_cast():
    ls = np.array([256, 257, 1, 0, 255], np.uint64)
    for pack in (0, 1):
        want = np.zeros(1 if pack else 5, np.uint8)
        oracle_lib().bbo_centroid_from_sum(ls.ctypes.data, 5, 1, pack, want.ctypes.data)
        assert (R.ref_centroid(ls, 1, bool(pack)) == want).all()
    assert R.ref_centroid(ls, 1, False).tolist() == [0, 1, 1, 0, 255]


def test_ref_isim_from_sum():
    lib = oracle_lib()
    for nf in R.CENTROID_FEATURES:
        ls = R.isim_sums(nf)
        for n in (0, 1, 2, 3, 255, 100_000):
            got, want = R.ref_isim_from_sum(ls, n), lib.bbo_isim_from_sum(ls.ctypes.data, nf, n)
            assert R.bits(np.float64(got)) == R.bits(np.float64(want)) or (n < 2 and np.isnan(got) and np.isnan(want))
        assert R.ref_isim_from_sum(np.zeros(nf, np.uint64), 7) == 1.0 == lib.bbo_isim_from_sum(np.zeros(nf, np.uint64).ctypes.data, nf, 7)
    ls, n = R.isim_wrap_sums()
    assert sum(int(v) ** 2 for v in ls) >= 1 << 64  # the second moment does wrap
    assert R.bits(np.float64(R.ref_isim_from_sum(ls, n))) == R.bits(np.float64(lib.bbo_isim_from_sum(ls.ctypes.data, 64, n)))


@pytest.mark.parametrize("k,f", [c for c in R.PAIR_GAP_CASES if c[0] <= 5])
def test_ref_pair_min_gap(k, f):
    r"""Against the oracle's iSIM of the summed pair (the GPU file runs k = 300 too; its pairs go through the same function)."""
    sums, sizes = R.pair_gap_inputs(k, f)
    assert (sums <= sizes[:, None]).all()
    best = 1.0
    for i in range(k - 1):
        for j in range(i + 1, k):
            x = sums[i] + sums[j]
            best = min(best, 1.0 - oracle_lib().bbo_isim_from_sum(x.ctypes.data, f, int(sizes[i] + sizes[j])))
    assert R.ref_pair_min_gap(sums, sizes) == best
    if (k, f) == (2, 8):
        assert best == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# assignment: kernel_refs.exact against the oracle's counts, on the case lists of test_hip_assign_edges.py
# ---------------------------------------------------------------------------------------------------------------------


def assert_exact_is_the_oracles(q, c):
    r"""Per query: the distance row is (u - i) / u of the oracle's counts (0.0 for an empty union), no centroid is nearer than
    exact()'s index by exact cross-multiplication, none before it is as near, and its counts are the oracle's."""
    idx, inter, union, d = R.exact(q, c)
    for k in range(len(q)):
        _, i, u = o_arr_vec(c, q[k])
        i, u = i.astype(np.int64), u.astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.where(u == 0, 0.0, (u - i).astype(np.float64) / u.astype(np.float64))
        assert (R.bits(d[k]) == R.bits(want)).all()
        b = int(idx[k])
        assert (int(inter[k]), int(union[k])) == (int(i[b]), int(u[b]))
        n = i + (u == 0)  # an empty union is (1, 0): nearer than everything
        left, right = n * u[b], n[b] * u  # < 2^63 for rows of up to 2^31 bits
        assert not (left > right).any() and int(np.argmax(left == right)) == b


ASSIGN_CPU_CASES = [c for c in R.ASSIGN_WIDTH_CASES if c[1] <= 257] + [(16, 513, 700), (256, 513, 700)] + R.ASSIGN_DISPATCH_CASES


@pytest.mark.parametrize("nb,nq,nc", ASSIGN_CPU_CASES)
def test_exact_on_the_width_cases(nb, nq, nc):
    q, c = R.assign_inputs(nb, nq, nc)
    assert_exact_is_the_oracles(q, c)
    if nb <= 16 and nq > 200:  # density 1/2 on narrow rows: exact ties between different centroids occur
        d = R.exact(q, c)[3]
        assert ((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()


@pytest.mark.parametrize("nb", R.ASSIGN_WIDE_WIDTHS)
def test_exact_on_wide_rows(nb):
    r"""... and a scan that multiplies in 32 bits goes wrong on them."""
    q, c = R.assign_wide_inputs(nb)
    assert_exact_is_the_oracles(q, c)
    idx = R.exact(q, c)[0]
    wrong = 0
    for k in range(len(q)):
        _, i, u = o_arr_vec(c, q[k])
        wrong += R.first_argmin_int32(i, u) != idx[k]
    assert wrong > 0


@pytest.mark.parametrize("nc", R.MFMA_LIMIT_NCS)
def test_exact_on_the_matrix_core_limits(nc):
    q, c = R.mfma_limit_inputs(nc)
    assert_exact_is_the_oracles(q, c)
    assert {0, 2048} <= set(R.ref_popcount(q).tolist()) and 2048 in R.ref_popcount(c).tolist()


@pytest.mark.parametrize("nb", [w for w in R.ONE_HOT_WIDTHS if w <= 128])
def test_exact_on_one_hot_rows(nb):
    q, c, where = R.one_hot_inputs(nb)
    assert_exact_is_the_oracles(q, c)
    idx, inter, union, _ = R.exact(q, c)
    assert (idx == where).all() and (inter == 1).all() and (union == 1).all()
    assert (c[where] == q).all()


def test_strided_buffer_and_ranges():
    q = R.assign_inputs(16, 7, 5)[0]
    for name in R.ASSIGN_LAYOUTS:
        off, stride = R.ASSIGN_LAYOUTS[name][0], R.layout_stride(name, 16)
        flat = R.strided_buffer(q, off, stride)
        assert flat.nbytes == off + 6 * stride + 16
        assert all((flat[off + i * stride: off + i * stride + 16] == q[i]).all() for i in range(7))
        assert (flat[:off] == 0xFF).all() and (stride == 16 or (flat[off + 16: off + stride] == 0xFF).all())
    # the MI355X has 256 compute units
    assert [R.dist_queries_per_range(nq, nc, 256) for _, nq, nc in R.DIST_RANGE_CASES] == [10, 9, 10]
    assert [nq % R.dist_queries_per_range(nq, nc, 256) for _, nq, nc in R.DIST_RANGE_CASES] == [0, 2, 3]


# ---------------------------------------------------------------------------------------------------------------------
# medoids: the weighted reference of medoid_cases.py against the per-row one and against the reference's own values
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nf_short", [False, True])
@pytest.mark.parametrize("nb", [8, 260, 516])
@pytest.mark.parametrize("m", [1, 2, 3, 40, 3000])
def test_weighted_is_the_expanded_set(m, nb, nf_short):
    rng = np.random.default_rng([50, m, nb])
    distinct = np.packbits(rng.random((20, nb * 8)) < rng.uniform(0.05, 0.9, (20, 1)), axis=1)
    distinct[3] = 0
    distinct[4] = 0xFF
    mem = rng.integers(0, 20, m)
    nf = nb * 8 - 16 if nf_short else None
    values = mc.compl_isim_weighted(distinct, np.bincount(mem, minlength=20), nf)
    want = mc.compl_isim_set(distinct[mem], nf)
    assert values.shape == (20,)
    if m < 3:
        assert np.isnan(values).all() and np.isnan(want).all()
        return
    assert (R.bits(values[mem]) == R.bits(want)).all()
    assert mc.weighted_medoid(values, mem) == int(np.argmin(want))


def test_weighted_is_the_references_big_set():
    from pathlib import Path

    from bblean_amd.fingerprints import make_fake_fingerprints

    gold = np.load(Path(__file__).resolve().parent / "golden" / "medoids.npz")
    distinct, draw = mc.big_rows(make_fake_fingerprints)
    counts = np.bincount(draw, minlength=len(distinct))
    assert counts.min() > 0
    values = mc.compl_isim_weighted(distinct, counts)
    assert (R.bits(values) == R.bits(gold["big_compl_distinct"])).all()
    assert mc.weighted_medoid(values, draw) == int(gold["big_medoid"].reshape(-1)[0])


@pytest.mark.parametrize("m,nb,with_zero", [c for c in mc.PLANE_CASES if c[0] <= 1 << 20])
def test_plane_cases_select_their_instances(m, nb, with_zero):
    distinct, mem = mc.plane_distinct(nb), mc.plane_members(m, nb, with_zero)
    assert len(mem) == m and mem.min() == (0 if with_zero else 1) and mem.max() == 47
    kernel, wpl, planes = mc.instance_of(m, nb)
    assert kernel == ("wide" if nb == 516 else "rows") and (nb == 516 or (wpl, planes) == (1 if nb == 8 else 2, mc.PLANE_EXPECT[m]))
    ls = mc.column_sums(distinct, np.bincount(mem, minlength=48))
    assert int(ls[0]) == m - int((mem == 0).sum())
    for lo in (0, mc.FULL_CHUNK * mc.CHUNK):  # chunks whose count of the shared column is exactly 256
        assert (distinct[mem[lo:lo + mc.CHUNK], 0] & mc.SHARED_BIT).all()


def test_plane_instances_are_all_there():
    got = {mc.instance_of(m, nb) for m, nb, _ in mc.PLANE_CASES}
    assert {("rows", w, p) for w in (1, 2) for p in (16, 20, 24, 32)} - got == {("rows", 2, 16), ("rows", 2, 32)}
    assert {("wide", 0, 17), ("wide", 0, 21)} <= got
    # <2, 16> runs in tests/test_hip_medoid.py and in the word-boundary cases; <2, 32> needs 2^24 rows of more than 256 bytes
    assert mc.instance_of(5000, 260) == ("rows", 2, 16)


@pytest.mark.parametrize("first", mc.ARGMIN_FIRST)
def test_argmin_cases_put_the_first_copy_where_they_say(first):
    distinct, mem, r0 = mc.argmin_case(first)
    values = mc.compl_isim_weighted(distinct, np.bincount(mem, minlength=len(distinct)))
    assert np.flatnonzero(values == values.min()).tolist() == [r0]
    assert int(np.flatnonzero(mem == r0)[0]) == first == mc.weighted_medoid(values, mem)

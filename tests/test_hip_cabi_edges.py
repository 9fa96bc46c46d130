r"""Edge cases of the stateless kernels (bblean_amd/csrc/bb_kernels.hip) through the raw C ABI: the arguments the Python
wrappers never pass - strides, misaligned pointers, a supplied `card`, device outputs on a side stream, rows wider than
2048 bits - and the sizes at which a kernel takes another path (tile edges, second loop turns, row splits, the argmin
block's strided scan).  Every comparison is == on integers and on the uint64 bit patterns of the doubles, against the NumPy
references of kernel_refs.py (held against the C oracle by test_kernel_refs.py, on these same case lists).

Left untested: k_pack's block cap (65535 * 16 blocks of 256 output bytes) needs more than 2 GB of input."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kernel_refs as R

pytestmark = pytest.mark.gpu

SENT32 = 0xDEADBEEF
SENT_F64 = -12345.5


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def ok(lib, rc):
    assert rc == 0, (rc, lib.bbh_last_error())


def dev(torch, a: np.ndarray):
    r"""A device copy of a NumPy array, bit for bit (torch has no arithmetic on uint32 / uint64: they travel as int32 / int64)."""
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a).view(view) if view else np.ascontiguousarray(a)).cuda()


def host(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def at(x) -> int | None:
    r"""Address of a host array, a device tensor or None; of a view, its first element."""
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def row_stride(x) -> int:
    return x.strides[0] if isinstance(x, np.ndarray) else x.stride(0)


def call_arr_vec(lib, arr, n, nb, stride, vec, card=None, stream=None):
    r"""bbh_jt_arr_vec with all three outputs on the host -> (sim, inter, union)."""
    sim, inter, union = np.full(n, SENT_F64), np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
    ok(lib, lib.bbh_jt_arr_vec(at(arr), n, nb, stride, at(vec), at(card), sim.ctypes.data, inter.ctypes.data,
                               union.ctypes.data, stream))
    return sim, inter, union


def call_popcount(lib, arr, n, nb, stride, stream=None):
    out = np.full(n, SENT32, np.uint32)
    ok(lib, lib.bbh_popcount_rows(at(arr), n, nb, stride, out.ctypes.data, stream))
    return out


def assert_arr_vec(got, want):
    assert (got[1] == want[1]).all(), "inter"
    assert (got[2] == want[2]).all(), "union"
    assert (R.bits(got[0]) == R.bits(want[0])).all(), "sim"


# ---------------------------------------------------------------------------------------------------------------------
# arr-vec / popcount
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,nb", R.ARR_VEC_CASES)
def test_arr_vec_widths_and_tiles(lib, n, nb):
    arr, vecs = R.arr_vec_inputs(n, nb)
    assert (call_popcount(lib, arr, n, nb, nb) == R.ref_popcount(arr)).all()
    for vec in vecs:
        assert_arr_vec(call_arr_vec(lib, arr, n, nb, nb, vec), R.ref_arr_vec(arr, vec))


@pytest.mark.parametrize("off_arr,off_vec", [(1, 0), (8, 0), (0, 1), (0, 8), (8, 8)])
def test_arr_vec_misaligned_device_pointers(lib, torch, off_arr, off_vec):
    r"""A 16-aligned width whose data (or only whose vector) does not start on a 16-byte boundary: the generic kernel."""
    n, nb = 130, 128
    arr, vecs = R.arr_vec_inputs(n, nb)
    flat = torch.zeros(n * nb + 16, dtype=torch.uint8, device="cuda")
    d_arr = flat[off_arr:off_arr + n * nb]
    d_arr.copy_(dev(torch, arr).reshape(-1))
    assert d_arr.data_ptr() % 16 == off_arr
    for vec in vecs:
        vflat = torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")
        d_vec = vflat[off_vec:off_vec + nb]
        d_vec.copy_(dev(torch, vec))
        assert d_vec.data_ptr() % 16 == off_vec
        assert_arr_vec(call_arr_vec(lib, d_arr, n, nb, nb, d_vec), R.ref_arr_vec(arr, vec))
    assert (call_popcount(lib, d_arr, n, nb, nb) == R.ref_popcount(arr)).all()


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", list(R.STRIDE_LAYOUTS))
def test_arr_vec_strided_views(lib, torch, name, where):
    r"""row_stride != nbytes: the results of a view are those of its contiguous copy.  The host views go through the staging
    copy, which may read (n - 1) * row_stride + nbytes bytes and no more - "cols_44_300_of_300" ends with its buffer."""
    base = R.stride_base(name)
    view_of = R.STRIDE_LAYOUTS[name][2]
    ref = np.ascontiguousarray(view_of(base))
    n, nb = ref.shape
    view = view_of(dev(torch, base)) if where == "device" else view_of(base)
    stride = row_stride(view)
    assert stride != nb and n == R.STRIDE_ROWS
    vec = ref[5].copy()
    assert (call_popcount(lib, view, n, nb, stride) == R.ref_popcount(ref)).all()
    assert_arr_vec(call_arr_vec(lib, view, n, nb, stride, vec), R.ref_arr_vec(ref, vec))
    # and bit for bit what the contiguous copy gives
    assert_arr_vec(call_arr_vec(lib, view, n, nb, stride, vec), call_arr_vec(lib, ref, n, nb, nb, vec))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n,nb", [(130, 256), (65, 48), (70, 272)])
def test_arr_vec_supplied_card(lib, torch, n, nb, where):
    r"""The true popcounts give what NULL gives; other values are used as they are: union = card + |vec| - inter."""
    arr, vecs = R.arr_vec_inputs(n, nb)
    true = R.ref_popcount(arr)
    fake = (true * 3 + 7).astype(np.uint32)
    put = (lambda a: dev(torch, a)) if where == "device" else (lambda a: a)
    for vec in vecs:
        assert_arr_vec(call_arr_vec(lib, arr, n, nb, nb, vec, put(true)), call_arr_vec(lib, arr, n, nb, nb, vec))
        got = call_arr_vec(lib, arr, n, nb, nb, vec, put(fake))
        assert_arr_vec(got, R.ref_arr_vec(arr, vec, fake))
        assert (got[2] == fake + R.POP8[vec].sum() - got[1]).all()


@pytest.mark.parametrize("n,nb", [(130, 256), (65, 80), (70, 100)])
def test_arr_vec_device_outputs_on_side_stream(lib, torch, n, nb):
    r"""Inputs produced on a torch side stream (non-blocking: the default stream does not wait for it), the call enqueued on
    that stream, every output in device memory: nothing is copied, the stream orders it all."""
    arr, vecs = R.arr_vec_inputs(n, nb)
    src, vsrc = dev(torch, arr), dev(torch, vecs[0])
    d_arr, d_vec = torch.zeros_like(src), torch.zeros_like(vsrc)
    sim = torch.full((n,), SENT_F64, dtype=torch.float64, device="cuda")
    inter, union, pc = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d_arr.copy_(src ^ 0xFF).bitwise_xor_(0xFF)
        d_vec.copy_(vsrc)
        ok(lib, lib.bbh_jt_arr_vec(d_arr.data_ptr(), n, nb, nb, d_vec.data_ptr(), None, sim.data_ptr(), inter.data_ptr(),
                                   union.data_ptr(), s.cuda_stream))
        ok(lib, lib.bbh_popcount_rows(d_arr.data_ptr(), n, nb, nb, pc.data_ptr(), s.cuda_stream))
    s.synchronize()
    assert_arr_vec((host(sim, np.float64), host(inter, np.uint32), host(union, np.uint32)), R.ref_arr_vec(arr, vecs[0]))
    assert (host(pc, np.uint32) == R.ref_popcount(arr)).all()


def test_arr_vec_no_rows(lib):
    arr, vec = np.zeros((1, 256), np.uint8), np.zeros(256, np.uint8)
    sim, inter, union = np.full(4, SENT_F64), np.full(4, SENT32, np.uint32), np.full(4, SENT32, np.uint32)
    ok(lib, lib.bbh_jt_arr_vec(arr.ctypes.data, 0, 256, 256, vec.ctypes.data, None, sim.ctypes.data, inter.ctypes.data,
                               union.ctypes.data, None))
    pc = np.full(4, SENT32, np.uint32)
    ok(lib, lib.bbh_popcount_rows(arr.ctypes.data, 0, 256, 256, pc.ctypes.data, None))
    assert (sim == SENT_F64).all() and (inter == SENT32).all() and (union == SENT32).all() and (pc == SENT32).all()


# ---------------------------------------------------------------------------------------------------------------------
# best match
# ---------------------------------------------------------------------------------------------------------------------


def call_best_match(lib, q, nq, c, nc, nb, with_sims, stream=None):
    idx = np.full(nq, -7, np.int32)
    inter, union = np.full(nq, SENT32, np.uint32), np.full(nq, SENT32, np.uint32)
    sims = np.full((nq, nc), SENT_F64) if with_sims else None
    ok(lib, lib.bbh_jt_best_match(at(q), nq, at(c), nc, nb, idx.ctypes.data, inter.ctypes.data, union.ctypes.data, at(sims), stream))
    return idx, inter, union, sims


def assert_best_match(got, want):
    assert got[0].tolist() == want[0].tolist(), "idx"
    assert (got[1] == want[1]).all() and (got[2] == want[2]).all(), "inter / union"
    if got[3] is not None:
        assert (R.bits(got[3]) == R.bits(want[3])).all(), "sims"


@pytest.mark.parametrize("with_sims", [False, True])
def test_best_match_products_pass_2_to_32(lib, with_sims):
    r"""65 536-bit rows: 65536 * 65536 = 2^32.  With 32-bit products the comparison read 0 > 65535 * 65536 and kept index 0
    (observed on an MI355X before k_best_match_generic multiplied in 64 bits)."""
    q, c = R.best_match_overflow_inputs()
    got = call_best_match(lib, q, 1, c, 2, 8192, with_sims)
    assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == (1, 65536, 65536)
    assert_best_match(got, R.ref_best_match(q, c))


@pytest.mark.parametrize("with_sims", [False, True])
def test_best_match_wide_random_rows(lib, with_sims):
    q, c = R.best_match_wide_inputs()
    want = R.ref_best_match(q, c)
    assert want[0][1] == 2  # c[4] == c[2] is q[1]'s maximum: the first of the two
    assert_best_match(call_best_match(lib, q, 3, c, 9, 16384, with_sims), want)


@pytest.mark.parametrize("with_sims", [False, True])
def test_best_match_misaligned_is_generic_and_equal(lib, torch, with_sims):
    r"""2048-bit rows 4 bytes off a 16-byte boundary take the generic kernel: same answer as the fast one on the aligned copy."""
    nq, nc, nb = 130, 9, 256
    q, c = R.best_match_inputs(nq, nc, nb, 2)
    c[5] = c[3]
    qflat = torch.zeros(nq * nb + 16, dtype=torch.uint8, device="cuda")
    cflat = torch.zeros(nc * nb + 16, dtype=torch.uint8, device="cuda")
    dq, dc = qflat[4:4 + nq * nb], cflat[4:4 + nc * nb]
    dq.copy_(dev(torch, q).reshape(-1))
    dc.copy_(dev(torch, c).reshape(-1))
    assert dq.data_ptr() % 16 == 4 and dc.data_ptr() % 16 == 4
    off = call_best_match(lib, dq, nq, dc, nc, nb, with_sims)
    aligned = call_best_match(lib, dev(torch, q), nq, dev(torch, c), nc, nb, with_sims)  # queries and centroids as device tensors
    want = R.ref_best_match(q, c)
    assert_best_match(off, want)
    assert_best_match(aligned, want)


@pytest.mark.parametrize("zero_centroid", [True, False])
def test_best_match_single_centroid(lib, zero_centroid):
    r"""nq = 257 (two blocks of the fast kernel, the second with one row), nc = 1.  Against an all-zero centroid every union
    is the query's popcount, and the all-zero queries report union 0, inter 0, index 0."""
    q, c = R.best_match_inputs(257, 1, 256, 1)
    if zero_centroid:
        c[:] = 0
    got = call_best_match(lib, q, 257, c, 1, 256, True)
    assert_best_match(got, R.ref_best_match(q, c))
    zero_q = np.flatnonzero(R.ref_popcount(q) == 0)
    assert len(zero_q) > 0 and (got[0] == 0).all()
    if zero_centroid:
        assert (got[1] == 0).all() and (got[2] == R.ref_popcount(q)).all() and (got[2][zero_q] == 0).all()
        assert (R.bits(got[3]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# most dissimilar
# ---------------------------------------------------------------------------------------------------------------------


def call_most_dissimilar(lib, Y, n, nb, nf, s1, s2, stream=None):
    i1, i2 = C.c_int64(-7), C.c_int64(-7)
    ok(lib, lib.bbh_most_dissimilar(at(Y), n, nb, nf, C.byref(i1), C.byref(i2), at(s1), at(s2), stream))
    return i1.value, i2.value


def check_most_dissimilar(lib, torch, Y, nf):
    n, nb = Y.shape
    w1, w2, ws1, ws2 = R.ref_most_dissimilar(Y, nf)
    s1, s2 = np.full(n, SENT_F64), np.full(n, SENT_F64)
    assert call_most_dissimilar(lib, Y, n, nb, nf, s1, s2) == (w1, w2)
    assert (R.bits(s1) == R.bits(ws1)).all() and (R.bits(s2) == R.bits(ws2)).all()
    assert call_most_dissimilar(lib, Y, n, nb, nf, None, None) == (w1, w2)
    d1, d2 = (torch.full((n,), SENT_F64, dtype=torch.float64, device="cuda") for _ in range(2))
    assert call_most_dissimilar(lib, dev(torch, Y), n, nb, nf, d1, d2) == (w1, w2)
    torch.cuda.synchronize()
    assert (R.bits(host(d1, np.float64)) == R.bits(ws1)).all() and (R.bits(host(d2, np.float64)) == R.bits(ws2)).all()
    return w1, w2


@pytest.mark.parametrize("n,nb,nf", R.MOST_DISSIMILAR_CASES)
def test_most_dissimilar_strided_scan(lib, torch, n, nb, nf):
    check_most_dissimilar(lib, torch, R.most_dissimilar_inputs(n, nb, nf), nf)


@pytest.mark.parametrize("second_pass", [False, True])
def test_most_dissimilar_tie_between_threads(lib, torch, second_pass):
    r"""The minimum sits in identical rows 45 and 300, which threads 45 and 44 of the argmin block scan: 45 must win."""
    got = check_most_dissimilar(lib, torch, R.most_dissimilar_tie_inputs(second_pass), 2048)
    assert got == ((10, 45) if second_pass else (45, got[1]))


# ---------------------------------------------------------------------------------------------------------------------
# add_rows / isim_rows / unpack / pack
# ---------------------------------------------------------------------------------------------------------------------


def call_add_rows(lib, arr, n, n_cols, packed, nf, out=None, stream=None):
    o = np.full(nf, SENT32, np.uint64) if out is None else out
    ok(lib, lib.bbh_add_rows(at(arr), n, n_cols, packed, nf, at(o), stream))
    return o


def call_isim_rows(lib, arr, n, n_cols, packed, nf):
    out, warn = C.c_double(SENT_F64), C.c_int(-7)
    ok(lib, lib.bbh_isim_rows(at(arr), n, n_cols, packed, nf, C.byref(out), C.byref(warn), None))
    return out.value, warn.value


@pytest.mark.parametrize("n,nb,nf", R.ADD_ROWS_PACKED_CASES)
def test_add_rows_packed_row_splits(lib, torch, n, nb, nf):
    arr = R.add_rows_packed_inputs(n, nb, nf)
    want = R.ref_add_rows_packed(arr, nf)
    assert (call_add_rows(lib, arr, n, nb, 1, nf) == want).all()
    d_out = torch.full((nf,), -1, dtype=torch.int64, device="cuda")
    call_add_rows(lib, dev(torch, arr), n, nb, 1, nf, d_out)
    torch.cuda.synchronize()
    assert (host(d_out, np.uint64) == want).all()
    isim, warn = call_isim_rows(lib, arr, n, nb, 1, nf)
    assert warn == 0 and R.bits(np.float64(isim)) == R.bits(np.float64(R.ref_isim_rows(want, n)))


@pytest.mark.parametrize("n", R.ADD_ROWS_NS)
def test_add_rows_unpacked_row_splits(lib, n):
    arr = R.add_rows_unpacked_inputs(n)
    cols = arr.shape[1]
    want = R.ref_add_rows_unpacked(arr)
    assert (call_add_rows(lib, arr, n, cols, 0, cols) == want).all()
    isim, warn = call_isim_rows(lib, arr, n, cols, 0, cols)
    assert warn == 0 and R.bits(np.float64(isim)) == R.bits(np.float64(R.ref_isim_rows(want, n)))


@pytest.mark.parametrize("n,nb,nf", R.UNPACK_CASES)
def test_unpack_second_turn_and_short_rows(lib, n, nb, nf):
    arr = R.add_rows_packed_inputs(n, nb, nf)
    out = np.full((n, nf), 0xAA, np.uint8)
    ok(lib, lib.bbh_unpack(arr.ctypes.data, n, nb, nf, out.ctypes.data, None))
    assert (out == R.ref_unpack(arr, nf)).all()


@pytest.mark.parametrize("nf", R.PACK_FEATURES)
def test_pack_ragged_last_byte(lib, nf):
    rng = np.random.default_rng([23, nf])
    un = (rng.random((37, nf)) < 0.4).astype(np.uint8) * rng.integers(1, 256, (37, nf), dtype=np.uint8)
    out = np.full((37, (nf + 7) // 8), 0xAA, np.uint8)
    ok(lib, lib.bbh_pack(un.ctypes.data, 37, nf, out.ctypes.data, None))
    assert (out == R.ref_pack(un)).all()


# ---------------------------------------------------------------------------------------------------------------------
# centroid / iSIM from sums
# ---------------------------------------------------------------------------------------------------------------------


def call_centroid(lib, ls, width, nf, n_samples, pack):
    out = np.full((nf + 7) // 8 if pack else nf, 0xAA, np.uint8)
    ok(lib, lib.bbh_centroid_from_sum(at(ls), width, nf, n_samples, pack, out.ctypes.data, None))
    return out


def call_isim(lib, ls, width, nf, n_objects):
    out, warn = C.c_double(SENT_F64), C.c_int(-7)
    ok(lib, lib.bbh_isim_from_sum(at(ls), width, nf, n_objects, C.byref(out), C.byref(warn), None))
    return out.value, warn.value


@pytest.mark.parametrize("n_samples", R.CENTROID_SAMPLES)
@pytest.mark.parametrize("nf", R.CENTROID_FEATURES)
def test_centroid_ties_widths_and_ragged_bytes(lib, torch, n_samples, nf):
    ls = R.centroid_sums(n_samples, nf)
    for pack in (0, 1):
        want = R.ref_centroid(ls, n_samples, bool(pack))
        for width, dt in R.LS_WIDTHS.items():
            assert (call_centroid(lib, ls.astype(dt), width, nf, n_samples, pack) == want).all(), (width, pack)
        assert (call_centroid(lib, dev(torch, ls), 8, nf, n_samples, pack) == want).all()


def test_centroid_single_sample_casts_to_uint8(lib):
    r"""n_samples = 1 is a cast to uint8 (_py_similarity.py:36-41): 256 -> 0, 257 -> 1."""
    ls = np.array([256, 257, 1, 0, 255], np.uint64)
    for width in (2, 4, 8):
        for pack in (0, 1):
            got = call_centroid(lib, ls.astype(R.LS_WIDTHS[width]), width, 5, 1, pack)
            assert (got == R.ref_centroid(ls, 1, bool(pack))).all()
    assert call_centroid(lib, ls.astype(np.uint16), 2, 5, 1, 0).tolist() == [0, 1, 1, 0, 255]
    assert call_centroid(lib, ls.astype(np.uint16), 2, 5, 1, 1).tolist() == [0b01101000]


@pytest.mark.parametrize("nf", R.CENTROID_FEATURES)
def test_isim_from_sum_widths(lib, torch, nf):
    ls = R.isim_sums(nf)
    for n in (2, 3, 255, 100_000):
        want = R.bits(np.float64(R.ref_isim_from_sum(ls, n)))
        for width, dt in R.LS_WIDTHS.items():
            got, warn = call_isim(lib, ls.astype(dt), width, nf, n)
            assert warn == 0 and R.bits(np.float64(got)) == want, (width, n)
        got, warn = call_isim(lib, dev(torch, ls), 8, nf, n)
        assert warn == 0 and R.bits(np.float64(got)) == want
    for width, dt in R.LS_WIDTHS.items():
        for n in (0, 1):
            got, warn = call_isim(lib, ls.astype(dt), width, nf, n)
            assert np.isnan(got) and warn == 1
        assert call_isim(lib, np.zeros(nf, dt), width, nf, 7) == (1.0, 0)


def test_isim_from_sum_moments_wrap(lib):
    ls, n = R.isim_wrap_sums()
    got, warn = call_isim(lib, ls, 8, 64, n)
    assert warn == 0 and R.bits(np.float64(got)) == R.bits(np.float64(R.ref_isim_from_sum(ls, n)))


# ---------------------------------------------------------------------------------------------------------------------
# pair min gap
# ---------------------------------------------------------------------------------------------------------------------


def call_pair_gap(lib, sums, sizes, k, f, stream=None):
    out = C.c_double(SENT_F64)
    ok(lib, lib.bbh_isim_pair_min_gap(at(sums), at(sizes), k, f, C.byref(out), stream))
    return out.value


@pytest.mark.parametrize("k,f", R.PAIR_GAP_CASES)
def test_pair_min_gap(lib, torch, k, f):
    sums, sizes = R.pair_gap_inputs(k, f)
    want = R.bits(np.float64(R.ref_pair_min_gap(sums, sizes)))
    if k == 0:  # (an empty array has no address worth passing: any non-NULL pointer, never read)
        sums, sizes = np.zeros((1, f), np.uint64), np.zeros(1, np.uint64)
    assert R.bits(np.float64(call_pair_gap(lib, sums, sizes, k, f))) == want
    assert R.bits(np.float64(call_pair_gap(lib, dev(torch, sums), dev(torch, sizes), k, f))) == want
    assert R.bits(np.float64(call_pair_gap(lib, dev(torch, sums), sizes, k, f))) == want


def test_pair_min_gap_device_sums_on_side_stream(lib, torch):
    r"""`sums` written by work queued on a non-blocking side stream, the call on that stream: the host-side moments must
    be taken from a copy that waits for that work (a plain hipMemcpy does not, and read the zeros that were there before)."""
    k, f = 5, 2048
    sums, sizes = R.pair_gap_inputs(k, f)
    src, d_sizes = dev(torch, sums), dev(torch, sizes)
    d_sums = torch.zeros_like(src)
    busy = torch.randint(0, 1 << 30, (1 << 22,), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(4):  # a few milliseconds of queued work in front of the write
            busy = busy.sort().values
        d_sums.copy_(src)
        got = call_pair_gap(lib, d_sums, d_sizes, k, f, s.cuda_stream)
    s.synchronize()
    assert R.bits(np.float64(got)) == R.bits(np.float64(R.ref_pair_min_gap(sums, sizes)))


# ---------------------------------------------------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------------------------------------------------


def invalid_calls(lib):
    r"""name -> (call, outputs): every call must return BBH_ERR_INVALID and leave its sentinel-filled outputs alone."""
    a = np.zeros((4, 256), np.uint8)
    v = np.zeros(256, np.uint8)
    u8 = np.zeros((4, 2048), np.uint8)
    ls = np.zeros(64, np.uint64)
    sizes = np.full(4, 2, np.uint64)
    A, V, U8, LS, SZ = a.ctypes.data, v.ctypes.data, u8.ctypes.data, ls.ctypes.data, sizes.ctypes.data
    cases = {}

    def add(name, fn, n_out=1):
        outs = [np.full(4 * 2048, 0xAAAAAAAAAAAAAAAA, np.uint64) for _ in range(n_out)]
        cases[name] = (lambda: fn(*[o.ctypes.data for o in outs]), outs)

    f64p, intp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
    add("popcount: row_stride < nbytes", lambda o: lib.bbh_popcount_rows(A, 4, 256, 255, o, None))
    add("popcount: nbytes = 0", lambda o: lib.bbh_popcount_rows(A, 4, 0, 256, o, None))
    add("popcount: n < 0", lambda o: lib.bbh_popcount_rows(A, -1, 256, 256, o, None))
    add("arr_vec: row_stride < nbytes", lambda s, i, u: lib.bbh_jt_arr_vec(A, 4, 256, 128, V, None, s, i, u, None), 3)
    add("arr_vec: nbytes = 0", lambda s, i, u: lib.bbh_jt_arr_vec(A, 4, 0, 256, V, None, s, i, u, None), 3)
    add("arr_vec: n < 0", lambda s, i, u: lib.bbh_jt_arr_vec(A, -4, 256, 256, V, None, s, i, u, None), 3)
    add("arr_vec: vec = NULL", lambda s, i, u: lib.bbh_jt_arr_vec(A, 4, 256, 256, None, None, s, i, u, None), 3)
    add("best_match: nc = 0", lambda x, i, u, s: lib.bbh_jt_best_match(A, 4, A, 0, 256, x, i, u, s, None), 4)
    add("best_match: nq < 0", lambda x, i, u, s: lib.bbh_jt_best_match(A, -1, A, 4, 256, x, i, u, s, None), 4)
    add("best_match: nbytes = 0", lambda x, i, u, s: lib.bbh_jt_best_match(A, 4, A, 4, 0, x, i, u, s, None), 4)
    add("best_match: out_idx = NULL", lambda i, u, s: lib.bbh_jt_best_match(A, 4, A, 4, 256, None, i, u, s, None), 3)
    add("unpack: n_features % 8", lambda o: lib.bbh_unpack(A, 4, 256, 2044, o, None))
    add("unpack: n_features > nbytes * 8", lambda o: lib.bbh_unpack(A, 4, 256, 2056, o, None))
    add("unpack: nbytes = 0", lambda o: lib.bbh_unpack(A, 4, 0, 0, o, None))
    add("unpack: n < 0", lambda o: lib.bbh_unpack(A, -1, 256, 2048, o, None))
    add("pack: n < 0", lambda o: lib.bbh_pack(U8, -1, 2048, o, None))
    add("pack: n_features = 0", lambda o: lib.bbh_pack(U8, 4, 0, o, None))
    add("add_rows packed: n_features % 8", lambda o: lib.bbh_add_rows(A, 4, 256, 1, 2044, o, None))
    add("add_rows packed: n_features > nbytes * 8", lambda o: lib.bbh_add_rows(A, 4, 256, 1, 2056, o, None))
    add("add_rows unpacked: n_features != n_cols", lambda o: lib.bbh_add_rows(U8, 4, 2048, 0, 2040, o, None))
    add("add_rows: n < 0", lambda o: lib.bbh_add_rows(A, -1, 256, 1, 2048, o, None))
    add("isim_rows packed: n_features % 8",
        lambda o, w: lib.bbh_isim_rows(A, 4, 256, 1, 2044, C.cast(o, f64p), C.cast(w, intp), None), 2)
    add("isim_rows packed: n_features > nbytes * 8",
        lambda o, w: lib.bbh_isim_rows(A, 4, 256, 1, 2056, C.cast(o, f64p), C.cast(w, intp), None), 2)
    add("centroid: ls_width = 3", lambda o: lib.bbh_centroid_from_sum(LS, 3, 64, 4, 1, o, None))
    add("centroid: n_features = 0", lambda o: lib.bbh_centroid_from_sum(LS, 8, 0, 4, 1, o, None))
    add("isim_from_sum: ls_width = 3",
        lambda o, w: lib.bbh_isim_from_sum(LS, 3, 64, 4, C.cast(o, f64p), C.cast(w, intp), None), 2)
    md = lambda n, nb, nf: (lambda i1, i2, s1, s2: lib.bbh_most_dissimilar(A, n, nb, nf, C.cast(i1, i64p), C.cast(i2, i64p),
                                                                          s1, s2, None))
    add("most_dissimilar: n = 0", md(0, 256, 2048), 4)
    add("most_dissimilar: nbytes = 0", md(4, 0, 0), 4)
    add("most_dissimilar: n_features % 8", md(4, 256, 2044), 4)
    add("most_dissimilar: n_features > nbytes * 8", md(4, 256, 2056), 4)
    add("pair_min_gap: k < 0", lambda o: lib.bbh_isim_pair_min_gap(LS, SZ, -1, 16, C.cast(o, f64p), None))
    add("pair_min_gap: sums = NULL", lambda o: lib.bbh_isim_pair_min_gap(None, SZ, 4, 16, C.cast(o, f64p), None))
    add("pair_min_gap: n_features = 0", lambda o: lib.bbh_isim_pair_min_gap(LS, SZ, 4, 0, C.cast(o, f64p), None))
    cases["_keep"] = (None, [a, v, u8, ls, sizes])  # the inputs live as long as the table
    return cases


def test_invalid_arguments_are_refused_before_any_write(lib):
    cases = invalid_calls(lib)
    keep = cases.pop("_keep")
    assert len(cases) >= 30 and keep
    failed = []
    for name, (call, outs) in cases.items():
        rc = call()
        msg = lib.bbh_last_error() or b""
        if rc != 1 or not msg or any((o != 0xAAAAAAAAAAAAAAAA).any() for o in outs):
            failed.append((name, rc, msg))
    assert not failed, failed

r"""Edge cases of the top-k kernels (bblean_amd/csrc/bb_topk.hip) through the raw C ABI, `bbh_jt_topk`: every width
k_topk_bcnt is instantiated for at each of its workgroup sizes, the generic kernel (odd width, pointer offsets, strides,
rows of 65 536 bits), several table ranges and their exact merge, ranges shorter than k, the list's worst and best case,
empty unions, the exclusion, every combination of the optional outputs, device pointers on a side stream, host pointers, and
the argument checks.  The reference is topk_refs.exact_topk (held against the order itself by test_topk_refs.py).  Every
comparison is == on integers; every output buffer is a few elements longer than the call may write and pre-filled with
sentinels.

Left untested: the cap of 65 535 table ranges and row counts near 2^31 (the argument check of nc = 2^31 is here)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import kernel_refs as R
import topk_refs as T

pytestmark = pytest.mark.gpu

PAD = 5
SENT_IDX = -7
SENT32 = 0xDEADBEEF
INVALID = 1  # BBH_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def at(x):
    r"""Address of a host array, a device tensor, an address or None."""
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run_topk(lib, q, nq, stride, c, nc, nb, k, exclude=None, inter=True, union=True, stream=None):
    r"""bbh_jt_topk with host outputs of nq * k + PAD sentinels -> (rc, idx, inter | None, union | None)."""
    n = max(nq, 0) * max(k, 0) + PAD
    oi = np.full(n, SENT_IDX, np.int32)
    on = np.full(n, SENT32, np.uint32) if inter else None
    ou = np.full(n, SENT32, np.uint32) if union else None
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.int32)
    rc = lib.bbh_jt_topk(at(q), nq, stride, at(c), nc, nb, k, at(ex), at(oi), at(on), at(ou), stream)
    return rc, oi, on, ou


def untouched(*arrays):
    sent = {np.dtype(np.int32): SENT_IDX, np.dtype(np.uint32): SENT32}
    return all((a == sent[a.dtype]).all() for a in arrays if a is not None)


def assert_topk(lib, got, want, nq, k, what=""):
    rc, oi, on, ou = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    n = nq * k
    assert untouched(oi[n:], None if on is None else on[n:], None if ou is None else ou[n:]), (what, "tail")
    bad = np.flatnonzero(oi[:n] != want[0].reshape(-1))
    assert bad.size == 0, (what, "idx", bad[:5], oi[bad[:5]], want[0].reshape(-1)[bad[:5]])
    if on is not None:
        assert (on[:n] == want[1].reshape(-1)).all(), (what, "inter")
    if ou is not None:
        assert (ou[:n] == want[2].reshape(-1)).all(), (what, "union")


def check(lib, q, c, k, exclude=None, what=""):
    r"""Host pointers, contiguous rows, all outputs, against exact_topk."""
    nq, nb = q.shape
    want = T.exact_topk(q, c, k, exclude)
    assert_topk(lib, run_topk(lib, q, nq, nb, c, len(c), nb, k, exclude), want, nq, k, what)
    return want


@functools.lru_cache(maxsize=None)
def fast_want(nb, nq, nc, k):
    q, c = T.assign_case(nb, nq, nc)
    return T.exact_topk(q, c, k)


# ---------------------------------------------------------------------------------------------------------------------
# k = 1 is bbh_jt_assign
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_WIDTH_CASES)
def test_k1_is_assign(lib, nb, nq, nc):
    q, c = T.assign_case(nb, nq, nc)
    oi, on, ou = np.empty(nq, np.int32), np.empty(nq, np.uint32), np.empty(nq, np.uint32)
    assert lib.bbh_jt_assign(at(q), nq, nb, at(c), nc, nb, at(oi), at(on), at(ou), None) == 0
    rc, ti, tn, tu = run_topk(lib, q, nq, nb, c, nc, nb, 1)
    assert rc == 0, lib.bbh_last_error()
    assert (ti[:nq] == oi).all() and (tn[:nq] == on).all() and (tu[:nq] == ou).all() and untouched(ti[nq:], tn[nq:], tu[nq:])


# ---------------------------------------------------------------------------------------------------------------------
# the usual widths
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("nb,nq,nc,k", T.FAST_CASES)
def test_every_fast_width(lib, torch, nb, nq, nc, k, where):
    r"""k_topk_bcnt<W32> for W32 = 2 .. 64 at workgroups of 256 (k = 1, 7) and 64 lanes (k = 63, 64): one, just under one,
    exactly one and just over one block of 256 queries, k = nc, and three blocks against several table ranges."""
    q, c = T.assign_case(nb, nq, nc)
    want = fast_want(nb, nq, nc, k)
    if where == "device":
        dq, dc = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
        assert dq.data_ptr() % 4 == 0 and dc.data_ptr() % 4 == 0
        got = run_topk(lib, dq, nq, nb, dc, nc, nb, k)
        torch.cuda.synchronize()
    else:
        got = run_topk(lib, q, nq, nb, c, nc, nb, k)
    assert_topk(lib, got, want, nq, k, (nb, nq, nc, k))


def test_block_of_128_lanes(lib):
    r"""9 <= k <= 24: the workgroup of 128 lanes, two and a part of a third."""
    nb, nq, nc = 64, 257, 63
    for k in (9, 24):
        assert T.topk_block(k) == 128
        q, c = T.assign_case(nb, nq, nc)
        check(lib, q, c, k, what=k)


# ---------------------------------------------------------------------------------------------------------------------
# the generic kernel
# ---------------------------------------------------------------------------------------------------------------------


def test_generic_width(lib):
    nb, nq, nc, k = T.GENERIC_WIDTH_CASE
    assert nb not in R.ASSIGN_FAST_WIDTHS
    q, c = T.assign_case(nb, nq, nc)
    check(lib, q, c, k)
    check(lib, q, c[:64], 64, what="k = nc")


@functools.lru_cache(maxsize=None)
def layout_case(nb):
    nq, nc, k = T.LAYOUT_SHAPE
    q, c = T.assign_case(nb, nq, nc)
    return q, c, T.exact_topk(q, c, k)


@pytest.mark.parametrize("name", list(R.ASSIGN_LAYOUTS))
@pytest.mark.parametrize("nb", [256, 16])
def test_device_alignment_and_strides(lib, torch, nb, name):
    r"""Device bases 4 and 1 bytes off and strides of nbytes + 4, nbytes + 1 and 2 x nbytes (0xFF between the rows):
    k_topk_bcnt where everything is 4-aligned, k_topk_generic otherwise, the same answer."""
    q, c, want = layout_case(nb)
    (nq, nc, k), (qoff, coff, _), stride = T.LAYOUT_SHAPE, R.ASSIGN_LAYOUTS[name], R.layout_stride(name, nb)
    fq = torch.from_numpy(R.strided_buffer(q, qoff, stride)).cuda()
    fc = torch.from_numpy(R.strided_buffer(c, coff, nb)).cuda()
    got = run_topk(lib, fq.data_ptr() + qoff, nq, stride, fc.data_ptr() + coff, nc, nb, k)
    torch.cuda.synchronize()
    assert_topk(lib, got, want, nq, k, (nb, name))


@pytest.mark.parametrize("name", ["stride+4", "stride+1", "stride x2"])
def test_host_strides(lib, name):
    nb = 16
    q, c, want = layout_case(nb)
    (nq, nc, k), stride = T.LAYOUT_SHAPE, R.layout_stride(name, nb)
    flat = R.strided_buffer(q, 0, stride)
    assert flat.nbytes == (nq - 1) * stride + nb
    assert_topk(lib, run_topk(lib, flat, nq, stride, c, nc, nb, k), want, nq, k, name)


@pytest.mark.parametrize("nb", R.ASSIGN_WIDE_WIDTHS)
def test_wide_rows_products_pass_2_to_32(lib, nb):
    r"""65 536-bit rows, k = nc = 40: the whole table in order, by 64-bit cross-multiplication; c[7] == c[5]."""
    nq, nc = R.ASSIGN_WIDE_SHAPE
    q, c = R.assign_wide_inputs(nb)
    want = check(lib, q, c, nc, what=nb)
    assert int(want[1].max()) * int(want[2].max()) >= 1 << 32
    assert want[0][0][0] == 1 and list(want[0][2][:2]) == [5, 7]
    check(lib, q, c, nc - 1, exclude=want[0][:, 0], what=(nb, "exclude"))


# ---------------------------------------------------------------------------------------------------------------------
# ranges and their merge
# ---------------------------------------------------------------------------------------------------------------------


def test_several_ranges(lib, cus):
    nb, nq, nc, k = T.SPLIT_CASE
    assert T.topk_ranges(nq, nc, k, True, cus)[1] > 2
    q, c = T.assign_case(nb, nq, nc)
    check(lib, q, c, k)
    q100, c100 = T.assign_case(100, nq, nc)  # the generic kernel, one wave per query
    assert T.topk_ranges(nq, nc, k, False, cus)[1] > 2
    check(lib, q100, c100, k, what="generic")


def test_range_shorter_than_k(lib, cus):
    nb, nq, nc, k = T.SHORT_RANGE_CASE
    per, nsplit = T.topk_ranges(nq, nc, k, True, cus)
    assert nsplit > 1 and nc - (nsplit - 1) * per < k
    q, c = T.assign_case(nb, nq, nc)
    check(lib, q, c, k)
    check(lib, q, c, k, exclude=[per - 1], what="exclude")
    q100, c100 = T.assign_case(100, nq, nc)
    assert T.topk_ranges(nq, nc, k, False, cus)[1] > 1
    check(lib, q100, c100, k, what="generic")


def test_places_decided_by_the_index_across_ranges(lib, cus):
    nb, nq, nc, k = T.TILED_CASE
    per, nsplit = T.topk_ranges(nq, nc, k, True, cus)
    assert nsplit > 1 and per % 5 != 0
    q, c = T.tiled_inputs()
    want = check(lib, q, c, k)
    assert all(len(np.unique(row)) <= 5 for row in want[3])


@pytest.mark.parametrize("reverse", [False, True])
def test_worst_and_best_case_of_the_list(lib, reverse):
    r"""Every row enters at the head of the list; reversed, nothing enters after the first k."""
    _, nc, k = T.NESTED_CASE
    q, c = T.nested_inputs(reverse)
    want = check(lib, q, c, k, what=reverse)
    assert want[0][0][0] == (0 if reverse else nc - 1)
    q8 = np.repeat(q, 70, axis=0)  # more than one wave, k = 7: the workgroup of 256
    check(lib, q8, c, 7, what=(reverse, 7))


def test_empty_unions_come_first(lib):
    nb, nq, nc, k = T.ZERO_CASE
    q, c = T.zero_inputs()
    want = check(lib, q, c, k)
    z = len(T.ZERO_ROWS)
    assert (want[0][:, :z] == np.array(T.ZERO_ROWS)).all() and (want[2][:, :z] == 0).all() and (want[1][:, :z] == 0).all()
    assert (want[1][:, z:] == 0).all() and (want[2][:, z:] > 0).all()
    check(lib, q, c, k, exclude=[T.ZERO_ROWS[0]] * nq, what="exclude a zero row")


# ---------------------------------------------------------------------------------------------------------------------
# exclude
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["best row", "-1", "nc", "inside a tie group"])
def test_exclude(lib, name):
    nb, nq, nc, k = T.EXCLUDE_SHAPE
    q, c, cases = T.exclude_inputs()
    want = check(lib, q, c, k, exclude=cases[name], what=name)
    if name in ("-1", "nc"):
        assert (want[0] == T.exact_topk(q, c, k)[0]).all()


def test_exclude_k_is_nc_minus_1(lib):
    nb, nq, nc = 16, 40, 41
    q, c = T.assign_case(nb, nq, nc)
    ex = np.arange(nq) % nc
    want = check(lib, q, c, nc - 1, exclude=ex)
    assert all(sorted(row.tolist() + [e]) == list(range(nc)) for row, e in zip(want[0], ex))
    q100, c100 = T.assign_case(100, nq, nc)
    check(lib, q100, c100, nc - 1, exclude=ex, what="generic")


def test_table_against_itself(lib):
    c = T.self_inputs()
    want = check(lib, c, c, 5, exclude=np.arange(len(c)))
    assert want[0][7, 0] == 30 and want[0][30, 0] == 7 and want[0][8, 0] == 50 and want[0][50, 0] == 8
    assert (want[1][[7, 30, 8, 50], 0] == want[2][[7, 30, 8, 50], 0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# outputs, streams, refusals
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc,k", T.OUTPUT_CASES)
def test_optional_outputs(lib, nb, nq, nc, k):
    q, c = T.assign_case(nb, nq, nc)
    want = T.exact_topk(q, c, k)
    for inter, union in ((True, False), (False, True), (False, False), (True, True)):
        got = run_topk(lib, q, nq, nb, c, nc, nb, k, None, inter, union)
        assert (got[2] is None) == (not inter) and (got[3] is None) == (not union)
        assert_topk(lib, got, want, nq, k, (nb, inter, union))


@pytest.mark.parametrize("nb,nq,nc,k", T.OUTPUT_CASES)
def test_device_outputs_on_side_stream(lib, torch, nb, nq, nc, k):
    r"""Inputs produced on a torch side stream, the call enqueued on that stream, every operand and output in device memory
    (the exclusion too), compared after synchronising that stream."""
    q, c = T.assign_case(nb, nq, nc)
    ex = (np.arange(nq) * 7) % nc
    want = T.exact_topk(q, c, k, ex)
    src_q, src_c = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    dq, dc = torch.zeros_like(src_q), torch.zeros_like(src_c)
    dex = torch.zeros(nq, dtype=torch.int32, device="cuda")
    n = nq * k
    oi = torch.full((n + PAD,), SENT_IDX, dtype=torch.int32, device="cuda")
    on = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
    ou = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dq.copy_(src_q ^ 0xFF).bitwise_xor_(0xFF)
        dc.copy_(src_c ^ 0xFF).bitwise_xor_(0xFF)
        dex.copy_(torch.from_numpy(ex.astype(np.int32)).cuda())
        rc = lib.bbh_jt_topk(dq.data_ptr(), nq, nb, dc.data_ptr(), nc, nb, k, dex.data_ptr(), oi.data_ptr(), on.data_ptr(),
                             ou.data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    gi, gn, gu = oi.cpu().numpy(), on.cpu().numpy().view(np.uint32), ou.cpu().numpy().view(np.uint32)
    assert (gi[n:] == SENT_IDX).all() and (gn[n:] == 0xFFFFFFFF).all() and (gu[n:] == 0xFFFFFFFF).all()
    assert (gi[:n] == want[0].reshape(-1)).all() and (gn[:n] == want[1].reshape(-1)).all()
    assert (gu[:n] == want[2].reshape(-1)).all()


# (nq, nc, nbytes, q_stride, k, exclude given)
REFUSED = {
    "nq < 0": (-1, 4, 16, 16, 1, False),
    "nc = 0": (4, 0, 16, 16, 1, False),
    "nc = 2^31": (4, 1 << 31, 16, 16, 1, False),
    "nbytes = 0": (4, 4, 0, 16, 1, False),
    "q_stride < nbytes": (4, 4, 16, 15, 1, False),
    "k = 0": (4, 4, 16, 16, 0, False),
    "k < 0": (4, 4, 16, 16, -1, False),
    "k = 65": (4, 100, 16, 16, 65, False),
    "k > nc": (4, 4, 16, 16, 5, False),
    "k = nc with exclude": (4, 4, 16, 16, 4, True),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID before anything is launched, outputs untouched."""
    nq, nc, nb, stride, k, with_ex = REFUSED[name]
    q, c = np.ones((4, 16), np.uint8), np.ones((100, 16), np.uint8)
    n = 4 * 65 + PAD
    oi, on, ou = np.full(n, SENT_IDX, np.int32), np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
    ex = np.zeros(4, np.int32) if with_ex else None
    rc = lib.bbh_jt_topk(at(q), nq, stride, at(c), nc, nb, k, at(ex), at(oi), at(on), at(ou), None)
    assert rc == INVALID and untouched(oi, on, ou) and lib.bbh_last_error(), name


def test_refusal_of_a_missing_index_output(lib):
    q = np.ones((4, 16), np.uint8)
    on, ou = np.full(4 + PAD, SENT32, np.uint32), np.full(4 + PAD, SENT32, np.uint32)
    assert lib.bbh_jt_topk(at(q), 4, 16, at(q), 4, 16, 1, None, None, at(on), at(ou), None) == INVALID
    assert untouched(on, ou)


def test_limits_accepted(lib):
    r"""k = nc without exclude and k = nc - 1 with it are the last accepted values."""
    q, c = T.assign_case(16, 40, 41)
    check(lib, q, c[:4], 4)
    check(lib, q, c[:4], 3, exclude=np.zeros(40, np.int64))


def test_no_queries(lib):
    r"""nq = 0 is OK and writes nothing."""
    q, c = np.ones((4, 16), np.uint8), np.ones((4, 16), np.uint8)
    got = run_topk(lib, q, 0, 16, c, 4, 16, 2)
    assert got[0] == 0 and untouched(*got[1:])

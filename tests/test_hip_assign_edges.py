r"""Edge cases of the assignment kernels (bblean_amd/csrc/bb_assign.hip) through the raw C ABI, `bbh_jt_assign` and
`bbh_jt_dist_matrix`: every width the popcount kernels are instantiated for, the dispatch boundary, device pointers and
strides that are 4- but not 16-aligned or odd, several queries per grid range and the third grid dimension of the distance
matrix, rows of 65 536 bits, the matrix-core kernel at its accumulator and union bounds, the K order of its two operands,
every combination of the optional outputs, a non-blocking side stream, and the argument checks.  The reference is
kernel_refs.exact (held against the C oracle by test_kernel_refs.py on these same case lists).  Every comparison is == on
integers and on the uint64 bit patterns of the distances; every output buffer is a few elements longer than the call may
write and pre-filled with sentinels.

Left untested: the cap of 65 535 centroid ranges of the assign grid (it needs more than 4 M centroids: at least 64 per
range), and centroid counts near 2^31 (the argument check of nc = 2^31 is here, a call with that many rows is not)."""
from __future__ import annotations

import contextlib
import functools
import os

import numpy as np
import pytest

import kernel_refs as R

pytestmark = pytest.mark.gpu

PAD = 5
SENT_IDX = -7
SENT32 = 0xDEADBEEF
SENT_F64 = -12345.5
INVALID = 1  # BBH_ERR_INVALID


@contextlib.contextmanager
def forced(mode):
    r"""BBHIP_ASSIGN for the calls inside (the library reads it at every call)."""
    old = os.environ.pop("BBHIP_ASSIGN", None)
    if mode is not None:
        os.environ["BBHIP_ASSIGN"] = mode
    try:
        yield
    finally:
        os.environ.pop("BBHIP_ASSIGN", None)
        if old is not None:
            os.environ["BBHIP_ASSIGN"] = old


def modes_for(nbytes):
    return (None, "bcnt", "mfma") if nbytes == 256 else (None, "bcnt")


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def at(x):
    r"""Address of a host array, a device tensor, an address or None."""
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run_assign(lib, q, nq, stride, c, nc, nb, inter=True, union=True, stream=None):
    r"""bbh_jt_assign with host outputs of nq + PAD sentinels -> (rc, idx, inter | None, union | None)."""
    n = max(nq, 0) + PAD
    oi = np.full(n, SENT_IDX, np.int32)
    on = np.full(n, SENT32, np.uint32) if inter else None
    ou = np.full(n, SENT32, np.uint32) if union else None
    rc = lib.bbh_jt_assign(at(q), nq, stride, at(c), nc, nb, at(oi), at(on), at(ou), stream)
    return rc, oi, on, ou


def run_dist(lib, q, nq, stride, c, nc, nb, stream=None):
    out = np.full(max(nq, 0) * max(nc, 0) + PAD, SENT_F64)
    rc = lib.bbh_jt_dist_matrix(at(q), nq, stride, at(c), nc, nb, at(out), stream)
    return rc, out


def untouched(*arrays):
    sent = {np.dtype(np.int32): SENT_IDX, np.dtype(np.uint32): SENT32, np.dtype(np.float64): SENT_F64}
    return all((a == sent[a.dtype]).all() for a in arrays if a is not None)


def assert_assign(lib, got, want, nq, what=""):
    rc, oi, on, ou = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    assert untouched(oi[nq:], None if on is None else on[nq:], None if ou is None else ou[nq:]), (what, "tail")
    bad = np.flatnonzero(oi[:nq] != want[0])
    assert bad.size == 0, (what, "idx", bad[:5], oi[bad[:5]], want[0][bad[:5]])
    if on is not None:
        assert (on[:nq] == want[1]).all(), (what, "inter")
    if ou is not None:
        assert (ou[:nq] == want[2]).all(), (what, "union")


def assert_dist(lib, got, want, what=""):
    rc, out = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    assert untouched(out[want.size:]), (what, "tail")
    bad = np.flatnonzero(R.bits(out[:want.size]) != R.bits(want).reshape(-1))
    assert bad.size == 0, (what, "dist", bad[:5], out[bad[:5]], want.reshape(-1)[bad[:5]])


def check_both(lib, q, c, nq, nc, nb, stride, want, what, mfma_ok=True, dist=True):
    r"""bbh_jt_assign under every mode the width allows and bbh_jt_dist_matrix, on the given pointers.  Where the 16-byte
    rule of the matrix-core kernel fails, the forced mode is refused and writes nothing."""
    for mode in modes_for(nb):
        with forced(mode):
            got = run_assign(lib, q, nq, stride, c, nc, nb)
        if mode == "mfma" and not mfma_ok:
            assert got[0] == INVALID and untouched(*got[1:]), (what, mode)
        else:
            assert_assign(lib, got, want, nq, (what, mode))
    if dist:
        assert_dist(lib, run_dist(lib, q, nq, stride, c, nc, nb), want[3], what)


@functools.lru_cache(maxsize=None)
def width_case(nb, nq, nc):
    q, c = R.assign_inputs(nb, nq, nc)
    return q, c, R.exact(q, c)


# ---------------------------------------------------------------------------------------------------------------------
# widths and dispatch
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_WIDTH_CASES)
def test_every_fast_width(lib, torch, nb, nq, nc, where):
    r"""k_assign_bcnt<W32> and k_jaccard_dist<W32> for W32 = 2, 4, 8, 16, 32, 64: one, just under one, exactly one and just
    over one query block of 256, and three blocks against several centroid ranges."""
    assert nb in (8, 16, 32, 64, 128, 256) and sorted({w for w, _, _ in R.ASSIGN_WIDTH_CASES}) == [8, 16, 32, 64, 128, 256]
    q, c, want = width_case(nb, nq, nc)
    if nq > 2:
        assert not q[nq // 2].any() and not c[nc // 3].any()
    if where == "device":
        dq, dc = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
        assert dq.data_ptr() % 16 == 0 and dc.data_ptr() % 16 == 0
        check_both(lib, dq, dc, nq, nc, nb, nb, want, (nb, nq, nc))
        torch.cuda.synchronize()
    else:
        check_both(lib, q, c, nq, nc, nb, nb, want, (nb, nq, nc))


@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_DISPATCH_CASES)
def test_dispatch_boundary(lib, nb, nq, nc):
    r"""Both sides of nq >= 64 and nc >= 64, the rule that sends 2048-bit rows to the matrix cores."""
    q, c, want = width_case(nb, nq, nc)
    check_both(lib, q, c, nq, nc, nb, nb, want, (nb, nq, nc))


# ---------------------------------------------------------------------------------------------------------------------
# alignment and strides
# ---------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def align_case(nb):
    nq, nc = R.ASSIGN_ALIGN_SHAPE
    q, c = R.assign_inputs(nb, nq, nc)
    return q, c, R.exact(q, c)


@pytest.mark.parametrize("name", list(R.ASSIGN_LAYOUTS))
@pytest.mark.parametrize("nb", [256, 16])
def test_device_alignment_and_strides(lib, torch, nb, name):
    r"""Device bases 4 and 1 bytes off a 16-byte boundary and strides of nbytes + 4, nbytes + 1 and 2 x nbytes (0xFF between
    the rows): another kernel, the same answer as the contiguous aligned call."""
    q, c, want = align_case(nb)
    (nq, nc), (qoff, coff, _), stride = R.ASSIGN_ALIGN_SHAPE, R.ASSIGN_LAYOUTS[name], R.layout_stride(name, nb)
    fq = torch.from_numpy(R.strided_buffer(q, qoff, stride)).cuda()
    fc = torch.from_numpy(R.strided_buffer(c, coff, nb)).cuda()
    assert fq.data_ptr() % 16 == 0 and fc.data_ptr() % 16 == 0
    qa, ca = fq.data_ptr() + qoff, fc.data_ptr() + coff
    mfma_ok = nb == 256 and qa % 16 == 0 and ca % 16 == 0 and stride % 16 == 0
    assert mfma_ok == (name == "stride x2" and nb == 256)
    check_both(lib, qa, ca, nq, nc, nb, stride, want, (nb, name), mfma_ok)
    aligned = run_assign(lib, torch.from_numpy(q).cuda(), nq, nb, torch.from_numpy(c).cuda(), nc, nb)
    assert_assign(lib, aligned, want, nq, (nb, "aligned"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["stride+4", "stride+1", "stride x2"])
@pytest.mark.parametrize("nb", [256, 16])
def test_host_strides(lib, nb, name):
    r"""The same strided layouts from host memory: the staging copy takes (nq - 1) * q_stride + nbytes bytes, and the
    buffer ends with the last row's last byte."""
    q, c, want = align_case(nb)
    (nq, nc), stride = R.ASSIGN_ALIGN_SHAPE, R.layout_stride(name, nb)
    flat = R.strided_buffer(q, 0, stride)
    assert flat.nbytes == (nq - 1) * stride + nb
    check_both(lib, flat, c, nq, nc, nb, stride, want, (nb, name), mfma_ok=nb == 256 and stride % 16 == 0)


# ---------------------------------------------------------------------------------------------------------------------
# distance matrix: query ranges and the third grid dimension
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", R.DIST_RANGE_CASES)
def test_dist_several_queries_per_range(lib, torch, nb, nq, nc):
    r"""k_jaccard_dist's loop over the queries of a grid range.  With the 256 compute units of an MI355X a range holds 10,
    9 and 10 queries; the last range of (4097, 257) and (5003, 300) is ragged, (5000, 300) divides evenly."""
    per = R.dist_queries_per_range(nq, nc, torch.cuda.get_device_properties(0).multi_processor_count)
    assert per > 1
    if (nq, nc) != (5000, 300):
        assert nq % per != 0
    q, c, want = width_case(nb, nq, nc)
    assert_dist(lib, run_dist(lib, q, nq, nb, c, nc, nb), want[3], (nq, nc))
    assert_assign(lib, run_assign(lib, q, nq, nb, c, nc, nb), want, nq, (nq, nc))


def test_dist_ragged_range_exists(torch):
    assert any(nq % R.dist_queries_per_range(nq, nc, torch.cuda.get_device_properties(0).multi_processor_count)
               for _, nq, nc in R.DIST_RANGE_CASES)


def test_dist_grid_z(lib):
    r"""k_jaccard_dist_generic: more queries than blockIdx.y holds."""
    nb, nq, nc = R.DIST_GRID_Z_CASE
    assert nq > 65535 and nb not in R.ASSIGN_FAST_WIDTHS
    q, c, want = width_case(nb, nq, nc)
    assert_dist(lib, run_dist(lib, q, nq, nb, c, nc, nb), want[3], "grid z")
    assert_assign(lib, run_assign(lib, q, nq, nb, c, nc, nb), want, nq, "grid z")


# ---------------------------------------------------------------------------------------------------------------------
# wide rows
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb", R.ASSIGN_WIDE_WIDTHS)
def test_wide_rows_products_pass_2_to_32(lib, nb):
    r"""k_assign_generic on 65 536-bit rows: the cross-multiplication needs 64 bits."""
    nq, nc = R.ASSIGN_WIDE_SHAPE
    q, c = R.assign_wide_inputs(nb)
    want = R.exact(q, c)
    assert int(want[1].max()) * int(want[2].max()) >= 1 << 32
    assert want[0][0] == 1 and want[1][0] == want[2][0] == nb * 8  # the all-ones pair behind the row with one bit less
    assert want[0][2] == 5 and (c[5] == c[7]).all()
    check_both(lib, q, c, nq, nc, nb, nb, want, nb)


# ---------------------------------------------------------------------------------------------------------------------
# matrix cores
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nc", R.MFMA_LIMIT_NCS)
def test_matrix_cores_at_their_limits(lib, nc):
    r"""Accumulators of 2048 (all ones against all ones), the union of 6144 of an all-ones query with a padded centroid
    row, all-zero rows on both sides, and padded rows in every lane group (nc = 1, 65) and in a whole wave half (nc = 1, 129
    in the second tile)."""
    nq = R.MFMA_LIMIT_NQ
    q, c = R.mfma_limit_inputs(nc)
    want = R.exact(q, c)
    assert R.ref_popcount(q).max() == 2048 and R.ref_popcount(c).max() == 2048 and want[1].max() == 2048
    assert R.ref_popcount(q).min() == 0
    check_both(lib, q, c, nq, nc, 256, 256, want, nc)


@pytest.mark.parametrize("nb", R.ONE_HOT_WIDTHS)
def test_one_hot_rows_same_k_order(lib, nb):
    r"""Every bit position alone, against the same rows in another order: both operands must take the bits through the same
    order, in the LDS expansion of the matrix-core kernel and in the word loops of the popcount kernels."""
    q, c, where = R.one_hot_inputs(nb)
    n = nb * 8
    want = R.exact(q, c)
    assert (want[0] == where).all() and (want[1] == 1).all() and (want[2] == 1).all() and len(c) == n + 1
    check_both(lib, q, c, n, n + 1, nb, nb, want, nb)


# ---------------------------------------------------------------------------------------------------------------------
# outputs, streams, refusals
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_OUTPUT_CASES)
def test_optional_outputs(lib, nb, nq, nc):
    q, c, want = width_case(nb, nq, nc)
    for inter, union in ((True, False), (False, True), (False, False), (True, True)):
        for mode in modes_for(nb):
            with forced(mode):
                got = run_assign(lib, q, nq, nb, c, nc, nb, inter, union)
            assert (got[2] is None) == (not inter) and (got[3] is None) == (not union)
            assert_assign(lib, got, want, nq, (nb, inter, union, mode))


@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_OUTPUT_CASES)
def test_device_outputs_on_side_stream(lib, torch, nb, nq, nc):
    r"""Inputs produced on a torch side stream (non-blocking: the default stream does not wait for it), the calls enqueued
    on that stream, every output in device memory and compared after synchronising that stream."""
    q, c, want = width_case(nb, nq, nc)
    src_q, src_c = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    dq, dc = torch.zeros_like(src_q), torch.zeros_like(src_c)
    modes = modes_for(nb)
    oi = [torch.full((nq + PAD,), SENT_IDX, dtype=torch.int32, device="cuda") for _ in modes]
    on = [torch.full((nq + PAD,), -1, dtype=torch.int32, device="cuda") for _ in modes]
    ou = [torch.full((nq + PAD,), -1, dtype=torch.int32, device="cuda") for _ in modes]
    od = torch.full((nq * nc + PAD,), SENT_F64, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dq.copy_(src_q ^ 0xFF).bitwise_xor_(0xFF)
        dc.copy_(src_c ^ 0xFF).bitwise_xor_(0xFF)
        for k, mode in enumerate(modes):
            with forced(mode):
                rc = lib.bbh_jt_assign(dq.data_ptr(), nq, nb, dc.data_ptr(), nc, nb, oi[k].data_ptr(), on[k].data_ptr(),
                                       ou[k].data_ptr(), s.cuda_stream)
            assert rc == 0, (mode, lib.bbh_last_error())
        rc = lib.bbh_jt_dist_matrix(dq.data_ptr(), nq, nb, dc.data_ptr(), nc, nb, od.data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    for k, mode in enumerate(modes):
        gi, gn, gu = oi[k].cpu().numpy(), on[k].cpu().numpy().view(np.uint32), ou[k].cpu().numpy().view(np.uint32)
        assert (gi[nq:] == SENT_IDX).all() and (gn[nq:] == 0xFFFFFFFF).all() and (gu[nq:] == 0xFFFFFFFF).all(), mode
        assert (gi[:nq] == want[0]).all() and (gn[:nq] == want[1]).all() and (gu[:nq] == want[2]).all(), mode
    gd = od.cpu().numpy()
    assert (gd[nq * nc:] == SENT_F64).all()
    assert (R.bits(gd[:nq * nc]) == R.bits(want[3]).reshape(-1)).all()


# (nq, nc, nbytes, q_stride): refused by both entry points
REFUSED_BY_BOTH = {
    "nq < 0": (-1, 4, 16, 16),
    "nc = 0": (4, 0, 16, 16),
    "nbytes = 0": (4, 4, 0, 16),
    "q_stride < nbytes": (4, 4, 16, 15),
}


@pytest.mark.parametrize("name", list(REFUSED_BY_BOTH))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID before anything is launched, outputs untouched."""
    nq, nc, nb, stride = REFUSED_BY_BOTH[name]
    q, c = np.ones((4, 16), np.uint8), np.ones((4, 16), np.uint8)
    got = run_assign(lib, q, nq, stride, c, nc, nb)
    assert got[0] == INVALID and untouched(*got[1:]) and lib.bbh_last_error(), name
    out = np.full(16 + PAD, SENT_F64)
    assert lib.bbh_jt_dist_matrix(at(q), nq, stride, at(c), nc, nb, at(out), None) == INVALID and untouched(out), name


def test_refusals_of_one_entry_point(lib):
    q, c = np.ones((4, 16), np.uint8), np.ones((4, 16), np.uint8)
    got = run_assign(lib, q, 4, 16, c, 1 << 31, 16)  # nc = 2^31: the centroid index is an int32
    assert got[0] == INVALID and untouched(*got[1:])
    on, ou = np.full(4 + PAD, SENT32, np.uint32), np.full(4 + PAD, SENT32, np.uint32)
    assert lib.bbh_jt_assign(at(q), 4, 16, at(c), 4, 16, None, at(on), at(ou), None) == INVALID  # NULL out_idx
    assert untouched(on, ou)
    assert lib.bbh_jt_dist_matrix(at(q), 4, 16, at(c), 4, 16, None, None) == INVALID  # NULL out


def test_no_queries(lib):
    r"""nq = 0 is OK and writes nothing."""
    q, c = np.ones((4, 16), np.uint8), np.ones((4, 16), np.uint8)
    got = run_assign(lib, q, 0, 16, c, 4, 16)
    assert got[0] == 0 and untouched(*got[1:])
    rc, out = run_dist(lib, q, 0, 16, c, 4, 16)
    assert rc == 0 and untouched(out)

r"""Edge cases of the radius-search kernels (bblean_amd/csrc/bb_radius.hip) through the raw C ABI, `bbh_jt_radius`: every
width k_radius_bcnt is instantiated for, radii on, just below and just above realised distances (the table of smallest
passing intersections at 32-byte rows, the division at 100-byte rows), the generic kernel (odd width, pointer offsets,
strides, rows of 65 600 bits), several table ranges, the exclusion, the capacity protocol, every combination of the optional
outputs, device pointers on a side stream, and the argument checks.  The reference is radius_refs.exact_radius (held
against the semantics by test_radius_refs.py).  Every comparison is == on integers; every output buffer is a few elements
longer than the call may write and pre-filled with sentinels.

Left untested: the cap of 65 535 table ranges, row counts near 2^31 (the argument check of nc = 2^31 is here) and a total
beyond 2^31 entries."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import kernel_refs as R
import radius_refs as X
import topk_refs as T

pytestmark = pytest.mark.gpu

PAD = 7
SENT_IDX = -7
SENT32 = 0xDEADBEEF
SENT64 = -0x0123456789ABCDEF
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


def run_radius(lib, q, nq, stride, c, nc, nb, radius, exclude=None, capacity=None, room=0, inter=True, union=True,
               idx=True, stream=None):
    r"""bbh_jt_radius with host outputs of `room` + PAD sentinels (capacity = room unless given)
    -> (rc, offsets, total, idx | None, inter | None, union | None)."""
    off = np.full(max(nq, 0) + 1 + PAD, SENT64, np.int64)
    tot = np.full(1 + PAD, SENT64, np.int64)
    oi = np.full(room + PAD, SENT_IDX, np.int32) if idx else None
    on = np.full(room + PAD, SENT32, np.uint32) if inter else None
    ou = np.full(room + PAD, SENT32, np.uint32) if union else None
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.int32)
    rc = lib.bbh_jt_radius(at(q), nq, stride, at(c), nc, nb, radius, at(ex), room if capacity is None else capacity,
                           at(off), at(tot), at(oi), at(on), at(ou), stream)
    return rc, off, tot, oi, on, ou


def untouched(*arrays):
    sent = {np.dtype(np.int32): SENT_IDX, np.dtype(np.uint32): SENT32, np.dtype(np.int64): SENT64}
    return all((a == sent[a.dtype]).all() for a in arrays if a is not None)


def assert_radius(lib, got, want, nq, filled=True, what=""):
    r"""Offsets and total always; the first total entries of the outputs where `filled`, sentinels everywhere else."""
    rc, off, tot, oi, on, ou = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    n = int(want[0][-1])
    assert (off[:nq + 1] == want[0]).all() and untouched(off[nq + 1:]), (what, "offsets")
    assert tot[0] == n and untouched(tot[1:]), (what, "total", int(tot[0]), n)
    if not filled:
        assert untouched(oi, on, ou), (what, "filled beyond the capacity")
        return
    assert untouched(None if oi is None else oi[n:], None if on is None else on[n:], None if ou is None else ou[n:]), (what, "tail")
    if oi is not None:
        bad = np.flatnonzero(oi[:n] != want[1])
        assert bad.size == 0, (what, "idx", bad[:5], oi[bad[:5]], want[1][bad[:5]])
    if on is not None:
        assert (on[:n] == want[2]).all(), (what, "inter")
    if ou is not None:
        assert (ou[:n] == want[3]).all(), (what, "union")


def check(lib, q, c, radius, exclude=None, what=""):
    r"""Host pointers, contiguous rows, all outputs, room for exactly the answer, against exact_radius."""
    nq, nb = q.shape
    want = X.exact_radius(q, c, radius, exclude)
    got = run_radius(lib, q, nq, nb, c, len(c), nb, radius, exclude, room=int(want[0][-1]))
    assert_radius(lib, got, want, nq, what=(what, radius))
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the usual widths
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", R.ASSIGN_WIDTH_CASES)
def test_every_fast_width(lib, nb, nq, nc):
    r"""k_radius_bcnt<W32> for W32 = 2 .. 64: one, just under one, exactly one and just over one block of 256 queries, and
    three blocks against several table ranges; the all-zero query and row (u == 0) are in.  No hits, the identical rows and
    empty unions, every row, and half of the pairs."""
    q, c = X.assign_case(nb, nq, nc)
    for radius in X.FIXED_RADII + (X.median_radius(nb, nq, nc),):
        want = check(lib, q, c, radius, what=(nb, nq, nc))
        if radius == 1.0:
            assert want[0][-1] == nq * nc
        if radius == -1.0:
            assert want[0][-1] == 0


def test_device_rows_give_the_same(lib, torch):
    nb, nq, nc = 64, 513, 700
    q, c = X.assign_case(nb, nq, nc)
    radius = X.median_radius(nb, nq, nc)
    want = X.exact_radius(q, c, radius)
    dq, dc = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    assert dq.data_ptr() % 4 == 0 and dc.data_ptr() % 4 == 0
    got = run_radius(lib, dq, nq, nb, dc, nc, nb, radius, room=int(want[0][-1]))
    assert_radius(lib, got, want, nq)


# ---------------------------------------------------------------------------------------------------------------------
# on, just below and just above a realised distance
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb", [32, 100])
@pytest.mark.parametrize("all_ones", [False, True])
def test_boundary(lib, nb, all_ones):
    r"""A query against its 241 nested subsets: d takes every multiple of 1 / 240 (of 1 / 256 for the all-ones query, where
    u = nbits at 32 bytes).  For ten realised values v, 1 / 3 among them: the hit count steps exactly at v - radius v takes
    the pair at v, the float64 just below does not, the float64 just above takes nothing more.  32 bytes: the table of
    k_radius_bcnt; 100 bytes: the division of k_radius_generic."""
    q, c, n_set = X.boundary_inputs(nb, all_ones)
    d = R.exact(q, c)[3][0]
    for v in X.boundary_values(n_set):
        lo, at_v, hi = X.boundary_radii(v)
        counts = [int(check(lib, q, c, r, what=(nb, all_ones, v))[0][-1]) for r in (lo, at_v, hi)]
        assert counts[1] == counts[0] + 1 == counts[2] == int((d <= v).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the generic kernel
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", X.GENERIC_CASES)
def test_generic_widths(lib, nb, nq, nc):
    r"""100-byte rows, and 8200-byte rows (65 600 bits, beyond any table; c[7] == c[5], an all-zero row)."""
    q, c = X.assign_case(nb, nq, nc) if nb == 100 else R.assign_wide_inputs(nb)
    assert q.shape == (nq, nb) and c.shape == (nc, nb)
    d = R.exact(q, c)[3]
    for radius in X.FIXED_RADII + (float(np.median(d)), float(np.sort(d, axis=None)[d.size // 4])):
        check(lib, q, c, radius, what=nb)
    check(lib, q, c, float(np.median(d)), exclude=np.arange(nq) % nc, what=(nb, "exclude"))


@functools.lru_cache(maxsize=None)
def layout_case(nb):
    nq, nc = X.LAYOUT_SHAPE
    q, c = X.assign_case(nb, nq, nc)
    radius = X.median_radius(nb, nq, nc)
    return q, c, radius, X.exact_radius(q, c, radius)


@pytest.mark.parametrize("name", list(R.ASSIGN_LAYOUTS))
@pytest.mark.parametrize("nb", [256, 16])
def test_device_alignment_and_strides(lib, torch, nb, name):
    r"""Device bases 4 and 1 bytes off and strides of nbytes + 4, nbytes + 1 and 2 x nbytes (0xFF between the rows):
    k_radius_bcnt where everything is 4-aligned, k_radius_generic otherwise, the same answer."""
    q, c, radius, want = layout_case(nb)
    (nq, nc), (qoff, coff, _), stride = X.LAYOUT_SHAPE, R.ASSIGN_LAYOUTS[name], R.layout_stride(name, nb)
    fq = torch.from_numpy(R.strided_buffer(q, qoff, stride)).cuda()
    fc = torch.from_numpy(R.strided_buffer(c, coff, nb)).cuda()
    got = run_radius(lib, fq.data_ptr() + qoff, nq, stride, fc.data_ptr() + coff, nc, nb, radius, room=int(want[0][-1]))
    assert_radius(lib, got, want, nq, what=(nb, name))


@pytest.mark.parametrize("name", ["stride+4", "stride+1", "stride x2"])
def test_host_strides(lib, name):
    nb = 16
    q, c, radius, want = layout_case(nb)
    (nq, nc), stride = X.LAYOUT_SHAPE, R.layout_stride(name, nb)
    flat = R.strided_buffer(q, 0, stride)
    assert flat.nbytes == (nq - 1) * stride + nb
    assert_radius(lib, run_radius(lib, flat, nq, stride, c, nc, nb, radius, room=int(want[0][-1])), want, nq, what=name)


# ---------------------------------------------------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------------------------------------------------


def test_several_ranges(lib, cus):
    r"""Five distinct rows tiled to 700 and a radius at a realised distance: hits on both sides of every range edge, each
    lane's part of the output starting where the ranges before it end."""
    nb, nq, nc = X.SPLIT_CASE
    per, nsplit = X.radius_ranges(nq, nc, True, cus)
    assert nsplit > 2
    q, c = X.split_inputs()
    radius = X.split_radius()
    want = check(lib, q, c, radius)
    hits = want[1][want[0][0]:want[0][1]]
    for s in range(1, nsplit):
        assert ((hits >= s * per - 5) & (hits < s * per)).any() and ((hits >= s * per) & (hits < s * per + 5)).any()
    check(lib, q, c, radius, exclude=[per - 1, per, nc - 1], what="exclude at the edges")
    q100 = np.concatenate([q, np.zeros((nq, 68), np.uint8)], axis=1)  # the generic kernel, one wave per query: the
    c100 = np.concatenate([c, np.zeros((nc, 68), np.uint8)], axis=1)  # same counts, so the same answer
    assert X.radius_ranges(nq, nc, False, cus)[1] > 2
    w100 = check(lib, q100, c100, radius, what="generic")
    assert (w100[1] == want[1]).all() and (w100[0] == want[0]).all()


def test_scan_over_several_turns(lib):
    r"""2500 queries: k_radius_scan takes three turns of 1024 (the last one ragged) with a carry between them, and
    k_radius_bcnt ten query tiles."""
    nb, nq, nc = 8, 2500, 70
    q, c = X.assign_case(nb, nq, nc)
    want = check(lib, q, c, X.median_radius(nb, nq, nc))
    assert want[0][1024] > 0 and want[0][2048] > want[0][1024] and want[0][-1] > want[0][2048]
    q100, c100 = X.assign_case(100, nq, 9)
    check(lib, q100, c100, X.median_radius(100, nq, 9), what="generic")


# ---------------------------------------------------------------------------------------------------------------------
# exclude
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["best row", "-1", "nc", "inside a tie group"])
def test_exclude(lib, name):
    q, c, cases, radius = X.exclude_inputs()
    want = check(lib, q, c, radius, exclude=cases[name], what=name)
    plain = X.exact_radius(q, c, radius)
    if name in ("-1", "nc"):
        assert (want[1] == plain[1]).all()
    else:
        assert want[0][-1] < plain[0][-1]


def test_every_row_without_the_excluded_one(lib):
    nb, nq, nc = 16, 40, 41
    q, c = X.assign_case(nb, nq, nc)
    ex = np.arange(nq) % nc
    want = check(lib, q, c, 1.0, exclude=ex)
    assert want[0][-1] == nq * (nc - 1)
    want = check(lib, q, c, float("inf"), exclude=ex)
    assert want[0][-1] == nq * (nc - 1)
    assert check(lib, q, c, float("-inf"), exclude=ex)[0][-1] == 0


def test_table_against_itself(lib):
    c = T.self_inputs()
    want = check(lib, c, c, 0.0, exclude=np.arange(len(c)))
    assert want[1].tolist() == [30, 50, 7, 8] and (want[2] == want[3]).all()
    assert check(lib, c, c, 0.0)[0][-1] == len(c) + 4
    assert check(lib, c, c, -0.0)[0][-1] == len(c) + 4


# ---------------------------------------------------------------------------------------------------------------------
# the capacity protocol
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb", [X.CAPACITY_CASE[0], 100])
def test_capacity_protocol(lib, nb):
    r"""The call always writes the offsets and the total; it fills the outputs only where the whole answer fits."""
    _, nq, nc = X.CAPACITY_CASE
    q, c = X.assign_case(nb, nq, nc)
    radius = X.median_radius(nb, nq, nc)
    want = X.exact_radius(q, c, radius)
    total = int(want[0][-1])
    assert total > 7
    # the pure count: capacity 0, no outputs at all
    got = run_radius(lib, q, nq, nb, c, nc, nb, radius, capacity=0, idx=False, inter=False, union=False)
    assert got[3] is None and got[4] is None and got[5] is None
    assert_radius(lib, got, want, nq, filled=False, what="count")
    # capacity 0 with outputs: still nothing filled
    assert_radius(lib, run_radius(lib, q, nq, nb, c, nc, nb, radius, capacity=0, room=total), want, nq, filled=False)
    # one short: offsets and total written, every output still sentinel
    got = run_radius(lib, q, nq, nb, c, nc, nb, radius, capacity=total - 1, room=total)
    assert_radius(lib, got, want, nq, filled=False, what="total - 1")
    # exactly enough, and more than enough: the tail stays sentinel
    assert_radius(lib, run_radius(lib, q, nq, nb, c, nc, nb, radius, room=total), want, nq, what="total")
    assert_radius(lib, run_radius(lib, q, nq, nb, c, nc, nb, radius, room=total + 7), want, nq, what="total + 7")


def test_no_hits_and_a_capacity(lib):
    r"""total = 0 <= capacity: nothing to fill, the outputs untouched."""
    nb, nq, nc = X.CAPACITY_CASE
    q, c = X.assign_case(nb, nq, nc)
    want = X.exact_radius(q, c, -1.0)
    assert_radius(lib, run_radius(lib, q, nq, nb, c, nc, nb, -1.0, room=9), want, nq)


def test_no_queries(lib):
    r"""nq = 0: offsets = [0], total 0, nothing else written."""
    q, c = np.ones((4, 16), np.uint8), np.ones((4, 16), np.uint8)
    got = run_radius(lib, q, 0, 16, c, 4, 16, 0.5, room=3)
    assert got[0] == 0 and got[1][0] == 0 and untouched(got[1][1:]) and got[2][0] == 0 and untouched(got[2][1:])
    assert untouched(*got[3:])


# ---------------------------------------------------------------------------------------------------------------------
# outputs, streams, refusals
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nb,nq,nc", X.OUTPUT_CASES)
def test_optional_outputs(lib, nb, nq, nc):
    q, c = X.assign_case(nb, nq, nc)
    radius = X.median_radius(nb, nq, nc)
    want = X.exact_radius(q, c, radius)
    for inter, union in ((True, False), (False, True), (False, False), (True, True)):
        got = run_radius(lib, q, nq, nb, c, nc, nb, radius, room=int(want[0][-1]), inter=inter, union=union)
        assert (got[4] is None) == (not inter) and (got[5] is None) == (not union)
        assert_radius(lib, got, want, nq, what=(nb, inter, union))


@pytest.mark.parametrize("nb,nq,nc", X.OUTPUT_CASES)
def test_device_outputs_on_side_stream(lib, torch, nb, nq, nc):
    r"""Inputs produced on a torch side stream, the call enqueued on that stream, every operand and output in device memory
    (the exclusion, the offsets and the total too), compared after synchronising that stream."""
    q, c = X.assign_case(nb, nq, nc)
    ex = (np.arange(nq) * 7) % nc
    radius = X.median_radius(nb, nq, nc)
    want = X.exact_radius(q, c, radius, ex)
    n = int(want[0][-1])
    src_q, src_c = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    dq, dc = torch.zeros_like(src_q), torch.zeros_like(src_c)
    dex = torch.zeros(nq, dtype=torch.int32, device="cuda")
    off = torch.full((nq + 1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    tot = torch.full((1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    oi = torch.full((n + PAD,), SENT_IDX, dtype=torch.int32, device="cuda")
    on = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
    ou = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dq.copy_(src_q ^ 0xFF).bitwise_xor_(0xFF)
        dc.copy_(src_c ^ 0xFF).bitwise_xor_(0xFF)
        dex.copy_(torch.from_numpy(ex.astype(np.int32)).cuda())
        rc = lib.bbh_jt_radius(dq.data_ptr(), nq, nb, dc.data_ptr(), nc, nb, radius, dex.data_ptr(), n + 3, off.data_ptr(),
                               tot.data_ptr(), oi.data_ptr(), on.data_ptr(), ou.data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    goff, gtot = off.cpu().numpy(), tot.cpu().numpy()
    assert (goff[:nq + 1] == want[0]).all() and untouched(goff[nq + 1:]) and gtot[0] == n and untouched(gtot[1:])
    gi, gn, gu = oi.cpu().numpy(), on.cpu().numpy().view(np.uint32), ou.cpu().numpy().view(np.uint32)
    assert (gi[n:] == SENT_IDX).all() and (gn[n:] == 0xFFFFFFFF).all() and (gu[n:] == 0xFFFFFFFF).all()
    assert (gi[:n] == want[1]).all() and (gn[:n] == want[2]).all() and (gu[:n] == want[3]).all()


# (nq, nc, nbytes, q_stride, radius, capacity)
REFUSED = {
    "nq < 0": (-1, 4, 16, 16, 0.5, 8),
    "nc = 0": (4, 0, 16, 16, 0.5, 8),
    "nc = 2^31": (4, 1 << 31, 16, 16, 0.5, 8),
    "nbytes = 0": (4, 4, 0, 16, 0.5, 8),
    "nbytes < 0": (4, 4, -16, 16, 0.5, 8),
    "q_stride < nbytes": (4, 4, 16, 15, 0.5, 8),
    "NaN radius": (4, 4, 16, 16, float("nan"), 8),
    "capacity < 0": (4, 4, 16, 16, 0.5, -1),
}


def refusal_buffers():
    return (np.full(5 + PAD, SENT64, np.int64), np.full(1 + PAD, SENT64, np.int64), np.full(16 + PAD, SENT_IDX, np.int32),
            np.full(16 + PAD, SENT32, np.uint32), np.full(16 + PAD, SENT32, np.uint32))


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID before anything is launched, every output untouched."""
    nq, nc, nb, stride, radius, capacity = REFUSED[name]
    q, c = np.ones((4, 16), np.uint8), np.ones((100, 16), np.uint8)
    off, tot, oi, on, ou = refusal_buffers()
    rc = lib.bbh_jt_radius(at(q), nq, stride, at(c), nc, nb, radius, None, capacity, at(off), at(tot), at(oi), at(on),
                           at(ou), None)
    assert rc == INVALID and untouched(off, tot, oi, on, ou) and lib.bbh_last_error(), name


@pytest.mark.parametrize("missing", ["offsets", "total", "idx with a capacity"])
def test_refusal_of_a_missing_output(lib, missing):
    q = np.ones((4, 16), np.uint8)
    off, tot, oi, on, ou = refusal_buffers()
    args = {"offsets": (None, at(tot), at(oi)), "total": (at(off), None, at(oi)), "idx with a capacity": (at(off), at(tot), None)}
    o, t, i = args[missing]
    assert lib.bbh_jt_radius(at(q), 4, 16, at(q), 4, 16, 0.5, None, 16, o, t, i, at(on), at(ou), None) == INVALID
    assert untouched(off, tot, oi, on, ou)

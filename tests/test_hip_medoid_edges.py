r"""Edge cases of the segmented complementary iSIM (bblean_amd/csrc/bb_medoid.hip) through the raw C ABI,
`bbh_compl_isim_segments`: every plane instance of k_seg_rows and the wide kernel on sets of 65 535 to 2^24 rows (given as
`members` over 48 distinct rows, against the weighted reference of medoid_cases.py), column counts of exactly 256 in a chunk
and of exactly m in a set, the turns and ties of k_seg_argmin, the word-count boundaries of the two-words-per-lane kernels,
many large sets in one call, every combination of outputs and of host / device residency, a side stream, misaligned rows,
and the argument checks.  Everything is compared with ==: positions, and the float64 values with their NaN positions
compared separately.  Output buffers are longer than the call may write and pre-filled with sentinels.

Left untested: sets of 2^31 rows and more (refused by an argument check, which is here; the largest set that runs is 2^24
rows, the smallest that selects the 32-plane instance), sets between 2^24 and 2^31 rows, whose counts use planes 25 .. 30
of that same instance, and k_seg_rows<2, 32>: 2^24 rows of more than 256 bytes, where the one set of that size here has 8-byte
rows to stay within a few seconds."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest

import medoid_cases as mc

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "medoids.npz"
PAD = 5
SENT_F64 = -12345.5
SENT_I64 = -7
INVALID = 1  # BBH_ERR_INVALID


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def at(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run(lib, rows, n_rows, nb, stride, members, offsets, k, nf, total, compl=True, medoid=True, stream=None):
    r"""bbh_compl_isim_segments with host outputs of total + PAD and k + PAD sentinels -> (rc, compl | None, medoid | None)."""
    oc = np.full(total + PAD, SENT_F64) if compl else None
    om = np.full(max(k, 0) + PAD, SENT_I64, np.int64) if medoid else None
    rc = lib.bbh_compl_isim_segments(at(rows), n_rows, nb, stride, at(members), at(offsets), k, nf, at(oc), at(om), stream)
    return rc, oc, om


def untouched(*arrays):
    return all((a == (SENT_F64 if a.dtype == np.float64 else SENT_I64)).all() for a in arrays if a is not None)


def same(lib, got, med, compl, what=""):
    rc, oc, om = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    if om is not None:
        assert untouched(om[len(med):]), (what, "medoid tail")
        assert np.array_equal(om[:len(med)], med), (what, np.flatnonzero(om[:len(med)] != med)[:10], om[:5], med[:5])
    if oc is not None:
        assert untouched(oc[len(compl):]), (what, "values tail")
        g = oc[:len(compl)]
        nan = np.isnan(compl)
        assert np.array_equal(np.isnan(g), nan), (what, "NaN positions")
        bad = np.flatnonzero((g != compl) & ~nan)
        assert bad.size == 0, (what, bad[:10], g[bad[:5]], compl[bad[:5]])


def one_set(lib, distinct, mem, want_values, want_medoid, what):
    m, nb = len(mem), distinct.shape[1]
    off = np.array([0, m], dtype=np.int64)
    got = run(lib, distinct, len(distinct), nb, nb, mem, off, 1, nb * 8, m)
    same(lib, got, np.array([want_medoid], dtype=np.int64), want_values[mem], what)


# ---------------------------------------------------------------------------------------------------------------------
# plane instances
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m,nb,with_zero", mc.PLANE_CASES)
def test_every_plane_instance(lib, m, nb, with_zero):
    r"""k_seg_rows<1 | 2, 16 | 20 | 24 | 32> and k_seg_rows_wide with up to 21 planes.  Without the zero row the shared
    column's count is exactly m: every plane set at 65 535 and 2^20 - 1, only the top plane at the powers of two (at 2^24
    that is plane 24, the first of the third group of partial sums).  Rows 0 .. 255 and one later chunk hold only rows with
    the shared column: a chunk count of exactly 256, the ninth chunk plane."""
    distinct = mc.plane_distinct(nb)
    mem = mc.plane_members(m, nb, with_zero)
    counts = np.bincount(mem, minlength=len(distinct))
    # the shape selects the instance it is here for
    kernel, wpl, planes = mc.instance_of(m, nb)
    assert m > mc.SMALL_MAX and int(m).bit_length() in (16, 17, 20, 21, 25)
    words = (nb + 3) // 4
    assert words == {8: 2, 260: 65, 512: 128, 516: 129}[nb]
    if nb == 516:
        assert kernel == "wide" and planes == int(m).bit_length() > 12
    else:
        assert (kernel, wpl, planes) == ("rows", 1 if nb == 8 else 2, mc.PLANE_EXPECT[m])
    ls = mc.column_sums(distinct, counts)
    shared = (distinct[:, 0] & mc.SHARED_BIT) != 0
    assert shared[mem[:mc.CHUNK]].all() and shared[mem[mc.FULL_CHUNK * mc.CHUNK:(mc.FULL_CHUNK + 1) * mc.CHUNK]].all()
    assert (counts[0] > 0) == with_zero and counts[1:].min() > 0
    if not with_zero:
        assert int(ls[0]) == m == int(ls.max())
    if m == 1 << 24:
        assert int(ls.max()) >> 24 == 1
    values = mc.compl_isim_weighted(distinct, counts)
    one_set(lib, distinct, mem, values, mc.weighted_medoid(values, mem), (m, nb, with_zero))


# ---------------------------------------------------------------------------------------------------------------------
# argmin
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("first", mc.ARGMIN_FIRST)
def test_argmin_turns_and_ties(lib, first):
    r"""512 partials, two turns of k_seg_argmin's scan.  The minimal row's copies tie across chunks, threads, waves and
    turns; the first copy's position is the medoid."""
    distinct, mem, r0 = mc.argmin_case(first)
    m = len(mem)
    assert m == mc.ARGMIN_M and (m + mc.CHUNK - 1) // mc.CHUNK == 512
    values = mc.compl_isim_weighted(distinct, np.bincount(mem, minlength=len(distinct)))
    assert np.flatnonzero(values == values.min()).tolist() == [r0]
    copies = np.flatnonzero(mem == r0)
    assert copies[0] == first and mc.weighted_medoid(values, mem) == first
    if first == m - 1:
        assert len(copies) == 1
    else:
        assert len({int(p) // mc.CHUNK for p in copies}) == len(copies) >= 3
    one_set(lib, distinct, mem, values, first, first)


def test_argmin_every_row_ties(lib):
    distinct = mc.plane_distinct(8)
    mem = np.full(mc.ARGMIN_M, 5, dtype=np.int64)
    values = mc.compl_isim_weighted(distinct, np.bincount(mem, minlength=len(distinct)))
    one_set(lib, distinct, mem, values, 0, "one row")


# ---------------------------------------------------------------------------------------------------------------------
# word boundaries, many sets
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("m", mc.WORD_MS)
@pytest.mark.parametrize("nb,nf", mc.WORD_CASES)
def test_word_boundaries(lib, nb, nf, m):
    r"""65 words: lane 0 owns two words and every other lane one; 2072 and 2056 features end inside the 65th word; 128 words
    fill both words of every lane; 129 words are the first width of the wide kernel.  Contiguous rows, no members."""
    kernel, wpl, _ = mc.instance_of(m, nf // 8)
    words = (nf // 8 + 3) // 4
    assert words == {260: 65, 512: 128, 516: 129}[nb]
    assert kernel == ("wide" if words > 128 else "small" if m <= 2047 else "rows") and (kernel == "wide" or wpl == 2)
    rows = mc.word_rows(nb, m)
    if nf < nb * 8:
        assert rows[:, nf // 8:].any()  # bits past n_features are set
    off = np.array([0, m], dtype=np.int64)
    med, compl = mc.compl_isim_segments(rows, off, None, nf)
    same(lib, run(lib, rows, m, nb, nb, None, off, 1, nf, m), med, compl, (nb, nf, m))


@functools.lru_cache(maxsize=None)
def many():
    rows, off, mem = mc.many_sets()
    return rows, off, mem, mc.compl_isim_segments(rows, off, mem)


def test_many_large_sets_in_one_call(lib):
    r"""The counters, planes and partials of the large path are reused set after set on the stream."""
    rows, off, mem, (med, compl) = many()
    sizes = np.diff(off)
    assert (sizes > mc.SMALL_MAX).sum() == 7 and sizes[0] > mc.SMALL_MAX and sizes[-1] > mc.SMALL_MAX
    assert (sizes < 3).sum() >= 3 and sizes.max() == 6000
    same(lib, run(lib, rows, len(rows), 64, 64, mem, off, len(sizes), 512, len(mem)), med, compl, "many")


# ---------------------------------------------------------------------------------------------------------------------
# outputs, residency, streams, alignment
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("compl,medoid", [(True, False), (False, True), (False, False)])
def test_optional_outputs(lib, compl, medoid):
    rows, off, mem, (med, val) = many()
    got = run(lib, rows, len(rows), 64, 64, mem, off, len(off) - 1, 512, len(mem), compl, medoid)
    assert (got[1] is None) == (not compl) and (got[2] is None) == (not medoid)
    same(lib, got, med, val, (compl, medoid))


@pytest.mark.parametrize("dev_rows", [False, True])
@pytest.mark.parametrize("dev_off", [False, True])
@pytest.mark.parametrize("dev_mem", [False, True])
def test_mixed_residency(lib, torch, dev_rows, dev_off, dev_mem):
    r"""Every host / device combination of rows, offsets and members on the hand-made sets, against the reference's values."""
    from bblean_amd import make_fake_fingerprints

    gold = np.load(GOLD)
    rows = mc.hand_rows(make_fake_fingerprints)
    off, mem = mc.hand_index()
    put = lambda a, on_dev: torch.from_numpy(a).cuda() if on_dev else a  # noqa: E731
    a_rows, a_off, a_mem = put(rows, dev_rows), put(off, dev_off), put(mem, dev_mem)
    got = run(lib, a_rows, len(rows), 256, 256, a_mem, a_off, len(off) - 1, 2048, len(mem))
    same(lib, got, gold["hand_medoid"], gold["hand_compl"], (dev_rows, dev_off, dev_mem))
    torch.cuda.synchronize()


def test_device_outputs_on_side_stream(lib, torch):
    r"""Inputs produced on a non-blocking side stream, the call enqueued on it, both outputs in device memory."""
    rows, off, mem, (med, val) = many()
    k, total = len(off) - 1, len(mem)
    src = torch.from_numpy(rows).cuda()
    d_rows = torch.zeros_like(src)
    d_mem = torch.zeros(total, dtype=torch.int64, device="cuda")
    src_mem = torch.from_numpy(mem).cuda()
    oc = torch.full((total + PAD,), SENT_F64, dtype=torch.float64, device="cuda")
    om = torch.full((k + PAD,), SENT_I64, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        d_rows.copy_(src ^ 0xFF).bitwise_xor_(0xFF)
        d_mem.copy_(src_mem + 1).sub_(1)
        rc = lib.bbh_compl_isim_segments(d_rows.data_ptr(), len(rows), 64, 64, d_mem.data_ptr(), at(off), k, 512,
                                         oc.data_ptr(), om.data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    same(lib, (0, oc.cpu().numpy(), om.cpu().numpy()), med, val, "side stream")


@pytest.mark.parametrize("shift", [1, 4])
def test_misaligned_device_rows(lib, torch, shift):
    r"""A device base 1 and 4 bytes off with row_stride = nbytes (64): byte loads for the odd base, word loads at + 4."""
    rows, off, mem, (med, val) = many()
    flat = torch.zeros(rows.size + 16, dtype=torch.uint8, device="cuda")
    flat[shift:shift + rows.size].copy_(torch.from_numpy(rows).cuda().reshape(-1))
    assert flat.data_ptr() % 16 == 0
    got = run(lib, flat.data_ptr() + shift, len(rows), 64, 64, mem, off, len(off) - 1, 512, len(mem))
    same(lib, got, med, val, shift)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

GOOD = dict(rows=True, n_rows=50, nb=16, stride=16, members=None, offsets=[0, 10, 30, 50], k=3, nf=128)
REFUSALS = {
    "NULL rows": (dict(rows=False), "need rows"),
    "NULL offsets": (dict(offsets=None), "need rows"),
    "k = 0": (dict(k=0), "need rows"),
    "n_rows = 0": (dict(n_rows=0), "need rows"),
    "row_stride < nbytes": (dict(stride=15), "need rows"),
    "n_features = 0": (dict(nf=0), "divisible by 8"),
    "n_features = 12": (dict(nf=12), "divisible by 8"),
    "n_features wider than the row": (dict(nf=16 * 8 + 8), "divisible by 8"),
    "offsets[0] = 1": (dict(offsets=[1, 10, 30, 50]), "start at 0"),
    "decreasing offsets": (dict(offsets=[0, 30, 10, 50]), "decrease"),
    "empty set in the middle": (dict(offsets=[0, 10, 10, 50]), "is empty"),
    "offsets[k] > n_rows": (dict(offsets=[0, 10, 30, 51]), "offsets name"),
    "members holding -1": (dict(members=-1), "not a row"),
    "members holding n_rows": (dict(members=50), "not a row"),
    # n_features * m * m >= 2^63, from the offsets alone: checked before the rows the offsets name are counted or touched
    "2^31 rows": (dict(offsets=[0, 1 << 31], k=1), "2^63"),
    "2^26 rows of 2^11 features": (dict(offsets=[0, 1 << 26], k=1, nb=256, stride=256, nf=2048), "2^63"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID with the message of the check that is meant, before any launch, outputs untouched."""
    change, message = REFUSALS[name]
    a = dict(GOOD, **change)
    rows = np.ones((50, 256), np.uint8)
    off = None if a["offsets"] is None else np.array(a["offsets"], dtype=np.int64)
    mem = None
    if a["members"] is not None:
        mem = np.arange(50, dtype=np.int64)
        mem[17] = a["members"]
    oc, om = np.full(50 + PAD, SENT_F64), np.full(3 + PAD, SENT_I64, np.int64)
    rc = lib.bbh_compl_isim_segments(at(rows) if a["rows"] else None, a["n_rows"], a["nb"], a["stride"], at(mem), at(off),
                                     a["k"], a["nf"], at(oc), at(om), None)
    assert rc == INVALID, (name, rc)
    assert message in lib.bbh_last_error().decode(), (name, lib.bbh_last_error())
    assert untouched(oc, om), name


def test_refusal_table_starts_from_a_valid_call(lib):
    rows = np.ones((50, 256), np.uint8)
    off = np.array(GOOD["offsets"], dtype=np.int64)
    got = run(lib, rows, 50, 16, 16, None, off, 3, 128, 50)
    assert got[0] == 0 and (got[2][:3] == 0).all() and not untouched(got[1][:50])
    got = run(lib, rows, 50, 16, 16, np.arange(50, dtype=np.int64), off, 3, 128, 50)
    assert got[0] == 0 and (got[2][:3] == 0).all()

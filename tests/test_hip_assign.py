r"""GPU: `jt_assign_packed` / `jt_dist_matrix_packed` (bblean_amd/csrc/bb_assign.hip) against NumPy's exact integers.
Everything is compared with `==`: indices, counts, and the bit patterns of the float64 distances."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

from kernel_refs import exact
from sklearn_cases import CASES, rows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "sklearn.npz"
TQ = 128  # query / centroid tile edge of k_assign_mfma; the popcount kernels tile queries by 256
MODES = (None, "bcnt", "mfma")


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
    return MODES if nbytes == 256 else (None, "bcnt")


def check(q, c, what=""):
    from bblean_amd.similarity import jt_assign_packed, jt_dist_matrix_packed

    idx, inter, union, d = exact(q, c)
    for mode in modes_for(q.shape[1]):
        with forced(mode):
            gi, gn, gu = jt_assign_packed(q, c, return_counts=True)
            only = jt_assign_packed(q, c)
        assert gi.dtype == np.int32 and gn.dtype == np.uint32 and gu.dtype == np.uint32
        bad = np.flatnonzero(gi != idx)
        assert bad.size == 0, (what, mode, bad[:5], gi[bad[:5]], idx[bad[:5]])
        assert (gn == inter).all() and (gu == union).all(), (what, mode)
        assert (only == idx).all(), (what, mode)
    gd = jt_dist_matrix_packed(q, c)
    assert gd.dtype == np.float64 and gd.shape == d.shape
    assert (gd.view(np.uint64) == d.view(np.uint64)).all(), what


def rand_rows(rng, n, nbytes, density=None):
    if density is None:
        return rng.integers(0, 256, (n, nbytes), dtype=np.uint8)
    return np.packbits(rng.random((n, nbytes * 8)) < density, axis=1)


def test_mfma_i8_operand_maps():
    r"""One v_mfma_i32_16x16x64_i8 tile with full-range int8 data: the A / B / D lane maps bb_assign.hip documents."""
    from bblean_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    for _ in range(3):
        a = rng.integers(-128, 128, (16, 64), dtype=np.int8)
        b = rng.integers(-128, 128, (64, 16), dtype=np.int8)
        d = np.zeros((16, 16), dtype=np.int32)
        _lib.check(lib.bbh_mfma_i8_probe(a.ctypes.data, b.ctypes.data, d.ctypes.data, None))
        assert (d == a.astype(np.int32) @ b.astype(np.int32)).all()
    # rows and columns are not interchangeable: a one-hot pair lands on exactly one element
    a = np.zeros((16, 64), np.int8)
    b = np.zeros((64, 16), np.int8)
    a[3, 37] = 5
    b[37, 11] = -7
    d = np.zeros((16, 16), dtype=np.int32)
    _lib.check(lib.bbh_mfma_i8_probe(a.ctypes.data, b.ctypes.data, d.ctypes.data, None))
    want = np.zeros((16, 16), np.int32)
    want[3, 11] = -35
    assert (d == want).all()


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_centroids(name):
    from bblean_amd import make_fake_fingerprints
    from bblean_amd.similarity import jt_assign_packed, jt_dist_matrix_packed

    gold = np.load(GOLD)
    _, qry = rows(CASES[name], make_fake_fingerprints)
    if not CASES[name]["packed"]:
        qry = np.packbits(qry, axis=1)
    cents = gold[f"{name}_centroids"]
    check(qry, cents, name)
    for mode in modes_for(qry.shape[1]):
        with forced(mode):
            assert (jt_assign_packed(qry, cents).astype(np.int64) + 1 == gold[f"{name}_labels"]).all(), mode
    keep = gold[f"{name}_dist_rows"]
    got = jt_dist_matrix_packed(qry[keep], cents)
    assert (got.view(np.uint64) == gold[f"{name}_dist"].view(np.uint64)).all()


@pytest.mark.parametrize("nbytes", [1, 8, 16, 100, 253, 256, 257])
def test_widths_and_tile_edges(nbytes):
    rng = np.random.default_rng(1000 + nbytes)
    shapes = [(1, 1), (1, 300), (TQ - 1, TQ + 1), (TQ, TQ), (TQ + 1, TQ - 1), (131, 257), (257, 61), (255, 2 * TQ),
              (2 * TQ + 1, 3 * TQ + 7)]
    for nq, nc in shapes:
        dens = 0.05 if nbytes >= 100 else None  # sparse wide rows; small rows at density 1/2 give many exact ties
        q = rand_rows(rng, nq, nbytes, dens)
        c = rand_rows(rng, nc, nbytes, dens)
        if nq > 2:
            q[nq // 2] = 0
        if nc > 3:
            c[nc // 3] = 0
        check(q, c, (nbytes, nq, nc))


@pytest.mark.parametrize("nbytes", [16, 256])
def test_duplicate_centroids_first_index_wins(nbytes):
    r"""Every centroid row occurs many times, in every centroid range of the split grid (nq is small, so the grid
    splits the centroids): the lowest index of the equal distances must win."""
    rng = np.random.default_rng(77)
    base = rand_rows(rng, 7, nbytes, 0.2)
    for nq, nc in [(5, 3000), (130, 5000), (3, 40000)]:
        c = base[np.arange(nc) % 7]
        c[:7] = base[::-1]  # the first occurrence of base[k] is row 6 - k
        q = np.concatenate([base[:3], rand_rows(rng, nq - 3, nbytes, 0.2)])
        idx, _, _, _ = exact(q, c)
        assert (idx[:3] == [6, 5, 4]).all()
        check(q, c, (nbytes, nq, nc))


@pytest.mark.parametrize("nbytes", [8, 256])
def test_all_zero_queries(nbytes):
    rng = np.random.default_rng(9)
    q = rand_rows(rng, 200, nbytes, 0.1)
    q[[0, 17, 199]] = 0
    c = rand_rows(rng, 700, nbytes, 0.1)
    c[c.sum(1) == 0, 0] = 1  # no all-zero centroid: every distance of a zero query is 1 -> index 0
    idx, _, union, _ = exact(q, c)
    assert (idx[[0, 17, 199]] == 0).all() and (union[[0, 17, 199]] > 0).all()
    check(q, c, "no zero centroid")
    c[[333, 650]] = 0  # now the empty union (distance 0) wins, at its first index
    idx, inter, union, _ = exact(q, c)
    assert (idx[[0, 17, 199]] == 333).all() and (union[[0, 17, 199]] == 0).all() and (inter[[0, 17, 199]] == 0).all()
    check(q, c, "zero centroid")


def test_device_tensors_and_strided_queries():
    import torch

    from bblean_amd.similarity import jt_assign_packed, jt_dist_matrix_packed

    rng = np.random.default_rng(21)
    for nbytes in (16, 256):
        wide = rand_rows(rng, 600, 2 * nbytes, 0.1)
        c = rand_rows(rng, 300, nbytes, 0.1)
        tw = torch.from_numpy(wide).cuda()
        tc = torch.from_numpy(c).cuda()
        views = [(tw[:, :nbytes], wide[:, :nbytes]), (tw[::2, nbytes:], wide[::2, nbytes:])]
        for tq, hq in views:
            assert not tq.is_contiguous()
            idx, inter, union, d = exact(np.ascontiguousarray(hq), c)
            for mode in modes_for(nbytes):
                with forced(mode):
                    gi, gn, gu = jt_assign_packed(tq, tc, return_counts=True)
                assert gi.is_cuda and gi.dtype == torch.int32
                assert (gi.cpu().numpy() == idx).all(), (nbytes, mode)
                assert (gn.cpu().numpy().view(np.uint32) == inter).all() and (gu.cpu().numpy().view(np.uint32) == union).all()
            gd = jt_dist_matrix_packed(tq, tc)
            assert gd.is_cuda and gd.dtype == torch.float64
            assert (gd.cpu().numpy().view(np.uint64) == d.view(np.uint64)).all()
            assert (jt_assign_packed(tq, c).cpu().numpy() == idx).all()  # host centroids beside device queries


def test_host_queries_go_through_in_slabs(monkeypatch):
    from bblean_amd.similarity import jt_assign_packed, jt_dist_matrix_packed

    rng = np.random.default_rng(3)
    q = rand_rows(rng, 1000, 256, 0.1)
    c = rand_rows(rng, 150, 256, 0.1)
    idx, inter, union, d = exact(q, c)
    monkeypatch.setenv("BBHIP_SLAB_KB", "64")  # 256 rows per call
    gi, gn, gu = jt_assign_packed(q, c, return_counts=True)
    assert (gi == idx).all() and (gn == inter).all() and (gu == union).all()
    assert (jt_dist_matrix_packed(q, c).view(np.uint64) == d.view(np.uint64)).all()


def test_errors():
    from bblean_amd.similarity import jt_assign_packed

    with pytest.raises(RuntimeError):
        jt_assign_packed(np.zeros((4, 16), np.uint8), np.zeros((4, 8), np.uint8))
    with pytest.raises(RuntimeError):
        jt_assign_packed(np.zeros((4, 16), np.uint8), np.zeros((0, 16), np.uint8))
    with forced("mfma"), pytest.raises(RuntimeError):
        jt_assign_packed(np.zeros((4, 16), np.uint8), np.ones((4, 16), np.uint8))
    assert jt_assign_packed(np.zeros((0, 16), np.uint8), np.ones((4, 16), np.uint8)).shape == (0,)


def test_more_centroids_than_best_match_takes():
    r"""nc = 2^20 + 4097 (bbh_jt_best_match refuses nc > 2^20) against jt_best_match_packed on the two halves,
    combined by exact cross-multiplication on the host.  No all-zero rows: the two orderings agree."""
    from bblean_amd.similarity import jt_assign_packed, jt_best_match_packed

    rng = np.random.default_rng(2020)
    nc, nq = (1 << 20) + 4097, 256
    c = rng.integers(0, 256, (nc, 256), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 256), dtype=np.uint8)
    c[12345] = q[7]  # one exact match, and its duplicate in the other half: the first must win
    c[nc - 5] = q[7]
    with pytest.raises(RuntimeError):
        jt_best_match_packed(q, c)
    half = nc // 2
    i0, n0, u0, _ = jt_best_match_packed(q, c[:half])
    i1, n1, u1, _ = jt_best_match_packed(q, c[half:])
    second = n1.astype(np.int64) * u0.astype(np.int64) > n0.astype(np.int64) * u1.astype(np.int64)  # strict: ties stay in the first half
    want_i = np.where(second, i1.astype(np.int64) + half, i0).astype(np.int32)
    want_n = np.where(second, n1, n0)
    want_u = np.where(second, u1, u0)
    assert want_i[7] == 12345
    import torch

    tc = torch.from_numpy(c).cuda()
    tq = torch.from_numpy(q).cuda()
    for mode in MODES:
        with forced(mode):
            gi, gn, gu = jt_assign_packed(tq, tc, return_counts=True)
        assert (gi.cpu().numpy() == want_i).all(), mode
        assert (gn.cpu().numpy().view(np.uint32) == want_n).all() and (gu.cpu().numpy().view(np.uint32) == want_u).all(), mode

r"""GPU: `jt_compl_isim_segments` (bblean_amd/csrc/bb_medoid.hip) and everything that sits on it, against the reference's
values (tests/golden/medoids.npz) and against a NumPy restatement of the exact arithmetic.  Everything is compared with
`==`: positions, and the float64 values with their NaN positions compared separately.  No tolerance anywhere."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import warnings
from pathlib import Path

import numpy as np
import pytest

import medoid_cases as mc

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "medoids.npz"
SMALL_MAX = 2047  # bb_medoid.hip: the largest set the one-wave kernel takes


def same(got_med, got_compl, med, compl, what=""):
    got_med, got_compl = np.asarray(got_med), np.asarray(got_compl)
    assert got_med.dtype == np.int64 and got_compl.dtype == np.float64, what
    assert np.array_equal(got_med, med), (what, np.flatnonzero(got_med != med)[:10])
    assert np.array_equal(np.isnan(got_compl), np.isnan(compl)), what
    ok = ~np.isnan(compl)
    bad = np.flatnonzero(got_compl[ok] != compl[ok])
    assert bad.size == 0, (what, bad[:10], got_compl[ok][bad[:5]], compl[ok][bad[:5]])


@contextlib.contextmanager
def slab_kb(kb):
    old = os.environ.pop("BBHIP_SLAB_KB", None)
    os.environ["BBHIP_SLAB_KB"] = str(kb)
    try:
        yield
    finally:
        os.environ.pop("BBHIP_SLAB_KB", None)
        if old is not None:
            os.environ["BBHIP_SLAB_KB"] = old


def launches(name):
    from bblean_amd import _lib

    n = C.c_int64(0)
    ms = C.c_double(0.0)
    _lib.check(_lib.load().bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return int(n.value)


@contextlib.contextmanager
def profiling():
    from bblean_amd import _lib

    lib = _lib.load()
    lib.bbh_profile_reset()
    lib.bbh_profile_enable(1)
    try:
        yield
    finally:
        lib.bbh_profile_enable(0)
        lib.bbh_profile_reset()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def tree_rows():
    from bblean_amd import make_fake_fingerprints

    return mc.tree_rows(make_fake_fingerprints)


def test_golden_tree_sets(gold, tree_rows):
    import torch

    from bblean_amd.similarity import jt_compl_isim_segments

    off, mem, compl, med = gold["tree_offsets"], gold["tree_members"], gold["tree_compl"], gold["tree_medoid"]
    assert (np.diff(off) >= 3).sum() >= 500
    # the tree's own member lists
    same(*jt_compl_isim_segments(tree_rows, off, mem), med, compl, "members")
    # contiguous sets
    flat = tree_rows[mem]
    same(*jt_compl_isim_segments(flat, off), med, compl, "contiguous")
    # the same sets through a shuffled members
    perm = np.random.default_rng(3).permutation(len(flat))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    same(*jt_compl_isim_segments(flat[perm], off, inv), med, compl, "shuffled members")
    # positions only
    m2, c2 = jt_compl_isim_segments(flat, off, return_compl=False)
    assert c2 is None and np.array_equal(m2, med)
    # device tensors in -> device tensors out
    dm, dc = jt_compl_isim_segments(torch.from_numpy(tree_rows).cuda(), torch.from_numpy(off).cuda(),
                                    torch.from_numpy(mem).cuda())
    assert dm.is_cuda and dc.is_cuda and dm.dtype == torch.int64 and dc.dtype == torch.float64
    same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, "device")
    dm, dc = jt_compl_isim_segments(torch.from_numpy(flat).cuda(), off)
    same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, "device rows, host offsets")
    # a row stride larger than nbytes: 4-byte aligned rows and rows at odd addresses
    for width in (272, 259):
        wide = np.full((len(flat), width), 0xFF, dtype=np.uint8)
        wide[:, :256] = flat
        view = wide[:, :256]
        assert view.strides == (width, 1)
        same(*jt_compl_isim_segments(view, off), med, compl, f"stride {width}")
        dv = torch.from_numpy(wide).cuda()[:, :256]
        dm, dc = jt_compl_isim_segments(dv, off)
        same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, f"device stride {width}")
    # several slabs of whole sets: 2048 rows of 256 bytes each
    with slab_kb(512):
        same(*jt_compl_isim_segments(tree_rows, off, mem), med, compl, "slabs, members")
        same(*jt_compl_isim_segments(flat, off), med, compl, "slabs, contiguous")


def test_golden_hand_sets(gold):
    import torch

    from bblean_amd import make_fake_fingerprints
    from bblean_amd.similarity import jt_compl_isim_segments

    rows = mc.hand_rows(make_fake_fingerprints)
    off, mem = mc.hand_index()
    assert np.array_equal(off, gold["hand_offsets"]) and np.array_equal(mem, gold["hand_members"])
    compl, med = gold["hand_compl"], gold["hand_medoid"]
    tied = sum(int((compl[a:b] == compl[a:b].min()).sum() > 1) for a, b in zip(off[:-1], off[1:]) if b - a >= 3)
    assert tied >= 5
    same(*jt_compl_isim_segments(rows, off, mem), med, compl, "members")
    same(*jt_compl_isim_segments(rows[mem], off), med, compl, "contiguous")
    dm, dc = jt_compl_isim_segments(torch.from_numpy(rows).cuda(), off, torch.from_numpy(mem).cuda())
    same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, "device")
    # every set alone: the result does not depend on what else is in the call
    for g in range(len(off) - 1):
        sel = rows[mem[off[g]:off[g + 1]]]
        m1, c1 = jt_compl_isim_segments(sel, np.array([0, len(sel)]))
        same(m1, c1, med[g:g + 1], compl[off[g]:off[g + 1]], f"set {g}")


def test_golden_big_set(gold):
    import torch

    from bblean_amd import make_fake_fingerprints
    from bblean_amd.similarity import jt_compl_isim_segments

    distinct, draw = mc.big_rows(make_fake_fingerprints)
    compl = gold["big_compl_distinct"][draw]
    med = gold["big_medoid"]
    assert not np.isnan(compl).any() and len(draw) == 70000
    off = np.array([0, len(draw)], dtype=np.int64)
    same(*jt_compl_isim_segments(distinct, off, draw), med, compl, "members")
    same(*jt_compl_isim_segments(distinct[draw], off), med, compl, "contiguous")
    dm, dc = jt_compl_isim_segments(torch.from_numpy(distinct).cuda(), off, torch.from_numpy(draw).cuda())
    same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, "device")
    with slab_kb(512):  # a single set larger than a slab is uploaded as it is
        same(*jt_compl_isim_segments(distinct, off, draw), med, compl, "one set beyond the slab")


def random_case(c):
    r"""(rows, offsets, members | None, n_features | None) of randomised case c: heavy-tailed set sizes on both sides of
    the small / large bound."""
    rng = np.random.default_rng(1000 + c)
    nbits = (64, 1024, 2048, 4096)[c % 4]
    k = (1, 6, 150, 2500)[(c // 4) % 4]
    sizes = np.minimum((rng.pareto(0.8, k) * 1.5).astype(np.int64) + 1, 5000)
    while sizes.sum() > 9000:  # keep the NumPy side cheap: halve the sets until the case has at most 9000 random rows
        sizes = np.maximum(sizes // 2, 1)
    if c % 3 == 0:  # both sides of the bound, and the bound itself
        edge = np.array([SMALL_MAX, SMALL_MAX + 1, SMALL_MAX - 1, 3, 2, 1, 64, 65, 257], dtype=np.int64)
        sizes[: min(k, len(edge))] = edge[: min(k, len(edge))]
    elif c % 3 == 1:
        sizes[-1] = int(rng.integers(SMALL_MAX + 1, 2 * SMALL_MAX))
    if k == 1:
        sizes[0] = (2500, SMALL_MAX + 1, 40, SMALL_MAX, 700, 9000)[c % 6]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offsets[-1])
    nb = nbits // 8
    density = (0.05, 0.3, 0.5, 0.9)[c % 4]
    n_distinct = max(4, total // (1 + c % 3))  # repeated rows (ties) in two of three cases
    distinct = np.packbits(rng.random((n_distinct, nbits)) < density, axis=1)
    distinct[0] = 0
    if c % 2:
        members = rng.integers(0, n_distinct, total).astype(np.int64)
        rows = distinct
    else:
        members = None
        rows = distinct[rng.integers(0, n_distinct, total)]
    return rows, offsets, members, (nbits - 8 if c % 5 == 4 else None)


def test_randomised_shapes():
    import torch

    from bblean_amd.similarity import jt_compl_isim_segments

    with profiling():
        for c in range(32):
            rows, off, mem, nf = random_case(c)
            med, compl = mc.compl_isim_segments(rows, off, mem, nf)
            same(*jt_compl_isim_segments(rows, off, mem, n_features=nf), med, compl, f"case {c}")
            if c % 4 == 1:
                dm, dc = jt_compl_isim_segments(torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda(),
                                                None if mem is None else torch.from_numpy(mem).cuda(), n_features=nf)
                same(dm.cpu().numpy(), dc.cpu().numpy(), med, compl, f"case {c}, device")
        # rows wider than the kernels keep in registers, and rows that are not a whole number of words
        rng = np.random.default_rng(77)
        for nbytes, sizes in ((1024, [5, 1, 300, 2, 40]), (9, [3, 700, 2100, 2]), (516, [10, 2050])):
            rows = rng.integers(0, 256, (sum(sizes), nbytes), dtype=np.uint8)
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            med, compl = mc.compl_isim_segments(rows, off)
            same(*jt_compl_isim_segments(rows, off), med, compl, f"{nbytes} bytes")
        assert launches("compl_isim_seg/small") > 0
        assert launches("compl_isim_seg/large") > 0
        assert launches("compl_isim_seg") == launches("compl_isim_seg/small") + launches("compl_isim_seg/large")


@pytest.fixture(scope="module")
def fitted():
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = np.array(make_fake_fingerprints(3000, seed=5), dtype=np.uint8)
    tree = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter").fit(fps)
    return tree, fps


def test_similarity_functions_equal_the_unpacked_path():
    from bblean_amd import make_fake_fingerprints
    from bblean_amd.similarity import estimate_jt_std, jt_compl_isim, jt_isim_medoid, jt_stratified_sampling

    fps = np.array(make_fake_fingerprints(400, seed=21), dtype=np.uint8)
    fps[7] = fps[3]
    bits = np.unpackbits(fps, axis=1)
    old = jt_compl_isim(bits, input_is_packed=False)
    new = jt_compl_isim(fps)
    assert new.dtype == np.float64 and np.array_equal(new, old)
    for n_features in (None, 2048, 1024):
        for pack in (True, False):
            b = bits if n_features is None else bits[:, :n_features]
            i_old, m_old = jt_isim_medoid(b, input_is_packed=False, pack=pack)
            i_new, m_new = jt_isim_medoid(fps, n_features=n_features, pack=pack)
            assert i_new == i_old and m_new.dtype == m_old.dtype and np.array_equal(m_new, m_old), (n_features, pack)
    assert np.array_equal(jt_stratified_sampling(fps, 20), jt_stratified_sampling(bits, 20, input_is_packed=False))
    assert estimate_jt_std(fps, 30) == estimate_jt_std(bits, 30, input_is_packed=False)
    for n in (1, 2):  # the warning and the NaN array stay
        with pytest.warns(RuntimeWarning, match="len\\(fps\\) must be >= 3"):
            out = jt_compl_isim(fps[:n])
        assert out.shape == (n,) and np.isnan(out).all()
        assert jt_isim_medoid(fps[:n])[0] == 0


def test_tree_medoids_equal_the_unpacked_path(fitted):
    import torch

    tree, fps = fitted
    bits = np.unpackbits(fps, axis=1)
    for sort in (True, False):
        for pack in (True, False):
            old = tree.get_medoids_mol_ids(bits, sort=sort, pack=pack, input_is_packed=False)
            new = tree.get_medoids_mol_ids(fps, sort=sort, pack=pack)
            assert new["mol_ids"] == old["mol_ids"]
            assert new["medoids"].dtype == old["medoids"].dtype and np.array_equal(new["medoids"], old["medoids"])
            assert np.array_equal(tree.get_medoids(fps, sort=sort, pack=pack), old["medoids"])
            dev = tree.get_medoids_mol_ids(torch.from_numpy(fps).cuda(), sort=sort, pack=pack)
            assert dev["medoids"].is_cuda and dev["medoids"].dtype == torch.uint8
            assert dev["mol_ids"] == old["mol_ids"] and np.array_equal(dev["medoids"].cpu().numpy(), old["medoids"])


def test_dbi_with_medoids_equals_the_unpacked_path(fitted):
    from bblean_amd.metrics import jt_dbi

    tree, fps = fitted
    bits = np.unpackbits(fps, axis=1)
    ids = tree.get_cluster_mol_ids()[:40]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        old = jt_dbi([bits[m] for m in ids], centrals="medoid", input_is_packed=False)
        new = jt_dbi([fps[m] for m in ids], centrals="medoid")
    assert new == old


def test_fast_path_is_taken(fitted):
    from bblean_amd.similarity import jt_compl_isim

    tree, fps = fitted
    with profiling():
        tree.get_medoids(fps)
        assert launches("compl_isim_seg") >= 1
        assert launches("isim_from_sum") == 0
    with profiling():
        jt_compl_isim(fps[:1000])
        assert launches("compl_isim_seg") >= 1
        assert launches("isim_from_sum") == 0


def test_device_index_errors():
    r"""Argument checks of device-resident index arrays: refused before any row is read."""
    import torch

    from bblean_amd.similarity import jt_compl_isim_segments

    rows = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (50, 256), dtype=np.uint8)).cuda()
    off = torch.tensor([0, 10, 30, 50], dtype=torch.int64).cuda()
    mem = torch.arange(50, dtype=torch.int64).cuda()
    jt_compl_isim_segments(rows, off, mem)
    bad = mem.clone()
    bad[17] = 50
    with pytest.raises((RuntimeError, ValueError), match="not a row"):
        jt_compl_isim_segments(rows, off, bad)
    bad[17] = -1
    with pytest.raises((RuntimeError, ValueError), match="not a row"):
        jt_compl_isim_segments(rows, off, bad)
    with pytest.raises((RuntimeError, ValueError), match="decrease"):
        jt_compl_isim_segments(rows, torch.tensor([0, 30, 10, 50], dtype=torch.int64).cuda(), mem)
    with pytest.raises((RuntimeError, ValueError)):
        jt_compl_isim_segments(rows, torch.tensor([0, 30, 60], dtype=torch.int64).cuda())

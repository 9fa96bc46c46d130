r"""GPU: radius search through the Python face - `similarity.jt_radius_packed` on host and device input against the
distance matrix, host slabs, the second library call, sorted segments against top-k, and `radius_neighbors` /
`radius_neighbors_graph` / `centroid_radius_neighbors` of the estimator on the cases of tests/golden/sklearn.npz, whose stored
`transform` rows were made by the reference, and against scikit-learn's own brute-force radius search."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np
import pytest

import kernel_refs as R
import radius_refs as X
import topk_refs as T
from sklearn_cases import CASES, rows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "sklearn.npz"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def fitted(name):
    import bblean_amd.sklearn as bs
    from bblean_amd import make_fake_fingerprints

    case = CASES[name]
    fit_x, qry = rows(case, make_fake_fingerprints)
    cls = bs.BitBirch if case["packed"] else bs.UnpackedBitBirch
    return cls(threshold=case["thr"], branching_factor=case["bf"]).fit(fit_x), qry


def segments(off, arr):
    return [arr[off[a]:off[a + 1]] for a in range(len(off) - 1)]


class CountingLibrary:
    r"""The loaded library with its `bbh_jt_radius` calls recorded as (nq, capacity)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "bbh_jt_radius":
            return fn

        def counted(*args):
            self.calls.append((args[1], args[8]))
            return fn(*args)

        return counted


@pytest.fixture()
def counting(monkeypatch):
    from bblean_amd import _lib

    spy = CountingLibrary(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: spy)
    return spy


@pytest.mark.parametrize("nb,nq,nc", [(256, 300, 500), (16, 300, 70), (100, 70, 70)])
def test_host_and_device_agree_with_the_distance_matrix(nb, nq, nc):
    import torch

    from bblean_amd.similarity import jt_dist_matrix_packed, jt_radius_packed

    q, c = X.assign_case(nb, nq, nc)
    full = jt_dist_matrix_packed(q, c)
    radius = float(np.sort(full, axis=None)[full.size // 50])  # a realised distance: 2 % of the pairs
    want = X.exact_radius(q, c, radius)
    off, idx, dist, inter, union = jt_radius_packed(q, c, radius, return_counts=True)
    assert off.dtype == np.int64 and idx.dtype == np.int32 and dist.dtype == np.float64
    assert inter.dtype == np.uint32 and union.dtype == np.uint32
    assert off.shape == (nq + 1,) and idx.shape == dist.shape == inter.shape == union.shape == (int(off[-1]),)
    assert (off == want[0]).all() and (idx == want[1]).all() and (inter == want[2]).all() and (union == want[3]).all()
    for a in range(nq):
        hits = np.flatnonzero(full[a] <= radius)
        assert (idx[off[a]:off[a + 1]] == hits).all()
        assert (R.bits(dist[off[a]:off[a + 1]]) == R.bits(full[a, hits])).all()
    assert len(jt_radius_packed(q, c, radius)) == 3

    tq, tc = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    out = jt_radius_packed(tq, tc, radius, return_counts=True)
    assert all(t.is_cuda for t in out) and out[0].dtype == torch.int64 and out[1].dtype == torch.int32
    assert out[2].dtype == torch.float64 and out[3].dtype == out[4].dtype == torch.uint32
    assert (out[0].cpu().numpy() == off).all() and (out[1].cpu().numpy() == idx).all()
    assert (R.bits(out[2].cpu().numpy()) == R.bits(dist)).all()
    assert (out[3].cpu().numpy() == inter).all() and (out[4].cpu().numpy() == union).all()
    mixed = jt_radius_packed(tq, c, radius)  # host table with device queries
    assert mixed[1].is_cuda and (mixed[1].cpu().numpy() == idx).all()
    two = jt_radius_packed(q, tc, radius)    # device table with host queries
    assert isinstance(two[1], np.ndarray) and (two[1] == idx).all() and (R.bits(two[2]) == R.bits(dist)).all()


def test_exclude_on_host_and_device():
    import torch

    from bblean_amd.similarity import jt_radius_packed

    c = T.self_inputs()
    ex = np.arange(len(c))
    radius = float(np.sort(R.exact(c, c)[3], axis=None)[len(c) * 6])
    want = X.exact_radius(c, c, radius, ex)
    assert want[0][-1] > 8
    off, idx, dist = jt_radius_packed(c, c, radius, exclude=ex)
    assert (off == want[0]).all() and (idx == want[1]).all() and (R.bits(dist) == R.bits(want[4])).all()
    tc = torch.from_numpy(c).cuda()
    for dev_ex in (ex, torch.from_numpy(ex).cuda(), torch.from_numpy(ex.astype(np.int32)).cuda()):
        got = jt_radius_packed(tc, tc, radius, exclude=dev_ex)
        assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == want[1]).all()
        assert (R.bits(got[2].cpu().numpy()) == R.bits(want[4])).all()
    assert (jt_radius_packed(c, c, radius, exclude=torch.from_numpy(ex).cuda())[1] == want[1]).all()


def test_host_slabs(monkeypatch, counting):
    r"""Three slabs of host queries (the last one ragged), the table staged once, the exclusion cut with the queries and
    the offsets rebased; one library call per slab."""
    from bblean_amd import similarity as S

    nb, nq, nc = 16, 300, 70
    monkeypatch.setenv("BBHIP_SLAB_KB", "2")  # 2 KiB / 16 bytes = 128 rows
    assert S._slab_rows(nb) == 128 and -(-nq // 128) == 3
    q, c = X.assign_case(nb, nq, nc)
    ex = (np.arange(nq) * 3) % nc
    d = R.exact(q, c)[3]
    radius = float(np.sort(d, axis=None)[d.size // 10])
    want = X.exact_radius(q, c, radius, ex)
    parts = [int(want[0][min(nq, lo + 128)] - want[0][lo]) for lo in range(0, nq, 128)]
    assert min(parts) > 0 and max(parts) <= S._radius_first_capacity(44, nc)  # the first capacity holds every slab's part
    off, idx, dist, inter, union = S.jt_radius_packed(q, c, radius, exclude=ex, return_counts=True)
    assert [n for n, _ in counting.calls] == [128, 128, 44]
    assert (off == want[0]).all() and (idx == want[1]).all() and (inter == want[2]).all() and (union == want[3]).all()
    assert (R.bits(dist) == R.bits(want[4])).all()


def test_second_call_when_the_first_capacity_is_too_small(counting):
    r"""radius = 1: every pair, more than the first capacity; the second call has room for exactly the total.  A radius
    whose answer fits takes one call.  The same on device input."""
    import torch

    from bblean_amd import similarity as S

    nb, nq, nc = 16, 300, 70
    q, c = X.assign_case(nb, nq, nc)
    first = S._radius_first_capacity(nq, nc)
    assert first < nq * nc
    want = X.exact_radius(q, c, 1.0)
    for qq in (q, torch.from_numpy(q).cuda()):
        counting.calls.clear()
        off, idx, dist = S.jt_radius_packed(qq, c, 1.0)
        assert counting.calls == [(nq, first), (nq, nq * nc)]
        off, idx, dist = (np.asarray(t.cpu()) if hasattr(t, "cpu") else t for t in (off, idx, dist))
        assert (off == want[0]).all() and (idx == want[1]).all() and (R.bits(dist) == R.bits(want[4])).all()
        counting.calls.clear()
        S.jt_radius_packed(qq, c, 0.0)
        assert counting.calls == [(nq, first)]


@pytest.mark.parametrize("nb,nq,nc,k", [(256, 300, 500, 10), (16, 300, 70, 7)])
def test_sorted_segments_start_with_top_k(nb, nq, nc, k):
    r"""sort=True orders a segment by (distance, row number): its first k entries are jt_topk_packed's, ties included (16
    bytes at density 1/2: ties are common).  On host and device input."""
    import torch

    from bblean_amd.similarity import jt_radius_packed, jt_topk_packed

    q, c = X.assign_case(nb, nq, nc)
    tidx, tdist = jt_topk_packed(q, c, k)
    radius = float(np.median(tdist[:, -1]))  # about half of the queries have at least k hits
    plain = jt_radius_packed(q, c, radius)
    for qq in (q, torch.from_numpy(q).cuda()):
        off, idx, dist, inter, union = (np.asarray(t.cpu()) if hasattr(t, "cpu") else t
                                        for t in jt_radius_packed(qq, c, radius, return_counts=True, sort=True))
        assert (off == plain[0]).all()
        long = 0
        for a in range(nq):
            si, sd = idx[off[a]:off[a + 1]], dist[off[a]:off[a + 1]]
            order = np.lexsort((plain[1][off[a]:off[a + 1]], plain[2][off[a]:off[a + 1]]))
            assert (si == plain[1][off[a]:off[a + 1]][order]).all() and (R.bits(sd) == R.bits(plain[2][off[a]:off[a + 1]][order])).all()
            u64, i64 = union[off[a]:off[a + 1]].astype(np.int64), inter[off[a]:off[a + 1]].astype(np.int64)
            assert (R.bits(sd) == R.bits(np.where(u64 == 0, 0.0, (u64 - i64) / np.maximum(u64, 1)))).all()
            if len(si) >= k:
                long += 1
                assert (si[:k] == tidx[a]).all() and (R.bits(sd[:k]) == R.bits(tdist[a])).all()
        assert long >= nq // 4


@pytest.mark.parametrize("name", list(CASES))
def test_radius_neighbors_against_the_reference_rows(gold, name):
    r"""For the `transform` rows the reference produced: radius_neighbors is flatnonzero(row <= r) and the row's values
    there, at the merge threshold (the default radius) and at two realised distances."""
    import torch

    est, qry = fitted(name)
    keep = gold[f"{name}_dist_rows"]
    gd = gold[f"{name}_dist"]
    flat = np.sort(gd, axis=None)
    radii = (None, float(flat[flat.size // 100]), float(flat[flat.size // 10]))
    for radius in radii:
        r = 1.0 - CASES[name]["thr"] if radius is None else radius
        dist, ind = est.radius_neighbors(qry, radius)
        assert dist.dtype == ind.dtype == object and dist.shape == ind.shape == (qry.shape[0],)
        only = est.radius_neighbors(qry, radius, return_distance=False)
        for j, a in enumerate(keep):
            hits = np.flatnonzero(gd[j] <= r)
            assert ind[a].dtype == np.int64 and dist[a].dtype == np.float64
            assert (ind[a] == hits).all() and (R.bits(dist[a]) == R.bits(gd[j, hits])).all() and (only[a] == hits).all()
    assert sum(len(a) for a in ind[keep]) > len(keep)
    packed = qry if CASES[name]["packed"] else np.packbits(qry, axis=1)
    off, ti, td = est.radius_neighbors(torch.from_numpy(packed).cuda(), radii[2], input_is_packed=True)
    assert off.is_cuda and off.dtype == ti.dtype == torch.int64 and td.dtype == torch.float64
    assert (ti.cpu().numpy() == np.concatenate(list(ind))).all() and (R.bits(td.cpu().numpy()) == R.bits(np.concatenate(list(dist)))).all()
    assert (off.cpu().numpy() == np.concatenate([[0], np.cumsum([len(a) for a in ind])])).all()
    assert len(est.radius_neighbors(torch.from_numpy(packed).cuda(), radii[2], return_distance=False, input_is_packed=True)) == 2


@pytest.mark.parametrize("name", ["B", "D"])
def test_scikit_learn_parity(name):
    r"""`sklearn.neighbors.NearestNeighbors(radius, metric="jaccard", algorithm="brute")` on the unpacked booleans: the same
    index sets and distances; the order inside a query is scikit-learn's to choose, so sets are compared, and the sorted
    order only on queries without tied distances."""
    from sklearn.neighbors import NearestNeighbors

    est, qry = fitted(name)
    nbits = CASES[name]["nbits"]
    cents = np.unpackbits(est._packed_centers.cpu().numpy(), axis=1)[:, :nbits].astype(bool)
    qbits = (np.unpackbits(qry, axis=1)[:, :nbits] if CASES[name]["packed"] else qry).astype(bool)[:200]
    q200 = qry[:200]
    full = est.transform(q200)
    radius = float(np.sort(full, axis=None)[full.size // 50])
    nn = NearestNeighbors(radius=radius, metric="jaccard", algorithm="brute").fit(cents)
    sd, si = nn.radius_neighbors(qbits)
    dist, ind = est.radius_neighbors(q200, radius)
    total = 0
    for a in range(len(q200)):
        order = np.argsort(si[a], kind="stable")
        assert (si[a][order] == ind[a]).all() and (R.bits(sd[a][order]) == R.bits(dist[a])).all()
        total += len(ind[a])
    assert total > len(q200)
    sd, si = nn.radius_neighbors(qbits, sort_results=True)
    dist, ind = est.radius_neighbors(q200, radius, sort_results=True)
    untied = 0
    for a in range(len(q200)):
        assert (np.diff(dist[a]) >= 0).all() and sorted(ind[a]) == sorted(si[a])
        if len(np.unique(dist[a])) == len(dist[a]):
            untied += len(dist[a]) >= 2
            assert (si[a] == ind[a]).all() and (R.bits(sd[a]) == R.bits(dist[a])).all()
    assert untied >= 1 or nbits == 64  # (64-bit rows: few distinct distances, most queries with two hits have a tie)


@pytest.mark.parametrize("name", ["A", "B"])
def test_centroids_among_themselves(name):
    r"""X=None and centroid_radius_neighbors: every centroid without itself."""
    est, _ = fitted(name)
    cents = est._packed_centers.cpu().numpy()
    K = len(cents)
    radius = 1.0 - CASES[name]["thr"]
    want = X.exact_radius(cents, cents, radius, np.arange(K))
    assert want[0][-1] > 0
    dist, ind = est.radius_neighbors()
    assert ind.shape == (K,) and all(a not in ind[a] for a in range(K))
    assert (np.concatenate(list(ind)) == want[1]).all() and (R.bits(np.concatenate(list(dist))) == R.bits(want[4])).all()
    off, ci, cd = est.centroid_radius_neighbors(radius)
    assert off.dtype == ci.dtype == np.int64 and cd.dtype == np.float64
    assert (off == want[0]).all() and (ci == want[1]).all() and (R.bits(cd) == R.bits(want[4])).all()
    unsorted = np.array(est.get_centroids(sort=False))
    wu = X.exact_radius(unsorted, unsorted, radius, np.arange(K))
    uo, ui, ud = est.centroid_radius_neighbors(radius, sort=False)
    assert (uo == wu[0]).all() and (ui == wu[1]).all() and (R.bits(ud) == R.bits(wu[4])).all()


def test_equal_rows_are_neighbours_but_no_row_is_its_own():
    r"""A table with two pairs of equal rows against itself at radius 0."""
    from bblean_amd.similarity import jt_radius_packed

    c = T.self_inputs()
    off, idx, dist = jt_radius_packed(c, c, 0.0, exclude=np.arange(len(c)))
    assert idx.tolist() == [30, 50, 7, 8] and (dist == 0.0).all()
    assert [int(off[a + 1] - off[a]) for a in (7, 8, 30, 50)] == [1, 1, 1, 1] and off[-1] == 4
    off, idx, dist = jt_radius_packed(c, c, 0.0)
    assert off[-1] == len(c) + 4 and all(a in idx[off[a]:off[a + 1]] for a in range(len(c)))


def test_plain_tree(tmp_path):
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(1500, seed=5)
    tree = BitBirch(branching_factor=50, threshold=0.5, merge_criterion="diameter").fit(fps)
    cents = np.array(tree.get_centroids())
    K = len(cents)
    radius = float(np.sort(R.exact(cents, cents)[3], axis=None)[K + 4 * K])  # about two neighbours each
    want = X.exact_radius(cents, cents, radius, np.arange(K))
    off, ind, dist = tree.centroid_radius_neighbors(radius)
    assert off[-1] > 0 and (off == want[0]).all() and (ind == want[1]).all() and (R.bits(dist) == R.bits(want[4])).all()


@pytest.mark.parametrize("name", ["B", "D"])
def test_radius_neighbors_graph(name):
    r"""Both modes against the CSR triple, with queries and with X=None."""
    from bblean_amd.similarity import jt_radius_packed

    est, qry = fitted(name)
    cents = est._packed_centers
    K = int(cents.shape[0])
    packed = qry if CASES[name]["packed"] else np.packbits(qry, axis=1)
    radius = 1.0 - CASES[name]["thr"]
    for X_in, q, ex in ((qry, packed, None), (None, cents, np.arange(K, dtype=np.int32))):
        off, idx, dist = (np.asarray(t.cpu()) if hasattr(t, "cpu") else t for t in jt_radius_packed(q, cents, radius, exclude=ex))
        assert off[-1] > 0
        g = est.radius_neighbors_graph(X_in) if X_in is None else est.radius_neighbors_graph(X_in, radius)
        assert g.format == "csr" and g.shape == (len(off) - 1, K) and g.dtype == np.float64
        assert (g.indptr == off).all() and (g.indices == idx).all() and (g.data == 1.0).all()
        gd = est.radius_neighbors_graph(X_in, radius, mode="distance")
        assert (gd.indptr == off).all() and (gd.indices == idx).all() and (R.bits(gd.data) == R.bits(dist)).all()

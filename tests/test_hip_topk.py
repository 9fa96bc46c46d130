r"""GPU: top-k through the Python face - `similarity.jt_topk_packed` on host and device input against the distance matrix,
host slabs, and `kneighbors` / `centroid_neighbors` of the estimator on the four cases of tests/golden/sklearn.npz, whose
stored `transform` rows were made by the reference."""
from __future__ import annotations

import functools
import pickle
from pathlib import Path

import numpy as np
import pytest

import kernel_refs as R
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


@pytest.mark.parametrize("nb,nq,nc,k", [(256, 300, 500, 10), (16, 300, 70, 64), (100, 70, 70, 9)])
def test_host_and_device_agree_with_the_distance_matrix(nb, nq, nc, k):
    import torch

    from bblean_amd.similarity import jt_dist_matrix_packed, jt_topk_packed

    q, c = T.assign_case(nb, nq, nc)
    want = T.exact_topk(q, c, k)
    idx, dist, inter, union = jt_topk_packed(q, c, k, return_counts=True)
    assert idx.dtype == np.int32 and dist.dtype == np.float64 and inter.dtype == np.uint32 and union.dtype == np.uint32
    assert idx.shape == dist.shape == inter.shape == union.shape == (nq, k)
    assert (idx == want[0]).all() and (inter == want[1]).all() and (union == want[2]).all()
    full = jt_dist_matrix_packed(q, c)
    assert (R.bits(dist) == R.bits(np.take_along_axis(full, idx.astype(np.int64), 1))).all()
    assert (idx == np.argsort(full, axis=1, kind="stable")[:, :k]).all()

    tq, tc = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    out = jt_topk_packed(tq, tc, k, return_counts=True)
    assert all(t.is_cuda for t in out) and out[0].dtype == torch.int32 and out[1].dtype == torch.float64
    assert (out[0].cpu().numpy() == idx).all() and (R.bits(out[1].cpu().numpy()) == R.bits(dist)).all()
    assert out[2].dtype == out[3].dtype == torch.uint32
    assert (out[2].cpu().numpy() == inter).all() and (out[3].cpu().numpy() == union).all()
    mixed = jt_topk_packed(tq, c, k)  # host table with device queries
    assert mixed[0].is_cuda and (mixed[0].cpu().numpy() == idx).all()
    two = jt_topk_packed(q, tc, k)    # device table with host queries
    assert isinstance(two[0], np.ndarray) and (two[0] == idx).all() and (R.bits(two[1]) == R.bits(dist)).all()


def test_exclude_on_host_and_device():
    import torch

    from bblean_amd.similarity import jt_topk_packed

    c = T.self_inputs()
    ex = np.arange(len(c))
    want = T.exact_topk(c, c, 5, ex)
    idx, dist = jt_topk_packed(c, c, 5, exclude=ex)
    assert (idx == want[0]).all() and (R.bits(dist) == R.bits(want[3])).all()
    tc = torch.from_numpy(c).cuda()
    for dev_ex in (ex, torch.from_numpy(ex).cuda(), torch.from_numpy(ex.astype(np.int32)).cuda()):
        got = jt_topk_packed(tc, tc, 5, exclude=dev_ex)
        assert (got[0].cpu().numpy() == want[0]).all() and (R.bits(got[1].cpu().numpy()) == R.bits(want[3])).all()
    assert (jt_topk_packed(c, c, 5, exclude=torch.from_numpy(ex).cuda())[0] == want[0]).all()


def test_host_slabs(monkeypatch):
    r"""Three slabs of host queries (the last one ragged), the table staged once, the exclusion cut with the queries."""
    from bblean_amd import similarity as S

    nb, nq, nc, k = 16, 300, 70, 12
    monkeypatch.setenv("BBHIP_SLAB_KB", "2")  # 2 KiB / 16 bytes = 128 rows
    assert S._slab_rows(nb) == 128 and -(-nq // 128) == 3
    q, c = T.assign_case(nb, nq, nc)
    ex = (np.arange(nq) * 3) % nc
    want = T.exact_topk(q, c, k, ex)
    idx, dist, inter, union = S.jt_topk_packed(q, c, k, exclude=ex, return_counts=True)
    assert (idx == want[0]).all() and (inter == want[1]).all() and (union == want[2]).all()
    assert (R.bits(dist) == R.bits(want[3])).all()


@pytest.mark.parametrize("name", list(CASES))
def test_kneighbors_against_the_reference_rows(gold, name):
    r"""For the `transform` rows the reference produced: kneighbors is the stable argsort of the row, and its values."""
    import torch

    est, qry = fitted(name)
    keep = gold[f"{name}_dist_rows"]
    gd = gold[f"{name}_dist"]
    order = np.argsort(gd, axis=1, kind="stable")
    labels = est.predict(qry)
    for k in (1, 5, 64):
        dist, ind = est.kneighbors(qry, k)
        assert isinstance(ind, np.ndarray) and ind.dtype == np.int64 and dist.dtype == np.float64
        assert ind.shape == dist.shape == (qry.shape[0], k)
        assert (ind[keep] == order[:, :k]).all()
        assert (R.bits(dist[keep]) == R.bits(np.take_along_axis(gd, order[:, :k], 1))).all()
        assert (est.kneighbors(qry, k, return_distance=False) == ind).all()
        if k == 1:
            assert (ind[:, 0] + 1 == labels).all() and (est.subcluster_labels_[ind[:, 0]] == labels).all()
    packed = qry if CASES[name]["packed"] else np.packbits(qry, axis=1)
    td, ti = est.kneighbors(torch.from_numpy(packed).cuda(), 5, input_is_packed=True)
    d5, i5 = est.kneighbors(qry, 5)
    assert ti.is_cuda and ti.dtype == torch.int64 and (ti.cpu().numpy() == i5).all()
    assert (R.bits(td.cpu().numpy()) == R.bits(d5)).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_centroid_neighbours(name):
    est, _ = fitted(name)
    cents = est._packed_centers.cpu().numpy()
    K = len(cents)
    want = T.exact_topk(cents, cents, 5, np.arange(K))
    dist, ind = est.kneighbors(None, 5)
    assert ind.dtype == np.int64 and (ind == want[0]).all() and (R.bits(dist) == R.bits(want[3])).all()
    assert (ind != np.arange(K)[:, None]).all()
    ci, cd = est.centroid_neighbors(5)
    assert (ci == ind).all() and (R.bits(cd) == R.bits(dist)).all()
    assert (np.array(est.get_centroids(sort=True)) == cents).all()
    # chain order: the same graph under the permutation of get_centroids(sort=False)
    ui, ud = est.centroid_neighbors(5, sort=False)
    unsorted = np.array(est.get_centroids(sort=False))
    wu = T.exact_topk(unsorted, unsorted, 5, np.arange(K))
    assert (ui == wu[0]).all() and (R.bits(ud) == R.bits(wu[3])).all()
    twin = pickle.loads(pickle.dumps(est))
    d2, i2 = twin.kneighbors(None, 5)
    assert (i2 == ind).all() and (R.bits(d2) == R.bits(dist)).all()


def test_plain_tree_and_save_load(tmp_path):
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(1500, seed=5)
    tree = BitBirch(branching_factor=50, threshold=0.5, merge_criterion="diameter").fit(fps)
    cents = np.array(tree.get_centroids())
    K = len(cents)
    assert K > 6
    ind, dist = tree.centroid_neighbors(6)
    want = T.exact_topk(cents, cents, 6, np.arange(K))
    assert ind.shape == (K, 6) and (ind == want[0]).all() and (R.bits(dist) == R.bits(want[3])).all()
    tree.save(tmp_path / "t.bb")
    back = BitBirch.load(tmp_path / "t.bb")
    i2, d2 = back.centroid_neighbors(6)
    assert (i2 == ind).all() and (R.bits(d2) == R.bits(dist)).all()

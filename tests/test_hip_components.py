r"""GPU: connected components through the Python face - `similarity.jt_components_packed` on host and device rows against
components_refs.exact_components, and `BitBirch.centroid_components` / `link_clusters` on a fitted tree against scipy's
components of the CSR that `centroid_radius_neighbors` returns."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import components_refs as C
import kernel_refs as R

pytestmark = pytest.mark.gpu

THRESHOLD = 0.5
CASES = {name: (rows, r) for name, rows, r in C.all_cases()}
FACE_CASES = ["chain permuted 0.4", "star hub 511 " + repr(C.STAR_R), "block 0.13", "block 0.14", "bridge C at 256",
              "width 256 " + repr(C.width_radii(256)[1]), "width 100 " + repr(C.width_radii(100)[1]),
              "degenerate zero rows, r = 0"]


@pytest.mark.parametrize("name", FACE_CASES)
def test_host_and_device_rows(name):
    import torch

    from bblean_amd.similarity import jt_components_packed

    rows, radius = CASES[name]
    n = len(rows)
    roots, labels, count = C.expected(name)
    got = jt_components_packed(rows, radius)
    assert len(got) == 2 and got[1] == count and isinstance(got[1], int)
    assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64 and got[0].shape == (n,) and (got[0] == labels).all()
    lab, cnt, rts = jt_components_packed(rows, radius, return_roots=True)
    assert cnt == count and (lab == labels).all() and rts.dtype == np.int64 and (rts == roots).all()

    t = torch.from_numpy(rows).cuda()
    lab_t, cnt_t, rts_t = jt_components_packed(t, radius, return_roots=True)
    assert lab_t.is_cuda and rts_t.is_cuda and lab_t.dtype == rts_t.dtype == torch.int32 and cnt_t == count
    assert lab_t.shape == rts_t.shape == (n,)
    assert (lab_t.cpu().numpy() == labels).all() and (rts_t.cpu().numpy() == roots).all()
    two = jt_components_packed(t, radius)
    assert len(two) == 2 and (two[0].cpu().numpy() == labels).all()
    wide = torch.zeros((n, rows.shape[1] + 4), dtype=torch.uint8, device="cuda")
    wide[:, :rows.shape[1]] = t
    assert (jt_components_packed(wide[:, :rows.shape[1]], radius)[0].cpu().numpy() == labels).all()  # a strided view


def test_no_rows_and_one_row():
    from bblean_amd.similarity import jt_components_packed

    lab, cnt, rts = jt_components_packed(np.zeros((0, 32), np.uint8), 0.3, return_roots=True)
    assert cnt == 0 and lab.shape == rts.shape == (0,) and lab.dtype == np.int64
    lab, cnt = jt_components_packed(np.ones((1, 32), np.uint8), 0.3)
    assert cnt == 1 and lab.tolist() == [0]


@functools.lru_cache(maxsize=None)
def tree():
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(3000, seed=5)
    return BitBirch(branching_factor=50, threshold=THRESHOLD, merge_criterion="diameter").fit(fps), fps


@functools.lru_cache(maxsize=None)
def tree_radius() -> float:
    r"""A realised distance between centroids with about one neighbour each: components of every size."""
    cents = np.array(tree()[0].get_centroids())
    K = len(cents)
    return float(np.sort(R.exact(cents, cents)[3], axis=None)[K + 2 * K])


def csr_components(model, radius, sort):
    off, ind, _ = model.centroid_radius_neighbors(radius, sort=sort)
    K = len(off) - 1
    return connected_components(csr_matrix((np.ones(len(ind), np.int8), ind, off), shape=(K, K)), directed=False)


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("default_radius", [False, True])
def test_centroid_components_are_the_components_of_the_radius_graph(sort, default_radius):
    model, _ = tree()
    radius = 1.0 - THRESHOLD if default_radius else tree_radius()
    count, want = csr_components(model, radius, sort)
    before = (model._global_clustering_centroid_labels, model._n_global_clusters)
    labels, n = model.centroid_components(None if default_radius else radius, sort=sort)
    K = len(model.get_centroids())
    assert labels.dtype == np.int64 and labels.shape == (K,) and n == count and (labels == want).all()
    if not default_radius:
        assert 1 < n < K
    assert (model._global_clustering_centroid_labels, model._n_global_clusters) == before


def test_link_clusters_then_save_and_load(tmp_path):
    import warnings

    from bblean_amd import BitBirch

    model, fps = tree()
    radius = tree_radius()
    count, want = csr_components(model, radius, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert model.link_clusters(radius) is model
    assert model._n_global_clusters == count and (model._global_clustering_centroid_labels == want + 1).all()
    assign = model.get_assignments(global_clusters=True)
    plain = model.get_assignments()
    assert (assign == (want + 1).astype(np.uint64)[plain.astype(np.int64) - 1]).all()  # cluster p of sort=True carries label p + 1
    merged = model.get_cluster_mol_ids(global_clusters=True)
    clusters = model.get_cluster_mol_ids()
    assert len(merged) == count
    assert all(sorted(merged[lab]) == sorted(i for p in np.flatnonzero(want == lab) for i in clusters[p]) for lab in range(count))
    model.save(tmp_path / "linked.bb")
    back = BitBirch.load(tmp_path / "linked.bb")
    assert back._n_global_clusters == count and (back._global_clustering_centroid_labels == want + 1).all()
    assert (back.get_assignments(global_clusters=True) == assign).all()
    assert back.get_cluster_mol_ids(global_clusters=True) == merged
    model._global_clustering_centroid_labels, model._n_global_clusters = None, 0

r"""GPU: leader clustering through the Python face - `similarity.jt_leaders_packed` on host and device rows against
leaders_refs.exact_leaders, and `BitBirch.centroid_leaders` / `lead_clusters` on a fitted tree against a sequential sphere
exclusion over the CSR that `centroid_radius_neighbors` returns."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import components_refs as C
import kernel_refs as R
import leaders_refs as L

pytestmark = pytest.mark.gpu

THRESHOLD = 0.5
FACE_CASES = ["chain permuted 0.4", "star hub 511 " + repr(C.STAR_R), "block 0.13", "block 0.14", "bridge C at 256",
              "width 256 " + repr(C.width_radii(256)[1]), "width 100 " + repr(C.width_radii(100)[1]),
              "degenerate zero rows, r = 0", L.LATE, L.WEIGHTS_FLIP, L.ZERO_WEIGHTS]


@pytest.mark.parametrize("name", FACE_CASES)
def test_host_and_device_rows(name):
    import torch

    from bblean_amd.similarity import jt_leaders_packed

    rows, radius, w = L.case(name)
    rows, w = rows.copy(), w.copy()
    n = len(rows)
    centre, labels, count, dens = L.expected(name, False, False)
    got = jt_leaders_packed(rows, radius)
    assert len(got) == 2 and got[1] == count and isinstance(got[1], int)
    assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64 and got[0].shape == (n,) and (got[0] == labels).all()
    lab, cnt, cen, den = jt_leaders_packed(rows, radius, return_centres=True, return_density=True)
    assert cnt == count and (lab == labels).all() and cen.dtype == np.int64 and (cen == centre).all()
    assert den.dtype == np.uint64 and (den == dens).all()
    lab, cnt, den = jt_leaders_packed(rows, radius, return_density=True)
    assert (lab == labels).all() and (den == dens).all()

    for ties in ("low", "high"):
        centre, labels, count, dens = L.expected(name, True, ties == "high")
        for weights in (w, w.astype(np.int64), w.tolist()):
            lab, cnt, cen, den = jt_leaders_packed(rows, radius, weights=weights, ties=ties, return_centres=True, return_density=True)
            assert cnt == count and (lab == labels).all() and (cen == centre).all() and (den == dens).all()
        t = torch.from_numpy(rows).cuda()
        on_device = [w, torch.from_numpy(w.astype(np.int64)).cuda()]
        if int(w.max()) < 2 ** 31:  # (an int32 tensor cannot hold more; weights flip / zero weights come this way)
            on_device.append(torch.from_numpy(w.astype(np.int32)).cuda())
        for weights in on_device:
            lab_t, cnt_t, cen_t, den_t = jt_leaders_packed(t, radius, weights=weights, ties=ties, return_centres=True, return_density=True)
            assert lab_t.is_cuda and cen_t.is_cuda and den_t.is_cuda and cnt_t == count
            assert lab_t.dtype == cen_t.dtype == torch.int32 and den_t.dtype == torch.int64
            assert lab_t.shape == cen_t.shape == den_t.shape == (n,)
            assert (lab_t.cpu().numpy() == labels).all() and (cen_t.cpu().numpy() == centre).all()
            assert (den_t.cpu().numpy().view(np.uint64) == dens).all()
    two = jt_leaders_packed(t, radius, weights=w, ties="high")
    assert len(two) == 2 and (two[0].cpu().numpy() == labels).all()
    wide = torch.zeros((n, rows.shape[1] + 4), dtype=torch.uint8, device="cuda")
    wide[:, :rows.shape[1]] = t
    assert (jt_leaders_packed(wide[:, :rows.shape[1]], radius, weights=w, ties="high")[0].cpu().numpy() == labels).all()  # a strided view


def test_device_weights_out_of_range():
    import torch

    from bblean_amd.similarity import jt_leaders_packed

    t = torch.zeros((4, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(t, 0.3, weights=torch.tensor([1, 2, 2 ** 32, 1], device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(t, 0.3, weights=torch.tensor([1, -2, 3, 1], device="cuda"))
    with pytest.raises(TypeError, match="weights"):
        jt_leaders_packed(t, 0.3, weights=torch.ones(4, device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(t, 0.3, weights=torch.ones(5, dtype=torch.int64, device="cuda"))


def test_no_rows_and_one_row():
    from bblean_amd.similarity import jt_leaders_packed

    lab, cnt, cen, den = jt_leaders_packed(np.zeros((0, 32), np.uint8), 0.3, return_centres=True, return_density=True)
    assert cnt == 0 and lab.shape == cen.shape == den.shape == (0,) and lab.dtype == np.int64 and den.dtype == np.uint64
    lab, cnt, den = jt_leaders_packed(np.ones((1, 32), np.uint8), 0.3, weights=[5], return_density=True)
    assert cnt == 1 and lab.tolist() == [0] and den.tolist() == [5]


@functools.lru_cache(maxsize=None)
def tree():
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(3000, seed=5)
    return BitBirch(branching_factor=50, threshold=THRESHOLD, merge_criterion="diameter").fit(fps), fps


@functools.lru_cache(maxsize=None)
def tree_radius() -> float:
    r"""A realised distance between centroids with about one neighbour each: clusters of every size."""
    cents = np.array(tree()[0].get_centroids())
    K = len(cents)
    return float(np.sort(R.exact(cents, cents)[3], axis=None)[K + 2 * K])


def csr_leaders(model, radius, sort, weighted):
    r"""Sequential sphere exclusion over the CSR of `centroid_radius_neighbors`."""
    off, ind, _ = model.centroid_radius_neighbors(radius, sort=sort)
    K = len(off) - 1
    w = np.array([len(m) for m in model.get_cluster_mol_ids(sort=sort)], np.int64) if weighted else np.ones(K, np.int64)
    dens = np.array([w[p] + w[ind[off[p]:off[p + 1]]].sum() for p in range(K)], np.int64)
    centre = np.full(K, -1, np.int64)
    for p in np.lexsort((np.arange(K), -dens)).tolist():
        if centre[p] >= 0:
            continue
        centre[p] = p
        nb = ind[off[p]:off[p + 1]]
        centre[nb[centre[nb] < 0]] = p
    labels, count = L.labels_of(centre)
    return labels.astype(np.int64), count, centre


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("default_radius", [False, True])
@pytest.mark.parametrize("weighted", [True, False])
def test_centroid_leaders_are_the_sphere_exclusion_of_the_radius_graph(sort, default_radius, weighted):
    model, _ = tree()
    radius = 1.0 - THRESHOLD if default_radius else tree_radius()
    want_labels, want_count, want_centres = csr_leaders(model, radius, sort, weighted)
    before = (model._global_clustering_centroid_labels, model._n_global_clusters)
    labels, n, centres = model.centroid_leaders(None if default_radius else radius, sort=sort, weighted=weighted)
    K = len(model.get_centroids())
    assert labels.dtype == centres.dtype == np.int64 and labels.shape == centres.shape == (K,)
    assert n == want_count and (labels == want_labels).all() and (centres == want_centres).all()
    if not default_radius:
        assert 1 < n < K
    assert (model._global_clustering_centroid_labels, model._n_global_clusters) == before


def test_lead_clusters_then_save_and_load(tmp_path):
    import warnings

    from bblean_amd import BitBirch

    model, fps = tree()
    radius = tree_radius()
    want, count, _ = csr_leaders(model, radius, True, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert model.lead_clusters(radius) is model
    try:
        assert model._n_global_clusters == count and (model._global_clustering_centroid_labels == want + 1).all()
        assign = model.get_assignments(global_clusters=True)
        plain = model.get_assignments()
        assert (assign == (want + 1).astype(np.uint64)[plain.astype(np.int64) - 1]).all()  # cluster p of sort=True carries label p + 1
        merged = model.get_cluster_mol_ids(global_clusters=True)
        clusters = model.get_cluster_mol_ids()
        assert len(merged) == count
        assert all(sorted(merged[lab]) == sorted(i for p in np.flatnonzero(want == lab) for i in clusters[p]) for lab in range(count))
        model.save(tmp_path / "led.bb")
        back = BitBirch.load(tmp_path / "led.bb")
        assert back._n_global_clusters == count and (back._global_clustering_centroid_labels == want + 1).all()
        assert (back.get_assignments(global_clusters=True) == assign).all()
        assert back.get_cluster_mol_ids(global_clusters=True) == merged
    finally:
        model._global_clustering_centroid_labels, model._n_global_clusters = None, 0

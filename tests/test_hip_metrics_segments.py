r"""GPU: the clustering indices on the segmented kernels (bblean_amd/metrics.py over bb_cluster_stats.hip) against values
the reference produced (tests/golden/make_golden_metrics_segments.py), against the evaluation per cluster in the same
process (exactly equal), from a fitted tree, and by the number of launches they record."""
from __future__ import annotations

import ctypes as C
import contextlib
import warnings
from pathlib import Path

import numpy as np
import pytest

from bblean_amd.fingerprints import make_fake_fingerprints, unpack_fingerprints

pytestmark = pytest.mark.gpu
GOLD = np.load(Path(__file__).parent / "golden" / "metrics_segments.npz")
RTOL = 1e-12  # the stated tolerance of test_hip_metrics.py: np.dot runs on whatever BLAS the machine has


def golden_case(c):
    seed, n = (int(x) for x in GOLD[f"c{c}_case"][:2])
    fps = make_fake_fingerprints(n, seed=seed, pack=True)
    sizes = GOLD[f"c{c}_sizes"]
    members = GOLD[f"c{c}_members"]
    return fps, sizes, members, [fps[m] for m in np.split(members, np.cumsum(sizes)[:-1])]


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


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


# ---------------------------------------------------------------------------------------------------------------------
# the reference's values
# ---------------------------------------------------------------------------------------------------------------------


def test_golden_many_clusters():
    r"""202 clusters, sizes 1 and 2 and 2 100 among them, two of them copies of one row; then a twin of cluster 7."""
    from bblean_amd.metrics import ClusterSets, jt_dbi, jt_isim_chi

    fps, sizes, members, clusters = golden_case(0)
    twin = int(GOLD["c0_case"][2])
    assert len(clusters) >= 200 and {1, 2} <= set(sizes.tolist()) and sizes.max() > 2047
    want = GOLD["c0_values"]
    assert np.isfinite(want[:3]).all() and np.isinf(want[3])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for what, given in (("list", clusters), ("sets", ClusterSets(fps, off, members))):
        with quiet():
            got = [jt_isim_chi(given), jt_dbi(given), jt_dbi(given, centrals="medoid")]
        print(what, got, want[:3].tolist())
        np.testing.assert_allclose(np.array(got), want[:3], rtol=RTOL, atol=0, err_msg=what)
    with quiet():
        assert jt_dbi(clusters + [clusters[twin]]) == np.inf


def test_golden_with_dunn_packed_and_unpacked():
    from bblean_amd.metrics import jt_dbi, jt_isim_chi, jt_isim_dunn

    fps, sizes, members, clusters = golden_case(1)
    assert sizes.min() >= 2
    unpacked = [unpack_fingerprints(c) for c in clusters]
    got = [jt_isim_chi(clusters), jt_dbi(clusters), jt_dbi(clusters, centrals="medoid"), jt_isim_dunn(clusters),
           jt_isim_chi(unpacked, input_is_packed=False), jt_dbi(unpacked, input_is_packed=False),
           jt_dbi(unpacked, centrals="medoid", input_is_packed=False), jt_isim_dunn(unpacked, input_is_packed=False)]
    print(got, GOLD["c1_values"].tolist())
    np.testing.assert_allclose(np.array(got), GOLD["c1_values"], rtol=RTOL, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# the new path against the old one
# ---------------------------------------------------------------------------------------------------------------------


def indices(given, packed=True, given_centrals=None, **kw):
    r"""All three indices with every choice of centrals."""
    from bblean_amd.metrics import jt_dbi, jt_isim_chi, jt_isim_dunn

    p = dict(input_is_packed=packed, **kw)
    with quiet():
        out = [jt_isim_chi(given, **p), jt_dbi(given, **p), jt_dbi(given, centrals="medoid", **p), jt_isim_dunn(given, **p)]
        if given_centrals is not None:
            out += [jt_isim_chi(given, centrals=given_centrals, **p), jt_dbi(given, centrals=given_centrals, **p)]
            if packed:
                out.append(jt_isim_chi(given, all_fps_central=given_centrals[0], **p))
    return out


def same_values(a, b, what):
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and (a[~np.isnan(a)] == b[~np.isnan(b)]).all(), (what, a, b)


@pytest.mark.parametrize("c", [0, 1])
def test_segmented_equals_per_cluster(c):
    r"""List input, ClusterSets with and without members, host and device rows: exactly the per-cluster path's values."""
    import torch

    from bblean_amd.metrics import ClusterSets

    fps, sizes, members, clusters = golden_case(c)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cents = [x[0] for x in clusters]  # any packed rows do as given centrals
    old = indices(clusters, given_centrals=cents, _segmented=False)
    same_values(indices(clusters, given_centrals=cents), old, "list")
    same_values(indices(ClusterSets(fps, off, members), given_centrals=cents), old, "sets with members")
    flat = np.concatenate(clusters)
    same_values(indices(ClusterSets(flat, off), given_centrals=cents), old, "sets without members")
    same_values(indices(ClusterSets(torch.from_numpy(fps).cuda(), off, members), given_centrals=cents), old, "device rows")
    same_values(indices(ClusterSets(fps, off, members), given_centrals=cents, _segmented=False), old, "sets, per cluster")
    if c == 1:
        unpacked = [unpack_fingerprints(x) for x in clusters]
        ucents = [x[0] for x in unpacked]
        same_values(indices(unpacked, False, ucents), indices(unpacked, False, ucents, _segmented=False), "unpacked")


@pytest.fixture(scope="module")
def fitted():
    import torch

    from bblean_amd import BitBirch

    fps = make_fake_fingerprints(4000, seed=7)
    tree = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter").fit(torch.from_numpy(fps).cuda())
    return fps, tree


def test_tree_cluster_sets(fitted):
    r"""`tree.cluster_sets(fps)` of a fitted 4 000-row tree, host and device rows: the indices of the list built from
    `get_cluster_mol_ids()`, segmented and per cluster."""
    import torch

    fps, tree = fitted
    clusters = [fps[np.array(m)] for m in tree.get_cluster_mol_ids()]
    assert len(clusters) > 50
    want = indices(clusters)
    same_values(indices(clusters, _segmented=False), want, "per cluster")
    same_values(indices(tree.cluster_sets(fps)), want, "host rows")
    same_values(indices(tree.cluster_sets(torch.from_numpy(fps).cuda())), want, "device rows")
    unsorted = [fps[np.array(m)] for m in tree.get_cluster_mol_ids(sort=False)]
    same_values(indices(tree.cluster_sets(fps, sort=False)), indices(unsorted), "leaf order")


# ---------------------------------------------------------------------------------------------------------------------
# launches, warnings
# ---------------------------------------------------------------------------------------------------------------------


def test_launch_count_does_not_grow_with_k():
    from bblean_amd.metrics import jt_dbi, jt_isim_chi

    fps = make_fake_fingerprints(2400, seed=3, pack=True)
    counts = []
    for k in (40, 400):
        clusters = np.split(fps, k)  # 60 or 6 rows each
        with profiling():
            jt_isim_chi(clusters)
            jt_dbi(clusters)
            jt_dbi(clusters, centrals="medoid")
            counts.append({n: launches(n) for n in ("cluster_stats_seg", "dbi_pairs", "jt_arr_vec", "compl_isim_seg",
                                                    "add_rows", "centroid_from_sum", "jt_best_match")})
    print(counts)
    assert counts[0] == counts[1]
    assert counts[0]["cluster_stats_seg"] >= 3 and counts[0]["dbi_pairs"] == 2 and counts[0]["jt_arr_vec"] == 1
    assert counts[0]["add_rows"] == 0 and counts[0]["centroid_from_sum"] == 0 and counts[0]["jt_best_match"] == 0


def test_zero_division_warnings():
    r"""Identical centroids: 0 / 0 where neither cluster scatters, x / 0 where they do - NumPy's RuntimeWarnings in the
    reference, raised here from the kernel's flags."""
    from bblean_amd.metrics import jt_dbi

    fps, sizes, members, clusters = golden_case(0)
    few = clusters[5:12] + clusters[-2:]  # the two copies of one row among them
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        jt_dbi(few)
    text = [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
    assert any("invalid value" in t for t in text) and not any("divide by zero" in t for t in text), text
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert jt_dbi(few + [clusters[7]]) == np.inf
    text = [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning)]
    assert any("invalid value" in t for t in text) and any("divide by zero" in t for t in text), text
    for segmented in (None, False):  # the per-cluster path warns there too (NumPy does)
        with pytest.warns(RuntimeWarning, match="divide by zero"):
            jt_dbi(few + [clusters[7]], _segmented=segmented)


def test_dunn_warns_for_a_singleton():
    from bblean_amd.metrics import jt_isim_dunn

    fps, sizes, members, clusters = golden_case(0)
    assert len(clusters[1]) == 1
    for segmented in (None, False):
        with pytest.warns(RuntimeWarning, match="Expected n_objects >= 2"):
            jt_isim_dunn(clusters[:6], _segmented=segmented)


def test_slabs_of_whole_sets():
    r"""Host rows beyond a slab go through in slabs of whole sets: the same values."""
    import os

    from bblean_amd.similarity import jt_cluster_stats_segments

    fps, sizes, members, clusters = golden_case(1)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    want = jt_cluster_stats_segments(fps, off, members, want=("centroids", "isim", "dist", "sums"))
    old = os.environ.get("BBHIP_SLAB_KB")
    os.environ["BBHIP_SLAB_KB"] = "32"  # 128 rows of 256 bytes
    try:
        got = jt_cluster_stats_segments(fps, off, members, want=("centroids", "isim", "dist", "sums"))
        cen = jt_cluster_stats_segments(fps, off, members, centrals=want["centroids"], want=("dist",))
    finally:
        os.environ.pop("BBHIP_SLAB_KB")
        if old is not None:
            os.environ["BBHIP_SLAB_KB"] = old
    for w in want:
        assert np.array_equal(got[w].view(np.uint8), want[w].view(np.uint8)), w
    assert np.array_equal(cen["dist"], want["dist"])

r"""CPU: `metrics.ClusterSets` and the argument checks of `jt_cluster_stats_segments` (made before the library is loaded),
which inputs `_Clustering` hands to the segmented kernels and which it keeps on the per-cluster path, the float64
reductions of the indices over a NumPy stand-in for the library calls, and the gather order of `BitBirch.cluster_sets`
on the oracle engine."""
from __future__ import annotations

import numpy as np
import pytest

import cluster_stats_refs as cs
import kernel_refs as R

ROWS = np.arange(48, dtype=np.uint8).reshape(6, 8)


@pytest.fixture
def no_library(monkeypatch):
    from bblean_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("kwargs, message", [
    (dict(fps=np.zeros(8, np.uint8), offsets=[0, 1]), "2-dimensional uint8"),
    (dict(fps=np.zeros((6, 8), np.uint16), offsets=[0, 6]), "2-dimensional uint8"),
    (dict(fps=ROWS, offsets=[1, 6]), "start at 0"),
    (dict(fps=ROWS, offsets=[0, 4, 3, 6]), "decrease"),
    (dict(fps=ROWS, offsets=[0, 7]), "more rows"),
    (dict(fps=ROWS, offsets=[0, 3, 3, 6]), "must be > 0"),
    (dict(fps=ROWS, offsets=[0]), "at least one set"),
    (dict(fps=ROWS, offsets=[0.0, 6.0]), "integer"),
    (dict(fps=ROWS, offsets=[0, 3], members=[0, 1, 6]), "row numbers"),
    (dict(fps=ROWS, offsets=[0, 4], members=[0, 1, 2]), "more rows"),
    (dict(fps=ROWS, offsets=[0, 6], n_features=12), "divisible by 8"),
    (dict(fps=ROWS, offsets=[0, 6], n_features=72), "divisible by 8"),
])
def test_argument_errors(no_library, kwargs, message):
    from bblean_amd.metrics import ClusterSets
    from bblean_amd.similarity import jt_cluster_stats_segments

    with pytest.raises(ValueError, match=message):
        ClusterSets(**kwargs)
    with pytest.raises(ValueError, match=message):
        jt_cluster_stats_segments(**kwargs)


@pytest.mark.parametrize("kwargs, message", [
    (dict(want=()), "want must name"),
    (dict(want=("centroid",)), "want must name"),
    (dict(centrals=np.zeros((1, 8), np.uint8)), "one packed row per set"),
    (dict(centrals=np.zeros((2, 7), np.uint8)), "one packed row per set"),
    (dict(centrals=np.zeros((2, 8), np.int16)), "one packed row per set"),
    (dict(centrals=np.zeros(16, np.uint8)), "one packed row per set"),
])
def test_stats_argument_errors(no_library, kwargs, message):
    from bblean_amd.similarity import jt_cluster_stats_segments

    with pytest.raises(ValueError, match=message):
        jt_cluster_stats_segments(ROWS, [0, 2, 6], **kwargs)


def test_cluster_sets_container():
    from bblean_amd.metrics import ClusterSets

    s = ClusterSets(ROWS, [0, 2, 5], members=[5, 0, 3, 3, 1], n_features=56)
    assert len(s) == 2 and s.sizes.tolist() == [2, 3] and s.n_features == 56
    assert s.offsets.dtype == np.int64 and s.members.dtype == np.int64
    got = s.to_list()
    assert [g.tolist() for g in got] == [ROWS[[5, 0], :7].tolist(), ROWS[[3, 3, 1], :7].tolist()]
    plain = ClusterSets(ROWS, np.array([0, 4, 6], dtype=np.int32))
    assert plain.members is None and [len(g) for g in plain.to_list()] == [4, 2] and plain.n_features == 64


def test_entry_points_are_declared_and_bound():
    from bblean_amd import _lib, metrics, similarity

    assert len(_lib._PROTOTYPES["bbh_cluster_stats_segments"][1]) == 15
    assert len(_lib._PROTOTYPES["bbh_dbi_worst_ratios"][1]) == 8
    assert "jt_cluster_stats_segments" in similarity.__all__ and "ClusterSets" in metrics.__all__
    assert cs.DBI_TILE == 64


# ---------------------------------------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------------------------------------


def packed_clusters(sizes=(3, 1, 5), nb=8, seed=0):
    rng = np.random.default_rng(seed)
    return [R.density_rows(rng, m, nb, 0.2, 0.7) for m in sizes]


def test_routing(no_library):
    from bblean_amd.metrics import ClusterSets, _Clustering

    cl = packed_clusters()
    seg = _Clustering(cl, True, None)
    assert seg.sets is not None and seg.sizes == [3, 1, 5] and seg.total == 9 and len(seg) == 3
    assert (seg.sets.fps == np.concatenate(cl)).all() and seg.sets.offsets.tolist() == [0, 3, 4, 9]
    assert _Clustering(cl, True, 56).sets.n_features == 56
    un = [np.unpackbits(c, axis=1) for c in cl]
    seg = _Clustering(un, False, None)  # packed once, as a whole
    assert seg.sets is not None and (seg.sets.fps == np.concatenate(cl)).all() and seg.sets.n_features == 64
    sets = ClusterSets(np.concatenate(cl), [0, 3, 4, 9])
    assert _Clustering(sets, True, None).sets is sets
    # everything else keeps the calls per cluster
    old = _Clustering(sets, True, None, segmented=False)
    assert old.sets is None and [c.tolist() for c in old.given] == [c.tolist() for c in cl] and old.given_packed
    assert _Clustering(cl, True, None, segmented=False).sets is None
    assert _Clustering(cl + [np.zeros((2, 9), np.uint8)], True, None).sets is None          # ragged widths
    assert _Clustering([c.astype(np.uint16) for c in cl], True, None).sets is None           # wider dtype
    assert _Clustering(cl + [np.zeros((0, 8), np.uint8)], True, None).sets is None           # an empty cluster
    assert _Clustering([u[:, :60] for u in un], False, None).sets is None                    # 60 features
    assert _Clustering(cl, True, 60).sets is None and _Clustering(cl, True, 72).sets is None
    assert _Clustering([c.tolist() for c in cl], True, None).sets is None                    # not arrays
    assert _Clustering([], True, None).sets is None
    with pytest.raises(ValueError, match="too large"):
        big = ClusterSets.__new__(ClusterSets)
        big.fps, big.offsets, big.members, big.n_features = None, np.array([0, 1 << 31]), None, 2048
        _Clustering(big, True, None)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reductions, over NumPy stand-ins for the library calls
# ---------------------------------------------------------------------------------------------------------------------


@pytest.fixture
def numpy_library(no_library, monkeypatch):
    from bblean_amd import metrics, similarity

    calls = []

    def stats(fps, offsets, members=None, n_features=None, centrals=None, want=("centroids", "isim", "dist")):
        calls.append(tuple(want))
        ref = cs.ref_cluster_stats(fps, np.asarray(offsets), members, n_features, centrals)
        return {w: ref[("centroids", "isim", "dist", "sums").index(w)] for w in want}

    def sim(arr, vec):
        calls.append("jt_sim_packed")
        return R.ref_arr_vec(arr, vec)[0]

    def worst(centrals, scatter):
        calls.append("dbi")
        return cs.ref_worst_ratios(np.asarray(centrals), scatter)

    monkeypatch.setattr(similarity, "jt_cluster_stats_segments", stats)
    monkeypatch.setattr(similarity, "jt_sim_packed", sim)
    monkeypatch.setattr(metrics, "_dbi_worst_ratios", worst)
    return calls


def test_chi_and_dbi_reductions(numpy_library):
    r"""The indices as the reference writes them (metrics.py:47-159), restated with the NumPy references."""
    from bblean_amd.metrics import jt_dbi, jt_isim_chi

    cl = packed_clusters((4, 1, 7, 2, 30), 8, seed=5)
    k, n = len(cl), sum(len(c) for c in cl)
    cents = [R.ref_centroid(R.ref_add_rows_packed(c, 64), len(c), True) for c in cl]
    whole = R.ref_centroid(R.ref_add_rows_packed(np.concatenate(cl), 64), n, True)
    bcss = wcss = 0.0
    scatter = []
    for c, cen in zip(cl, cents):
        bcss += len(c) * (1 - R.ref_arr_vec(cen[None], whole)[0].item()) ** 2
        d = 1 - R.ref_arr_vec(c, cen)[0]
        wcss += np.dot(d, d)
        scatter.append(np.sum(d) / len(c))
    assert jt_isim_chi(cl) == bcss * (n - k) / (wcss * (k - 1))
    assert numpy_library == [("centroids",), ("centroids", "dist"), "jt_sim_packed"]
    del numpy_library[:]
    numer = 0.0
    for i in range(k):
        max_d = 0.0
        for j in range(k):
            if i != j:
                max_d = max(max_d, (scatter[i] + scatter[j]) / (1 - R.ref_arr_vec(cents[i][None], cents[j])[0].item()))
        numer += max_d
    assert jt_dbi(cl) == numer / n
    assert numpy_library == [("centroids", "dist"), "dbi"]
    assert jt_isim_chi(cl[:1]) == 0


def test_zero_division_warnings_come_from_the_flags(numpy_library):
    from bblean_amd.metrics import jt_dbi

    row = np.full((1, 8), 0x3C, np.uint8)
    with pytest.warns(RuntimeWarning, match="invalid value"):
        assert jt_dbi([np.repeat(row, 3, axis=0), np.repeat(row, 2, axis=0)]) == 0.0
    cl = packed_clusters((4, 6))
    with pytest.warns(RuntimeWarning, match="divide by zero"):
        assert jt_dbi([cl[0], cl[1], cl[0]]) == np.inf


# ---------------------------------------------------------------------------------------------------------------------
# BitBirch.cluster_sets on the oracle engine
# ---------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def oracle_tree():
    from oracle_engine import OracleEngine

    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(1500, seed=21)
    return fps, BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter", _engine_factory=OracleEngine).fit(fps)


def as_lists(sets):
    o = sets.offsets.tolist()
    return [sets.members[b:e].tolist() for b, e in zip(o[:-1], o[1:])]


@pytest.mark.parametrize("sort", [True, False])
def test_cluster_sets_gather_order(oracle_tree, sort):
    fps, tree = oracle_tree
    sets = tree.cluster_sets(fps, sort=sort)
    want = tree.get_cluster_mol_ids(sort=sort)
    assert len(want) > 20 and as_lists(sets) == want
    assert sets.fps is fps and sets.n_features == 2048
    assert sorted(sets.members.tolist()) == list(range(1500))


def test_cluster_sets_of_global_clusters(oracle_tree):
    fps, tree = oracle_tree
    n_leaves = len(tree.get_cluster_mol_ids())
    tree._global_clustering_centroid_labels = np.random.default_rng(0).integers(1, 6, n_leaves)
    tree._n_global_clusters = 5
    try:
        want = tree.get_cluster_mol_ids(global_clusters=True)
        assert len(want) == 5 and as_lists(tree.cluster_sets(fps, global_clusters=True)) == want
    finally:
        tree._global_clustering_centroid_labels = None
        tree._n_global_clusters = 0

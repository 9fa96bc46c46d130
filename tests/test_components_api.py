r"""CPU: the Python face of connected components (`similarity.jt_components_packed`, `BitBirch.centroid_components`,
`BitBirch.link_clusters`): signatures, the argument errors, which are raised before the library is called, and what
`link_clusters` stores, on a model fitted by the CPU oracle engine with `jt_components_packed` replaced by the NumPy
reference.  The answers of the library are checked on the GPU by tests/test_hip_components.py."""
from __future__ import annotations

import inspect
import warnings

import numpy as np
import pytest

import components_refs as C
from oracle_engine import OracleEngine
from test_radius_api import no_library  # noqa: F401  (the fixture)

THRESHOLD = 0.5


@pytest.fixture()
def fitted():
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(600, seed=11)
    return BitBirch(branching_factor=50, threshold=THRESHOLD, merge_criterion="diameter", _engine_factory=OracleEngine).fit(fps)


@pytest.fixture()
def reference_components(monkeypatch):
    r"""`jt_components_packed` computed by components_refs; records (n rows, radius) of every call."""
    from bblean_amd import similarity

    seen = []

    def fake(rows, radius, return_roots=False):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        seen.append((len(rows), radius))
        roots, labels, count = C.exact_components(rows, radius)
        out = (labels.astype(np.int64), count)
        return out + (roots.astype(np.int64),) if return_roots else out

    monkeypatch.setattr(similarity, "jt_components_packed", fake)
    return seen


def test_signatures():
    from bblean_amd import BitBirch, _lib, similarity

    assert "jt_components_packed" in similarity.__all__ and "bbh_jt_components" in _lib.EXPORTED_SYMBOLS
    p = inspect.signature(similarity.jt_components_packed).parameters
    assert list(p) == ["rows", "radius", "return_roots"] and p["return_roots"].default is False
    assert p["radius"].default is inspect.Parameter.empty
    p = inspect.signature(BitBirch.centroid_components).parameters
    assert list(p) == ["self", "radius", "sort"] and p["radius"].default is None and p["sort"].default is True
    p = inspect.signature(BitBirch.link_clusters).parameters
    assert list(p) == ["self", "radius"] and p["radius"].default is None


def test_prototype_has_the_header_s_eight_arguments():
    import ctypes as Ct

    from bblean_amd import _lib

    res, args = _lib._PROTOTYPES["bbh_jt_components"]
    assert res is Ct.c_int and len(args) == 8
    assert args[1] is args[2] is Ct.c_int64 and args[3] is Ct.c_double
    assert all(a is Ct.c_void_p for j, a in enumerate(args) if j not in (1, 2, 3))


@pytest.mark.parametrize("radius,exc", [(float("nan"), ValueError), (np.float64("nan"), ValueError), ("0.3", TypeError),
                                        (None, TypeError), (True, TypeError)])
def test_refuses_the_radius(no_library, radius, exc):  # noqa: F811
    from bblean_amd.similarity import jt_components_packed

    with pytest.raises(exc, match="radius"):
        jt_components_packed(np.zeros((5, 16), np.uint8), radius)


def test_refuses_the_rows(no_library):  # noqa: F811
    from bblean_amd.similarity import jt_components_packed

    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_components_packed(np.zeros(16, np.uint8), 0.3)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_components_packed(np.zeros((2, 3, 16), np.uint8), 0.3)
    with pytest.raises(TypeError, match="uint8"):
        jt_components_packed(np.zeros((5, 16), np.int32), 0.3)
    with pytest.raises(TypeError, match="uint8"):
        jt_components_packed(np.zeros((5, 16), np.float64), 0.3)
    with pytest.raises(RuntimeError, match="one byte"):
        jt_components_packed(np.zeros((5, 0), np.uint8), 0.3)


def test_model_refuses_before_the_library(no_library, fitted):  # noqa: F811
    from bblean_amd import BitBirch

    for call in (fitted.centroid_components, fitted.link_clusters):
        with pytest.raises(ValueError, match="radius"):
            call(float("nan"))
        with pytest.raises(TypeError, match="radius"):
            call("0.3")
    with pytest.raises(ValueError):
        BitBirch().centroid_components(0.3)
    with pytest.raises(ValueError):
        BitBirch().link_clusters()


def _partition(labels):
    return sorted(sorted(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels))


def test_centroid_components_leaves_the_model_alone(fitted, reference_components):
    model = fitted
    cents = np.array(model.get_centroids())
    before = dict(model.__dict__)
    K = len(cents)
    d = np.sort(C.R.exact(cents, cents)[3], axis=None)
    radius = float(d[K + 2 * K])  # about one neighbour each
    labels, count = model.centroid_components(radius)
    want = C.exact_components(cents, radius)
    assert 1 < count < K and count == want[2]
    assert labels.dtype == np.int64 and labels.shape == (K,) and (labels == want[1]).all()
    assert reference_components[-1] == (K, radius)
    assert model._global_clustering_centroid_labels is None and model._n_global_clusters == 0
    assert set(model.__dict__) == set(before) and all(model.__dict__[k] is before[k] for k in before)
    # sort=False: the same partition of the clusters, over the other positions
    unsorted = np.array(model.get_centroids(sort=False))
    lu, cu = model.centroid_components(radius, sort=False)
    assert cu == count and (lu == C.exact_components(unsorted, radius)[1]).all()
    order = model._leaf_order(True)
    back = np.empty(K, np.int64)
    back[order] = labels  # labels by leaf position
    assert _partition(back) == _partition(lu)
    # the default radius is the merge threshold as a distance
    model.centroid_components()
    assert reference_components[-1] == (K, 1.0 - THRESHOLD)


def test_link_clusters(fitted, reference_components):
    model = fitted
    with pytest.raises(ValueError):
        model.get_cluster_mol_ids(global_clusters=True)
    cents = np.array(model.get_centroids())
    K = len(cents)
    radius = float(np.sort(C.R.exact(cents, cents)[3], axis=None)[K + 2 * K])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no "experimental" warning: that one is global_clustering's
        assert model.link_clusters(radius) is model
    roots, labels, count = C.exact_components(cents, radius)
    assert 1 < count < K
    assert model._n_global_clusters == count
    assert (model._global_clustering_centroid_labels == labels.astype(np.int64) + 1).all()
    assert model._global_clustering_centroid_labels.dtype == np.int64
    clusters = model.get_cluster_mol_ids()
    merged = model.get_cluster_mol_ids(global_clusters=True)
    assert len(merged) == count
    for lab in range(count):
        members = [i for pos in np.flatnonzero(labels == lab) for i in clusters[pos]]
        assert merged[lab] == members  # exactly the members of the linked clusters, in cluster order
    assign = model.get_assignments(global_clusters=True)
    for lab in range(count):
        assert len(set(assign[merged[lab]].tolist())) == 1
    assert len(np.unique(assign)) == count
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.link_clusters()
    assert reference_components[-1] == (K, 1.0 - THRESHOLD)
    want = C.exact_components(cents, 1.0 - THRESHOLD)
    assert model._n_global_clusters == want[2] and (model._global_clustering_centroid_labels == want[1] + 1).all()

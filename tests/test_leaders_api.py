r"""CPU: the Python face of leader clustering (`similarity.jt_leaders_packed`, `BitBirch.centroid_leaders`,
`BitBirch.lead_clusters`): signatures, the argument errors, which are raised before the library is called, and what
`lead_clusters` stores, on a model fitted by the CPU oracle engine with `jt_leaders_packed` replaced by the NumPy reference.
The answers of the library are checked on the GPU by tests/test_hip_leaders.py."""
from __future__ import annotations

import inspect
import warnings

import numpy as np
import pytest

import leaders_refs as L
from oracle_engine import OracleEngine
from test_radius_api import no_library  # noqa: F401  (the fixture)

THRESHOLD = 0.5


@pytest.fixture()
def fitted():
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(600, seed=11)
    return BitBirch(branching_factor=50, threshold=THRESHOLD, merge_criterion="diameter", _engine_factory=OracleEngine).fit(fps)


@pytest.fixture()
def reference_leaders(monkeypatch):
    r"""`jt_leaders_packed` computed by leaders_refs; records (n rows, radius, weights, ties) of every call."""
    from bblean_amd import similarity

    seen = []

    def fake(rows, radius, weights=None, ties="low", return_centres=False, return_density=False):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        seen.append((len(rows), radius, None if weights is None else np.array(weights), ties))
        centre, label, count, dens = L.exact_leaders(rows, radius, weights, ties == "high")
        out = (label.astype(np.int64), count)
        if return_centres:
            out += (centre.astype(np.int64),)
        if return_density:
            out += (dens,)
        return out

    monkeypatch.setattr(similarity, "jt_leaders_packed", fake)
    return seen


def test_signatures():
    from bblean_amd import BitBirch, _lib, similarity

    assert "jt_leaders_packed" in similarity.__all__ and "bbh_jt_leaders" in _lib.EXPORTED_SYMBOLS
    p = inspect.signature(similarity.jt_leaders_packed).parameters
    assert list(p) == ["rows", "radius", "weights", "ties", "return_centres", "return_density"]
    assert p["radius"].default is inspect.Parameter.empty and p["weights"].default is None and p["ties"].default == "low"
    assert p["return_centres"].default is False and p["return_density"].default is False
    p = inspect.signature(BitBirch.centroid_leaders).parameters
    assert list(p) == ["self", "radius", "sort", "weighted"]
    assert p["radius"].default is None and p["sort"].default is True and p["weighted"].default is True
    p = inspect.signature(BitBirch.lead_clusters).parameters
    assert list(p) == ["self", "radius", "weighted"] and p["radius"].default is None and p["weighted"].default is True
    assert _lib.BBH_LEADERS_TIES_HIGH == 1


def test_prototype_has_the_header_s_eleven_arguments():
    import ctypes as Ct

    from bblean_amd import _lib

    res, args = _lib._PROTOTYPES["bbh_jt_leaders"]
    assert res is Ct.c_int and len(args) == 11
    assert args[1] is args[2] is Ct.c_int64 and args[3] is Ct.c_double and args[5] is Ct.c_uint32
    assert all(a is Ct.c_void_p for j, a in enumerate(args) if j not in (1, 2, 3, 5))


@pytest.mark.parametrize("radius,exc", [(float("nan"), ValueError), (np.float64("nan"), ValueError), ("0.3", TypeError),
                                        (None, TypeError), (True, TypeError)])
def test_refuses_the_radius(no_library, radius, exc):  # noqa: F811
    from bblean_amd.similarity import jt_leaders_packed

    with pytest.raises(exc, match="radius"):
        jt_leaders_packed(np.zeros((5, 16), np.uint8), radius)


def test_refuses_the_rows(no_library):  # noqa: F811
    from bblean_amd.similarity import jt_leaders_packed

    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_leaders_packed(np.zeros(16, np.uint8), 0.3)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_leaders_packed(np.zeros((2, 3, 16), np.uint8), 0.3)
    with pytest.raises(TypeError, match="uint8"):
        jt_leaders_packed(np.zeros((5, 16), np.int32), 0.3)
    with pytest.raises(TypeError, match="uint8"):
        jt_leaders_packed(np.zeros((5, 16), np.float64), 0.3)
    with pytest.raises(RuntimeError, match="one byte"):
        jt_leaders_packed(np.zeros((5, 0), np.uint8), 0.3)


@pytest.mark.parametrize("ties", ["LOW", "", None, 1, "lowest"])
def test_refuses_the_ties(no_library, ties):  # noqa: F811
    from bblean_amd.similarity import jt_leaders_packed

    with pytest.raises(ValueError, match="ties"):
        jt_leaders_packed(np.zeros((5, 16), np.uint8), 0.3, ties=ties)


def test_refuses_the_weights(no_library):  # noqa: F811
    from bblean_amd.similarity import jt_leaders_packed

    rows = np.zeros((5, 16), np.uint8)
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=np.ones(4, np.int64))  # the wrong length
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=np.ones((5, 1), np.int64))
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=np.array([1, 1, -1, 1, 1]))  # negative
    with pytest.raises(ValueError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=np.array([1, 1, 2 ** 32, 1, 1]))  # too large
    with pytest.raises(TypeError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=np.ones(5, np.float64))  # not integers
    with pytest.raises(TypeError, match="weights"):
        jt_leaders_packed(rows, 0.3, weights=[1, 1, 1.5, 1, 1])


def test_model_refuses_before_the_library(no_library, fitted):  # noqa: F811
    from bblean_amd import BitBirch

    for call in (fitted.centroid_leaders, fitted.lead_clusters):
        with pytest.raises(ValueError, match="radius"):
            call(float("nan"))
        with pytest.raises(TypeError, match="radius"):
            call("0.3")
    with pytest.raises(ValueError):
        BitBirch().centroid_leaders(0.3)
    with pytest.raises(ValueError):
        BitBirch().lead_clusters()


def _partition(labels):
    return sorted(sorted(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels))


def _radius(cents):
    K = len(cents)
    return float(np.sort(L.C.R.exact(cents, cents)[3], axis=None)[K + 2 * K])  # about one neighbour each


def test_centroid_leaders_leaves_the_model_alone(fitted, reference_leaders):
    model = fitted
    cents = np.array(model.get_centroids())
    sizes = np.array([len(m) for m in model.get_cluster_mol_ids()])
    before = dict(model.__dict__)
    K = len(cents)
    radius = _radius(cents)
    labels, count, centres = model.centroid_leaders(radius)
    want = L.exact_leaders(cents, radius, sizes)
    assert 1 < count < K and count == want[2]
    assert labels.dtype == centres.dtype == np.int64 and labels.shape == centres.shape == (K,)
    assert (labels == want[1]).all() and (centres == want[0]).all()
    n, r, w, ties = reference_leaders[-1]
    assert (n, r, ties) == (K, radius, "low") and (w == sizes).all()  # the weights are the clusters' n_samples
    assert model._global_clustering_centroid_labels is None and model._n_global_clusters == 0
    assert set(model.__dict__) == set(before) and all(model.__dict__[k] is before[k] for k in before)
    # unweighted
    lu, cu, ce = model.centroid_leaders(radius, weighted=False)
    assert reference_leaders[-1][2] is None
    want = L.exact_leaders(cents, radius)
    assert cu == want[2] and (lu == want[1]).all() and (ce == want[0]).all()
    # sort=False: over the other positions, with the weights in that order
    unsorted = np.array(model.get_centroids(sort=False))
    usizes = np.array([len(m) for m in model.get_cluster_mol_ids(sort=False)])
    lu, cu, ce = model.centroid_leaders(radius, sort=False)
    want = L.exact_leaders(unsorted, radius, usizes)
    assert cu == want[2] and (lu == want[1]).all() and (ce == want[0]).all()
    assert (reference_leaders[-1][2] == usizes).all()
    # the default radius is the merge threshold as a distance
    model.centroid_leaders()
    assert reference_leaders[-1][:2] == (K, 1.0 - THRESHOLD)


def test_lead_clusters(fitted, reference_leaders):
    model = fitted
    with pytest.raises(ValueError):
        model.get_cluster_mol_ids(global_clusters=True)
    cents = np.array(model.get_centroids())
    sizes = np.array([len(m) for m in model.get_cluster_mol_ids()])
    K = len(cents)
    radius = _radius(cents)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no "experimental" warning: that one is global_clustering's
        assert model.lead_clusters(radius) is model
    centre, labels, count, _ = L.exact_leaders(cents, radius, sizes)
    assert 1 < count < K
    assert model._n_global_clusters == count
    assert (model._global_clustering_centroid_labels == labels.astype(np.int64) + 1).all()
    assert model._global_clustering_centroid_labels.dtype == np.int64
    clusters = model.get_cluster_mol_ids()
    merged = model.get_cluster_mol_ids(global_clusters=True)
    assert len(merged) == count
    for lab in range(count):
        members = [i for pos in np.flatnonzero(labels == lab) for i in clusters[pos]]
        assert merged[lab] == members  # exactly the members of the led clusters, in cluster order
    assign = model.get_assignments(global_clusters=True)
    for lab in range(count):
        assert len(set(assign[merged[lab]].tolist())) == 1
    assert len(np.unique(assign)) == count
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.lead_clusters(weighted=False)
    assert reference_leaders[-1][:3] == (K, 1.0 - THRESHOLD, None)
    want = L.exact_leaders(cents, 1.0 - THRESHOLD)
    assert model._n_global_clusters == want[2] and (model._global_clustering_centroid_labels == want[1] + 1).all()

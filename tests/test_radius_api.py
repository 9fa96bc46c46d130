r"""CPU: the Python face of radius search (`similarity.jt_radius_packed`, `sklearn.BitBirch.radius_neighbors` /
`radius_neighbors_graph`, `BitBirch.centroid_radius_neighbors`): signatures, and the argument errors, which are raised
before the library is called.  The fitted models come from the CPU oracle engine.  Without a GPU a call that passes the
checks raises `BBHipError` (there is no CPU path); the answers are checked on the GPU by tests/test_hip_radius.py."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

from oracle_engine import OracleEngine
from sklearn_cases import CASES, rows


@pytest.fixture()
def no_library(monkeypatch):
    r"""Any call into the library fails the test."""
    from bblean_amd import _lib

    def boom():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", boom)


@pytest.fixture(scope="module")
def fitted():
    import bblean_amd.sklearn as bs
    from bblean_amd import make_fake_fingerprints

    fit_x, qry = rows(CASES["C"], make_fake_fingerprints)
    est = bs.BitBirch(threshold=CASES["C"]["thr"], branching_factor=CASES["C"]["bf"])
    est._engine_factory = OracleEngine
    return est.fit(fit_x), qry


def _gpu() -> bool:
    import torch

    return torch.cuda.is_available()


def test_signatures():
    import bblean_amd.sklearn as bs
    from bblean_amd import BitBirch, _lib, similarity

    assert "jt_radius_packed" in similarity.__all__ and "bbh_jt_radius" in _lib.EXPORTED_SYMBOLS
    p = inspect.signature(similarity.jt_radius_packed).parameters
    assert list(p) == ["queries", "rows", "radius", "exclude", "return_counts", "sort"]
    assert p["exclude"].default is None and p["return_counts"].default is False and p["sort"].default is False
    assert p["radius"].default is inspect.Parameter.empty
    for cls, packed in ((bs.BitBirch, True), (bs.UnpackedBitBirch, False)):
        p = inspect.signature(cls.radius_neighbors).parameters
        assert list(p) == ["self", "X", "radius", "return_distance", "sort_results", "input_is_packed", "n_features"]
        assert (p["X"].default, p["radius"].default, p["return_distance"].default, p["sort_results"].default) == (
            None, None, True, False)
        assert p["input_is_packed"].default is packed and p["n_features"].default is None
        p = inspect.signature(cls.radius_neighbors_graph).parameters
        assert list(p) == ["self", "X", "radius", "mode", "input_is_packed", "n_features"]
        assert (p["X"].default, p["radius"].default, p["mode"].default) == (None, None, "connectivity")
        assert p["input_is_packed"].default is packed and p["n_features"].default is None
    p = inspect.signature(BitBirch.centroid_radius_neighbors).parameters
    assert list(p) == ["self", "radius", "sort"] and p["sort"].default is True
    assert p["radius"].default is inspect.Parameter.empty


def test_prototype_has_the_header_s_fifteen_arguments():
    import ctypes as C

    from bblean_amd import _lib

    res, args = _lib._PROTOTYPES["bbh_jt_radius"]
    assert res is C.c_int and len(args) == 15
    assert args[6] is C.c_double and args[8] is C.c_int64 and args[1] is args[2] is args[4] is args[5] is C.c_int64
    assert all(a is C.c_void_p for j, a in enumerate(args) if j not in (1, 2, 4, 5, 6, 8))


@pytest.mark.parametrize("radius,exc", [(float("nan"), ValueError), (np.float64("nan"), ValueError), ("0.3", TypeError),
                                        (None, TypeError), (True, TypeError), (0.3 + 0j, TypeError)])
def test_jt_radius_packed_refuses_the_radius(no_library, radius, exc):
    from bblean_amd.similarity import jt_radius_packed

    q = np.zeros((5, 16), np.uint8)
    with pytest.raises(exc, match="radius"):
        jt_radius_packed(q, q, radius)


def test_jt_radius_packed_refuses_operands(no_library):
    from bblean_amd.similarity import jt_radius_packed

    q, c = np.zeros((5, 16), np.uint8), np.zeros((8, 32), np.uint8)
    with pytest.raises(RuntimeError, match="same packed width"):
        jt_radius_packed(q, c, 0.3)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_radius_packed(q[0], c, 0.3)
    with pytest.raises(RuntimeError):
        jt_radius_packed(q, np.zeros((0, 16), np.uint8), 0.3)
    with pytest.raises(ValueError, match="exclude"):
        jt_radius_packed(q, q, 0.3, exclude=np.arange(4))
    with pytest.raises(ValueError, match="exclude"):
        jt_radius_packed(q, q, 0.3, exclude=np.zeros(5))
    with pytest.raises(ValueError, match="exclude"):
        jt_radius_packed(q, q, 0.3, exclude=np.zeros((5, 1), np.int64))


def test_first_capacity():
    r"""32 entries per query, at least 4096, never more than all pairs."""
    from bblean_amd.similarity import _radius_first_capacity

    assert _radius_first_capacity(1, 1) == 1 and _radius_first_capacity(10, 100) == 1000
    assert _radius_first_capacity(10, 1000) == 4096 and _radius_first_capacity(1000, 1000) == 32000
    assert _radius_first_capacity(0, 5) == 0


def test_estimator_refuses_before_the_library(no_library, fitted):
    est, qry = fitted
    for call in (est.radius_neighbors, est.radius_neighbors_graph):
        with pytest.raises(ValueError, match="radius"):
            call(qry, float("nan"))
        with pytest.raises(TypeError, match="radius"):
            call(None, "0.3")
        with pytest.raises(ValueError, match="packed bytes"):
            call(qry[:, :-1], 0.3)
    with pytest.raises(ValueError, match="sort_results"):
        est.radius_neighbors(qry, 0.3, return_distance=False, sort_results=True)
    with pytest.raises(ValueError, match="mode"):
        est.radius_neighbors_graph(qry, 0.3, mode="similarity")
    with pytest.raises(ValueError, match="radius"):
        est.centroid_radius_neighbors(float("nan"))
    with pytest.raises(TypeError, match="radius"):
        est.centroid_radius_neighbors(None)


def test_radius_none_is_one_minus_the_threshold(monkeypatch, fitted):
    r"""The default radius of the estimator is its merge threshold as a distance; a given radius goes through as it is."""
    import bblean_amd.sklearn as bs

    est, qry = fitted
    seen = []

    def spy(queries, table, radius, exclude=None, return_counts=False, sort=False):
        seen.append((len(queries), radius, None if exclude is None else np.asarray(exclude).tolist(), sort))
        n = len(queries)
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)

    monkeypatch.setattr(bs, "jt_radius_packed", spy)
    K = len(est.subcluster_centers_)
    dist, ind = est.radius_neighbors(qry)
    assert seen[-1] == (len(qry), 1.0 - CASES["C"]["thr"], None, False)
    assert dist.dtype == ind.dtype == object and dist.shape == ind.shape == (len(qry),)
    assert all(a.dtype == np.int64 and len(a) == 0 for a in ind) and all(a.dtype == np.float64 for a in dist)
    est.radius_neighbors(None, sort_results=True)
    assert seen[-1] == (K, 1.0 - CASES["C"]["thr"], list(range(K)), True)
    est.radius_neighbors(qry, 0.25)
    assert seen[-1][1] == 0.25
    g = est.radius_neighbors_graph()
    assert seen[-1] == (K, 1.0 - CASES["C"]["thr"], list(range(K)), False) and g.shape == (K, K) and g.nnz == 0
    assert est.radius_neighbors_graph(qry, 0).shape == (len(qry), K) and seen[-1][1] == 0.0


def test_unfitted():
    import bblean_amd.sklearn as bs
    from bblean_amd import BitBirch
    from sklearn.exceptions import NotFittedError

    with pytest.raises(NotFittedError):
        bs.BitBirch().radius_neighbors(np.zeros((2, 256), np.uint8), 0.3)
    with pytest.raises(NotFittedError):
        bs.BitBirch().radius_neighbors_graph(np.zeros((2, 256), np.uint8), 0.3)
    with pytest.raises(ValueError):
        BitBirch().centroid_radius_neighbors(0.3)


def test_no_cpu_path(fitted):
    r"""A call that passes the checks reaches the library: without a device it raises, it does not compute on the host."""
    from bblean_amd import _lib
    from bblean_amd.similarity import jt_radius_packed

    est, qry = fitted
    calls = [lambda: jt_radius_packed(qry, qry, 0.3), lambda: jt_radius_packed(qry, qry, 0.3, exclude=np.arange(len(qry))),
             lambda: est.radius_neighbors(qry, 0.3), lambda: est.radius_neighbors(None),
             lambda: est.radius_neighbors_graph(qry), lambda: est.centroid_radius_neighbors(0.3)]
    for call in calls:
        if _gpu():
            call()
        else:
            with pytest.raises(_lib.BBHipError):
                call()

r"""CPU: the Python face of top-k (`similarity.jt_topk_packed`, `sklearn.BitBirch.kneighbors`,
`BitBirch.centroid_neighbors`): signatures, and the argument errors, which are raised before the library is called.  The
fitted models come from the CPU oracle engine.  Without a GPU a call that passes the checks raises `BBHipError` (there is
no CPU path); the answers are checked on the GPU by tests/test_hip_topk.py."""
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

    assert "jt_topk_packed" in similarity.__all__ and "bbh_jt_topk" in _lib.EXPORTED_SYMBOLS and _lib.BBH_TOPK_MAX == 64
    p = inspect.signature(similarity.jt_topk_packed).parameters
    assert list(p) == ["queries", "rows", "k", "exclude", "return_counts"]
    assert p["exclude"].default is None and p["return_counts"].default is False
    for cls, packed in ((bs.BitBirch, True), (bs.UnpackedBitBirch, False)):
        p = inspect.signature(cls.kneighbors).parameters
        assert list(p) == ["self", "X", "n_neighbors", "return_distance", "input_is_packed", "n_features"]
        assert (p["X"].default, p["n_neighbors"].default, p["return_distance"].default) == (None, 5, True)
        assert p["input_is_packed"].default is packed and p["n_features"].default is None
    p = inspect.signature(BitBirch.centroid_neighbors).parameters
    assert list(p) == ["self", "n_neighbors", "sort"] and p["sort"].default is True
    assert issubclass(bs.UnpackedBitBirch, bs.BitBirch)


@pytest.mark.parametrize("k,nc,exclude,names", [(0, 8, False, "BBH_TOPK_MAX"), (65, 100, False, "BBH_TOPK_MAX"),
                                                (9, 8, False, "nc"), (8, 8, True, "nc"), (-3, 8, True, "BBH_TOPK_MAX")])
def test_jt_topk_packed_refuses_k(no_library, k, nc, exclude, names):
    from bblean_amd.similarity import jt_topk_packed

    q, c = np.zeros((5, 16), np.uint8), np.zeros((nc, 16), np.uint8)
    with pytest.raises(ValueError, match=names):
        jt_topk_packed(q, c, k, exclude=np.arange(5) if exclude else None)


def test_jt_topk_packed_refuses_operands(no_library):
    from bblean_amd.similarity import jt_topk_packed

    q, c = np.zeros((5, 16), np.uint8), np.zeros((8, 32), np.uint8)
    with pytest.raises(RuntimeError, match="same packed width"):
        jt_topk_packed(q, c, 2)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        jt_topk_packed(q[0], c, 2)
    with pytest.raises(RuntimeError):
        jt_topk_packed(q, np.zeros((0, 16), np.uint8), 1)
    with pytest.raises(TypeError):
        jt_topk_packed(q, q, 2.0)
    with pytest.raises(ValueError, match="exclude"):
        jt_topk_packed(q, q, 2, exclude=np.arange(4))
    with pytest.raises(ValueError, match="exclude"):
        jt_topk_packed(q, q, 2, exclude=np.zeros(5))


def test_estimator_refuses_before_the_library(no_library, fitted):
    est, qry = fitted
    K = CASES["C"]["K"]
    assert K > 65
    for k in (0, 65):
        with pytest.raises(ValueError, match="BBH_TOPK_MAX"):
            est.kneighbors(qry, k)
        with pytest.raises(ValueError, match="BBH_TOPK_MAX"):
            est.kneighbors(None, k)
        with pytest.raises(ValueError, match="BBH_TOPK_MAX"):
            est.centroid_neighbors(k)
    with pytest.raises(ValueError, match="packed bytes"):
        est.kneighbors(qry[:, :-1], 3)


def test_more_neighbours_than_centroids(no_library):
    import bblean_amd.sklearn as bs
    from bblean_amd import BitBirch, make_fake_fingerprints

    fps = make_fake_fingerprints(40, seed=3)
    tree = BitBirch(branching_factor=50, threshold=0.9, merge_criterion="diameter", _engine_factory=OracleEngine).fit(fps)
    K = len(tree.get_centroids())
    assert 2 <= K < 64
    with pytest.raises(ValueError, match="nc"):
        tree.centroid_neighbors(K)
    est = bs.BitBirch(threshold=0.9)
    est._engine_factory = OracleEngine
    est.fit(fps)
    K = len(est.subcluster_centers_)
    with pytest.raises(ValueError, match="nc"):
        est.kneighbors(fps, K + 1)
    with pytest.raises(ValueError, match="nc"):
        est.kneighbors(None, K)


def test_unfitted():
    import bblean_amd.sklearn as bs
    from bblean_amd import BitBirch
    from sklearn.exceptions import NotFittedError

    with pytest.raises(NotFittedError):
        bs.BitBirch().kneighbors(np.zeros((2, 256), np.uint8), 1)
    with pytest.raises(ValueError):
        BitBirch().centroid_neighbors(1)


def test_no_cpu_path(fitted):
    r"""A call that passes the checks reaches the library: without a device it raises, it does not compute on the host."""
    from bblean_amd import _lib
    from bblean_amd.similarity import jt_topk_packed

    est, qry = fitted
    calls = [lambda: jt_topk_packed(qry, qry, 3), lambda: jt_topk_packed(qry, qry, 3, exclude=np.arange(len(qry))),
             lambda: est.kneighbors(qry, 3), lambda: est.kneighbors(None, 3), lambda: est.centroid_neighbors(3)]
    for call in calls:
        if _gpu():
            assert call()[0].shape[1] == 3
        else:
            with pytest.raises(_lib.BBHipError):
                call()

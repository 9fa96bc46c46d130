r"""CPU: the scikit-learn face (bblean_amd/sklearn.py) - estimator contract, the fixture's self-consistency, and `fit`
on the four fixture cases with the CPU oracle engine injected (predict / transform need the GPU:
tests/test_hip_sklearn.py)."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from oracle_engine import OracleEngine
from sklearn_cases import CASES, N_DIST_ROWS, rows

GOLD = Path(__file__).resolve().parent / "golden" / "sklearn.npz"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _case_rows(name):
    from bblean_amd import make_fake_fingerprints

    return rows(CASES[name], make_fake_fingerprints)


def test_import_and_params_round_trip():
    from sklearn.base import clone

    import bblean_amd.sklearn as bs

    est = bs.BitBirch(threshold=0.4, branching_factor=30, merge_criterion="radius", compute_labels=False)
    params = est.get_params()
    assert set(params) == {"threshold", "branching_factor", "merge_criterion", "tolerance", "compute_labels"}
    assert params["threshold"] == 0.4 and params["branching_factor"] == 30
    assert params["merge_criterion"] == "radius" and params["compute_labels"] is False
    est.set_params(threshold=0.5, branching_factor=40)
    assert est.threshold == 0.5 and est.branching_factor == 40
    twin = clone(est)
    assert type(twin) is bs.BitBirch and twin.get_params() == est.get_params()
    un = clone(bs.UnpackedBitBirch(threshold=0.3))
    assert type(un) is bs.UnpackedBitBirch and un.get_params()["threshold"] == 0.3
    # the class layout of the reference: mixins first, the estimator base, then the tree
    names = [c.__name__ for c in bs.BitBirch.__bases__]
    assert names == ["ClassNamePrefixFeaturesOutMixin", "ClusterMixin", "TransformerMixin", "BaseEstimator", "BitBirch"]
    assert bs.BitBirch._parameter_constraints == {}
    assert bs.BitBirch().__sklearn_tags__().input_tags.sparse is True


def test_package_imports_without_sklearn_module():
    import subprocess
    import sys

    code = "import sys, bblean_amd; assert 'sklearn' not in sys.modules and 'bblean_amd.sklearn' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(GOLD.parents[2]))


def test_unfitted_estimator_raises_not_fitted():
    from sklearn.exceptions import NotFittedError

    import bblean_amd.sklearn as bs

    x = np.zeros((3, 256), np.uint8)
    with pytest.raises(NotFittedError):
        bs.BitBirch().predict(x)
    with pytest.raises(NotFittedError):
        bs.UnpackedBitBirch().transform(np.zeros((3, 2048), np.uint8))


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_is_self_consistent(gold, name):
    r"""The stored labels are the first argmin of the stored distances, and the stored distances are (u - i) / u
    recomputed from the stored centroids in exact integers: the fixture cannot drift from the formula the kernels
    implement."""
    case = CASES[name]
    _, qry = _case_rows(name)
    if not case["packed"]:
        qry = np.packbits(qry, axis=1)
    cents = gold[f"{name}_centroids"]
    assert cents.shape == (case["K"], case["nbits"] // 8) and cents.dtype == np.uint8
    keep = gold[f"{name}_dist_rows"]
    dist = gold[f"{name}_dist"]
    assert dist.dtype == np.float64 and dist.shape == (keep.size, case["K"])
    assert (keep[:N_DIST_ROWS] == np.arange(N_DIST_ROWS)).all()
    qb = np.unpackbits(qry, axis=1).astype(np.int64)
    cb = np.unpackbits(cents, axis=1).astype(np.int64)
    inter = qb @ cb.T
    union = qb.sum(1)[:, None] + cb.sum(1)[None, :] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(union == 0, 0.0, (union - inter).astype(np.float64) / union.astype(np.float64))
    assert (want[keep].view(np.uint64) == dist.view(np.uint64)).all()
    labels = gold[f"{name}_labels"]
    assert labels.dtype == np.int64 and labels.shape == (qry.shape[0],)
    assert (labels == np.argmin(want, axis=1) + 1).all()
    assert (labels[keep] == np.argmin(dist, axis=1) + 1).all()
    zero_q = np.flatnonzero(qb.sum(1) == 0)
    assert zero_q.size >= 1 and np.isin(zero_q, keep).all()
    tied = int(((want == want.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert tied == int(gold[f"{name}_tied"][0])
    if name == "B":
        assert tied >= 25
        zero_c = np.flatnonzero(cb.sum(1) == 0)
        assert zero_c.size >= 1 and (labels[zero_q] - 1 == zero_c[0]).all() and zero_c[0] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_fit_matches_reference_with_oracle_engine(gold, name):
    import bblean_amd.sklearn as bs

    case = CASES[name]
    fit_x, _ = _case_rows(name)
    cls = bs.BitBirch if case["packed"] else bs.UnpackedBitBirch
    est = cls(threshold=case["thr"], branching_factor=case["bf"])
    est._engine_factory = OracleEngine  # read lazily when the engine is created; not a constructor parameter
    assert "_engine_factory" not in est.get_params()
    out = est.fit(fit_x)
    assert out is est
    cents = gold[f"{name}_centroids"]
    assert est.subcluster_centers_.dtype == np.uint8
    assert est.subcluster_centers_.shape == (case["K"], case["nbits"])
    assert (est.subcluster_centers_ == np.unpackbits(cents, axis=1)).all()
    assert (est.subcluster_labels_ == np.arange(1, case["K"] + 1)).all()
    assert est._n_features_out == case["K"]
    assert est.labels_.dtype == np.uint64 and (est.labels_ == gold[f"{name}_fit_labels"]).all()
    prefix = cls.__name__.lower()
    assert list(est.get_feature_names_out()[:2]) == [prefix + "0", prefix + "1"]
    assert not hasattr(est, "n_features_in_")  # as in the reference: fit never sets it, predict checks no width
    assert (np.asarray(est._packed_centers) == cents).all()


def test_fit_predict_and_compute_labels_false():
    import bblean_amd.sklearn as bs

    fit_x, _ = _case_rows("C")
    est = bs.BitBirch(threshold=0.4, compute_labels=False)
    est._engine_factory = OracleEngine
    est.fit(fit_x)
    assert not hasattr(est, "labels_")
    est2 = bs.BitBirch(threshold=0.4, compute_labels=False)
    est2._engine_factory = OracleEngine
    labels = est2.fit_predict(fit_x)
    assert labels.shape == (fit_x.shape[0],) and labels.min() == 1 and labels.max() == CASES["C"]["K"]
    with pytest.raises(ValueError):
        est2.partial_fit(None)

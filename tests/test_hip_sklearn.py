r"""GPU: the scikit-learn face end to end on the device engine, against what the reference produced
(tests/golden/sklearn.npz): fitted attributes, predict, transform (float64 bit patterns), fit_predict, partial_fit."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from sklearn_cases import CASES, rows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "sklearn.npz"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _fitted(name):
    import bblean_amd.sklearn as bs
    from bblean_amd import make_fake_fingerprints

    case = CASES[name]
    fit_x, qry = rows(case, make_fake_fingerprints)
    cls = bs.BitBirch if case["packed"] else bs.UnpackedBitBirch
    return cls(threshold=case["thr"], branching_factor=case["bf"]).fit(fit_x), fit_x, qry, cls


@pytest.mark.parametrize("name", list(CASES))
def test_case_end_to_end(gold, name):
    import torch

    case = CASES[name]
    est, fit_x, qry, cls = _fitted(name)
    cents = gold[f"{name}_centroids"]
    assert est.subcluster_centers_.dtype == np.uint8
    assert (est.subcluster_centers_ == np.unpackbits(cents, axis=1)).all()
    assert (est.subcluster_labels_ == np.arange(1, case["K"] + 1)).all() and est._n_features_out == case["K"]
    assert est.labels_.dtype == np.uint64 and (est.labels_ == gold[f"{name}_fit_labels"]).all()
    assert est._packed_centers.is_cuda and (est._packed_centers.cpu().numpy() == cents).all()

    labels = est.predict(qry)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64
    assert (labels == gold[f"{name}_labels"]).all()

    keep = gold[f"{name}_dist_rows"]
    dist = est.transform(qry)
    assert isinstance(dist, np.ndarray) and dist.dtype == np.float64 and dist.shape == (qry.shape[0], case["K"])
    assert (dist[keep].view(np.uint64) == gold[f"{name}_dist"].view(np.uint64)).all()
    assert (np.argmin(dist, axis=1) + 1 == labels).all()

    # a device tensor of packed rows is used in place and answered on the device
    packed = qry if case["packed"] else np.packbits(qry, axis=1)
    tq = torch.from_numpy(packed).cuda()
    tl = est.predict(tq, input_is_packed=True)
    assert tl.is_cuda and tl.dtype == torch.int64 and (tl.cpu().numpy() == labels).all()
    td = est.transform(tq, input_is_packed=True)
    assert td.is_cuda and (td.cpu().numpy().view(np.uint64) == dist.view(np.uint64)).all()
    with pytest.raises(ValueError):
        est.predict(tq[:, :-1].contiguous(), input_is_packed=True)

    # fit_predict, and partial_fit on a fresh estimator, give the same model
    twin = cls(threshold=case["thr"], branching_factor=case["bf"], compute_labels=False)
    assert (twin.fit_predict(fit_x) == gold[f"{name}_fit_labels"]).all()
    assert (twin.predict(qry) == labels).all()
    part = cls(threshold=case["thr"], branching_factor=case["bf"]).partial_fit(fit_x)
    assert (part.labels_ == gold[f"{name}_fit_labels"]).all() and (part.predict(qry) == labels).all()
    assert (est.fit_transform(fit_x[:50]).shape[0]) == 50


def test_unpacked_estimator_takes_both_forms(gold):
    est, _, qry, _ = _fitted("D")
    packed = np.packbits(qry, axis=1)
    assert (est.predict(packed, input_is_packed=True) == gold["D_labels"]).all()
    assert (est.predict(qry.astype(np.int64)) == gold["D_labels"]).all()  # validate_data keeps the dtype; cast to uint8

r"""The Python surface of tree routing - BitBirch.route, sklearn's predict_tree - over an oracle-backed engine whose route_packed is
the NumPy reference (route_refs.RefEngine): no GPU.  What the engine returns is checked elsewhere (test_route_refs.py,
test_hip_route.py); here, what Python makes of it: the mapping of leaf ids to cluster positions in both orders, the `novel`
label, packing and validation, the refusals."""
from __future__ import annotations

import numpy as np
import pytest

import route_refs as R
from bblean_amd import BitBirch
from oracle_engine import OracleEngine

C, OPS, Q = R.CASES["depth"]()
ROWS = OPS[0][1]
KW = dict(branching_factor=C["bf"], threshold=C["thr"], merge_criterion="diameter")


@pytest.fixture(scope="module")
def model():
    return BitBirch(**KW, _engine_factory=R.RefEngine).fit(ROWS)


@pytest.mark.parametrize("sort", [True, False])
def test_cluster_is_a_position_in_the_sorted_or_chain_order(model, sort):
    want = R.expected("depth")
    cluster, accept, sim = model.route(Q, sort=sort)
    assert cluster.dtype == np.int64 and accept.dtype == bool and sim.dtype == np.float64
    assert cluster.shape == accept.shape == sim.shape == (Q.shape[0],)
    assert (accept == want["accept"].astype(bool)).all()
    assert (sim == want["inter"] / np.maximum(want["union"], 1)).all()
    # the position names the BitFeature the engine named: same centroid, same members
    ids = model._leaves()["ids"][model._leaf_order(sort)]
    assert (ids[cluster] == want["leaf"]).all()
    cents = np.array(model.get_centroids(sort=sort))
    inter = np.unpackbits(cents[cluster] & Q, axis=1).sum(axis=1)
    union = np.unpackbits(cents[cluster] | Q, axis=1).sum(axis=1)
    assert (inter == want["inter"]).all() and (union == want["union"]).all()
    # a row of the tree that is accepted goes to the cluster that holds it ... when the tree routes it there
    members = model.get_cluster_mol_ids(sort=sort)
    held = [e for e in range(120, 150) if (e - 120) * 20 in members[cluster[e]]]
    assert len(held) >= 10, len(held)


def test_sorted_and_chain_order_name_the_same_clusters(model):
    a, b = model.route(Q, sort=True)[0], model.route(Q, sort=False)[0]
    order = model._leaf_order(True)
    assert (order[a] == b).all() and (a != b).any()


def test_unpacked_lists_and_n_features(model):
    base = model.route(Q)
    bits = np.unpackbits(Q, axis=1)
    for got in (model.route(bits, input_is_packed=False), model.route(list(Q)), model.route(Q, n_features=256),
                model.route(bits, input_is_packed=False, n_features=256)):
        assert all((u == v).all() for u, v in zip(got, base))


def test_the_model_is_not_changed(model):
    before = (model.get_cluster_mol_ids(), np.array(model.get_centroids()), model.num_fitted_fps, [int(v) for v in model._engine.stats()])
    model.route(Q)
    after = (model.get_cluster_mol_ids(), np.array(model.get_centroids()), model.num_fitted_fps, [int(v) for v in model._engine.stats()])
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]


def test_the_current_merge_criterion_decides(model):
    r"""set_merge after the fit: route answers with the criterion a fit would use now."""
    m = BitBirch(**KW, _engine_factory=R.RefEngine).fit(ROWS)
    base = m.route(Q)[1]
    m.set_merge("diameter", threshold=0.9)
    strict = m.route(Q)[1]
    assert strict.sum() < base.sum() and (m.route(Q)[0] == model.route(Q)[0]).all()


def test_refusals(model):
    with pytest.raises(ValueError, match="n_features=256"):
        model.route(Q[:, :16])  # 128 bits against a tree of 256
    with pytest.raises(ValueError, match="n_features=256"):
        model.route(np.unpackbits(Q, axis=1)[:, :200], input_is_packed=False)
    with pytest.raises(ValueError, match="at least 1 fingerprint"):
        model.route(Q[:0])
    with pytest.raises(ValueError, match="larger than the padded length"):
        model.route(Q, n_features=512)
    with pytest.raises(ValueError, match="not been fitted"):
        BitBirch(**KW, _engine_factory=R.RefEngine).route(Q)
    plain = BitBirch(**KW, _engine_factory=OracleEngine).fit(ROWS)
    with pytest.raises(NotImplementedError, match="route_packed"):
        plain.route(Q)
    released = BitBirch(**KW, _engine_factory=R.RefEngine).fit(ROWS)
    released.delete_internal_nodes()
    with pytest.raises(ValueError, match="Internal nodes were released"):
        released.route(Q)


def test_sklearn_predict_tree():
    pytest.importorskip("sklearn.base")
    from sklearn.exceptions import NotFittedError

    from bblean_amd.sklearn import BitBirch as SkBitBirch, UnpackedBitBirch

    est = SkBitBirch(threshold=C["thr"], branching_factor=C["bf"], merge_criterion="diameter")
    est._engine_factory = R.RefEngine
    with pytest.raises(NotFittedError):
        est.predict_tree(Q)
    est.fit(ROWS)
    ref = BitBirch(**KW, _engine_factory=R.RefEngine).fit(ROWS)
    cluster, accept, _ = ref.route(Q, sort=True)
    labels = est.predict_tree(Q)
    assert (labels == est.subcluster_labels_[cluster]).all() and labels.min() >= 1 and labels.max() <= len(est.subcluster_labels_)
    assert accept.any() and (~accept).any()
    for novel in (-1, 0):
        lab, acc = est.predict_tree(Q, novel=novel, return_accept=True)
        assert (acc == accept).all() and (lab == np.where(accept, cluster + 1, novel)).all()
    assert (est.predict_tree(Q, novel=None) == labels).all()
    # predict's numbering: label k is row k - 1 of subcluster_centers_
    cents = np.array(ref.get_centroids(sort=True, packed=False))
    assert (est.subcluster_centers_[labels - 1] == cents[cluster]).all()
    bits = np.unpackbits(Q, axis=1)
    assert (est.predict_tree(bits, input_is_packed=False) == labels).all()
    un = UnpackedBitBirch(threshold=C["thr"], branching_factor=C["bf"], merge_criterion="diameter")
    un._engine_factory = R.RefEngine
    un.fit(np.unpackbits(ROWS, axis=1))
    assert (un.predict_tree(bits) == labels).all() and (un.predict_tree(bits, novel=-1) == np.where(accept, labels, -1)).all()
    with pytest.raises(ValueError, match="n_features=256"):
        est.predict_tree(Q[:, :16])
    # (save / load and pickle need an engine that writes tree images: test_hip_route.py)

r"""`bblean.sklearn` on the MI355X engine: `BitBirch` / `UnpackedBitBirch` that respect the scikit-learn estimator
contract (reference bblean/sklearn.py), with the caveat the reference has: no global clustering.

Same constructor, mixin order, method signatures, fitted attributes and return dtypes as the reference classes.
`fit` is the device tree of `bblean_amd.bitbirch.BitBirch`; `predict` and `transform` - which the reference
computes on the CPU with `sklearn.metrics.pairwise_distances_argmin` / `pairwise_distances` on unpacked boolean
arrays (sklearn.py:136, :153) - run as HIP kernels on the PACKED centroids, which stay in HBM after `fit`
(`bblean_amd.similarity.jt_assign_packed`, `jt_dist_matrix_packed`).  The results are identical, ties and all-zero
rows included.  There is no NumPy fallback.

scikit-learn is imported by this module only; `import bblean_amd` works without it.
"""
from __future__ import annotations

import typing as tp

import numpy as np
from numpy.typing import NDArray
from sklearn.base import (
    BaseEstimator,
    ClassNamePrefixFeaturesOutMixin,
    ClusterMixin,
    TransformerMixin,
    _fit_context,
)
from sklearn.exceptions import NotFittedError
from sklearn.utils.validation import check_is_fitted, validate_data

from bblean_amd._merges import MergeCriterion
from bblean_amd.bitbirch import BitBirch as _BitBirch
from bblean_amd.fingerprints import pack_fingerprints, unpack_fingerprints
from bblean_amd.similarity import (
    _radius_check,
    _topk_check_k,
    jt_assign_packed,
    jt_dist_matrix_packed,
    jt_radius_packed,
    jt_topk_packed,
)

__all__ = ["BitBirch", "UnpackedBitBirch"]


def _is_dev(x: object) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


class BitBirch(
    ClassNamePrefixFeaturesOutMixin,
    ClusterMixin,
    TransformerMixin,
    BaseEstimator,
    _BitBirch,
):
    r"""BitBIRCH clustering as a scikit-learn estimator.

    Inputs are *packed* fingerprints by default; `UnpackedBitBirch` always takes unpacked ones.
    See `bblean_amd.bitbirch.BitBirch` for the algorithm's parameters."""

    _parameter_constraints: dict[str, list[tp.Any]] = {}
    _PICKLE_SKIP = frozenset({"_packed_centers"})  # a device tensor: rebuilt from the loaded tree (_after_load)

    def __init__(
        self,
        *,
        threshold: float = 0.65,
        branching_factor: int = 50,
        merge_criterion: str | MergeCriterion | None = None,
        tolerance: float | None = None,
        compute_labels: bool = True,
    ):
        super().__init__(
            threshold=threshold,
            branching_factor=branching_factor,
            merge_criterion=merge_criterion,
            tolerance=tolerance,
        )
        self.compute_labels = compute_labels

    @_fit_context(prefer_skip_nested_validation=True)
    def fit(  # type: ignore[override]
        self, X, y=None, input_is_packed: bool = True, n_features: int | None = None
    ) -> "BitBirch":
        _BitBirch.fit(self, X, input_is_packed=input_is_packed, n_features=n_features)
        order = self._leaf_order(True)  # largest cluster first, stable: get_centroids(sort=True)
        packed = self._leaves()["cents"][order]
        self.subcluster_centers_ = unpack_fingerprints(packed, self._n_features)
        self.subcluster_labels_ = np.arange(1, len(packed) + 1)
        self._n_features_out = len(packed)
        # the operand of predict / transform: packed, and in HBM when the engine keeps its tree there
        gather = getattr(self._engine, "gather_centroids", None)
        self._packed_centers = gather(order, device_out=True) if gather is not None else np.ascontiguousarray(packed)
        if self.compute_labels:
            self.labels_ = self.get_assignments()
        return self

    def _after_load(self) -> None:
        if hasattr(self, "subcluster_centers_"):  # fitted: the operand of predict / transform, as `fit` builds it
            order = self._leaf_order(True)
            gather = getattr(self._engine, "gather_centroids", None)
            if gather is not None:
                self._packed_centers = gather(order, device_out=True)
            else:
                self._packed_centers = np.ascontiguousarray(self._leaves()["cents"][order])

    @_fit_context(prefer_skip_nested_validation=True)
    def partial_fit(  # type: ignore[no-untyped-def]
        self, X=None, y=None, input_is_packed: bool = True, n_features: int | None = None
    ) -> "BitBirch":
        if X is None:
            raise ValueError()
        self.fit(X, input_is_packed=input_is_packed, n_features=n_features)
        if self.compute_labels:
            self.labels_ = self.get_assignments()
        return self

    # Overloaded since self.labels_ may not be set
    def fit_predict(  # type: ignore[override]
        self, X, y=None, input_is_packed: bool = True, n_features: int | None = None
    ) -> NDArray[np.integer]:
        self.fit(X, input_is_packed=input_is_packed, n_features=n_features)
        if not self.compute_labels:
            self.labels_ = self.get_assignments()
        return self.labels_

    def _packed_queries(self, X, input_is_packed: bool, n_features: int | None):  # type: ignore[no-untyped-def]
        r"""Packed uint8 rows of the width the centroids have.  A device tensor is used in place (validate_data would
        copy it to the host), so it is checked by hand; host input goes through validate_data as in the reference."""
        nbytes = int(self._packed_centers.shape[1])
        if _is_dev(X):
            if not input_is_packed:
                raise ValueError("device-resident input must be packed uint8")
            if X.dim() != 2 or str(X.dtype) != "torch.uint8":
                raise ValueError("device-resident input must be a 2-dimensional torch.uint8 tensor of packed rows")
            if X.stride(1) != 1:
                X = X.contiguous()
        else:
            X = validate_data(self, X, accept_sparse="csr", reset=False)
            if hasattr(X, "toarray"):
                X = X.toarray()
            X = X.astype(np.uint8, copy=False)
            if not input_is_packed:
                X = pack_fingerprints(X)
            elif n_features is not None and X.shape[1] * 8 != n_features:
                X = pack_fingerprints(unpack_fingerprints(X, n_features))
        if int(X.shape[1]) != nbytes:
            raise ValueError(f"X has {int(X.shape[1])} packed bytes per row, the fitted centroids have {nbytes}")
        return X

    def predict(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = True, n_features: int | None = None
    ):
        """Label (1..K) of the closest subcluster centroid of every row; a device tensor gives a device tensor."""
        check_is_fitted(self)
        dev = _is_dev(X)
        idx = jt_assign_packed(self._packed_queries(X, input_is_packed, n_features), self._packed_centers)
        if dev:
            return idx.long() + 1
        if _is_dev(idx):
            idx = idx.cpu().numpy()
        return self.subcluster_labels_[idx]

    def predict_tree(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = True, n_features: int | None = None, novel=None, return_accept: bool = False
    ):
        """Label (1..K, `predict`'s numbering) of the subcluster the TREE routes every row to: the one a further `fit` would
        try to merge the row into (`bblean_amd.bitbirch.BitBirch.route`), found in about depth x branching_factor compares
        per row instead of `predict`'s K.  It need not be the closest centroid.  Rows the merge criterion would not accept
        there - a `fit` would open a new subcluster for them - get the label `novel` where it is not None;
        ``return_accept=True`` returns ``(labels, accept)``.  The model is not changed.  A device tensor gives device
        tensors.  It needs the tree only, so it also works on what `load` returns."""
        if not getattr(self, "_is_init", False):
            raise NotFittedError(f"This {type(self).__name__} instance is not fitted yet. Call 'fit' before using this estimator.")
        dev = _is_dev(X)
        if dev:
            if X.dim() != 2 or str(X.dtype) != "torch.uint8":
                raise ValueError("device-resident input must be a 2-dimensional torch.uint8 tensor of packed rows")
        elif hasattr(X, "toarray"):
            X = X.toarray()
        # (the tree is all it needs: a model that `load` returned has no fitted sklearn attributes, and routes all the same)
        cluster, accept, _ = self.route(X, input_is_packed=input_is_packed, n_features=n_features, sort=True)
        labels = cluster + 1  # subcluster_labels_: 1..K in the order of get_centroids(sort=True)
        if novel is not None:
            labels = np.where(accept, labels, novel)
        if dev:
            import torch

            labels, accept = torch.from_numpy(np.ascontiguousarray(labels)).to(X.device), torch.from_numpy(accept).to(X.device)
        return (labels, accept) if return_accept else labels

    def transform(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = True, n_features: int | None = None
    ):
        """Jaccard distance of every row to every subcluster centroid, float64 (n, K)."""
        check_is_fitted(self)
        return jt_dist_matrix_packed(self._packed_queries(X, input_is_packed, n_features), self._packed_centers)

    def kneighbors(  # type: ignore[no-untyped-def]
        self, X=None, n_neighbors: int = 5, return_distance: bool = True, input_is_packed: bool = True,
        n_features: int | None = None
    ):
        """The `n_neighbors` nearest subcluster centroids of every row, nearest first (scikit-learn's
        `KNeighborsMixin.kneighbors`): ``(dist, ind)``, or ``ind`` alone.  ``ind`` holds zero-based positions in
        `subcluster_centers_` (the label is ``subcluster_labels_[ind]``), ``dist`` the Jaccard distances `transform` gives
        there; ties go to the lower position, as in `predict`.  ``X=None``: the fitted centroids themselves, each without
        itself (`centroid_neighbors`).  A device tensor gives device tensors."""
        check_is_fitted(self)
        n_centers = int(self._packed_centers.shape[0])
        if X is None:
            _topk_check_k(n_neighbors, n_centers, True)
            ind, dist = self.centroid_neighbors(n_neighbors, sort=True)
            return (dist, ind) if return_distance else ind
        k = _topk_check_k(n_neighbors, n_centers, False)
        dev = _is_dev(X)
        ind, dist = jt_topk_packed(self._packed_queries(X, input_is_packed, n_features), self._packed_centers, k)
        ind = ind.long() if dev else ind.astype(np.int64)
        return (dist, ind) if return_distance else ind

    def _radius_csr(self, X, radius, sort: bool, input_is_packed: bool, n_features: int | None):  # type: ignore[no-untyped-def]
        r"""The CSR triple of `jt_radius_packed` for `X` (None: the fitted centroids, each without itself) against the
        fitted centroids; ``radius=None`` is the merge threshold as a distance, ``1.0 - threshold``."""
        check_is_fitted(self)
        radius = _radius_check(1.0 - self.threshold if radius is None else radius)
        cents = self._packed_centers
        if X is None:
            return jt_radius_packed(cents, cents, radius, exclude=np.arange(int(cents.shape[0]), dtype=np.int32), sort=sort)
        return jt_radius_packed(self._packed_queries(X, input_is_packed, n_features), cents, radius, sort=sort)

    def radius_neighbors(  # type: ignore[no-untyped-def]
        self, X=None, radius: float | None = None, return_distance: bool = True, sort_results: bool = False,
        input_is_packed: bool = True, n_features: int | None = None
    ):
        """Every subcluster centroid within Jaccard distance `radius` of every row (scikit-learn's
        `RadiusNeighborsMixin.radius_neighbors`): ``(dist, ind)``, or ``ind`` alone, each an object array with one array
        per row.  ``ind`` holds int64 zero-based positions in `subcluster_centers_`, ascending (``sort_results=True``:
        by distance, then position; it needs ``return_distance=True``, as in scikit-learn); ``dist`` the distances
        `transform` gives there, and a centroid at `radius` exactly is in.  ``radius=None``: ``1.0 - threshold``, the
        merge threshold.  ``X=None``: the fitted centroids themselves, each without itself.

        A device tensor does not get object arrays: it gives the CSR triple ``(offsets int64 (n + 1,), ind int64, dist)``
        as device tensors (``(offsets, ind)`` without distances), row ``p``'s part being ``offsets[p]:offsets[p + 1]``."""
        if sort_results and not return_distance:
            raise ValueError("return_distance must be True if sort_results is True")
        dev = _is_dev(X)
        off, ind, dist = self._radius_csr(X, radius, sort_results, input_is_packed, n_features)
        if dev:
            return (off, ind.long(), dist) if return_distance else (off, ind.long())
        if _is_dev(ind):
            off, ind, dist = off.cpu().numpy(), ind.cpu().numpy(), dist.cpu().numpy()
        ind = ind.astype(np.int64)
        inds, dists = np.empty(len(off) - 1, dtype=object), np.empty(len(off) - 1, dtype=object)
        for p in range(len(off) - 1):
            inds[p], dists[p] = ind[off[p]:off[p + 1]], dist[off[p]:off[p + 1]]
        return (dists, inds) if return_distance else inds

    def radius_neighbors_graph(  # type: ignore[no-untyped-def]
        self, X=None, radius: float | None = None, mode: str = "connectivity", input_is_packed: bool = True,
        n_features: int | None = None
    ):
        """`radius_neighbors` as a `scipy.sparse.csr_matrix` of shape ``(n_queries, n_centroids)`` (scikit-learn's
        `radius_neighbors_graph`): ones where a centroid is within `radius` (``mode="connectivity"``), or the distances
        there (``mode="distance"``; a centroid at distance 0 is a stored zero).  Always on the host."""
        from scipy.sparse import csr_matrix

        if mode not in ("connectivity", "distance"):
            raise ValueError(f'mode must be "connectivity" or "distance", got {mode!r}')
        off, ind, dist = self._radius_csr(X, radius, False, input_is_packed, n_features)
        if _is_dev(ind):
            off, ind, dist = off.cpu().numpy(), ind.cpu().numpy(), dist.cpu().numpy()
        data = dist if mode == "distance" else np.ones(len(ind), dtype=np.float64)
        return csr_matrix((data, ind.astype(np.int64), off), shape=(len(off) - 1, int(self._packed_centers.shape[0])))

    def __sklearn_tags__(self):  # type: ignore[no-untyped-def]
        tags = super().__sklearn_tags__()
        tags.input_tags.sparse = True
        return tags


class UnpackedBitBirch(BitBirch):
    r"""The same estimator; inputs are *unpacked* fingerprints always."""

    def fit(  # type: ignore[no-untyped-def, override]
        self, X, y=None, input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().fit(X, y, input_is_packed=input_is_packed, n_features=n_features)

    def partial_fit(  # type: ignore[no-untyped-def]
        self, X, y=None, input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().partial_fit(X, y, input_is_packed=input_is_packed, n_features=n_features)

    def fit_predict(  # type: ignore[no-untyped-def, override]
        self, X, y=None, input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().fit_predict(X, y, input_is_packed=input_is_packed, n_features=n_features)

    def predict(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().predict(X, input_is_packed=input_is_packed, n_features=n_features)

    def predict_tree(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = False, n_features: int | None = None, novel=None, return_accept: bool = False
    ):
        return super().predict_tree(X, input_is_packed=input_is_packed, n_features=n_features, novel=novel,
                                    return_accept=return_accept)

    def transform(  # type: ignore[no-untyped-def]
        self, X, input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().transform(X, input_is_packed=input_is_packed, n_features=n_features)

    def kneighbors(  # type: ignore[no-untyped-def]
        self, X=None, n_neighbors: int = 5, return_distance: bool = True, input_is_packed: bool = False,
        n_features: int | None = None
    ):
        return super().kneighbors(X, n_neighbors, return_distance, input_is_packed=input_is_packed, n_features=n_features)

    def radius_neighbors(  # type: ignore[no-untyped-def]
        self, X=None, radius: float | None = None, return_distance: bool = True, sort_results: bool = False,
        input_is_packed: bool = False, n_features: int | None = None
    ):
        return super().radius_neighbors(X, radius, return_distance, sort_results, input_is_packed=input_is_packed,
                                        n_features=n_features)

    def radius_neighbors_graph(  # type: ignore[no-untyped-def]
        self, X=None, radius: float | None = None, mode: str = "connectivity", input_is_packed: bool = False,
        n_features: int | None = None
    ):
        return super().radius_neighbors_graph(X, radius, mode, input_is_packed=input_is_packed, n_features=n_features)

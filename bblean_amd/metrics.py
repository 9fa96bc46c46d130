r"""Clustering quality indices on Tanimoto similarity, evaluated with the HIP kernels.

Public names and argument meaning follow the reference's ``bblean/metrics.py`` (``jt_isim_chi``
`:47`, ``jt_dbi`` `:108`, ``jt_isim_dunn`` `:163`) so callers can switch imports.  The evaluation is
organised around one prepared view of the clustering (`_Clustering`) instead of per-cluster NumPy
loops: every cluster is resident as packed rows once, column sums are taken once per cluster by
`bbh_add_rows` (exact u64), similarities to a central fingerprint are one arr-vec launch per
cluster, and the k x k centroid similarities of the Davies-Bouldin index come from a single
batched all-pairs launch.  The float64 reductions that follow use the reference's operation order,
so the results are bit-identical (tests/test_hip_metrics.py, reference-generated goldens).
"""
from __future__ import annotations

import typing as tp

import numpy as np
from numpy.typing import NDArray

from bblean_amd import _lib
from bblean_amd import similarity as _sim
from bblean_amd.fingerprints import pack_fingerprints

__all__ = ["jt_isim_chi", "jt_isim_dunn", "jt_dbi"]

_Fps = NDArray[np.uint8]


class _Clustering:
    r"""A clustering as a list of fingerprint arrays plus everything the indices derive from it."""

    def __init__(self, clusters: tp.Sequence[_Fps], packed: bool, n_features: int | None) -> None:
        self.given = list(clusters)
        self.given_packed = packed
        self.n_features = n_features
        self.sizes = [len(c) for c in self.given]
        self.total = sum(self.sizes)
        self._packed: list[_Fps] | None = None
        self._sums: list[NDArray[np.uint64]] | None = None

    def __len__(self) -> int:
        return len(self.given)

    @property
    def packed(self) -> list[_Fps]:
        if self._packed is None:
            self._packed = self.given if self.given_packed else [pack_fingerprints(c) for c in self.given]
        return self._packed

    @property
    def column_sums(self) -> list[NDArray[np.uint64]]:
        if self._sums is None:
            self._sums = [_sim._sum_rows_u64(c, self.given_packed, self.n_features) for c in self.given]
        return self._sums

    def isims(self) -> list[float]:
        f = _sim.jt_isim_packed if self.given_packed else _sim.jt_isim_unpacked
        return [f(c) for c in self.given]

    def centrals(self, spec: tp.Sequence[_Fps] | str) -> list[_Fps]:
        r"""Packed central fingerprint of every cluster: ``"centroid"`` / ``"medoid"`` or given ones
        (given ones are in the representation of the clusters, like the reference expects)."""
        if not isinstance(spec, str):
            return list(spec) if self.given_packed else [pack_fingerprints(c) for c in spec]
        if spec == "centroid":
            return [_sim.centroid(c, input_is_packed=self.given_packed, n_features=self.n_features, pack=True)
                    for c in self.given]
        if spec == "medoid":
            rows = self.given
            if (self.given_packed and rows and all(isinstance(c, np.ndarray) and c.ndim == 2 and c.dtype == np.uint8
                                                    and len(c) and c.shape[1] == rows[0].shape[1] for c in rows)):
                nb = rows[0].shape[1]
                nf = nb * 8 if self.n_features is None else int(self.n_features)
                if 0 < nf <= nb * 8 and nf % 8 == 0 and _sim._seg_fits(nf, max(self.sizes)):
                    # one segmented call over the concatenated clusters instead of a call per row
                    offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
                    pos = _sim.jt_compl_isim_segments(np.concatenate(rows), offsets, n_features=nf, return_compl=False)[0]
                    return [c[int(i)][: nf // 8] for c, i in zip(rows, pos)]
            return [_sim.jt_isim_medoid(c, input_is_packed=self.given_packed, n_features=self.n_features, pack=True)[1]
                    for c in self.given]
        raise ValueError(f"Unknown arg {spec} use 'medoids|centroids'")

    def distances_to(self, centrals: tp.Sequence[_Fps]) -> list[NDArray[np.float64]]:
        r"""1 - Tanimoto of every member to its cluster's central: one launch per cluster."""
        return [1 - _sim.jt_sim_packed(rows, c) for rows, c in zip(self.packed, centrals)]


def _only_centroid(what: tp.Any, index: str) -> None:
    if isinstance(what, str) and what != "centroid":
        raise NotImplementedError(f"Currently only 'centroid' implemented for {index}")


def jt_isim_chi(
    cluster_fps: list[_Fps],
    all_fps_central: _Fps | str = "centroid",
    centrals: list[_Fps] | str = "centroid",
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
) -> float:
    r"""Calinski-Harabasz index on the Tanimoto iSIM; higher is better."""
    _only_centroid(all_fps_central, "CHI")
    _only_centroid(centrals, "CHI")
    cl = _Clustering(cluster_fps, input_is_packed, n_features)
    if isinstance(all_fps_central, str):  # majority vote over ALL fingerprints, from the per-cluster sums
        all_fps_central = _sim.centroid_from_sum(sum(cl.column_sums), cl.total)
    cents = cl.centrals(centrals)
    k = len(cl)
    if k <= 1:
        return 0
    spread = 1 - _sim.jt_sim_packed(np.stack(cents), all_fps_central)  # every central vs the global one: one launch
    between = 0.0
    within = 0.0
    for size, s, d in zip(cl.sizes, spread, cl.distances_to(cents)):
        between += size * s.item() ** 2
        within += np.dot(d, d)
    return between * (cl.total - k) / (within * (k - 1))


def jt_dbi(
    cluster_fps: list[_Fps],
    centrals: list[_Fps] | str = "centroid",
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
) -> float:
    r"""Davies-Bouldin index on the Tanimoto distance; lower is better."""
    cl = _Clustering(cluster_fps, input_is_packed, n_features)
    cents = cl.centrals(centrals)
    scatter = [np.sum(d) / size for d, size in zip(cl.distances_to(cents), cl.sizes)]
    if cl.total == 0:
        return 0
    # k x k central-to-central similarities in ONE batched launch (k^2 small calls in the reference)
    table = np.stack(cents)
    sims = _sim.jt_best_match_packed(table, table, return_sims=True)[3]
    assert sims is not None
    worst_sum = 0.0
    for i in range(len(cents)):
        worst = 0.0
        for j in range(len(cents)):
            if j != i:
                worst = max(worst, (scatter[i] + scatter[j]) / (1 - sims[i, j].item()))
        worst_sum += worst
    return worst_sum / cl.total


def jt_isim_dunn(
    cluster_fps: list[_Fps],
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
) -> float:
    r"""Dunn index variant of the BitBIRCH article; higher is better."""
    cl = _Clustering(cluster_fps, input_is_packed, n_features)
    diameters = cl.isims()
    widest = max(diameters)
    if widest == 0:
        return 1
    # the reference's quadratic pair loop (metrics.py:186-199: iSIM of the two clusters' combined column sums) as ONE call:
    # a wave per pair, one exact uint64 dot product each (until round 5: a launch and a 16 KB copy per pair)
    import ctypes as C

    lib = _lib.load()
    sums = np.ascontiguousarray(np.stack(cl.column_sums).astype(np.uint64, copy=False))
    sizes = np.ascontiguousarray(np.asarray(cl.sizes, dtype=np.uint64))
    out = C.c_double(1.0)
    _lib.check(lib.bbh_isim_pair_min_gap(sums.ctypes.data, sizes.ctypes.data, int(sums.shape[0]), int(sums.shape[1]), C.byref(out), None))
    return min(out.value, 1.00) / widest

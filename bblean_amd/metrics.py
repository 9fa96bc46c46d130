r"""Clustering quality indices on Tanimoto similarity, evaluated with the HIP kernels.

Public names and argument meaning follow the reference's ``bblean/metrics.py`` (``jt_isim_chi``
`:47`, ``jt_dbi`` `:108`, ``jt_isim_dunn`` `:163`) so callers can switch imports.  A clustering is
either the reference's list of arrays or a `ClusterSets` (one array of packed rows plus which rows
form which cluster; `BitBirch.cluster_sets` builds it from a fitted tree).  `ClusterSets`, and a list
of equally wide uint8 arrays, are evaluated by the segmented kernels: one
`bbh_cluster_stats_segments` call gives every cluster's centroid, iSIM, member-to-central distances
and column sums, and `bbh_dbi_worst_ratios` evaluates the pair loop of the Davies-Bouldin index
without a k x k matrix - a fixed number of launches whatever the number of clusters.  Anything else
keeps one prepared view per cluster (`_Clustering`): column sums by `bbh_add_rows`, one arr-vec
launch per cluster, the k x k centroid similarities in one batched launch.  On both paths the
float64 reductions that follow use the reference's operation order on the host, so the two paths
agree exactly and the results are the reference's (tests/test_hip_metrics.py,
tests/test_hip_metrics_segments.py, reference-generated goldens).
"""
from __future__ import annotations

import typing as tp

import numpy as np
from numpy.typing import NDArray

from bblean_amd import _lib
from bblean_amd import similarity as _sim
from bblean_amd.fingerprints import pack_fingerprints

__all__ = ["jt_isim_chi", "jt_isim_dunn", "jt_dbi", "ClusterSets"]

_Fps = NDArray[np.uint8]


class ClusterSets:
    r"""A clustering as ONE array of packed rows plus which rows form which cluster: cluster ``g`` is
    ``fps[offsets[g]:offsets[g + 1]]``, or ``fps[members[offsets[g]:offsets[g + 1]]]`` when ``members`` is given (the
    form of `similarity.jt_compl_isim_segments`).  ``fps`` is a 2-dimensional uint8 NumPy array or device tensor; offsets
    and members are kept as int64 NumPy arrays.  `jt_isim_chi`, `jt_dbi` and `jt_isim_dunn` take it in place of a list of
    arrays and then cost a fixed number of launches, whatever the number of clusters (`BitBirch.cluster_sets` builds it
    from a fitted tree)."""

    def __init__(self, fps: tp.Any, offsets: tp.Any, members: tp.Any = None, n_features: int | None = None) -> None:
        if _sim._is_dev(fps):
            if fps.dim() != 2 or str(fps.dtype) != "torch.uint8" or fps.stride(1) != 1:
                raise ValueError("fps must be a 2-dimensional uint8 array of packed rows")
        else:
            fps = np.asarray(fps)
            if fps.ndim != 2 or fps.dtype != np.uint8:
                raise ValueError("fps must be a 2-dimensional uint8 array of packed rows")
        n_rows, nb = int(fps.shape[0]), int(fps.shape[1])
        nf = nb * 8 if n_features is None else int(n_features)
        if nf <= 0 or nf % 8 != 0 or nf > nb * 8:
            raise ValueError("Only n_features divisible by 8 (and within the packed width) is supported")
        off = _sim._seg_host_index(offsets.cpu().numpy() if _sim._is_dev(offsets) else offsets, "offsets")
        if len(off) < 2:
            raise ValueError("offsets must name at least one set")
        if off[0] != 0:
            raise ValueError("offsets must start at 0")
        sizes = np.diff(off)
        if (sizes < 0).any():
            raise ValueError("offsets must not decrease")
        if (sizes == 0).any():
            raise ValueError("Size of fingerprints set must be > 0")
        mem = None
        if members is not None:
            mem = _sim._seg_host_index(members.cpu().numpy() if _sim._is_dev(members) else members, "members")
            if len(mem) and (int(mem.min()) < 0 or int(mem.max()) >= n_rows):
                raise ValueError("members must be row numbers of fps")
        if int(off[-1]) > (n_rows if mem is None else len(mem)):
            raise ValueError("offsets name more rows than there are")
        self.fps = fps
        self.offsets = off
        self.members = mem
        self.n_features = nf

    def __len__(self) -> int:
        return len(self.offsets) - 1

    @property
    def sizes(self) -> NDArray[np.int64]:
        return np.diff(self.offsets)

    def to_list(self) -> list[_Fps]:
        r"""The clusters as a list of host arrays (one per cluster: the form the reference takes)."""
        fps = self.fps.cpu().numpy() if _sim._is_dev(self.fps) else self.fps
        fps = fps[:, : self.n_features // 8]
        o = self.offsets.tolist()
        if self.members is None:
            return [fps[b:e] for b, e in zip(o[:-1], o[1:])]
        return [fps[self.members[b:e]] for b, e in zip(o[:-1], o[1:])]


def _host(x: tp.Any) -> NDArray[tp.Any]:
    return x.cpu().numpy() if _sim._is_dev(x) else x


def _as_sets(clusters: tp.Any, packed: bool, n_features: int | None) -> ClusterSets | None:
    r"""A list of clusters as `ClusterSets` where the segmented kernels take it: 2-dimensional uint8 arrays of one width
    (unpacked ones are packed once, as a whole), no empty cluster, every cluster small enough for exact moments."""
    rows = clusters
    if not rows or not all(isinstance(c, np.ndarray) and c.ndim == 2 and c.dtype == np.uint8 and len(c)
                           and c.shape[1] == rows[0].shape[1] for c in rows):
        return None
    width = rows[0].shape[1]
    if packed:
        nf = width * 8 if n_features is None else int(n_features)
        if not (0 < nf <= width * 8 and nf % 8 == 0):
            return None
    else:
        nf = width
        if nf == 0 or nf % 8 != 0:
            return None
    sizes = [len(c) for c in rows]
    if not _sim._seg_fits(nf, max(sizes)):
        return None
    flat = np.concatenate(rows)
    if not packed:
        flat = pack_fingerprints(flat)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return ClusterSets(flat, offsets, n_features=nf)


class _Clustering:
    r"""A clustering plus everything the indices derive from it.  Given as `ClusterSets`, or as a list that `_as_sets`
    accepts, it is evaluated by the segmented kernels (`self.sets`): a fixed number of calls for all clusters.  Anything
    else - ragged widths, wider dtypes, sets too large for exact moments, or ``segmented=False`` - keeps the calls per
    cluster."""

    def __init__(self, clusters: tp.Any, packed: bool, n_features: int | None, segmented: bool | None = None) -> None:
        self.sets: ClusterSets | None = None
        if isinstance(clusters, ClusterSets):
            if segmented is False:
                packed, n_features = True, clusters.n_features
                clusters = clusters.to_list()
            elif not _sim._seg_fits(clusters.n_features, int(clusters.sizes.max())):
                raise ValueError("a set is too large for exact 64-bit moments: n_features * m * m must stay below 2**63")
            else:
                self.sets = clusters
        else:
            clusters = list(clusters)
            if segmented is not False:
                self.sets = _as_sets(clusters, packed, n_features)
        self.given_packed = packed
        self.n_features = n_features
        if self.sets is not None:
            self.given: list[_Fps] = []
            self.sizes = self.sets.sizes.tolist()
        else:
            self.given = clusters
            self.sizes = [len(c) for c in self.given]
        self.total = sum(self.sizes)
        self._packed: list[_Fps] | None = None
        self._sums: list[NDArray[np.uint64]] | None = None

    def __len__(self) -> int:
        return len(self.sizes)

    # ------------------------------------------------------------------ segmented evaluation
    def stats(self, want: tuple[str, ...], centrals: tp.Any = None) -> dict[str, tp.Any]:
        r"""`similarity.jt_cluster_stats_segments` of the clusters; everything comes back on the host but the centroids,
        which stay where the rows are."""
        assert self.sets is not None
        st = self.sets
        out = _sim.jt_cluster_stats_segments(st.fps, st.offsets, st.members, st.n_features, centrals, want)
        return {w: (v if w == "centroids" else _host(v)) for w, v in out.items()}

    def all_central(self) -> tp.Any:
        r"""Majority vote over ALL fingerprints: the same call, with one set spanning everything."""
        assert self.sets is not None
        st = self.sets
        whole = np.array([0, self.total], dtype=np.int64)
        out = _sim.jt_cluster_stats_segments(st.fps, whole, st.members, st.n_features, None, ("centroids",))
        return out["centroids"][0]

    def given_centrals(self, spec: tp.Any) -> tp.Any:
        r"""Centrals handed in by the caller (in the representation of the clusters) as one packed table."""
        table = np.stack([np.asarray(c) for c in spec])
        return table if self.given_packed else pack_fingerprints(table)

    def medoids(self) -> tp.Any:
        assert self.sets is not None
        st = self.sets
        pos = _sim.jt_compl_isim_segments(st.fps, st.offsets, st.members, st.n_features, return_compl=False)[0]
        first = st.offsets[:-1]
        dev = _sim._is_dev(st.fps)
        if dev:
            import torch

            first = torch.from_numpy(first).to(st.fps.device)
        at = first + pos
        if st.members is not None:
            at = (torch.from_numpy(st.members).to(st.fps.device) if dev else st.members)[at]
        return st.fps[at][:, : st.n_features // 8]

    def slices(self, flat: NDArray[np.float64]) -> tp.Iterator[NDArray[np.float64]]:
        assert self.sets is not None
        o = self.sets.offsets.tolist()
        return (flat[b:e] for b, e in zip(o[:-1], o[1:]))

    def warn_small(self) -> None:
        r"""The RuntimeWarning `jt_isim_packed` raises for a set of fewer than 2 rows, once."""
        small = [n for n in self.sizes if n < 2]
        if small:
            import warnings

            warnings.warn(f"Invalid n_objects = {small[0]} in isim. Expected n_objects >= 2", RuntimeWarning, stacklevel=3)

    # ------------------------------------------------------------------ evaluation per cluster
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


def _warn_zero_division(flags: NDArray[np.uint32]) -> None:
    r"""The RuntimeWarnings NumPy raises in the reference's ``(S[i] + S[j]) / Mij`` for a zero ``Mij``."""
    import warnings

    if flags[0]:
        warnings.warn("divide by zero encountered in scalar divide", RuntimeWarning, stacklevel=3)
    if flags[1]:
        warnings.warn("invalid value encountered in scalar divide", RuntimeWarning, stacklevel=3)


def _dbi_worst_ratios(centrals: tp.Any, scatter: NDArray[np.float64]) -> tuple[NDArray[np.float64], NDArray[np.uint32]]:
    r"""`bbh_dbi_worst_ratios`: for every central the largest ``(S[i] + S[j]) / (1 - sim(i, j))`` over the others, and the
    counts of the pairs that divided by zero."""
    lib = _lib.load()
    if _sim._is_dev(centrals):
        import torch

        table, k, nb, stride = centrals, int(centrals.shape[0]), int(centrals.shape[1]), int(centrals.stride(0))
        st = torch.cuda.current_stream(centrals.device).cuda_stream
    else:
        table = np.ascontiguousarray(centrals, dtype=np.uint8)
        (k, nb), stride, st = table.shape, table.shape[1], None
    sc = np.ascontiguousarray(scatter, dtype=np.float64)
    worst = np.empty(k, dtype=np.float64)
    flags = np.zeros(2, dtype=np.uint32)
    _lib.check(lib.bbh_dbi_worst_ratios(_lib.ptr(table), k, nb, stride, sc.ctypes.data, worst.ctypes.data, flags.ctypes.data, st))
    return worst, flags


def jt_isim_chi(
    cluster_fps: list[_Fps] | ClusterSets,
    all_fps_central: _Fps | str = "centroid",
    centrals: list[_Fps] | str = "centroid",
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
    *,
    _segmented: bool | None = None,
) -> float:
    r"""Calinski-Harabasz index on the Tanimoto iSIM; higher is better."""
    _only_centroid(all_fps_central, "CHI")
    _only_centroid(centrals, "CHI")
    cl = _Clustering(cluster_fps, input_is_packed, n_features, _segmented)
    k = len(cl)
    if cl.sets is not None:
        if isinstance(all_fps_central, str):
            all_fps_central = cl.all_central()
        if isinstance(centrals, str):
            got = cl.stats(("centroids", "dist"))
            cents, dist = got["centroids"], got["dist"]
        else:
            cents = cl.given_centrals(centrals)
            dist = cl.stats(("dist",), cents)["dist"]
        if k <= 1:
            return 0
        if _sim._is_dev(cents) != _sim._is_dev(all_fps_central):
            cents, all_fps_central = _host(cents), _host(all_fps_central)
        spread = _host(1 - _sim.jt_sim_packed(cents, all_fps_central))  # every central vs the global one: one launch
        between = 0.0
        within = 0.0
        # the float64 reductions in the reference's order, over slices of the one distance array
        for size, s, d in zip(cl.sizes, spread, cl.slices(dist)):
            between += size * s.item() ** 2
            within += np.dot(d, d)
        return between * (cl.total - k) / (within * (k - 1))
    if isinstance(all_fps_central, str):  # majority vote over ALL fingerprints, from the per-cluster sums
        all_fps_central = _sim.centroid_from_sum(sum(cl.column_sums), cl.total)
    cents = cl.centrals(centrals)
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
    cluster_fps: list[_Fps] | ClusterSets,
    centrals: list[_Fps] | str = "centroid",
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
    *,
    _segmented: bool | None = None,
) -> float:
    r"""Davies-Bouldin index on the Tanimoto distance; lower is better."""
    cl = _Clustering(cluster_fps, input_is_packed, n_features, _segmented)
    if cl.sets is not None:
        if isinstance(centrals, str) and centrals == "centroid":
            got = cl.stats(("centroids", "dist"))
            table, dist = got["centroids"], got["dist"]
        else:
            if not isinstance(centrals, str):
                table = cl.given_centrals(centrals)
            elif centrals == "medoid":
                table = cl.medoids()
            else:
                raise ValueError(f"Unknown arg {centrals} use 'medoids|centroids'")
            dist = cl.stats(("dist",), table)["dist"]
        scatter = np.array([np.sum(d) / size for d, size in zip(cl.slices(dist), cl.sizes)], dtype=np.float64)
        # for every central its worst ratio against the others, without the k x k similarities; summed in index order
        worst, flags = _dbi_worst_ratios(table, scatter)
        _warn_zero_division(flags)
        worst_sum = 0.0
        for w in worst.tolist():
            worst_sum += w
        return worst_sum / cl.total
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
    cluster_fps: list[_Fps] | ClusterSets,
    input_is_packed: bool = True,
    n_features: int | None = None,
    verbose: bool = False,
    *,
    _segmented: bool | None = None,
) -> float:
    r"""Dunn index variant of the BitBIRCH article; higher is better."""
    cl = _Clustering(cluster_fps, input_is_packed, n_features, _segmented)
    if cl.sets is not None:
        got = cl.stats(("isim", "sums"))
        cl.warn_small()
        diameters = got["isim"].tolist()
        all_sums = got["sums"].view(np.uint64)
    else:
        diameters = cl.isims()
        all_sums = None
    widest = max(diameters)
    if widest == 0:
        return 1
    # the reference's quadratic pair loop (metrics.py:186-199: iSIM of the two clusters' combined column sums) as ONE call:
    # a wave per pair, one exact uint64 dot product each (until round 5: a launch and a 16 KB copy per pair)
    import ctypes as C

    lib = _lib.load()
    if all_sums is None:
        all_sums = np.stack(cl.column_sums).astype(np.uint64, copy=False)
    sums = np.ascontiguousarray(all_sums)
    sizes = np.ascontiguousarray(np.asarray(cl.sizes, dtype=np.uint64))
    out = C.c_double(1.0)
    _lib.check(lib.bbh_isim_pair_min_gap(sums.ctypes.data, sizes.ctypes.data, int(sums.shape[0]), int(sums.shape[1]), C.byref(out), None))
    return min(out.value, 1.00) / widest

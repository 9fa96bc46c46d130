r"""`BitBirch` with the reference's class surface, backed by the HBM-resident tree engine.

Drop-in for `bblean.bitbirch.BitBirch` (reference bitbirch.py:539-1473) on the hot path:
the per-fingerprint Python loop of `fit` / `_fit_buffers` (bitbirch.py:769-787,
:848-866) and everything it calls is ONE C-ABI call into libbbhip.so per batch; this
file only keeps what the reference keeps on the host *around* that loop:

  * molecule-index bookkeeping.  The reference stores a Python list on every
    `_BFSubcluster` and extends it on each merge (bitbirch.py:505, :524).  The engine
    instead returns, per inserted element, the id of the leaf BitFeature it ended in;
    member lists are rebuilt lazily as "elements grouped by leaf id, in insertion order",
    which is the same concatenation order (SURVEY.md section 8a rule 13).
  * result ordering: leaves in leaf-chain order, stably sorted by size (bitbirch.py:
    1216-1222), labels 1..K (bitbirch.py:1041-1042).
  * refine / recluster orchestration: dtype groups in first-seen order, exploded
    singletons appended to the uint8 group (bitbirch.py:1187-1308).
"""
from __future__ import annotations

import io
import json
import os
import pickle
import random
import struct
import tempfile
import typing as tp
import warnings
from pathlib import Path
from weakref import WeakSet

import numpy as np
from numpy.typing import NDArray

from bblean_amd._merges import BUILTIN_MERGES, MergeCriterion, get_merge_accept_fn
from bblean_amd.fingerprints import pack_fingerprints, unpack_fingerprints
from bblean_amd.utils import min_safe_uint

__all__ = ["BitBirch", "set_merge", "fit_concurrently"]

_Input = tp.Union[NDArray[np.integer], list]

_BITBIRCH_INSTANCES: "WeakSet[BitBirch]" = WeakSet()

# tree files (BitBirch.save / load, INTEGRATION.md "Tree files")
_TREE_FILE_MAGIC = b"BBAMDTREE\x00"
_TREE_FILE_FORMAT = "bblean_amd.tree"
_TREE_FILE_VERSION = 1


class _BadTreeFile(Exception):
    r"""What `BitBirch.load` turns into a ValueError that names the path."""

_global_merge_accept: MergeCriterion | None = None


def set_merge(merge_criterion: str, tolerance: float = 0.05) -> None:
    r"""Legacy global merge setter (reference bitbirch.py:104-129).  Discouraged."""
    warnings.warn(
        "Use of the global `set_merge` function is highly discouraged,\n"
        " instead use either: "
        " bb_tree = BitBirch(...)\n"
        " bb_tree.set_merge(merge_criterion=..., tolerance=...)\n"
        " or directly: `bb_tree = BitBirch(..., merge_criterion=..., tolerance=...)`.",
        UserWarning,
    )
    global _global_merge_accept
    _global_merge_accept = get_merge_accept_fn(merge_criterion, tolerance)
    for tree in _BITBIRCH_INSTANCES:
        tree._merge_accept_fn = _global_merge_accept
        tree._push_merge_to_engine()


def _validate_n_features(X: _Input, input_is_packed: bool, n_features: int | None = None) -> int:
    r"""Same checks and messages as the reference (bitbirch.py:133-159)."""
    if len(X) == 0:
        raise ValueError("Input must have at least 1 fingerprint")
    width = len(X[0]) if isinstance(X, list) else X.shape[1]
    if input_is_packed:
        padded = width * 8
        if n_features is None:
            return padded
        if padded < n_features:
            raise ValueError("n_features is larger than the padded length, which is inconsistent")
        return n_features
    if n_features is not None and n_features != width:
        raise ValueError(
            "n_features is redundant for non-packed inputs"
            " if passed, it must be equal to X.shape[1] (or len(X[0]))."
            f" For passed X the inferred n_features was {width}."
            " If this value is not what you expected,"
            " make sure the passed X is actually unpacked."
        )
    return width


def _dtype_name_for(n_samples: int) -> str:
    r"""dtype group of a leaf BitFeature: always min_safe_uint(n_samples)
    (bitbirch.py:480, :493; SURVEY.md section 8a rule 11)."""
    return min_safe_uint(int(n_samples)).name


class _IndexLists:
    r"""CSR holder for per-element molecule-index lists (avoids millions of Python
    lists on the way into `_fit_buffers`)."""

    __slots__ = ("counts", "flat")

    def __init__(self, counts: NDArray[np.int64], flat: NDArray[np.int64]) -> None:
        self.counts = counts
        self.flat = flat

    @classmethod
    def from_sequences(cls, seqs: tp.Iterable[tp.Sequence[int]], k: int) -> "_IndexLists":
        counts = np.empty(k, dtype=np.int64)
        chunks: list[NDArray[np.int64]] = []
        i = 0
        for i, s in zip(range(k), seqs):
            counts[i] = len(s)
            chunks.append(np.asarray(s, dtype=np.int64).reshape(-1))
        got = len(chunks)
        counts = counts[:got]
        flat = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int64)
        return cls(counts, flat)

    def __len__(self) -> int:
        return int(self.counts.size)

    def to_lists(self) -> list[list[int]]:
        offs = np.concatenate(([0], np.cumsum(self.counts))).tolist()  # (Python ints: indexing an array per cluster costs more)
        flat = self.flat.tolist()
        return [flat[a:b] for a, b in zip(offs[:-1], offs[1:])]


class _LeafBF:
    r"""Read-only view of one leaf BitFeature (what `_get_leaf_bfs` hands to
    `bblean.sklearn`, reference sklearn.py:90 / bitbirch.py:360-526)."""

    __slots__ = ("n_samples", "packed_centroid", "mol_indices", "n_features", "_tree", "_pos")

    def __init__(self, tree: "BitBirch", pos: int, n: int, cent: NDArray[np.uint8], mols: list[int]):
        self._tree = tree
        self._pos = pos
        self.n_samples = n
        self.packed_centroid = cent
        self.mol_indices = mols
        self.n_features = tree._n_features

    @property
    def dtype_name(self) -> str:
        return _dtype_name_for(self.n_samples)

    @property
    def unpacked_centroid(self) -> NDArray[np.uint8]:
        return unpack_fingerprints(self.packed_centroid, self.n_features)

    @property
    def _buffer(self) -> NDArray[np.integer]:
        width = min_safe_uint(self.n_samples).itemsize
        return self._tree._engine.gather_buffers(np.array([self._pos], dtype=np.int64), width)[0]

    @property
    def linear_sum(self) -> NDArray[np.integer]:
        return self._buffer[:-1]


class BitBirch:
    r"""BitBIRCH clustering on one MI355X; same constructor and methods as the reference
    class (bitbirch.py:596-643).  `_engine_factory` is a test hook (tests inject the CPU
    oracle to check this host logic without a GPU); the product default is the HIP
    engine and there is no CPU fallback."""

    def __init__(
        self,
        *,
        threshold: float = 0.65,
        branching_factor: int = 50,
        merge_criterion: str | MergeCriterion | None = None,
        tolerance: float | None = None,
        device: int = 0,
        _engine_factory: tp.Callable[..., tp.Any] | None = None,
    ):
        self.threshold = threshold
        self.branching_factor = branching_factor
        if _global_merge_accept is not None:
            if tolerance is not None:
                raise ValueError(
                    "tolerance can only be passed if "
                    "the *global* set_merge function has *not* been used"
                )
            if merge_criterion is not None:
                raise ValueError(
                    "merge_criterion can only be passed if "
                    "the *global* set_merge function has *not* been used"
                )
            self._merge_accept_fn = _global_merge_accept
        elif isinstance(merge_criterion, MergeCriterion):
            if tolerance is not None:
                raise ValueError("'tolerance' arg is disregarded for custom merge functions")
            self._merge_accept_fn = merge_criterion
        else:
            name = "diameter" if merge_criterion is None else merge_criterion
            self._merge_accept_fn = get_merge_accept_fn(name, 0.05 if tolerance is None else tolerance)

        self._device = device
        self._engine_factory = _engine_factory
        self._engine: tp.Any = None
        self._n_features: int = 0
        self._num_fitted_fps = 0
        self._is_init = False
        self._internal_released = False
        # one entry per fit call since the last reset: (leaf ids, counts | None, flat ids)
        self._log_leaf: list[NDArray[np.uint32]] = []
        self._log_counts: list[NDArray[np.int64] | None] = []
        self._log_ids: list[NDArray[np.int64]] = []
        self._cache: dict[str, tp.Any] = {}
        self._global_clustering_centroid_labels: NDArray[np.int64] | None = None
        self._n_global_clusters = 0
        _BITBIRCH_INSTANCES.add(self)

    # ---------------------------------------------------------------- properties ----
    @property
    def merge_criterion(self) -> str:
        return self._merge_accept_fn.name

    @merge_criterion.setter
    def merge_criterion(self, value: str) -> None:
        self.set_merge(criterion=value)

    @property
    def tolerance(self) -> float | None:
        return self._merge_accept_fn.tolerance

    @tolerance.setter
    def tolerance(self, value: float) -> None:
        self.set_merge(tolerance=value)

    @property
    def is_init(self) -> bool:
        return self._is_init

    @property
    def num_fitted_fps(self) -> int:
        return self._num_fitted_fps

    @property
    def _only_has_leaves(self) -> bool:
        return self._internal_released

    # ------------------------------------------------------------- configuration ----
    def set_merge(
        self,
        criterion: str | MergeCriterion | None = None,
        *,
        tolerance: float | None = None,
        threshold: float | None = None,
        branching_factor: int | None = None,
    ) -> None:
        r"""Same semantics as the reference (bitbirch.py:674-703), including that an
        unspecified tolerance resets it to 0.05 on criteria that have one."""
        if _global_merge_accept is not None:
            raise ValueError(
                "BitBirch.set_merge() can only called if "
                "the global set_merge() function has *not* been used"
            )
        _tolerance = 0.05 if tolerance is None else tolerance
        if isinstance(criterion, MergeCriterion):
            self._merge_accept_fn = criterion
        elif isinstance(criterion, str):
            self._merge_accept_fn = get_merge_accept_fn(criterion, _tolerance)
        if self._merge_accept_fn.has_tolerance:
            self._merge_accept_fn.tolerance = _tolerance
        elif tolerance is not None:
            raise ValueError(f"Can't set tolerance for {self._merge_accept_fn}")
        if threshold is not None:
            self.threshold = threshold
        if branching_factor is not None:
            self.branching_factor = branching_factor
        self._push_merge_to_engine()

    def _push_merge_to_engine(self) -> None:
        if self._engine is None:
            return
        fn = self._merge_accept_fn
        self._engine.set_merge(
            fn.code,
            0.0 if fn.tolerance is None else fn.tolerance,
            fn.tolerance_table(),
            self.threshold,
            self.branching_factor,
        )

    def _ensure_engine(self, n_features: int) -> None:
        if self._engine is not None and n_features != self._n_features:
            if self._is_init:
                raise ValueError(
                    f"tree was built with n_features={self._n_features}, got {n_features}"
                )
            # a reset (or never fitted) tree is re-initialised for the new width, like the
            # reference's _initialize_tree (bitbirch.py:880-884)
            close = getattr(self._engine, "close", None)
            if close is not None:
                close()
            self._engine = None
        if self._engine is not None:
            self._push_merge_to_engine()
            return
        fn = self._merge_accept_fn
        factory = self._engine_factory
        if factory is None:
            from bblean_amd._engine import HipEngine as factory  # no fallback: raises if absent
        self._engine = factory(
            self.branching_factor,
            self.threshold,
            fn.code,
            0.0 if fn.tolerance is None else fn.tolerance,
            fn.tolerance_table(),
            n_features,
            self._device,
        )
        self._n_features = n_features

    # ------------------------------------------------------------------ fitting ----
    def fit(
        self,
        X: _Input | Path | str | tp.Any,
        /,
        reinsert_indices: tp.Iterable[int] | None = None,
        input_is_packed: bool = True,
        n_features: int | None = None,
        max_fps: int | None = None,
    ) -> "BitBirch":
        r"""Insert fingerprints in order (reference bitbirch.py:705-788).

        ``X``: packed/unpacked array, list of rows, ``.npy`` path, or a device-resident
        ``torch.uint8`` tensor of packed rows (used in place, no PCIe copy).
        """
        rows, ids = self._prepare_fit(X, reinsert_indices, input_is_packed, n_features, max_fps)
        if len(ids):
            self._commit_fit(self._engine.fit_packed(rows), ids)
        return self

    def _prepare_fit(self, X, reinsert_indices, input_is_packed, n_features, max_fps):  # type: ignore[no-untyped-def]
        r"""Everything `fit` does before the hot loop: load / validate / pack the input, create the
        engine, resolve the molecule indices.  Returns (packed rows, indices)."""
        is_dev = hasattr(X, "data_ptr") and getattr(X, "is_cuda", False)
        if isinstance(X, (Path, str)):
            X = np.load(Path(X), mmap_mode="r")
            if max_fps is not None:
                X = X[:max_fps]
        elif max_fps is not None:
            X = X[:max_fps]
        if is_dev:
            if not input_is_packed:
                raise ValueError("device-resident input must be packed uint8")
            if X.shape[0] == 0:
                raise ValueError("Input must have at least 1 fingerprint")
            nf = X.shape[1] * 8 if n_features is None else n_features
            if X.shape[1] * 8 < nf:
                raise ValueError("n_features is larger than the padded length, which is inconsistent")
            rows: tp.Any = X
            n_rows = int(X.shape[0])
        else:
            nf = _validate_n_features(X, input_is_packed, n_features)
            arr = np.stack(X) if isinstance(X, list) else np.asarray(X)
            if input_is_packed:
                rows = np.ascontiguousarray(arr, dtype=np.uint8)
                if rows.shape[1] * 8 != nf:
                    # trailing pad bits beyond n_features are dropped by the reference's
                    # unpack(count=n_features); only byte-aligned n_features reach here
                    rows = pack_fingerprints(unpack_fingerprints(rows, nf))
            else:
                rows = pack_fingerprints(arr.astype(np.uint8, copy=False))
            n_rows = rows.shape[0]
        if nf % 8 != 0:
            raise RuntimeError("Only n_features divisible by 8 is supported")
        if self._only_has_leaves:
            raise ValueError("Internal nodes were released, call reset() before fit()")
        self._ensure_engine(nf)
        if reinsert_indices is None:
            ids = np.arange(self._num_fitted_fps, self._num_fitted_fps + n_rows, dtype=np.int64)
        elif isinstance(reinsert_indices, range):
            ids = np.arange(reinsert_indices.start, reinsert_indices.stop, reinsert_indices.step, dtype=np.int64)
        else:
            ids = np.fromiter(reinsert_indices, dtype=np.int64)
        if ids.size < n_rows:  # zip() in the reference stops at the shorter iterable
            n_rows = ids.size
            rows = rows[:n_rows]
        ids = ids[:n_rows]
        self._is_init = True
        return rows, ids

    def _commit_fit(self, leaf: NDArray[np.uint32], ids: NDArray[np.int64]) -> None:
        self._log_leaf.append(leaf)
        self._log_counts.append(None)
        self._log_ids.append(ids)
        self._num_fitted_fps += int(ids.size)
        self._cache.clear()

    def fit_reinsert(self, X, reinsert_indices, input_is_packed=True, n_features=None, max_fps=None):  # type: ignore[no-untyped-def]
        r""":meta private: (reference bitbirch.py:868-878)"""
        return self.fit(X, reinsert_indices, input_is_packed, n_features, max_fps)

    def _fit_buffers(
        self,
        X: _Input | Path | str,
        reinsert_index_seqs: tp.Iterable[tp.Sequence[int]] | tp.Literal["omit"] | _IndexLists = "omit",
    ) -> "BitBirch":
        r"""Insert BitFeature buffers ``[linear_sum | n_samples]`` in order
        (reference bitbirch.py:790-866)."""
        prepared = self._prepare_fit_buffers(X, reinsert_index_seqs)
        if prepared is not None:
            bufs, counts, flat = prepared
            self._commit_fit_buffers(self._engine.fit_buffers(bufs), counts, flat)
        return self

    def _prepare_fit_buffers(self, X, reinsert_index_seqs):  # type: ignore[no-untyped-def]
        r"""Everything `_fit_buffers` does before the hot loop.  Returns (buffers, member counts, member
        ids) or None when there is nothing to insert."""
        if isinstance(X, (Path, str)):
            X = np.load(Path(X), mmap_mode="r")
        is_dev = hasattr(X, "raw") and hasattr(X, "n_samples")  # _engine.DevTable: a table resident in HBM
        if is_dev:
            if len(X) == 0:
                raise ValueError("Input must have at least 1 fingerprint")
            nf = X.shape[1] - 1
            bufs = X
        else:
            nf = _validate_n_features(X, input_is_packed=False) - 1
        if is_dev:
            pass
        elif isinstance(X, list):
            first = np.asarray(X[0])
            bufs = np.stack([np.asarray(b).astype(first.dtype, copy=False) for b in X])
        else:
            bufs = np.asarray(X)
        if self._only_has_leaves:
            raise ValueError("Internal nodes were released, call reset() before fit()")
        self._ensure_engine(nf)
        k = bufs.shape[0]
        if isinstance(reinsert_index_seqs, str) and reinsert_index_seqs == "omit":
            # the reference zips against a generator of `num_fitted_fps` empty tuples
            k = min(k, self._num_fitted_fps)
            idx = _IndexLists(np.zeros(k, dtype=np.int64), np.zeros(0, dtype=np.int64))
            check = False
        elif isinstance(reinsert_index_seqs, _IndexLists):
            idx = reinsert_index_seqs
            check = True
        else:
            idx = _IndexLists.from_sequences(reinsert_index_seqs, k)
            check = True
        k = min(k, len(idx))
        bufs = bufs.rows(0, k) if is_dev else bufs[:k]
        counts = idx.counts[:k]
        flat = idx.flat[: int(counts.sum())]
        if check and k:
            n_col = (bufs.n_samples() if is_dev else bufs[:, -1]).astype(np.int64)
            bad = np.nonzero(counts != n_col)[0]
            if bad.size:
                i = int(bad[0])
                where = f" (buffer {i} of {k}" + (f", device table: {bufs.n_head} rows + {bufs.n_tail} packed)" if is_dev else ")")
                raise ValueError(
                    "Expected len(mol_indices) == buffer[-1],"
                    f" but found {int(counts[i])} != {int(n_col[i])}" + where
                )
        self._is_init = True
        if not k:
            return None
        return bufs, counts, flat

    def _commit_fit_buffers(self, leaf: NDArray[np.uint32], counts: NDArray, flat: NDArray) -> None:
        self._log_leaf.append(leaf)
        self._log_counts.append(counts.astype(np.int64))
        self._log_ids.append(flat.astype(np.int64))
        self._num_fitted_fps += int(counts.sum())
        self._cache.clear()

    # ----------------------------------------------------------- tree lifecycle ----
    def reset(self) -> None:
        r"""Drop the whole tree, keep merge parameters (reference bitbirch.py:1078)."""
        if self._engine is not None:
            self._engine.reset()
        self._num_fitted_fps = 0
        self._is_init = False
        self._internal_released = False
        self._log_leaf.clear()
        self._log_counts.clear()
        self._log_ids.clear()
        self._cache.clear()

    def delete_internal_nodes(self) -> None:
        r"""After this, only leaves may be read until `reset()` (bitbirch.py:1092-1104).
        Nothing is freed on the device (the pools are reused by the next fit); the flag
        reproduces the reference's state machine: it only trips once the root has split."""
        if self._engine is not None and int(self._engine.stats()[5]) > 1:
            self._internal_released = True

    # ----------------------------------------------------------------- results ----
    def _require_init(self) -> None:
        if not self._is_init:
            raise ValueError("The model has not been fitted yet.")

    def _leaves(self) -> dict[str, tp.Any]:
        r"""Leaf table in chain order + member lists, cached until the next fit."""
        self._require_init()
        if "leaves" in self._cache:
            return self._cache["leaves"]
        ids, ns, cents, _ = self._engine.export_leaves(None)
        k = ids.size
        # elements grouped by the leaf they ended in, insertion order inside a group
        if self._log_leaf:
            elem_leaf = np.concatenate(self._log_leaf)
            elem_cnt = np.concatenate(
                [np.ones(l.size, dtype=np.int64) if c is None else c
                 for l, c in zip(self._log_leaf, self._log_counts)]
            )
            flat_ids = np.concatenate(self._log_ids)
        else:
            elem_leaf = np.zeros(0, dtype=np.uint32)
            elem_cnt = np.zeros(0, dtype=np.int64)
            flat_ids = np.zeros(0, dtype=np.int64)
        elem_off = np.cumsum(elem_cnt) - elem_cnt
        order = np.argsort(elem_leaf, kind="stable")
        s_leaf = elem_leaf[order]
        s_cnt = elem_cnt[order]
        s_off = elem_off[order]
        total = int(s_cnt.sum())
        if total:
            dst_start = np.cumsum(s_cnt) - s_cnt
            gather = np.repeat(s_off - dst_start, s_cnt) + np.arange(total, dtype=np.int64)
            members = flat_ids[gather]
        else:
            members = np.zeros(0, dtype=np.int64)
        # per leaf id: [begin, end) into `members`
        max_id = int(max(ids.max(initial=0), s_leaf.max(initial=0))) + 1
        size_by_id = np.bincount(s_leaf, weights=s_cnt, minlength=max_id).astype(np.int64)
        end_by_id = np.cumsum(size_by_id)
        beg_by_id = end_by_id - size_by_id
        out = {
            "ids": ids,
            "n": ns,
            "cents": cents,
            "beg": beg_by_id[ids] if k else np.zeros(0, dtype=np.int64),
            "end": end_by_id[ids] if k else np.zeros(0, dtype=np.int64),
            "members": members,
        }
        self._cache["leaves"] = out
        return out

    def _leaf_order(self, sort: bool) -> NDArray[np.int64]:
        lv = self._leaves()
        k = lv["ids"].size
        if not sort:
            return np.arange(k, dtype=np.int64)
        # stable sort by n_samples, largest first (list.sort(reverse=True) is stable)
        return np.argsort(-lv["n"].astype(np.int64), kind="stable")

    def _members_of(self, positions: NDArray[np.int64]) -> list[list[int]]:
        lv = self._leaves()
        mem = lv["members"].tolist()
        beg = lv["beg"][positions].tolist()
        end = lv["end"][positions].tolist()
        return [mem[b:e] for b, e in zip(beg, end)]

    def get_cluster_mol_ids(self, sort: bool = True, global_clusters: bool = False) -> list[list[int]]:
        r"""Molecule indices of each cluster (reference bitbirch.py:969-988)."""
        lists = self._members_of(self._leaf_order(sort))
        if global_clusters:
            if self._global_clustering_centroid_labels is None:
                raise ValueError("Must perform global clustering before fetching global labels")
            labels = self._global_clustering_centroid_labels - 1
            return self._new_ids_from_labels(lists, labels, self._n_global_clusters)
        return lists

    @staticmethod
    def _new_ids_from_labels(members, labels, n_labels=None):  # type: ignore[no-untyped-def]
        if n_labels is None:
            n_labels = len(np.unique(labels))
        out: list[list[int]] = [[] for _ in range(n_labels)]
        for i, idxs in enumerate(members):
            out[labels[i]].extend(idxs)
        return out

    def get_centroids(self, sort: bool = True, packed: bool = True) -> list[NDArray[np.uint8]]:
        lv = self._leaves()
        cents = lv["cents"][self._leaf_order(sort)]
        if not packed:
            cents = unpack_fingerprints(cents, self._n_features)
        return list(cents)

    def centroid_neighbors(self, n_neighbors: int, sort: bool = True) -> tuple[NDArray[np.int64], NDArray[np.float64]]:
        r"""The `n_neighbors` nearest other centroids of every centroid: ``(ind, dist)``, both ``(K, n_neighbors)``, nearest
        first.  Positions are those of `get_centroids(sort=sort)`; a centroid is never its own neighbour, an identical other
        centroid is (at distance 0).  Jaccard distance, ties to the lower position (`similarity.jt_topk_packed`): the
        neighbour graph of the clustering in ``K x n_neighbors`` memory, on the device."""
        from bblean_amd.similarity import _topk_check_k, jt_topk_packed

        order = self._leaf_order(sort)
        k = _topk_check_k(n_neighbors, len(order), True)
        gather = getattr(self._engine, "gather_centroids", None)
        cents = gather(order, device_out=True) if gather is not None else np.ascontiguousarray(self._leaves()["cents"][order])
        ind, dist = jt_topk_packed(cents, cents, k, exclude=np.arange(len(order), dtype=np.int32))
        if hasattr(ind, "cpu"):
            ind, dist = ind.cpu().numpy(), dist.cpu().numpy()
        return ind.astype(np.int64), dist

    def centroid_radius_neighbors(self, radius: float, sort: bool = True) -> tuple[NDArray[np.int64], NDArray[np.int64], NDArray[np.float64]]:
        r"""Every other centroid within Jaccard distance `radius` of every centroid, as CSR ``(offsets, ind, dist)``:
        centroid ``p``'s neighbours are ``ind[offsets[p]:offsets[p + 1]]``, in ascending position.  Positions are those of
        `get_centroids(sort=sort)`; a centroid is never its own neighbour, an identical other centroid is (at distance 0).
        The threshold twin of `centroid_neighbors` (`similarity.jt_radius_packed`): the graph of the clustering at a merge
        threshold, in memory proportional to its edges, on the device."""
        from bblean_amd.similarity import _radius_check, jt_radius_packed

        radius = _radius_check(radius)
        order = self._leaf_order(sort)
        gather = getattr(self._engine, "gather_centroids", None)
        cents = gather(order, device_out=True) if gather is not None else np.ascontiguousarray(self._leaves()["cents"][order])
        off, ind, dist = jt_radius_packed(cents, cents, radius, exclude=np.arange(len(order), dtype=np.int32))
        if hasattr(ind, "cpu"):
            off, ind, dist = off.cpu().numpy(), ind.cpu().numpy(), dist.cpu().numpy()
        return off, ind.astype(np.int64), dist

    def centroid_components(self, radius: float | None = None, sort: bool = True) -> tuple[NDArray[np.int64], int]:
        r"""The connected components of the centroids at Jaccard distance `radius` (default ``1 - threshold``):
        ``(labels int64 (K,), n_components)`` over the positions of `get_centroids(sort=sort)`.  Two centroids are linked
        iff `centroid_radius_neighbors(radius)` lists one for the other; components are the transitive closure, labelled by
        their first member in ascending position, as ``scipy.sparse.csgraph.connected_components`` of that graph - computed
        on the device without the graph (`similarity.jt_components_packed`).  The model is left as it is."""
        from bblean_amd import similarity

        radius = similarity._radius_check(1.0 - self.threshold if radius is None else radius)
        order = self._leaf_order(sort)
        gather = getattr(self._engine, "gather_centroids", None)
        cents = gather(order, device_out=True) if gather is not None else np.ascontiguousarray(self._leaves()["cents"][order])
        labels, count = similarity.jt_components_packed(cents, radius)
        if hasattr(labels, "cpu"):
            labels = labels.cpu().numpy()
        return np.asarray(labels, dtype=np.int64), int(count)

    def link_clusters(self, radius: float | None = None) -> "BitBirch":
        r"""Merge the clusters whose centroids hang together at Jaccard distance `radius` (default ``1 - threshold``):
        single-linkage clustering of the centroids cut at `radius`, which is `centroid_components`.  Stores the labels
        where `global_clustering` stores its own (1-based, in ``sort=True`` order), so every ``global_clusters=True`` getter
        and `save` / `load` see the merged clusters."""
        labels, count = self.centroid_components(radius, sort=True)
        self._global_clustering_centroid_labels = labels + 1
        self._n_global_clusters = count
        return self

    def centroid_leaders(self, radius: float | None = None, sort: bool = True, weighted: bool = True) -> tuple[NDArray[np.int64], int, NDArray[np.int64]]:
        r"""Leader clustering (sphere exclusion, Taylor-Butina) of the centroids at Jaccard distance `radius` (default
        ``1 - threshold``): ``(labels int64 (K,), n_clusters, centres int64 (K,))`` over the positions of
        `get_centroids(sort=sort)`.  Two centroids are neighbours iff `centroid_radius_neighbors(radius)` lists one for the
        other.  The centroid with the most around it becomes a centre and takes its neighbours, then the best of the rest,
        and so on (`similarity.jt_leaders_packed`): every member is within `radius` of its centre, no two centres are within
        `radius` of each other.  With `weighted` every cluster counts with its number of molecules, so "the most around it"
        counts molecules, not centroids.  ``centres[p]`` is the position of ``p``'s centre, ``labels[p]`` the rank of that
        centre among the centres in ascending position.  Computed on the device without the graph.  The model is left as
        it is."""
        from bblean_amd import similarity

        radius = similarity._radius_check(1.0 - self.threshold if radius is None else radius)
        order = self._leaf_order(sort)
        weights = np.asarray(self._leaves()["n"], dtype=np.int64)[order] if weighted else None
        gather = getattr(self._engine, "gather_centroids", None)
        cents = gather(order, device_out=True) if gather is not None else np.ascontiguousarray(self._leaves()["cents"][order])
        labels, count, centres = similarity.jt_leaders_packed(cents, radius, weights=weights, return_centres=True)
        if hasattr(labels, "cpu"):
            labels, centres = labels.cpu().numpy(), centres.cpu().numpy()
        return np.asarray(labels, dtype=np.int64), int(count), np.asarray(centres, dtype=np.int64)

    def lead_clusters(self, radius: float | None = None, weighted: bool = True) -> "BitBirch":
        r"""Merge every cluster into the cluster of its leader at Jaccard distance `radius` (default ``1 - threshold``):
        `centroid_leaders`.  Unlike `link_clusters` a merged cluster has a centre and a radius: all of its centroids are
        within `radius` of the centre's.  Stores the labels where `global_clustering` stores its own (1-based, in
        ``sort=True`` order), so every ``global_clusters=True`` getter and `save` / `load` see the merged clusters."""
        labels, count, _ = self.centroid_leaders(radius, sort=True, weighted=weighted)
        self._global_clustering_centroid_labels = labels + 1
        self._n_global_clusters = count
        return self

    def route(self, X, input_is_packed: bool = True, n_features: int | None = None, sort: bool = True):  # type: ignore[no-untyped-def]
        r"""Route fingerprints through the fitted tree WITHOUT inserting them: ``(cluster, accept, sim)``, one entry per row.

        ``cluster`` (int64) is the position, in `get_centroids(sort=sort)` / `get_cluster_mol_ids(sort=sort)`, of the cluster
        the greedy descent of `fit` reaches for that row; ``accept`` (bool) whether the current merge criterion would let the
        row join it (False: a `fit` would start a new cluster there); ``sim`` (float64) the Tanimoto similarity of the row to
        that cluster's centroid.  This is the tree's own answer in about depth x branching_factor compares per row - not the
        globally nearest centroid, which `sklearn.BitBirch.predict` searches the whole table for.  The model is not changed.
        Input as for `fit` (packed or unpacked rows, a list of rows, a device-resident ``torch.uint8`` tensor of packed
        rows)."""
        self._require_init()
        if self._only_has_leaves:
            raise ValueError("Internal nodes were released: there is no tree to route through")
        route_packed = getattr(self._engine, "route_packed", None)
        if route_packed is None:
            raise NotImplementedError(f"{type(self._engine).__name__} has no route_packed: routing needs an engine that can walk its tree")
        is_dev = hasattr(X, "data_ptr") and getattr(X, "is_cuda", False)
        if is_dev:
            if not input_is_packed:
                raise ValueError("device-resident input must be packed uint8")
            if X.shape[0] == 0:
                raise ValueError("Input must have at least 1 fingerprint")
            nf = X.shape[1] * 8 if n_features is None else n_features
            if X.shape[1] * 8 < nf:
                raise ValueError("n_features is larger than the padded length, which is inconsistent")
            rows: tp.Any = X
        else:
            nf = _validate_n_features(X, input_is_packed, n_features)
            arr = np.stack(X) if isinstance(X, list) else np.asarray(X)
            if input_is_packed:
                rows = np.ascontiguousarray(arr, dtype=np.uint8)
                if rows.shape[1] * 8 != nf:
                    rows = pack_fingerprints(unpack_fingerprints(rows, nf))
            else:
                rows = pack_fingerprints(arr.astype(np.uint8, copy=False))
        if nf != self._n_features:
            raise ValueError(f"tree was built with n_features={self._n_features}, got {nf}")
        self._push_merge_to_engine()  # (the criterion a `fit` would act on now)
        leaf, accept, inter, union = route_packed(rows)
        lv = self._leaves()
        pos_of_id = np.full(int(lv["ids"].max(initial=0)) + 1, -1, dtype=np.int64)
        pos_of_id[lv["ids"]] = np.arange(lv["ids"].size, dtype=np.int64)
        order = self._leaf_order(sort)
        rank = np.empty(order.size, dtype=np.int64)
        rank[order] = np.arange(order.size, dtype=np.int64)  # chain position -> position in get_centroids(sort=sort)
        chain = pos_of_id[np.asarray(leaf, dtype=np.int64)]
        if (chain < 0).any():
            raise RuntimeError("the engine routed a row to a BitFeature id that is not a leaf of the tree")
        sim = np.asarray(inter, dtype=np.float64) / np.maximum(np.asarray(union, dtype=np.float64), 1.0)
        return rank[chain], np.asarray(accept).astype(bool), sim

    def get_centroids_mol_ids(self, sort: bool = True, packed: bool = True) -> dict[str, list]:
        r"""(reference bitbirch.py:895-907)"""
        return {
            "centroids": self.get_centroids(sort, packed),
            "mol_ids": self._members_of(self._leaf_order(sort)),
        }

    def get_assignments(
        self,
        n_mols: int | None = None,
        sort: bool = True,
        check_valid: bool = True,
        global_clusters: bool = False,
    ) -> NDArray[np.uint64]:
        r"""Cluster label (1..K) of every fitted fingerprint (bitbirch.py:1002-1047)."""
        if n_mols is not None:
            warnings.warn("The n_mols argument is redundant", DeprecationWarning)
        if n_mols is not None and n_mols != self.num_fitted_fps:
            raise ValueError(
                f"Provided n_mols {n_mols} is different"
                f" from the number of fitted fingerprints {self.num_fitted_fps}"
            )
        lv = self._leaves()
        order = self._leaf_order(sort)
        sizes = (lv["end"] - lv["beg"])[order]
        if global_clusters:
            if self._global_clustering_centroid_labels is None:
                raise ValueError("Must perform global clustering before fetching global labels")
            labels_per_leaf = np.asarray(self._global_clustering_centroid_labels, dtype=np.uint64)
        else:
            labels_per_leaf = np.arange(1, order.size + 1, dtype=np.uint64)
        assignments = np.zeros(self.num_fitted_fps, dtype=np.uint64)
        total = int(sizes.sum())
        if total:
            starts = lv["beg"][order]
            dst = np.cumsum(sizes) - sizes
            gather = np.repeat(starts - dst, sizes) + np.arange(total, dtype=np.int64)
            assignments[lv["members"][gather]] = np.repeat(labels_per_leaf[: order.size], sizes)
        if check_valid and (assignments == 0).any():
            raise ValueError("There are unasigned molecules")
        return assignments

    def dump_assignments(self, path, smiles=(), sort=True, global_clusters=False, check_valid=True):  # type: ignore[no-untyped-def]
        r"""(reference bitbirch.py:1049-1076)"""
        import pandas as pd

        if isinstance(smiles, str):
            smiles = [smiles]
        smiles = np.asarray(smiles, dtype=np.str_)
        a = self.get_assignments(sort=sort, check_valid=check_valid, global_clusters=global_clusters)
        if smiles.size and (len(a) != len(smiles)):
            raise ValueError(
                f"Len of the provided smiles {len(smiles)}"
                f" must match the number of fitted fingerprints {self.num_fitted_fps}"
            )
        df = pd.DataFrame({"assignments": a})
        if smiles.size:
            df["smiles"] = smiles
        df.to_csv(Path(path), index=False)

    def _get_leaf_bfs(self, sort: bool = True) -> list[_LeafBF]:
        lv = self._leaves()
        order = self._leaf_order(sort)
        lists = self._members_of(order)
        return [
            _LeafBF(self, int(p), int(lv["n"][p]), lv["cents"][p], m)
            for p, m in zip(order, lists)
        ]

    def _flat_members(self, sort: bool = True, global_clusters: bool = False) -> tuple[NDArray[np.int64], NDArray[np.int64]]:
        r"""`get_cluster_mol_ids` as two arrays, without a Python list per cluster: (offsets [k + 1], members
        [offsets[-1]]); cluster g is members[offsets[g]:offsets[g + 1]]."""
        lv = self._leaves()
        order = self._leaf_order(sort)
        if global_clusters:
            if self._global_clustering_centroid_labels is None:
                raise ValueError("Must perform global clustering before fetching global labels")
            # the leaves of a label one after the other, in leaf order (`_new_ids_from_labels`)
            labels = np.asarray(self._global_clustering_centroid_labels, dtype=np.int64)[: order.size] - 1
            n_labels = self._n_global_clusters if self._n_global_clusters is not None else len(np.unique(labels))
            order = order[np.argsort(labels, kind="stable")]
            leaf_sizes = (lv["end"] - lv["beg"])[order].astype(np.int64)
            sizes = np.bincount(labels, weights=(lv["end"] - lv["beg"])[self._leaf_order(sort)], minlength=n_labels).astype(np.int64)
        else:
            leaf_sizes = sizes = (lv["end"] - lv["beg"])[order].astype(np.int64)
        offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        total = int(offsets[-1])
        first = np.cumsum(leaf_sizes) - leaf_sizes  # where each leaf's members start in the flat array
        gather = np.repeat(lv["beg"][order] - first, leaf_sizes) + np.arange(total, dtype=np.int64)
        return offsets, np.ascontiguousarray(lv["members"][gather], dtype=np.int64)

    def cluster_sets(self, fps, sort: bool = True, global_clusters: bool = False):  # type: ignore[no-untyped-def]
        r"""The fitted clustering over the packed rows ``fps`` (NumPy array or device tensor, the rows that were fitted, in
        that order) as `metrics.ClusterSets`: ``jt_isim_chi(tree.cluster_sets(fps))`` scores it in a fixed number of
        launches.  The clusters are those of `get_cluster_mol_ids` with the same arguments, in the same order."""
        from bblean_amd.metrics import ClusterSets

        offsets, flat = self._flat_members(sort, global_clusters)
        nf = self._n_features
        return ClusterSets(fps, offsets, flat, nf if nf % 8 == 0 and 0 < nf <= fps.shape[1] * 8 else None)

    # medoids (reference bitbirch.py:909-967): packed rows take ONE segmented call over all clusters
    def get_medoids_mol_ids(self, fps, sort=True, pack=True, global_clusters=False, input_is_packed=True, n_features=None):  # type: ignore[no-untyped-def]
        from bblean_amd.similarity import _is_dev, _seg_fits, jt_compl_isim_segments, jt_isim_medoid

        members = self.get_cluster_mol_ids(sort=sort, global_clusters=global_clusters)
        on_device = _is_dev(fps) and fps.dim() == 2 and str(fps.dtype) == "torch.uint8"
        on_host = isinstance(fps, np.ndarray) and fps.ndim == 2 and fps.dtype == np.uint8
        if input_is_packed and (on_device or on_host) and len(members):
            nb = int(fps.shape[1])
            nf = nb * 8 if n_features is None else int(n_features)
            sizes = np.fromiter(map(len, members), dtype=np.int64, count=len(members))
            if 0 < nf <= nb * 8 and nf % 8 == 0 and _seg_fits(nf, int(sizes.max())):
                offsets, flat = self._flat_members(sort, global_clusters)
                if on_device:
                    import torch

                    flat_t = torch.from_numpy(flat).to(fps.device)
                    pos = jt_compl_isim_segments(fps, offsets, flat_t, nf, return_compl=False)[0]
                    medoids = fps[flat_t[torch.from_numpy(offsets[:-1]).to(fps.device) + pos]][:, : nf // 8]
                    if not pack:
                        shifts = torch.arange(7, -1, -1, device=fps.device, dtype=torch.uint8)
                        medoids = ((medoids.unsqueeze(-1) >> shifts) & 1).reshape(medoids.shape[0], nf)
                    return {"medoids": medoids.contiguous(), "mol_ids": members}
                pos = jt_compl_isim_segments(fps, offsets, flat, nf, return_compl=False)[0]
                medoids = fps[flat[offsets[:-1] + pos]][:, : nf // 8]
                if not pack:
                    medoids = unpack_fingerprints(medoids, nf)
                return {"medoids": medoids, "mol_ids": members}
        if input_is_packed:
            fps = unpack_fingerprints(fps, n_features)
        medoids = np.zeros((len(members), fps.shape[1]), dtype=np.uint8)
        for i, m in enumerate(members):
            medoids[i] = jt_isim_medoid(fps[m], input_is_packed=False, pack=False)[1]
        if pack:
            medoids = pack_fingerprints(medoids)
        return {"medoids": medoids, "mol_ids": members}

    def get_medoids(self, fps, sort=True, pack=True, global_clusters=False, input_is_packed=True, n_features=None):  # type: ignore[no-untyped-def]
        return self.get_medoids_mol_ids(fps, sort, pack, global_clusters, input_is_packed, n_features)["medoids"]

    # -------------------------------------------------- BitFeature tables / refine ----
    def _group_positions(self, positions: NDArray[np.int64]) -> dict[str, NDArray[np.int64]]:
        r"""Split leaf positions into dtype groups in first-seen order
        (`_prepare_bf_to_buffer_dicts`, bitbirch.py:1298-1308)."""
        lv = self._leaves()
        n = lv["n"][positions]
        code = np.where(n <= 255, 0, np.where(n <= 65535, 1, np.where(n <= 4294967295, 2, 3)))
        names = ["uint8", "uint16", "uint32", "uint64"]
        groups: dict[str, NDArray[np.int64]] = {}
        if positions.size:
            _, first = np.unique(code, return_index=True)
            for c in code[np.sort(first)]:
                groups[names[int(c)]] = positions[code == c]
        return groups

    def _bf_tables(
        self, positions: NDArray[np.int64], device: bool = False
    ) -> tuple[dict[str, tp.Any], dict[str, _IndexLists]]:
        r"""Array form of `_bf_to_np`: per dtype group a (k, F+1) buffer table gathered
        on the device and the member lists as CSR.  `device`: the tables stay in HBM (`DevTable`)
        when the engine can do that (multiround hands them to the next round / the exchange)."""
        lv = self._leaves()
        bufs: dict[str, tp.Any] = {}
        mols: dict[str, _IndexLists] = {}
        dev_ok = device and getattr(self._engine, "device_tables", False)
        for name, pos in self._group_positions(positions).items():
            if dev_ok:
                n_tail = 0
                if name == "uint8":  # the run of one-fingerprint BitFeatures the table ends with stays packed (DevTable.tail)
                    ones = lv["n"][pos] == 1
                    n_tail = int(ones.size if ones.all() else np.argmax(~ones[::-1]))
                bufs[name] = self._engine.gather_buffers(pos, np.dtype(name).itemsize, device_out=True, n_tail=n_tail)
            else:
                bufs[name] = self._engine.gather_buffers(pos, np.dtype(name).itemsize)
            beg, end = lv["beg"][pos], lv["end"][pos]
            cnt = end - beg
            total = int(cnt.sum())
            dst = np.cumsum(cnt) - cnt
            gather = np.repeat(beg - dst, cnt) + np.arange(total, dtype=np.int64)
            mols[name] = _IndexLists(cnt.astype(np.int64), lv["members"][gather])
        return bufs, mols

    def _refine_tables(
        self,
        X: tp.Any,
        initial_mol: int = 0,
        input_is_packed: bool = True,
        n_largest: int = 1,
        device: bool = False,
    ) -> tuple[dict[str, NDArray[np.integer]], dict[str, _IndexLists]]:
        r"""`_bf_to_np_refine` (bitbirch.py:1224-1290) in array form: the `n_largest`
        biggest leaves are exploded into singleton uint8 buffers rebuilt from the
        original fingerprints and appended to the uint8 group, after the survivors.
        `device`: the tables stay in HBM (`DevTable`; the exploded fingerprints join the uint8 table's packed
        singleton tail) when the engine can do that and the input is packed."""
        order = self._leaf_order(True)
        dev_ok = device and input_is_packed and getattr(self._engine, "device_tables", False)
        if n_largest == 0:
            return self._bf_tables(order, device=dev_ok)
        if n_largest < 1:
            raise ValueError("n_largest must be >= 1")
        largest, rest = order[:n_largest], order[n_largest:]
        bufs, mols = self._bf_tables(rest, device=dev_ok)
        F = self._n_features
        big_rows: list[NDArray[np.uint8]] = []
        big_ids: list[NDArray[np.int64]] = []
        for members in self._members_of(largest):
            mol_idxs = np.asarray(members, dtype=np.int64)
            arr_idxs = mol_idxs - initial_mol
            if isinstance(X, (Path, str)):
                fps = np.load(X, mmap_mode="r")[arr_idxs]
            elif isinstance(X, (list, tuple)) and len(X) and isinstance(X[0], (Path, str)):
                # a sequence of files: members are re-read in ascending global index
                srt = np.argsort(arr_idxs, kind="stable")
                fps = _rows_from_file_seq([Path(p) for p in X], arr_idxs[srt])
                mol_idxs = mol_idxs[srt]
            elif isinstance(X, list):
                fps = np.stack([np.asarray(X[i]) for i in arr_idxs])
            elif hasattr(X, "data_ptr") and getattr(X, "is_cuda", False):  # device-resident shard
                import torch

                fps = X[torch.from_numpy(arr_idxs).to(X.device)]
                if not dev_ok:
                    fps = fps.cpu().numpy()
            else:
                fps = np.asarray(X)[arr_idxs]
            if dev_ok:
                # packed rows: they go into the table's singleton tail as they are - which they must be: uint8, F / 8 columns
                # (the host path normalises through unpack_fingerprints; here a wrong width would only surface as an engine
                # error about row bytes much later)
                if not hasattr(fps, "data_ptr"):
                    fps = np.ascontiguousarray(fps)
                    if fps.dtype != np.uint8:
                        fps = fps.astype(np.uint8)
                if fps.ndim != 2 or int(fps.shape[1]) != F // 8 or (hasattr(fps, "data_ptr") and str(fps.dtype) != "torch.uint8"):
                    raise ValueError(f"packed fingerprints of {F} features must be uint8 rows of {F // 8} bytes, got {tuple(fps.shape)} {fps.dtype}")
                big_rows.append(fps)
                big_ids.append(mol_idxs)
                continue
            fps = np.asarray(fps)
            if input_is_packed:
                fps = unpack_fingerprints(fps.astype(np.uint8, copy=False), F)
            big_rows.append(fps.astype(np.uint8))
            big_ids.append(mol_idxs)
        if big_rows and dev_ok:
            import torch

            from bblean_amd._engine import DevTable

            tdev = torch.device("cuda", self._engine.device)
            parts = [r if hasattr(r, "data_ptr") else torch.from_numpy(np.ascontiguousarray(r, dtype=np.uint8)).to(tdev) for r in big_rows]
            ids = np.concatenate(big_ids)
            ones = np.ones(ids.size, dtype=np.int64)
            if "uint8" in bufs:
                tab = bufs["uint8"]
                if tab.tail is not None:
                    parts = [tab.tail] + parts
                bufs["uint8"] = DevTable(tab.raw, 1, torch.cat(parts) if len(parts) > 1 else parts[0])
                old = mols["uint8"]
                mols["uint8"] = _IndexLists(np.concatenate([old.counts, ones]), np.concatenate([old.flat, ids]))
            else:
                empty = torch.empty((0, F + 1), dtype=torch.uint8, device=tdev)
                bufs["uint8"] = DevTable(empty, 1, torch.cat(parts) if len(parts) > 1 else parts[0])
                mols["uint8"] = _IndexLists(ones, ids)
        elif big_rows:
            rows = np.concatenate(big_rows)
            extra = np.empty((rows.shape[0], F + 1), dtype=np.uint8)
            extra[:, :-1] = rows
            extra[:, -1] = 1
            ids = np.concatenate(big_ids)
            ones = np.ones(ids.size, dtype=np.int64)
            if "uint8" in bufs:
                bufs["uint8"] = np.concatenate([bufs["uint8"], extra])
                old = mols["uint8"]
                mols["uint8"] = _IndexLists(
                    np.concatenate([old.counts, ones]), np.concatenate([old.flat, ids])
                )
            else:
                bufs["uint8"] = extra
                mols["uint8"] = _IndexLists(ones, ids)
        return bufs, mols

    def _bf_to_np(self):  # type: ignore[no-untyped-def]
        r"""dict dtype-name -> list of buffers, dict dtype-name -> list of index lists
        (reference bitbirch.py:1292-1296)."""
        bufs, mols = self._bf_tables(self._leaf_order(True))
        return {k: list(v) for k, v in bufs.items()}, {k: v.to_lists() for k, v in mols.items()}

    def _bf_to_np_refine(self, X, initial_mol=0, input_is_packed=True, n_largest=1):  # type: ignore[no-untyped-def]
        bufs, mols = self._refine_tables(X, initial_mol, input_is_packed, n_largest)
        return {k: list(v) for k, v in bufs.items()}, {k: v.to_lists() for k, v in mols.items()}

    def refine_inplace(
        self,
        X: tp.Any,
        initial_mol: int = 0,
        input_is_packed: bool = True,
        n_largest: int = 1,
    ) -> "BitBirch":
        r"""Break the largest cluster(s) into singletons and re-fit every BitFeature
        (reference bitbirch.py:1187-1214)."""
        self._require_init()
        self.delete_internal_nodes()
        # (the tables stay in HBM when the engine can do that: gathered there, re-inserted from there - next to the old tree's
        # pools, which reset() keeps; when HBM does not hold both, the tables take the reference's way through host memory)
        try:
            bufs, mols = self._refine_tables(X, initial_mol, input_is_packed, n_largest, device=True)
        except Exception as exc:
            if not _is_out_of_memory(exc):
                raise
            bufs, mols = self._refine_tables(X, initial_mol, input_is_packed, n_largest, device=False)
        self.reset()
        for name in bufs:
            self._fit_buffers(bufs[name], reinsert_index_seqs=mols[name])
        return self

    def recluster_inplace(
        self,
        iterations: int = 1,
        extra_threshold: float = 0.0,
        shuffle: bool = False,
        seed: int | None = None,
        verbose: bool = False,
        stop_early: bool = False,
    ) -> "BitBirch":
        r"""Re-insert all leaf BitFeatures, optionally raising the threshold
        (reference bitbirch.py:1110-1185)."""
        self._require_init()
        singletons_before = 0
        for _ in range(iterations):
            order = self._leaf_order(True)
            n = self._leaves()["n"][order]
            singletons = int((n == 1).sum())
            if stop_early and (singletons == 0 or singletons == singletons_before):
                break
            singletons_before = singletons
            if verbose:
                print(f"Current number of clusters: {order.size}")
                print(f"Current number of singletons: {singletons}")
            if shuffle:
                perm = list(range(order.size))
                random.seed(seed)
                random.shuffle(perm)
                order = order[np.asarray(perm, dtype=np.int64)]
            try:
                bufs, mols = self._bf_tables(order, device=True)
            except Exception as exc:
                if not _is_out_of_memory(exc):
                    raise
                bufs, mols = self._bf_tables(order, device=False)
            self.reset()
            self.threshold += extra_threshold
            for name in bufs:
                self._fit_buffers(bufs[name], reinsert_index_seqs=mols[name])
        if verbose:
            n = self._leaves()["n"]
            print(f"Final number of clusters: {n.size}")
            print(f"Final number of singletons: {int((n == 1).sum())}")
        return self

    def global_clustering(self, n_clusters: int, *, method: str = "kmeans", **method_kwargs: tp.Any) -> "BitBirch":
        r""":meta private: experimental in the reference (bitbirch.py:1355-1434)."""
        warnings.warn(
            "Global clustering is an experimental features"
            " it will be modified without warning, please do not use"
        )
        self._require_init()
        if method not in {"agglomerative", "kmeans", "kmeans-normalized"}:
            raise ValueError(f"Unknown method {method}")
        from sklearn.cluster import AgglomerativeClustering, KMeans
        from sklearn.exceptions import ConvergenceWarning

        centrals = np.vstack(self.get_centroids(packed=False))
        num = len(centrals)
        k = n_clusters
        if num < k:
            warnings.warn(
                f"Number of subclusters found ({num}) by BitBIRCH is less "
                "than ({n_clusters}). Decrease k or the threshold.",
                ConvergenceWarning,
                stacklevel=2,
            )
            k = num
        data = centrals
        if method == "kmeans-normalized":
            data = centrals / np.linalg.norm(centrals, axis=1, keepdims=True)
        if method in ("kmeans", "kmeans-normalized"):
            predictor = KMeans(n_clusters=k, **method_kwargs)
        else:
            predictor = AgglomerativeClustering(n_clusters=k, **method_kwargs)
        self._global_clustering_centroid_labels = predictor.fit_predict(data) + 1
        self._n_global_clusters = n_clusters if num > n_clusters else num
        return self

    # ------------------------------------------------------------- persistence ----
    def save(self, path: Path | str, *, stage_bytes: int = 0) -> None:
        r"""Write the fitted tree to ONE file (INTEGRATION.md "Tree files"): a JSON header with the configuration, the
        host bookkeeping as ``.npy`` arrays and the engine's tree image, which the library writes straight to the file.
        The reference pickles the whole object (bitbirch.py:1321-1339); this file is no pickle and `load` unpickles nothing.
        A custom `MergeCriterion` object cannot be stored: only the built-in criteria, by name."""
        path = Path(path)
        self._check_storable()  # (before the target is touched: a refused save leaves an existing file as it was)
        tmp = path.with_name(f"{path.name}.{os.getpid()}.part")
        try:
            with open(tmp, "wb") as f:
                self._write_container(f, stage_bytes)
            os.replace(tmp, path)  # a save that fails half-way leaves nothing under the final name
        except BaseException:
            try:
                os.unlink(tmp)
            except OSError:
                pass
            raise

    @classmethod
    def load(
        cls,
        path: Path | str,
        device: int = 0,
        *,
        stage_bytes: int = 0,
        _engine_factory: tp.Callable[..., tp.Any] | None = None,
        _engine_loader: tp.Callable[..., tp.Any] | None = None,
    ) -> "BitBirch":
        r"""The tree `save` wrote, on `device` (reference bitbirch.py:1341-1353).  The saved merge criterion and tolerance
        are restored whether or not the module-level `set_merge` is in force.  `_engine_factory` / `_engine_loader` are
        test hooks like the constructor's: the loader - by default the factory's `load_image`, if it has one - is called
        with (file object, device) where the image starts.
        Anything wrong with the file - not a tree file, another version, truncated, an image that fails the library's
        check - is a ValueError that names the path."""
        path = Path(path)
        self = cls.__new__(cls)
        try:
            with open(path, "rb") as f:
                self._read_container(f, device, stage_bytes, _engine_factory, _engine_loader)
        except _BadTreeFile as exc:
            raise ValueError(f"{path}: {exc}") from None
        return self

    def _check_storable(self) -> None:
        fn = self._merge_accept_fn
        if fn.name not in BUILTIN_MERGES or type(fn) is not MergeCriterion or (fn.n_max, fn.decay) != (1000, 1e-3):
            raise ValueError(
                f"a custom MergeCriterion ({fn!r}) cannot be stored in a tree file: only the built-in criteria, by name"
            )
        if self._engine is not None and not hasattr(self._engine, "save_image"):
            raise ValueError(f"the engine {type(self._engine).__name__} cannot write a tree image")

    def _write_container(self, f: tp.BinaryIO, stage_bytes: int = 0) -> None:
        self._check_storable()  # (`save` has asked already, before it touched the target; __getstate__ comes here directly)
        fn = self._merge_accept_fn
        has_image = self._engine is not None
        arrays: dict[str, NDArray] = {}
        if self._log_leaf:
            arrays["log_leaf"] = np.concatenate(self._log_leaf).astype(np.uint32, copy=False)
            arrays["log_ids"] = np.concatenate(self._log_ids).astype(np.int64, copy=False)
            counts = [c for c in self._log_counts if c is not None]
            arrays["log_counts"] = np.concatenate(counts).astype(np.int64, copy=False) if counts else np.zeros(0, dtype=np.int64)
        if self._global_clustering_centroid_labels is not None:
            arrays["global_labels"] = np.asarray(self._global_clustering_centroid_labels, dtype=np.int64)
        header = {
            "format": _TREE_FILE_FORMAT,
            "version": _TREE_FILE_VERSION,
            "threshold": float(self.threshold),
            "branching_factor": int(self.branching_factor),
            "merge_criterion": fn.name,
            "tolerance": None if fn.tolerance is None else float(fn.tolerance),
            "n_features": int(self._n_features),
            "num_fitted_fps": int(self._num_fitted_fps),
            "is_init": bool(self._is_init),
            "internal_released": bool(self._internal_released),
            "n_global_clusters": int(self._n_global_clusters),
            # per fit call: [leaf ids, member ids, counts or -1 (a `fit` call: one id per element)]
            "log_calls": [[int(l.size), int(i.size), -1 if c is None else int(c.size)]
                          for l, i, c in zip(self._log_leaf, self._log_ids, self._log_counts)],
            "arrays": list(arrays),
            "has_image": has_image,
        }
        blob = json.dumps(header).encode("utf-8")
        f.write(_TREE_FILE_MAGIC + struct.pack("<II", _TREE_FILE_VERSION, len(blob)) + blob)
        for arr in arrays.values():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            f.write(struct.pack("<Q", buf.getbuffer().nbytes))
            f.write(buf.getbuffer())
        if has_image:
            at = f.tell()
            f.write(struct.pack("<Q", 0))
            n = int(self._engine.save_image(f, stage_bytes) if stage_bytes else self._engine.save_image(f))
            end = f.tell()
            f.seek(at)
            f.write(struct.pack("<Q", n))
            f.seek(end)
        f.flush()

    def _read_container(self, f, device, stage_bytes, engine_factory, engine_loader):  # type: ignore[no-untyped-def]
        def take(n: int, what: str) -> bytes:
            b = f.read(n)
            if len(b) != n:
                raise _BadTreeFile(f"the file is truncated ({what})")
            return b

        head = take(len(_TREE_FILE_MAGIC) + 8, "header")
        if head[: len(_TREE_FILE_MAGIC)] != _TREE_FILE_MAGIC:
            raise _BadTreeFile("not a BitBirch tree file (wrong magic)")
        version, n_json = struct.unpack("<II", head[len(_TREE_FILE_MAGIC):])
        if version != _TREE_FILE_VERSION:
            raise _BadTreeFile(f"tree file version {version} is not supported (this package reads version {_TREE_FILE_VERSION})")
        try:
            header = json.loads(take(n_json, "JSON header").decode("utf-8"))
            if header["format"] != _TREE_FILE_FORMAT or header["version"] != version:
                raise KeyError("format")
            fn = get_merge_accept_fn(header["merge_criterion"], 0.05 if header["tolerance"] is None else float(header["tolerance"]))
            names = [str(a) for a in header["arrays"]]
            calls = [(int(a), int(b), int(c)) for a, b, c in header["log_calls"]]
        except _BadTreeFile:
            raise
        except Exception as exc:
            raise _BadTreeFile(f"the header is not that of a tree file ({type(exc).__name__}: {exc})") from None
        arrays: dict[str, NDArray] = {}
        for name in names:
            (n,) = struct.unpack("<Q", take(8, f"array {name}"))
            try:
                arrays[name] = np.lib.format.read_array(io.BytesIO(take(n, f"array {name}")), allow_pickle=False)
            except _BadTreeFile:
                raise
            except Exception as exc:
                raise _BadTreeFile(f"array {name} cannot be read ({exc})") from None
        leaf = arrays.get("log_leaf", np.zeros(0, dtype=np.uint32))
        ids = arrays.get("log_ids", np.zeros(0, dtype=np.int64))
        cnts = arrays.get("log_counts", np.zeros(0, dtype=np.int64))
        if (sum(a for a, _, _ in calls), sum(b for _, b, _ in calls), sum(max(c, 0) for _, _, c in calls)) != (leaf.size, ids.size, cnts.size):
            raise _BadTreeFile("the per-call lengths do not match the bookkeeping arrays")
        engine = None
        if header["has_image"]:
            (n_image,) = struct.unpack("<Q", take(8, "image length"))
            at = f.tell()
            f.seek(0, 2)
            if f.tell() - at < n_image:
                raise _BadTreeFile("the file is truncated (tree image)")
            f.seek(at)
            loader = engine_loader if engine_loader is not None else getattr(engine_factory, "load_image", None)
            if loader is None:
                from bblean_amd._engine import HipEngine

                try:  # (host code: a bad image is refused here, before a device is asked for)
                    if HipEngine.check_image(f) != n_image:
                        raise RuntimeError("the image's length differs from the recorded one")
                except RuntimeError as exc:
                    raise _BadTreeFile(str(exc)) from None
                loader = HipEngine.load_image if not stage_bytes else (lambda fo, dev: HipEngine.load_image(fo, dev, stage_bytes))
            engine = loader(f, device)
            # The two halves must describe one tree.  Only the width is fixed for a tree's life: threshold, branching
            # factor and criterion may be changed between fits and reach the engine with the next one
            # (_push_merge_to_engine), so the header's values are the ones that hold.
            width = getattr(engine, "n_features", None)
            if width is not None and int(width) != int(header["n_features"]):
                close = getattr(engine, "close", None)
                if close is not None:
                    close()
                raise _BadTreeFile(f"the header records {header['n_features']} features and the tree image holds {width}")
        # everything was read: only now does the object come into being
        self.threshold = header["threshold"]
        self.branching_factor = header["branching_factor"]
        self._merge_accept_fn = fn
        self._device = device
        self._engine_factory = engine_factory
        self._engine = engine
        self._n_features = int(header["n_features"])
        self._num_fitted_fps = int(header["num_fitted_fps"])
        self._is_init = bool(header["is_init"])
        self._internal_released = bool(header["internal_released"])
        self._log_leaf, self._log_counts, self._log_ids = [], [], []
        a0 = b0 = c0 = 0
        for a, b, c in calls:
            self._log_leaf.append(leaf[a0:a0 + a])
            self._log_ids.append(ids[b0:b0 + b])
            self._log_counts.append(None if c < 0 else cnts[c0:c0 + c])
            a0, b0, c0 = a0 + a, b0 + b, c0 + max(c, 0)
        self._cache = {}
        self._global_clustering_centroid_labels = arrays.get("global_labels")
        self._n_global_clusters = int(header["n_global_clusters"])
        _BITBIRCH_INSTANCES.add(self)

    # pickle (and copy.deepcopy): the state is the tree file as bytes plus whatever else a subclass keeps on the instance -
    # the scikit-learn estimators' fitted attributes; BaseEstimator's own __getstate__ / __setstate__ call these through super()
    _PICKLE_SKIP: tp.ClassVar[frozenset] = frozenset()
    _OWN_ATTRS: tp.ClassVar[frozenset] = frozenset({
        "threshold", "branching_factor", "_merge_accept_fn", "_device", "_engine", "_n_features", "_num_fitted_fps", "_is_init",
        "_internal_released", "_log_leaf", "_log_counts", "_log_ids", "_cache", "_global_clustering_centroid_labels",
        "_n_global_clusters"})

    def __getstate__(self) -> dict[str, tp.Any]:
        with tempfile.TemporaryFile() as f:  # (the same code path as `save`: the library writes to a descriptor)
            self._write_container(f)
            f.seek(0)
            blob = f.read()
        extra = {k: v for k, v in self.__dict__.items() if k not in self._OWN_ATTRS and k not in self._PICKLE_SKIP}
        return {"_tree_file": blob, "_device": self._device, "_extra": extra}

    def __reduce_ex__(self, protocol: int):  # type: ignore[no-untyped-def]
        rv = super().__reduce_ex__(protocol)
        if protocol >= 5 and isinstance(rv, tuple) and len(rv) >= 3 and isinstance(rv[2], dict) and "_tree_file" in rv[2]:
            state = dict(rv[2])
            state["_tree_file"] = pickle.PickleBuffer(state["_tree_file"])  # out-of-band when the pickler has a buffer_callback
            rv = rv[:2] + (state,) + rv[3:]
        return rv

    def __setstate__(self, state: dict[str, tp.Any]) -> None:
        # sklearn's BaseEstimator.__setstate__ reaches this through super() and takes an AttributeError to mean "no
        # __setstate__ above me", then fills __dict__ with the raw state: one raised in here must not look like that
        try:
            self._set_state(state)
        except AttributeError as exc:
            raise RuntimeError(f"restoring a pickled {type(self).__name__} failed: {exc!r}") from exc

    def _set_state(self, state: dict[str, tp.Any]) -> None:
        extra = dict(state["_extra"])
        with tempfile.TemporaryFile() as f:
            f.write(memoryview(state["_tree_file"]))
            f.flush()
            f.seek(0)
            try:
                self._read_container(f, state["_device"], 0, extra.pop("_engine_factory", None), None)
            except _BadTreeFile as exc:
                raise ValueError(f"pickled tree: {exc}") from None
        self.__dict__.update(extra)
        self._after_load()

    def _after_load(self) -> None:
        r"""Hook for subclasses: rebuild what `_PICKLE_SKIP` left out."""

    def __repr__(self) -> str:
        fn = self._merge_accept_fn
        parts = [
            f"threshold={self.threshold}",
            f"branching_factor={self.branching_factor}",
            f"merge_criterion='{fn.name if fn.name in BUILTIN_MERGES else fn}'",
        ]
        if self.tolerance is not None:
            parts.append(f"tolerance={self.tolerance}")
        return f"{self.__class__.__name__}({', '.join(parts)})"


def _is_out_of_memory(exc: BaseException) -> bool:
    r"""A device allocation that failed: torch's OutOfMemoryError, the engine's MemoryError (BBH_ERR_CAPACITY) or a HIP error
    that says so."""
    if isinstance(exc, MemoryError):
        return True
    name = type(exc).__name__
    return "OutOfMemory" in name or "out of memory" in str(exc).lower()


def fit_concurrently(
    trees: tp.Sequence[BitBirch],
    inputs: tp.Sequence[tp.Any],
    reinsert_indices: tp.Sequence[tp.Iterable[int] | None] | None = None,
    input_is_packed: bool = True,
    n_features: int | None = None,
    max_fps: int | None = None,
) -> None:
    r"""`tree.fit(X)` for several independent trees at once - the shards of multiround's first
    round (reference multiround.py:401-422 runs them in a process pool).  On the HIP engine all
    trees insert in ONE kernel launch, one workgroup per tree, concurrently on different compute
    units; results are identical to calling `fit` on each tree in turn."""
    if len(trees) != len(inputs):
        raise ValueError("need one input per tree")
    prepared = []
    for i, (t, X) in enumerate(zip(trees, inputs)):
        ri = None if reinsert_indices is None else reinsert_indices[i]
        prepared.append(t._prepare_fit(X, ri, input_is_packed, n_features, max_fps))
    engines = [t._engine for t in trees]
    many = getattr(type(engines[0]), "fit_packed_many", None) if engines else None
    # a single tree takes the single-tree entry point: host / file-backed rows are then streamed through
    # two HBM slabs instead of being staged whole
    if len(engines) > 1 and many is not None and all(type(e) is type(engines[0]) for e in engines):
        leaves = many(engines, [rows for rows, _ in prepared])
    else:
        leaves = [e.fit_packed(rows) for e, (rows, _) in zip(engines, prepared)]
    for t, leaf, (_, ids) in zip(trees, leaves, prepared):
        if len(ids):
            t._commit_fit(leaf, ids)


def fit_buffers_concurrently(
    trees: tp.Sequence[BitBirch],
    tables: tp.Sequence[tp.Sequence[tuple[tp.Any, tp.Any]]],
) -> None:
    r"""`tree._fit_buffers(bufs, idx)` for every ``(bufs, idx)`` of ``tables[i]``, in order, for
    several independent trees at once: the trees of one multiround merge round (reference
    multiround.py:240-264, one process per tree there).  Step s inserts the s-th table of every
    tree that has one in ONE kernel launch (one workgroup per tree); results are identical to
    looping over the trees."""
    if len(trees) != len(tables):
        raise ValueError("need one table list per tree")
    steps = max((len(t) for t in tables), default=0)
    for s in range(steps):
        live, prepared = [], []
        for tree, tabs in zip(trees, tables):
            if s < len(tabs):
                prep = tree._prepare_fit_buffers(tabs[s][0], tabs[s][1])
                if prep is not None:
                    live.append(tree)
                    prepared.append(prep)
        if not live:
            continue
        engines = [t._engine for t in live]
        many = getattr(type(engines[0]), "fit_buffers_many", None)
        if len(engines) > 1 and many is not None and all(type(e) is type(engines[0]) for e in engines):
            leaves = many(engines, [p[0] for p in prepared])
        else:  # a single tree takes the single-tree entry point (streamed input, singleton fast path)
            leaves = [e.fit_buffers(p[0]) for e, p in zip(engines, prepared)]
        for tree, leaf, (_, counts, flat) in zip(live, leaves, prepared):
            tree._commit_fit_buffers(leaf, counts, flat)


def _rows_from_file_seq(files: tp.Sequence[Path], idxs: NDArray[np.int64]) -> NDArray[np.uint8]:
    r"""Rows `idxs` (ascending, global numbering over the concatenated files) read with
    memory-mapped loads (the job of `_get_fingerprints_from_file_seq`,
    reference fingerprints.py:273-321)."""
    if np.any(np.diff(idxs) < 0):
        raise ValueError("idxs must be sorted")
    out: list[NDArray[np.uint8]] = []
    base = 0
    taken = 0
    for f in files:
        arr = np.load(f, mmap_mode="r")
        n = arr.shape[0]
        hi = int(np.searchsorted(idxs, base + n, side="left"))
        if hi > taken:
            out.append(np.asarray(arr[idxs[taken:hi] - base]).astype(np.uint8, copy=False))
            taken = hi
        base += n
    if taken != idxs.size:
        raise ValueError("idxs could not be extracted from files")
    return np.concatenate(out) if out else np.zeros((0, 0), dtype=np.uint8)

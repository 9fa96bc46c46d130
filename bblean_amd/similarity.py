r"""`bblean.similarity` function surface on the MI355X kernels.

Same names, argument meaning and error behaviour as the reference module
(bblean/similarity.py:12-35) and the pybind11 functions it re-exports
(bblean/csrc/similarity.cpp:473-521).  Every function that the reference backs with
C++ runs here as a HIP kernel through the C ABI (include/bbhip.h); the thin composites
the reference writes in Python on top of them (`jt_isim_radius*`, `jt_sim_matrix_packed`,
`estimate_jt_std`, ...) are the same thin composites here.  There is no NumPy fallback.

Inputs may be NumPy arrays (staged to HBM for the call) or CUDA/HIP ``torch`` tensors
(used in place; outputs are then device tensors as well where that makes sense).
"""
from __future__ import annotations

import ctypes as C
import os
import typing as tp
import warnings

import numpy as np
from numpy.typing import NDArray

from bblean_amd import _lib
from bblean_amd.fingerprints import pack_fingerprints, unpack_fingerprints

__all__ = [
    "jt_isim_from_sum",
    "jt_isim",
    "jt_sim_packed",
    "jt_most_dissimilar_packed",
    "jt_isim_radius_from_sum",
    "jt_isim_radius_compl_from_sum",
    "jt_isim_diameter_from_sum",
    "jt_isim_radius",
    "jt_isim_radius_compl",
    "jt_isim_diameter",
    "centroid_from_sum",
    "centroid",
    "jt_isim_medoid",
    "jt_compl_isim",
    "jt_stratified_sampling",
    "jt_sim_matrix_packed",
    "jt_best_match_packed",
    "jt_assign_packed",
    "jt_dist_matrix_packed",
    "jt_topk_packed",
    "jt_radius_packed",
    "jt_components_packed",
    "jt_leaders_packed",
    "jt_compl_isim_segments",
    "jt_cluster_stats_segments",
]


def _is_dev(x: object) -> bool:
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _u8_2d(a: object, what: str = "Input array") -> tuple[object, int, int, int]:
    r"""(keepalive, n, nbytes, row_stride) of a 2-D uint8 array / device tensor."""
    if _is_dev(a):
        if a.dim() != 2:  # type: ignore[attr-defined]
            raise RuntimeError(f"{what} must be 2-dimensional")
        assert a.stride(1) == 1  # type: ignore[attr-defined]
        return a, int(a.shape[0]), int(a.shape[1]), int(a.stride(0))  # type: ignore[attr-defined]
    arr = np.asarray(a)
    if arr.ndim != 2:
        raise RuntimeError(f"{what} must be 2-dimensional")
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    return arr, arr.shape[0], arr.shape[1], arr.shape[1]


# ------------------------------------------------------------------ popcount -------
def _popcount_2d(a: object) -> NDArray[np.uint32]:
    r"""Row popcounts (similarity.cpp:99-141)."""
    lib = _lib.load()
    arr, n, nb, stride = _u8_2d(a)
    out = np.empty(n, dtype=np.uint32)
    _lib.check(lib.bbh_popcount_rows(_lib.ptr(arr), n, nb, stride, out.ctypes.data, None))
    return out


def _popcount_1d(a: NDArray[np.uint8]) -> int:
    r"""Popcount of one packed row (similarity.cpp:63-94)."""
    arr = np.asarray(a)
    if arr.ndim != 1:
        raise RuntimeError("Input array must be 1-dimensional")
    return int(_popcount_2d(arr.reshape(1, -1))[0])


# ------------------------------------------------------------ arr-vec Tanimoto -----
def _jt_sim_arr_vec_packed(arr: object, vec: object) -> NDArray[np.float64]:
    r"""Tanimoto of every packed row of ``arr`` against the packed row ``vec``
    (similarity.cpp:374-377).  float64, exact integer popcounts, one IEEE division."""
    lib = _lib.load()
    a, n, nb, stride = _u8_2d(arr, "arr")
    if _is_dev(vec):
        v = vec
        vdim, vlen = v.dim(), int(v.shape[-1])  # type: ignore[attr-defined]
    else:
        v = np.ascontiguousarray(vec, dtype=np.uint8)
        vdim, vlen = v.ndim, v.shape[-1] if v.ndim else 0
    if vdim != 1:
        raise RuntimeError("arr must be 2D, vec must be 1D")
    if vlen != nb:
        raise RuntimeError("Shapes should be (N, F) for arr and (F,) for vec")
    if _is_dev(a):
        import torch

        out_t = torch.empty(n, dtype=torch.float64, device=a.device)  # type: ignore[attr-defined]
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(
            lib.bbh_jt_arr_vec(_lib.ptr(a), n, nb, stride, _lib.ptr(v), None, _lib.ptr(out_t), None, None, st)
        )
        return out_t  # type: ignore[return-value]
    out = np.empty(n, dtype=np.float64)
    _lib.check(
        lib.bbh_jt_arr_vec(_lib.ptr(a), n, nb, stride, _lib.ptr(v), None, out.ctypes.data, None, None, None)
    )
    return out


def _jt_counts_arr_vec_packed(arr: object, vec: object) -> tuple[NDArray[np.uint32], NDArray[np.uint32]]:
    r"""Exact (intersection, union) popcounts of the same kernel (debug / parity)."""
    lib = _lib.load()
    a, n, nb, stride = _u8_2d(arr, "arr")
    v = np.ascontiguousarray(vec, dtype=np.uint8)
    inter = np.empty(n, dtype=np.uint32)
    union = np.empty(n, dtype=np.uint32)
    _lib.check(
        lib.bbh_jt_arr_vec(_lib.ptr(a), n, nb, stride, v.ctypes.data, None, None,
                           inter.ctypes.data, union.ctypes.data, None)
    )
    return inter, union


def jt_sim_packed(x: NDArray[np.uint8], y: NDArray[np.uint8]) -> NDArray[np.float64]:
    r"""General wrapper (similarity.py:218-236): two vectors, or a vector and an array."""
    xd = x.dim() if _is_dev(x) else np.ndim(x)  # type: ignore[attr-defined]
    yd = y.dim() if _is_dev(y) else np.ndim(y)  # type: ignore[attr-defined]
    if xd == 1 and yd == 1:
        return _jt_sim_arr_vec_packed(x.reshape(1, -1), y)[0]
    if xd == 2:
        return _jt_sim_arr_vec_packed(x, y)
    if yd == 2:
        return _jt_sim_arr_vec_packed(y, x)
    raise ValueError("Expected either two 1D vectors, or one 1D vector and one 2D array")


def jt_best_match_packed(
    queries: NDArray[np.uint8], centroids: NDArray[np.uint8], return_sims: bool = False
) -> tuple[NDArray[np.int32], NDArray[np.uint32], NDArray[np.uint32], NDArray[np.float64] | None]:
    r"""Batched descent step: first-argmax Tanimoto of each query against all centroid
    rows (`_jt_sim_arr_vec_packed` + `np.argmax`, bitbirch.py:317-320, for a whole
    batch of incoming fingerprints at once)."""
    lib = _lib.load()
    q, nq, nb, _ = _u8_2d(queries, "queries")
    c, nc, nb2, _ = _u8_2d(centroids, "centroids")
    if nb != nb2:
        raise RuntimeError("queries and centroids must have the same packed width")
    idx = np.empty(nq, dtype=np.int32)
    inter = np.empty(nq, dtype=np.uint32)
    union = np.empty(nq, dtype=np.uint32)
    sims = np.empty((nq, nc), dtype=np.float64) if return_sims else None
    _lib.check(
        lib.bbh_jt_best_match(_lib.ptr(q), nq, _lib.ptr(c), nc, nb, idx.ctypes.data,
                              inter.ctypes.data, union.ctypes.data,
                              sims.ctypes.data if sims is not None else None, None)
    )
    return idx, inter, union, sims


# ------------------------------------------------- assignment to fitted clusters ---
def _slab_rows(row_bytes: int) -> int:
    r"""Host rows staged per call: `BBHIP_SLAB_KB` (default 256 MiB) names the slab, as for the tree's input."""
    kb = int(os.environ.get("BBHIP_SLAB_KB", str(256 * 1024)))
    return max(1, (kb * 1024) // max(1, row_bytes))


def _assign_operands(queries: object, centroids: object) -> tuple[object, int, int, int, object, int]:
    q, nq, nb, q_stride = _u8_2d(queries, "queries")
    if _is_dev(q) and str(q.dtype) != "torch.uint8":  # type: ignore[attr-defined]
        raise RuntimeError("queries must be uint8")
    if _is_dev(centroids):
        c = centroids if centroids.is_contiguous() else centroids.contiguous()  # type: ignore[attr-defined]
        if c.dim() != 2 or str(c.dtype) != "torch.uint8":  # type: ignore[attr-defined]
            raise RuntimeError("centroids must be 2-dimensional uint8")
        nc, nb2 = int(c.shape[0]), int(c.shape[1])  # type: ignore[attr-defined]
    else:
        c, nc, nb2, _ = _u8_2d(centroids, "centroids")
    if nb != nb2:
        raise RuntimeError("queries and centroids must have the same packed width")
    if nc < 1:
        raise RuntimeError("need at least one centroid row")
    return q, nq, nb, q_stride, c, nc


def jt_assign_packed(queries: object, centroids: object, return_counts: bool = False):  # type: ignore[no-untyped-def]
    r"""Nearest centroid of every packed query row: the FIRST index of the minimum Jaccard distance
    ``(u - i) / u`` (0 where ``u == 0``), i.e. `sklearn.metrics.pairwise_distances_argmin(..., metric="jaccard")`
    as the reference's `BitBirch.predict` calls it (sklearn.py:136) - on packed rows, on the device.

    Returns int32 indices; with ``return_counts`` also the winning pair's exact uint32 intersection and union.
    Device tensors in -> device tensors out, on the current stream; host queries larger than a slab
    (`BBHIP_SLAB_KB`) are staged slab by slab, so a memory-mapped file of any size can be assigned."""
    lib = _lib.load()
    q, nq, nb, q_stride, c, nc = _assign_operands(queries, centroids)
    if _is_dev(q):
        import torch

        dev = q.device  # type: ignore[attr-defined]
        if not _is_dev(c):
            c = torch.from_numpy(c).to(dev)
        idx_t = torch.empty(nq, dtype=torch.int32, device=dev)
        cnt_t = torch.empty((2, nq), dtype=torch.int32, device=dev) if return_counts else None
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.bbh_jt_assign(_lib.ptr(q), nq, q_stride, _lib.ptr(c), nc, nb, _lib.ptr(idx_t),
                                     int(cnt_t[0].data_ptr()) if cnt_t is not None else None,
                                     int(cnt_t[1].data_ptr()) if cnt_t is not None else None, st))
        return (idx_t, cnt_t[0], cnt_t[1]) if cnt_t is not None else idx_t
    idx = np.empty(nq, dtype=np.int32)
    inter = np.empty(nq, dtype=np.uint32) if return_counts else None
    union = np.empty(nq, dtype=np.uint32) if return_counts else None
    slab = _slab_rows(nb)
    cdev: object = c
    if nq > slab and not _is_dev(c):  # several calls: the centroids are staged once
        import torch

        cdev = torch.from_numpy(c).cuda()
    for lo in range(0, nq, slab):
        hi = min(nq, lo + slab)
        part = q[lo:hi]  # type: ignore[index]
        _lib.check(lib.bbh_jt_assign(part.ctypes.data, hi - lo, q_stride, _lib.ptr(cdev), nc, nb,
                                     idx[lo:hi].ctypes.data,
                                     inter[lo:hi].ctypes.data if inter is not None else None,
                                     union[lo:hi].ctypes.data if union is not None else None, None))
    return (idx, inter, union) if return_counts else idx


def jt_dist_matrix_packed(queries: object, centroids: object):  # type: ignore[no-untyped-def]
    r"""The ``nq x nc`` float64 Jaccard distances ``(u - i) / u`` (one division of exact integers, 0.0 where
    ``u == 0``): bit for bit `sklearn.metrics.pairwise_distances(..., metric="jaccard")` on the unpacked rows, which
    is what the reference's `BitBirch.transform` returns (sklearn.py:153).  Device in -> device out."""
    lib = _lib.load()
    q, nq, nb, q_stride, c, nc = _assign_operands(queries, centroids)
    if _is_dev(q):
        import torch

        dev = q.device  # type: ignore[attr-defined]
        if not _is_dev(c):
            c = torch.from_numpy(c).to(dev)
        out_t = torch.empty((nq, nc), dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.bbh_jt_dist_matrix(_lib.ptr(q), nq, q_stride, _lib.ptr(c), nc, nb, _lib.ptr(out_t), st))
        return out_t
    out = np.empty((nq, nc), dtype=np.float64)
    slab = _slab_rows(max(nb, nc * 8))
    cdev = c
    if nq > slab and not _is_dev(c):
        import torch

        cdev = torch.from_numpy(c).cuda()
    for lo in range(0, nq, slab):
        hi = min(nq, lo + slab)
        _lib.check(lib.bbh_jt_dist_matrix(q[lo:hi].ctypes.data, hi - lo, q_stride, _lib.ptr(cdev), nc, nb,  # type: ignore[index]
                                          out[lo:hi].ctypes.data, None))
    return out


def _topk_check_k(k: object, nc: int, excluding: bool) -> int:
    r"""The limits of `bbh_jt_topk`, checked before the library is called."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"k must be an integer, got {type(k).__name__}")
    k = int(k)
    if k < 1 or k > _lib.BBH_TOPK_MAX:
        raise ValueError(f"k = {k}: need 1 <= k <= BBH_TOPK_MAX = {_lib.BBH_TOPK_MAX}")
    most = nc - 1 if excluding else nc
    if k > most:
        raise ValueError(f"k = {k} neighbours asked of nc = {nc} rows" + (", each query excluding one" if excluding else ""))
    return k


def jt_topk_packed(queries: object, rows: object, k: int, exclude: object = None, return_counts: bool = False):  # type: ignore[no-untyped-def]
    r"""The ``k`` nearest rows of ``rows`` for every packed query row, best first: ``(idx int32 (nq, k), dist float64
    (nq, k))``, equal to ``np.argsort(d, axis=1, kind="stable")[:, :k]`` of ``d = jt_dist_matrix_packed(queries, rows)``
    and the values of ``d`` there - without the ``nq x nc`` matrix.  The order is `jt_assign_packed`'s (``k = 1`` is its
    answer), decided on the exact integer counts.  ``dist`` is ``(u - i) / u`` as one float64 division of those counts,
    0.0 where ``u == 0``; with ``return_counts`` the uint32 intersections and unions follow.

    ``exclude``: optional, one row number per query that this query skips (a value outside ``[0, nc)`` skips nothing);
    ``jt_topk_packed(c, c, k, exclude=np.arange(len(c)))`` is the neighbour graph of a table.  ``1 <= k <= 64``
    (``BBH_TOPK_MAX``) and ``k <= nc`` (``nc - 1`` with ``exclude``), else `ValueError`.

    Device tensors in -> device tensors out, on the current stream; host queries larger than a slab (`BBHIP_SLAB_KB`) are
    staged slab by slab with the table staged once."""
    q, nq, nb, q_stride, c, nc = _assign_operands(queries, rows)
    k = _topk_check_k(k, nc, exclude is not None)
    if exclude is not None and not _is_dev(exclude):
        exclude = np.ascontiguousarray(exclude)
        if exclude.ndim != 1 or exclude.dtype.kind not in "iu" or exclude.shape[0] != nq:
            raise ValueError("exclude must hold one integer row number per query")
        exclude = np.clip(exclude, -1, nc).astype(np.int32)
    elif exclude is not None:
        if exclude.dim() != 1 or int(exclude.shape[0]) != nq or str(exclude.dtype) not in ("torch.int32", "torch.int64"):  # type: ignore[attr-defined]
            raise ValueError("exclude must hold one integer row number per query")
    lib = _lib.load()
    if _is_dev(q):
        import torch

        dev = q.device  # type: ignore[attr-defined]
        if not _is_dev(c):
            c = torch.from_numpy(c).to(dev)
        ex_t = None
        if exclude is not None:
            ex_t = torch.from_numpy(exclude).to(dev) if not _is_dev(exclude) else exclude.clamp(-1, nc).to(torch.int32).contiguous()  # type: ignore[attr-defined]
        idx_t = torch.empty((nq, k), dtype=torch.int32, device=dev)
        cnt_t = torch.empty((2, nq, k), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.bbh_jt_topk(_lib.ptr(q), nq, q_stride, _lib.ptr(c), nc, nb, k, _lib.ptr(ex_t), _lib.ptr(idx_t),
                                   int(cnt_t[0].data_ptr()), int(cnt_t[1].data_ptr()), st))
        i_t, u_t = cnt_t[0], cnt_t[1]
        dist_t = torch.where(u_t == 0, 0.0, (u_t - i_t).double() / u_t.double())
        return (idx_t, dist_t, i_t.view(torch.uint32), u_t.view(torch.uint32)) if return_counts else (idx_t, dist_t)
    if _is_dev(exclude):
        exclude = exclude.clamp(-1, nc).to("cpu").numpy().astype(np.int32)  # type: ignore[attr-defined]
    idx = np.empty((nq, k), dtype=np.int32)
    inter = np.empty((nq, k), dtype=np.uint32)
    union = np.empty((nq, k), dtype=np.uint32)
    slab = _slab_rows(nb)
    cdev: object = c
    if nq > slab and not _is_dev(c):  # several calls: the table is staged once
        import torch

        cdev = torch.from_numpy(c).cuda()
    for lo in range(0, nq, slab):
        hi = min(nq, lo + slab)
        part = q[lo:hi]  # type: ignore[index]
        _lib.check(lib.bbh_jt_topk(part.ctypes.data, hi - lo, q_stride, _lib.ptr(cdev), nc, nb, k,
                                   exclude[lo:hi].ctypes.data if exclude is not None else None,
                                   idx[lo:hi].ctypes.data, inter[lo:hi].ctypes.data, union[lo:hi].ctypes.data, None))
    u64, i64 = union.astype(np.int64), inter.astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.where(u64 == 0, 0.0, (u64 - i64).astype(np.float64) / u64.astype(np.float64))
    return (idx, dist, inter, union) if return_counts else (idx, dist)


def _radius_check(radius: object) -> float:
    r"""A real number that is not NaN, checked before the library is called."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise TypeError(f"radius must be a real number, got {type(radius).__name__}")
    r = float(radius)
    if r != r:
        raise ValueError("radius is NaN")
    return r


def _radius_first_capacity(nq: int, nc: int) -> int:
    r"""Entries the first `bbh_jt_radius` call of a slab has room for: 32 per query and at least 4096, never more than
    all pairs.  Radius queries on fingerprints usually return a few rows per query, and 32 entries cost 384 bytes of
    outputs per query; an answer that does not fit costs a second call, at about twice the time."""
    return min(nq * nc, max(4096, 32 * nq))


def jt_radius_packed(queries: object, rows: object, radius: float, exclude: object = None, return_counts: bool = False,  # type: ignore[no-untyped-def]
                     sort: bool = False):
    r"""Every row of ``rows`` within Jaccard distance ``radius`` of every packed query row, as CSR: ``(offsets int64
    (nq + 1,), idx int32 (total,), dist float64 (total,))``; query ``q``'s hits are ``idx[offsets[q]:offsets[q + 1]]``,
    equal to ``np.flatnonzero(d[q] <= radius)`` of ``d = jt_dist_matrix_packed(queries, rows)`` and in that (ascending)
    order - without the ``nq x nc`` matrix.  A pair at ``radius`` bit for bit is a hit; ``radius < 0`` gives nothing,
    ``radius >= 1`` every row.  ``dist`` is ``(u - i) / u`` as one float64 division of the exact counts, 0.0 where
    ``u == 0``; with ``return_counts`` the uint32 intersections and unions follow.

    ``exclude``: optional, one row number per query that this query skips (a value outside ``[0, nc)`` skips nothing);
    ``jt_radius_packed(c, c, r, exclude=np.arange(len(c)))`` is the threshold graph of a table.  ``sort=True`` orders every
    query's hits by (distance, row number) instead: its first ``k`` entries are then `jt_topk_packed`'s.

    Device tensors in -> device tensors out, on the current stream (the call synchronises it: the size of the answer
    decides what is allocated).  Host queries go slab by slab (`BBHIP_SLAB_KB`) with the table staged once.  Every slab
    takes one library call when the answer fits the first capacity (`_radius_first_capacity`: 32 entries per query, at
    least 4096), else a second one at the exact size."""
    q, nq, nb, q_stride, c, nc = _assign_operands(queries, rows)
    radius = _radius_check(radius)
    if exclude is not None and not _is_dev(exclude):
        exclude = np.ascontiguousarray(exclude)
        if exclude.ndim != 1 or exclude.dtype.kind not in "iu" or exclude.shape[0] != nq:
            raise ValueError("exclude must hold one integer row number per query")
        exclude = np.clip(exclude, -1, nc).astype(np.int32)
    elif exclude is not None:
        if exclude.dim() != 1 or int(exclude.shape[0]) != nq or str(exclude.dtype) not in ("torch.int32", "torch.int64"):  # type: ignore[attr-defined]
            raise ValueError("exclude must hold one integer row number per query")
    lib = _lib.load()
    total = np.zeros(1, dtype=np.int64)
    if _is_dev(q):
        import torch

        dev = q.device  # type: ignore[attr-defined]
        if not _is_dev(c):
            c = torch.from_numpy(c).to(dev)
        ex_t = None
        if exclude is not None:
            ex_t = torch.from_numpy(exclude).to(dev) if not _is_dev(exclude) else exclude.clamp(-1, nc).to(torch.int32).contiguous()  # type: ignore[attr-defined]
        off_t = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        cap = _radius_first_capacity(nq, nc)
        while True:
            idx_t = torch.empty(cap, dtype=torch.int32, device=dev)
            cnt_t = torch.empty((2, cap), dtype=torch.int32, device=dev)
            _lib.check(lib.bbh_jt_radius(_lib.ptr(q), nq, q_stride, _lib.ptr(c), nc, nb, radius, _lib.ptr(ex_t), cap,
                                         _lib.ptr(off_t), total.ctypes.data, _lib.ptr(idx_t) if cap else None,
                                         int(cnt_t[0].data_ptr()) if cap else None, int(cnt_t[1].data_ptr()) if cap else None, st))
            n = int(total[0])
            if n <= cap:
                break
            cap = n
        idx_t, i_t, u_t = idx_t[:n], cnt_t[0, :n], cnt_t[1, :n]
        dist_t = torch.where(u_t == 0, 0.0, (u_t - i_t).double() / u_t.double())
        if sort and n:
            seg = torch.repeat_interleave(torch.arange(nq, device=dev), off_t[1:] - off_t[:-1])
            o1 = torch.sort(dist_t, stable=True).indices
            order = o1[torch.sort(seg[o1], stable=True).indices]
            idx_t, dist_t, i_t, u_t = idx_t[order], dist_t[order], i_t[order], u_t[order]
        return (off_t, idx_t, dist_t, i_t.view(torch.uint32), u_t.view(torch.uint32)) if return_counts else (off_t, idx_t, dist_t)
    if _is_dev(exclude):
        exclude = exclude.clamp(-1, nc).to("cpu").numpy().astype(np.int32)  # type: ignore[attr-defined]
    slab = _slab_rows(nb)
    cdev: object = c
    if nq > slab and not _is_dev(c):  # several calls: the table is staged once
        import torch

        cdev = torch.from_numpy(c).cuda()
    offsets = np.zeros(nq + 1, dtype=np.int64)
    parts: list[tuple[np.ndarray, np.ndarray, np.ndarray]] = []
    for lo in range(0, nq, slab):
        hi = min(nq, lo + slab)
        part = q[lo:hi]  # type: ignore[index]
        off = np.empty(hi - lo + 1, dtype=np.int64)
        cap = _radius_first_capacity(hi - lo, nc)
        while True:
            out = np.empty((3, cap), dtype=np.uint32)
            _lib.check(lib.bbh_jt_radius(part.ctypes.data, hi - lo, q_stride, _lib.ptr(cdev), nc, nb, radius,
                                         exclude[lo:hi].ctypes.data if exclude is not None else None, cap, off.ctypes.data,
                                         total.ctypes.data, out[0].ctypes.data if cap else None,
                                         out[1].ctypes.data if cap else None, out[2].ctypes.data if cap else None, None))
            n = int(total[0])
            if n <= cap:
                break
            cap = n
        offsets[lo + 1:hi + 1] = offsets[lo] + off[1:]
        parts.append((out[0, :n].view(np.int32), out[1, :n], out[2, :n]))
    if parts:
        idx, inter, union = (np.concatenate([p[j] for p in parts]) for j in range(3))
    else:
        idx, inter, union = np.empty(0, np.int32), np.empty(0, np.uint32), np.empty(0, np.uint32)
    u64, i64 = union.astype(np.int64), inter.astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.where(u64 == 0, 0.0, (u64 - i64).astype(np.float64) / u64.astype(np.float64))
    if sort and len(idx):
        order = np.lexsort((dist, np.repeat(np.arange(nq), np.diff(offsets))))  # stable: equal distances keep the index order
        idx, dist, inter, union = idx[order], dist[order], inter[order], union[order]
    return (offsets, idx, dist, inter, union) if return_counts else (offsets, idx, dist)


def jt_components_packed(rows: object, radius: float, return_roots: bool = False):  # type: ignore[no-untyped-def]
    r"""The connected components of a packed table at Jaccard distance ``radius``: ``(labels, n_components)``.  Rows ``a``
    and ``b`` are linked iff ``jt_radius_packed(rows, rows, radius)`` reports the pair (``(u - i) / u <= radius`` as one
    float64 division, 0.0 where ``u == 0``; a pair at ``radius`` bit for bit is linked); components are the transitive
    closure, i.e. single-linkage clustering cut at ``radius``.  ``labels[v]`` is the rank of the component's first row
    among the first rows of all components, which is the labelling of
    ``scipy.sparse.csgraph.connected_components(d <= radius, directed=False)`` - without the graph: no edge is stored.
    With ``return_roots`` the first row of every row's component follows.  ``radius = 0`` groups duplicates, ``radius < 0``
    leaves every row alone, ``radius >= 1`` gives one component.

    NumPy rows -> int64 NumPy labels (and roots); a device tensor -> device tensors, int32 as `jt_topk_packed`'s indices,
    on the current stream (the call synchronises it)."""
    radius = _radius_check(radius)
    if not _is_dev(rows):
        arr = np.asarray(rows)
        if arr.ndim == 2 and arr.dtype != np.uint8:
            raise TypeError(f"rows must be packed uint8, got {arr.dtype}")
    elif str(rows.dtype) != "torch.uint8":  # type: ignore[attr-defined]
        raise TypeError(f"rows must be packed uint8, got {rows.dtype}")  # type: ignore[attr-defined]
    c, n, nb, stride = _u8_2d(rows, "rows")
    if nb < 1:
        raise RuntimeError("rows must have at least one byte per row")
    if n >= 2 ** 31:
        raise ValueError(f"{n} rows: need fewer than 2^31")
    lib = _lib.load()
    count = np.zeros(1, dtype=np.int64)
    if _is_dev(c):
        import torch

        if stride != nb:
            c = c.contiguous()  # type: ignore[attr-defined]
        dev = c.device  # type: ignore[attr-defined]
        out_t = torch.empty((2, n), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.bbh_jt_components(_lib.ptr(c), n, nb, radius, int(out_t[0].data_ptr()) if return_roots and n else None,
                                         int(out_t[1].data_ptr()) if n else None, count.ctypes.data, st))
        return (out_t[1], int(count[0]), out_t[0]) if return_roots else (out_t[1], int(count[0]))
    out = np.empty((2, n), dtype=np.int32)
    _lib.check(lib.bbh_jt_components(c.ctypes.data, n, nb, radius, out[0].ctypes.data if return_roots and n else None,  # type: ignore[attr-defined]
                                     out[1].ctypes.data if n else None, count.ctypes.data, None))
    labels = out[1].astype(np.int64)
    return (labels, int(count[0]), out[0].astype(np.int64)) if return_roots else (labels, int(count[0]))


def _leaders_weights(weights: object, n: int) -> object:
    r"""Weights of `jt_leaders_packed`, checked before the library is called: ``n`` integers in ``[0, 2^32)``.  Host values
    come back as a contiguous uint32 array; a device tensor (int32 or int64, one reduction checks the range) as the int32
    tensor that holds the same 32 bits."""
    if _is_dev(weights):
        import torch

        if weights.dim() != 1 or int(weights.shape[0]) != n:  # type: ignore[attr-defined]
            raise ValueError(f"weights must hold one integer per row ({n})")
        if weights.dtype not in (torch.int32, torch.int64):  # type: ignore[attr-defined]
            raise TypeError(f"weights on the device must be int32 or int64, got {weights.dtype}")  # type: ignore[attr-defined]
        if n:
            lo, hi = (int(v) for v in torch.aminmax(weights))  # type: ignore[call-overload]
            if lo < 0 or hi >= 2 ** 32:
                raise ValueError("weights must lie in [0, 2^32)")
        if weights.dtype == torch.int64:  # type: ignore[attr-defined]
            weights = weights.contiguous().view(torch.int32)[::2]  # type: ignore[attr-defined]  # (the low words: little endian)
        return weights.contiguous()  # type: ignore[attr-defined]
    arr = np.asarray(weights)
    if arr.ndim != 1 or arr.shape[0] != n:
        raise ValueError(f"weights must hold one integer per row ({n})")
    if arr.dtype.kind not in "iu":
        raise TypeError(f"weights must be integers, got {arr.dtype}")
    if n and (int(arr.min()) < 0 or int(arr.max()) >= 2 ** 32):
        raise ValueError("weights must lie in [0, 2^32)")
    return np.ascontiguousarray(arr.astype(np.uint32))


def jt_leaders_packed(rows: object, radius: float, weights: object = None, ties: str = "low", return_centres: bool = False,  # type: ignore[no-untyped-def]
                      return_density: bool = False):
    r"""Leader clustering (sphere exclusion, Taylor-Butina) of a packed table at Jaccard distance ``radius``:
    ``(labels, n_clusters[, centres][, density])``.  Rows ``a != b`` are neighbours iff ``jt_radius_packed(rows, rows,
    radius)`` reports the pair (``(u - i) / u <= radius`` as one float64 division, 0.0 where ``u == 0``; a pair at
    ``radius`` bit for bit is a neighbour pair).  ``density[a]`` is ``weights[a]`` plus the weights of ``a``'s neighbours
    (all 1 without ``weights``), exact.  The rows are walked in priority order - the higher density first, among equal
    densities the lower row first (``ties="high"``: the higher row) - and a row that is not yet taken becomes a centre
    and takes all of its neighbours that are not yet taken; densities are never recomputed.  So every member is within
    ``radius`` of its centre and no two centres are within ``radius`` of each other - without the graph: no edge is stored.

    ``labels[v]`` is the rank of ``v``'s centre among the centres in ascending row index (`jt_components_packed`'s rule);
    ``centres[v]`` is the row index of ``v``'s centre, a centre names itself.  The order in which the sequential procedure
    creates the clusters is the centres sorted by ``(-density, row)`` (``ties="high"``: ``(-density, -row)``).
    ``radius = 0`` groups duplicates, ``radius < 0`` leaves every row alone, ``radius >= 1`` gives one cluster.

    ``weights``: optional, one integer in ``[0, 2^32)`` per row; 0 is allowed.  NumPy rows -> int64 NumPy labels and
    centres, uint64 density; a device tensor -> int32 device labels and centres, int64 device density, on the current
    stream (the call synchronises it).  Device weights are int32 or int64."""
    radius = _radius_check(radius)
    if ties not in ("low", "high"):
        raise ValueError(f'ties must be "low" or "high", got {ties!r}')
    if not _is_dev(rows):
        arr = np.asarray(rows)
        if arr.ndim == 2 and arr.dtype != np.uint8:
            raise TypeError(f"rows must be packed uint8, got {arr.dtype}")
    elif str(rows.dtype) != "torch.uint8":  # type: ignore[attr-defined]
        raise TypeError(f"rows must be packed uint8, got {rows.dtype}")  # type: ignore[attr-defined]
    c, n, nb, stride = _u8_2d(rows, "rows")
    if nb < 1:
        raise RuntimeError("rows must have at least one byte per row")
    if n >= 2 ** 31:
        raise ValueError(f"{n} rows: need fewer than 2^31")
    if weights is not None:
        weights = _leaders_weights(weights, n)
    flags = _lib.BBH_LEADERS_TIES_HIGH if ties == "high" else 0
    lib = _lib.load()
    count = np.zeros(1, dtype=np.int64)
    if _is_dev(c):
        import torch

        if stride != nb:
            c = c.contiguous()  # type: ignore[attr-defined]
        dev = c.device  # type: ignore[attr-defined]
        if weights is not None and not _is_dev(weights):
            weights = torch.from_numpy(weights.view(np.int32)).to(dev)
        out_t = torch.empty((2, n), dtype=torch.int32, device=dev)
        dens_t = torch.empty(n, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.bbh_jt_leaders(_lib.ptr(c), n, nb, radius, _lib.ptr(weights) if n else None, flags,
                                      int(out_t[0].data_ptr()) if return_centres and n else None,
                                      int(out_t[1].data_ptr()) if n else None, count.ctypes.data,
                                      int(dens_t.data_ptr()) if return_density and n else None, st))
        res: tuple = (out_t[1], int(count[0]))
        if return_centres:
            res += (out_t[0],)
        if return_density:
            res += (dens_t,)
        return res
    out = np.empty((2, n), dtype=np.int32)
    dens = np.empty(n, dtype=np.uint64)
    _lib.check(lib.bbh_jt_leaders(c.ctypes.data, n, nb, radius, _lib.ptr(weights) if n else None, flags,  # type: ignore[attr-defined]
                                  out[0].ctypes.data if return_centres and n else None, out[1].ctypes.data if n else None,
                                  count.ctypes.data, dens.ctypes.data if return_density and n else None, None))
    res = (out[1].astype(np.int64), int(count[0]))
    if return_centres:
        res += (out[0].astype(np.int64),)
    if return_density:
        res += (dens,)
    return res


def jt_sim_matrix_packed(arr: NDArray[np.uint8]) -> NDArray[np.float64]:
    r"""All-pairs Tanimoto matrix (similarity.py:239-247): one batched kernel instead of
    N sequential arr-vec calls; the diagonal is 1 as in the reference."""
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    _, _, _, sims = jt_best_match_packed(a, a, return_sims=True)
    assert sims is not None
    np.fill_diagonal(sims, 1.0)
    return sims


# ---------------------------------------------------------- pack / unpack ---------
def _unpack_fingerprints_hip(a: NDArray[np.uint8], n_features: int | None = None) -> NDArray[np.uint8]:
    r"""`_cpp_similarity.unpack_fingerprints` (similarity.cpp:204-214)."""
    lib = _lib.load()
    arr = np.ascontiguousarray(a, dtype=np.uint8)
    if arr.ndim not in (1, 2):
        raise RuntimeError("Input array must be 1- or 2-dimensional")
    two = arr.reshape(1, -1) if arr.ndim == 1 else arr
    n, nb = two.shape
    nf = nb * 8 if n_features is None else int(n_features)
    if nf % 8 != 0:
        raise RuntimeError("Only n_features divisible by 8 is supported")
    out = np.empty((n, nf), dtype=np.uint8)
    _lib.check(lib.bbh_unpack(two.ctypes.data, n, nb, nf, out.ctypes.data, None))
    return out[0] if arr.ndim == 1 else out


# --------------------------------------------------- linear sums and centroids ----
def _add_rows(arr: NDArray[np.uint8]) -> NDArray[np.uint64]:
    r"""Column sums (similarity.cpp:381-400)."""
    lib = _lib.load()
    a = np.asarray(arr)
    if a.ndim != 2:
        raise RuntimeError("Input array must be 2-dimensional")
    a = np.ascontiguousarray(a, dtype=np.uint8)
    out = np.empty(a.shape[1], dtype=np.uint64)
    _lib.check(lib.bbh_add_rows(a.ctypes.data, a.shape[0], a.shape[1], 0, a.shape[1], out.ctypes.data, None))
    return out


def _as_uint_ls(linear_sum: NDArray[np.integer]) -> NDArray[np.integer]:
    ls = np.ascontiguousarray(linear_sum)
    if ls.dtype.kind == "u" and ls.dtype.itemsize in (1, 2, 4, 8):
        return ls
    return ls.astype(np.uint64)  # pybind11 forcecast (similarity.cpp:48-50)


def centroid_from_sum(
    linear_sum: NDArray[np.integer], n_samples: int, *, pack: bool = True
) -> NDArray[np.uint8]:
    r"""Majority-vote centroid from a linear sum (_py_similarity.py:12-42,
    similarity.cpp:216-271): ``n<=1`` -> cast, else bit = ``ls >= n*0.5``."""
    lib = _lib.load()
    ls = _as_uint_ls(linear_sum)
    if ls.ndim != 1:
        raise RuntimeError("linear_sum must be 1-dimensional")
    nf = ls.shape[0]
    out = np.empty((nf + 7) // 8 if pack else nf, dtype=np.uint8)
    _lib.check(
        lib.bbh_centroid_from_sum(ls.ctypes.data, ls.dtype.itemsize, nf, int(n_samples), int(pack),
                                  out.ctypes.data, None)
    )
    return out


def centroid(
    fps: NDArray[np.uint8],
    input_is_packed: bool = True,
    n_features: int | None = None,
    *,
    pack: bool = True,
) -> NDArray[np.uint8]:
    r"""Majority-vote centroid of a set of fingerprints (_py_similarity.py:45-62)."""
    lib = _lib.load()
    a = np.ascontiguousarray(fps, dtype=np.uint8)
    nf = (a.shape[1] * 8 if n_features is None else n_features) if input_is_packed else a.shape[1]
    ls = np.empty(nf, dtype=np.uint64)
    _lib.check(lib.bbh_add_rows(a.ctypes.data, a.shape[0], a.shape[1], int(input_is_packed), nf, ls.ctypes.data, None))
    return centroid_from_sum(ls, len(a), pack=pack)


# ------------------------------------------------------------------- iSIM ---------
def jt_isim_from_sum(linear_sum: NDArray[np.integer], n_objects: int) -> float:
    r"""iSIM Tanimoto from a column sum (similarity.cpp:273-301): exact u64 moments,
    then ``a=(q-s)/2.0; a/((a+n*s)-q)`` in IEEE f64.  ``n_objects < 2`` warns and
    returns NaN (similarity.cpp:275-279)."""
    lib = _lib.load()
    ls = _as_uint_ls(linear_sum)
    if ls.ndim != 1:
        raise RuntimeError("linear_sum must be a 1D array")
    out = C.c_double(0.0)
    warn = C.c_int(0)
    _lib.check(
        lib.bbh_isim_from_sum(ls.ctypes.data, ls.dtype.itemsize, ls.shape[0], int(n_objects),
                              C.byref(out), C.byref(warn), None)
    )
    if warn.value:
        warnings.warn(
            f"Invalid n_objects = {n_objects} in isim. Expected n_objects >= 2",
            RuntimeWarning,
            stacklevel=2,
        )
    return float(out.value)


def _isim_rows(arr: NDArray[np.integer], packed: bool, n_features: int | None) -> float:
    lib = _lib.load()
    a = np.asarray(arr)
    if a.dtype != np.uint8:
        # the reference sums wider dtypes with NumPy first (similarity.py:67-90)
        u = unpack_fingerprints(a.astype(np.uint8), n_features) if packed else a
        return jt_isim_from_sum(np.sum(u, axis=0, dtype=np.uint64), len(a))
    a = np.ascontiguousarray(a)
    nf = (a.shape[1] * 8 if n_features is None else n_features) if packed else a.shape[1]
    out = C.c_double(0.0)
    warn = C.c_int(0)
    _lib.check(lib.bbh_isim_rows(a.ctypes.data, a.shape[0], a.shape[1], int(packed), nf,
                                 C.byref(out), C.byref(warn), None))
    if warn.value:
        warnings.warn(
            f"Invalid n_objects = {len(a)} in isim. Expected n_objects >= 2",
            RuntimeWarning,
            stacklevel=3,
        )
    return float(out.value)


def jt_isim_unpacked(arr: NDArray[np.integer]) -> float:
    return _isim_rows(arr, False, None)


def jt_isim_packed(arr: NDArray[np.integer], n_features: int | None = None) -> float:
    return _isim_rows(arr, True, n_features)


def jt_isim(fps: NDArray[np.integer], input_is_packed: bool = True, n_features: int | None = None) -> float:
    r"""Average Tanimoto of a set via iSIM (similarity.py:106-140)."""
    if input_is_packed:
        return jt_isim_packed(fps, n_features)
    return jt_isim_unpacked(fps)


def _sum_rows_u64(arr: NDArray[np.integer], input_is_packed: bool, n_features: int | None) -> NDArray[np.uint64]:
    lib = _lib.load()
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    nf = (a.shape[1] * 8 if n_features is None else n_features) if input_is_packed else a.shape[1]
    ls = np.empty(nf, dtype=np.uint64)
    _lib.check(lib.bbh_add_rows(a.ctypes.data, a.shape[0], a.shape[1], int(input_is_packed), nf, ls.ctypes.data, None))
    return ls


def jt_isim_radius_compl_from_sum(ls: NDArray[np.integer], n: int) -> float:
    r"""1 - radius (similarity.py:192-202)."""
    cen = centroid_from_sum(ls, n, pack=False)
    ls_1 = np.add(ls, cen, dtype=np.uint64)
    jt = jt_isim_from_sum(ls, n)
    jt_1 = jt_isim_from_sum(ls_1, n + 1)
    return (jt_1 * (n + 1) - jt * (n - 1)) / 2


def jt_isim_radius_from_sum(ls: NDArray[np.integer], n: int) -> float:
    return 1 - jt_isim_radius_compl_from_sum(ls, n)


def jt_isim_diameter_from_sum(ls: NDArray[np.integer], n: int) -> float:
    return 1 - jt_isim_from_sum(ls, n)


def jt_isim_diameter(arr: NDArray[np.integer], input_is_packed: bool = True, n_features: int | None = None) -> float:
    return jt_isim_diameter_from_sum(_sum_rows_u64(arr, input_is_packed, n_features), len(arr))


def jt_isim_radius(arr: NDArray[np.integer], input_is_packed: bool = True, n_features: int | None = None) -> float:
    return jt_isim_radius_from_sum(_sum_rows_u64(arr, input_is_packed, n_features), len(arr))


def jt_isim_radius_compl(arr: NDArray[np.integer], input_is_packed: bool = True, n_features: int | None = None) -> float:
    return jt_isim_radius_compl_from_sum(_sum_rows_u64(arr, input_is_packed, n_features), len(arr))


# ------------------------------------------------------------ split primitive -----
def jt_most_dissimilar_packed(
    Y: NDArray[np.uint8], n_features: int | None = None
) -> tuple[int, int, NDArray[np.float64], NDArray[np.float64]]:
    r"""The node-split primitive (similarity.cpp:413-471): majority centroid of Y, the
    row least similar to it (fp_1), the row least similar to fp_1 (fp_2), and the
    similarities of all rows to both.  First index wins ties."""
    lib = _lib.load()
    y = np.asarray(Y)
    if y.ndim != 2:
        raise RuntimeError("Input array must be 2-dimensional")
    y = np.ascontiguousarray(y, dtype=np.uint8)
    n, nb = y.shape
    nf = nb * 8 if n_features is None else int(n_features)
    i1, i2 = C.c_int64(0), C.c_int64(0)
    s1 = np.empty(n, dtype=np.float64)
    s2 = np.empty(n, dtype=np.float64)
    _lib.check(lib.bbh_most_dissimilar(y.ctypes.data, n, nb, nf, C.byref(i1), C.byref(i2),
                                       s1.ctypes.data, s2.ctypes.data, None))
    return int(i1.value), int(i2.value), s1, s2


# ---------------------------------------------------- analysis-side composites ----
def _seg_fits(n_features: int, largest: int) -> bool:
    r"""The exact uint64 moments of a set of `largest` rows fit (bbhip.h, bbh_compl_isim_segments)."""
    return largest < 2**31 and n_features * largest * largest < 2**63


def _seg_host_index(a: object, what: str) -> NDArray[np.int64]:
    arr = np.asarray(a)
    if arr.ndim != 1 or arr.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a 1-dimensional integer array")
    return np.ascontiguousarray(arr, dtype=np.int64)


class _SegArgs(tp.NamedTuple):
    r"""The checked arguments of a segmented call (`jt_compl_isim_segments`, `jt_cluster_stats_segments`)."""

    rows: tp.Any      # 2-D uint8 rows, NumPy or device tensor
    n_rows: int
    nb: int
    stride: int
    nf: int
    off: tp.Any       # int64 offsets, NumPy or device tensor
    k: int
    mem: tp.Any       # int64 members, NumPy or device tensor, or None
    total: int        # offsets[-1]
    on_device: bool   # the call runs on device tensors and the current stream


def _seg_args(fps, offsets, members, n_features) -> _SegArgs:  # type: ignore[no-untyped-def]
    dev = _is_dev(fps)
    if dev:
        if fps.dim() != 2 or str(fps.dtype) != "torch.uint8" or fps.stride(1) != 1:
            raise ValueError("fps must be a 2-dimensional uint8 array of packed rows")
        rows, n_rows, nb, stride = fps, int(fps.shape[0]), int(fps.shape[1]), int(fps.stride(0))
    else:
        rows = np.asarray(fps)
        if rows.ndim != 2 or rows.dtype != np.uint8:
            raise ValueError("fps must be a 2-dimensional uint8 array of packed rows")
        if rows.shape[0] and (rows.strides[1] != 1 or rows.strides[0] < rows.shape[1]):
            rows = np.ascontiguousarray(rows)
        n_rows, nb = rows.shape
        stride = int(rows.strides[0]) if n_rows else nb
    nf = nb * 8 if n_features is None else int(n_features)
    if nf <= 0 or nf % 8 != 0 or nf > nb * 8:
        raise ValueError("Only n_features divisible by 8 (and within the packed width) is supported")
    off_dev = _is_dev(offsets)
    mem_dev = _is_dev(members)
    if off_dev:
        if offsets.dim() != 1 or str(offsets.dtype) != "torch.int64" or not offsets.is_contiguous():
            raise ValueError("offsets must be a contiguous 1-dimensional int64 tensor")
        off = offsets
        k = int(off.shape[0]) - 1
    else:
        off = _seg_host_index(offsets, "offsets")
        k = len(off) - 1
    if k < 1:
        raise ValueError("offsets must name at least one set")
    if mem_dev:
        if members.dim() != 1 or str(members.dtype) != "torch.int64" or not members.is_contiguous():
            raise ValueError("members must be a contiguous 1-dimensional int64 tensor")
        mem = members
        n_mem = int(mem.shape[0])
    elif members is not None:
        mem = _seg_host_index(members, "members")
        n_mem = len(mem)
        if n_mem and (int(mem.min()) < 0 or int(mem.max()) >= n_rows):
            raise ValueError("members must be row numbers of fps")
    else:
        mem, n_mem = None, n_rows
    if not off_dev:
        if off[0] != 0:
            raise ValueError("offsets must start at 0")
        sizes = np.diff(off)
        if (sizes < 0).any():
            raise ValueError("offsets must not decrease")
        if (sizes == 0).any():
            raise ValueError("Size of fingerprints set must be > 0")
        if int(off[-1]) > n_mem:
            raise ValueError("offsets name more rows than there are")
        if not _seg_fits(nf, int(sizes.max())):
            raise ValueError("a set is too large for exact 64-bit moments: n_features * m * m must stay below 2**63")
    on_device = dev or off_dev or mem_dev
    if on_device:
        if not dev:
            raise ValueError("offsets / members on the device need fps on the device")
        total = int(off[-1].item()) if off_dev else int(off[-1])
        if total < 0 or total > n_mem:
            raise ValueError("offsets name more rows than there are")
    else:
        total = int(off[-1])
    return _SegArgs(rows, n_rows, nb, stride, nf, off, k, mem, total, on_device)


def _seg_slabs(a: _SegArgs):  # type: ignore[no-untyped-def]
    r"""Host rows beyond a slab (`BBHIP_SLAB_KB`) as slabs of whole sets, a set larger than a slab a slab of its own, each
    gathered with one `take`: yields (g0, g1, lo, hi, contiguous rows of the sets g0 .. g1, their offsets from 0)."""
    g0 = 0
    slab = _slab_rows(a.nb)
    while g0 < a.k:
        g1 = int(np.searchsorted(a.off, a.off[g0] + slab, side="right")) - 1
        g1 = min(a.k, max(g1, g0 + 1))
        lo, hi = int(a.off[g0]), int(a.off[g1])
        part = np.ascontiguousarray(a.rows[lo:hi]) if a.mem is None else a.rows.take(a.mem[lo:hi], axis=0)
        yield g0, g1, lo, hi, part, np.ascontiguousarray(a.off[g0:g1 + 1] - lo)
        g0 = g1


def _seg_one_call(a: _SegArgs) -> bool:
    slab = _slab_rows(a.nb)
    return a.total <= slab and (a.mem is None or a.n_rows <= slab)


def jt_compl_isim_segments(fps, offsets, members=None, n_features=None, return_compl=True):  # type: ignore[no-untyped-def]
    r"""Complementary iSIM (`jt_compl_isim`) and medoid position (`jt_isim_medoid`) of ``k`` independent sets of packed
    rows in one call.  Set ``g`` is ``fps[offsets[g]:offsets[g + 1]]``, or ``fps[members[offsets[g]:offsets[g + 1]]]``
    when ``members`` is given.  Returns ``(positions, compl)``: int64 ``[k]``, the position INSIDE each set of the first
    minimum of its values (0 for sets of 1 or 2 rows), and float64 ``[offsets[-1]]`` in set order (NaN for sets of 1 or 2
    rows), or ``None`` with ``return_compl=False``.  Bit for bit the reference's values (_py_similarity.py:65-117).

    NumPy in -> NumPy out; device tensors in -> device tensors out, on the current stream.  Host rows beyond a slab
    (`BBHIP_SLAB_KB`) go through in slabs of whole sets, gathered on the host with one `take` per slab."""
    a = _seg_args(fps, offsets, members, n_features)
    rows, n_rows, nb, stride, nf, off, k, mem, total = a[:9]
    lib = _lib.load()
    if a.on_device:
        import torch

        d = rows.device
        med_t = torch.empty(k, dtype=torch.int64, device=d)
        compl_t = torch.empty(total, dtype=torch.float64, device=d) if return_compl else None
        st = torch.cuda.current_stream(d).cuda_stream
        _lib.check(lib.bbh_compl_isim_segments(_lib.ptr(rows), n_rows, nb, stride, _lib.ptr(mem), _lib.ptr(off), k, nf,
                                               _lib.ptr(compl_t), _lib.ptr(med_t), st))
        return med_t, compl_t
    med = np.empty(k, dtype=np.int64)
    compl = np.empty(total, dtype=np.float64) if return_compl else None
    if _seg_one_call(a):
        part = rows if mem is not None else rows[:total]
        _lib.check(lib.bbh_compl_isim_segments(part.ctypes.data, len(part), nb, stride, _lib.ptr(mem), off.ctypes.data, k, nf,
                                               _lib.ptr(compl), med.ctypes.data, None))
        return med, compl
    for g0, g1, lo, hi, part, sub in _seg_slabs(a):
        _lib.check(lib.bbh_compl_isim_segments(part.ctypes.data, hi - lo, nb, nb, None, sub.ctypes.data, g1 - g0, nf,
                                               compl[lo:hi].ctypes.data if compl is not None else None,
                                               med[g0:g1].ctypes.data, None))
    return med, compl


_STATS = ("centroids", "isim", "dist", "sums")


def jt_cluster_stats_segments(fps, offsets, members=None, n_features=None, centrals=None, want=("centroids", "isim", "dist")):  # type: ignore[no-untyped-def]
    r"""What the clustering indices (`bblean_amd.metrics`) need of ``k`` independent sets of packed rows, in one call.  The
    sets are given as for `jt_compl_isim_segments`.  Returns a dict with the entries named in ``want``:

    - ``"centroids"``: uint8 ``[k, n_features // 8]``, `centroid` of each set, packed
    - ``"isim"``: float64 ``[k]``, `jt_isim_packed` of each set (NaN for a set of one row, without a warning)
    - ``"dist"``: float64 ``[offsets[-1]]`` in set order, ``1 - jt_sim_packed(set, central)`` with the set's centroid as
      the central, or row ``g`` of ``centrals`` (``[k, >= n_features // 8]`` uint8) when given
    - ``"sums"``: uint64 ``[k, n_features]``, the column sums of each set

    Bit for bit what those functions give set by set.  NumPy in -> NumPy out; device tensors in -> device tensors out, on
    the current stream.  Host rows beyond a slab (`BBHIP_SLAB_KB`) go through in slabs of whole sets."""
    want = tuple(want)
    if not want or any(w not in _STATS for w in want):
        raise ValueError(f"want must name some of {_STATS}")
    a = _seg_args(fps, offsets, members, n_features)
    rows, n_rows, nb, stride, nf, off, k, mem, total = a[:9]
    cen, c_stride = None, 0
    if centrals is not None:
        if _is_dev(centrals):
            if not a.on_device:
                raise ValueError("centrals on the device need fps on the device")
            ok = centrals.dim() == 2 and str(centrals.dtype) == "torch.uint8" and centrals.stride(1) == 1
            cen = centrals
            c_stride = int(cen.stride(0)) if ok else 0
        else:
            cen = np.asarray(centrals)
            ok = cen.ndim == 2 and cen.dtype == np.uint8
            if ok:
                cen = np.ascontiguousarray(cen)
                c_stride = int(cen.shape[1])
        if not ok or int(cen.shape[0]) != k or int(cen.shape[1]) < nf // 8:
            raise ValueError("centrals must be a 2-dimensional uint8 array of one packed row per set")
    lib = _lib.load()
    shapes = {"centroids": ((k, nf // 8), "uint8"), "isim": ((k,), "float64"), "dist": ((total,), "float64"),
              "sums": ((k, nf), "uint64")}
    if a.on_device:
        import torch

        d = rows.device
        if cen is not None and not _is_dev(cen):
            cen = torch.from_numpy(cen).to(d)
        # (torch has no uint64 arithmetic, the column sums are handed out as int64: the same bits, and they are < 2^63)
        out_t = {w: torch.empty(shapes[w][0], dtype=getattr(torch, shapes[w][1].replace("uint64", "int64")), device=d)
                 for w in want}
        st = torch.cuda.current_stream(d).cuda_stream
        _lib.check(lib.bbh_cluster_stats_segments(_lib.ptr(rows), n_rows, nb, stride, _lib.ptr(mem), _lib.ptr(off), k, nf,
                                                  _lib.ptr(cen), c_stride, *(_lib.ptr(out_t.get(w)) for w in _STATS), st))
        return out_t
    out = {w: np.empty(shapes[w][0], dtype=shapes[w][1]) for w in want}
    if _seg_one_call(a):
        part = rows if mem is not None else rows[:total]
        _lib.check(lib.bbh_cluster_stats_segments(part.ctypes.data, len(part), nb, stride, _lib.ptr(mem), off.ctypes.data, k, nf,
                                                  _lib.ptr(cen), c_stride, *(_lib.ptr(out.get(w)) for w in _STATS), None))
        return out
    for g0, g1, lo, hi, part, sub in _seg_slabs(a):
        sl = {"centroids": slice(g0, g1), "isim": slice(g0, g1), "dist": slice(lo, hi), "sums": slice(g0, g1)}
        _lib.check(lib.bbh_cluster_stats_segments(part.ctypes.data, hi - lo, nb, nb, None, sub.ctypes.data, g1 - g0, nf,
                                                  cen[g0:g1].ctypes.data if cen is not None else None, c_stride,
                                                  *(out[w][sl[w]].ctypes.data if w in out else None for w in _STATS), None))
    return out


def _is_packed_u8(fps: object) -> bool:
    return isinstance(fps, np.ndarray) and fps.dtype == np.uint8 and fps.ndim == 2


def jt_compl_isim(fps: NDArray[np.uint8], input_is_packed: bool = True, n_features: int | None = None) -> NDArray[np.float64]:
    r"""Complementary iSIM of every row (_py_similarity.py:65-83).  Packed uint8 rows: one segmented call."""
    if input_is_packed and _is_packed_u8(fps):
        nf = fps.shape[1] * 8 if n_features is None else int(n_features)
        if len(fps) >= 3 and nf > 0 and nf % 8 == 0 and nf <= fps.shape[1] * 8 and _seg_fits(nf, len(fps)):
            return jt_compl_isim_segments(fps, np.array([0, len(fps)], dtype=np.int64), n_features=nf)[1]
    if input_is_packed:
        fps = unpack_fingerprints(fps, n_features)
    n_objects = len(fps) - 1
    if n_objects < 2:
        warnings.warn("Invalid fps. len(fps) must be >= 3", RuntimeWarning, stacklevel=2)
        return np.full(len(fps), fill_value=np.nan, dtype=np.float64)
    total = _sum_rows_u64(fps, False, None)
    return np.array([jt_isim_from_sum(total - fp, n_objects) for fp in fps], dtype=np.float64)


def jt_isim_medoid(fps: NDArray[np.uint8], input_is_packed: bool = True, n_features: int | None = None, pack: bool = True) -> tuple[int, NDArray[np.uint8]]:
    r"""(_py_similarity.py:91-117)"""
    if not fps.size:
        raise ValueError("Size of fingerprints set must be > 0")
    if input_is_packed and _is_packed_u8(fps):
        nf = fps.shape[1] * 8 if n_features is None else int(n_features)
        if len(fps) >= 3 and nf > 0 and nf % 8 == 0 and nf <= fps.shape[1] * 8 and _seg_fits(nf, len(fps)):
            idx = int(jt_compl_isim_segments(fps, np.array([0, len(fps)], dtype=np.int64), n_features=nf,
                                             return_compl=False)[0][0])
            m = unpack_fingerprints(fps[idx], n_features)  # only the winning row
            return (idx, pack_fingerprints(m)) if pack else (idx, m)
    if input_is_packed:
        fps = unpack_fingerprints(fps, n_features)
    idx = 0 if len(fps) < 3 else int(np.argmin(jt_compl_isim(fps, input_is_packed=False)))
    m = fps[idx]
    return (idx, pack_fingerprints(m)) if pack else (idx, m)


def jt_stratified_sampling(fps: NDArray[np.uint8], n_samples: int, input_is_packed: bool = True, n_features: int | None = None) -> NDArray[np.int64]:
    r"""(similarity.py:276-304)"""
    if n_samples == 0:
        return np.array([], dtype=np.int64)
    if n_samples > len(fps):
        raise ValueError("n_samples must be <= len(fps)")
    order = np.argsort(jt_compl_isim(fps, input_is_packed, n_features))
    return np.array([s[0] for s in np.array_split(order, n_samples)])


def estimate_jt_std(fps: NDArray[np.uint8], n_samples: int | None = None, input_is_packed: bool = True, n_features: int | None = None) -> float:
    r"""(similarity.py:250-273)"""
    num = len(fps)
    if n_samples is None:
        n_samples = max(num // 1000, 50)
    sample = fps[jt_stratified_sampling(fps, n_samples, input_is_packed, n_features)]
    if not input_is_packed:
        sample = pack_fingerprints(sample)
    m = jt_sim_matrix_packed(sample)
    iu = np.triu_indices(len(sample), k=1)
    return float(np.std(m[iu]))

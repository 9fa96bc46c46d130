r"""CPU-oracle engine for tests: same five operations as bblean_amd._engine.HipEngine,
backed by oracle/libbboracle.so.  TEST INFRASTRUCTURE - never imported by the product."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
_LIB = None
_W = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
# bbo_tree_split_counts, in its order ("small": of the smaller half, the one the engine sums)
SPLIT_COUNTS = ("splits", "internal", "root", "majority_tie", "argmin1_tie", "argmin2_tie", "equal_sims", "equal_sims_pairs_differ",
                "fp1_is_fp2", "n1_eq_n2", "n1_gt_n2", "small_over_255", "small_over_65535", "small_mod16_0", "small_mod16_1", "zero_row",
                "small_all_single", "small_u8_with_single", "small_over_16", "m_over_124", "fp1_row0", "fp1_last_row", "_22", "_23")
# bbo_tree_storage and bbo_tree_thaw_counts, in their order (bb_oracle.h)
STORAGE = ("used_blocks", "runs", "cold", "full", "thaws", "sealed_now", "live", "pools")
THAW_COUNTS = ("leaf", "internal", "first_leaf", "last_leaf", "middle_leaf", "parent_thawed_too", "then_merge", "then_append", "leaf_then_split",
               "internal_then_split", "then_new_root", "whole_path_new_root", "thawed_leaf_splits", "in_place_half_keeps_record", "cold_but_full", "leaf_parent",
               "top_level", "leaf_under_thawed_parent", "append_len0", "append_len1", "append_len2", "append_len3", "_22", "_23")


def oracle_lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    so = REPO / "oracle" / "libbboracle.so"
    src = REPO / "oracle" / "bb_oracle.c"
    if not so.is_file() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run(["make", "-C", str(REPO / "oracle"), "libbboracle.so"], check=True,
                       capture_output=True)
    lib = C.CDLL(str(so))
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    protos = {
        "bbo_popcount_rows": (None, [vp, i64, i64, vp]),
        "bbo_jt_arr_vec": (None, [vp, i64, i64, vp, vp, vp, vp, vp]),
        "bbo_unpack": (None, [vp, i64, i64, i64, vp]),
        "bbo_pack": (None, [vp, i64, i64, vp]),
        "bbo_centroid_from_sum": (None, [vp, i64, i64, C.c_int, vp]),
        "bbo_isim_from_sum": (f64, [vp, i64, i64]),
        "bbo_add_rows": (None, [vp, i64, i64, vp]),
        "bbo_most_dissimilar": (None, [vp, i64, i64, i64, C.POINTER(i64), C.POINTER(i64), vp, vp]),
        "bbo_isim_radius_compl_from_sum": (f64, [vp, i64, i64]),
        "bbo_merge_accept": (C.c_int, [C.c_int, f64, f64, vp, i64, vp, i64, vp, i64, i64, i64]),
        "bbo_tree_create": (vp, [i32, f64, i32, f64, vp, i64, i32]),
        "bbo_tree_destroy": (None, [vp]),
        "bbo_tree_set_merge": (None, [vp, i32, f64, vp, i64, f64, i32]),
        "bbo_tree_reset": (None, [vp]),
        "bbo_tree_fit_packed": (C.c_int, [vp, vp, i64, vp]),
        "bbo_tree_fit_buffers": (C.c_int, [vp, vp, i32, i64, vp]),
        "bbo_tree_leaf_count": (i64, [vp]),
        "bbo_tree_export_leaves": (None, [vp, vp, vp, vp, vp]),
        "bbo_tree_gather_buffers": (C.c_int, [vp, vp, i64, i32, vp]),
        "bbo_tree_stats": (None, [vp, vp]),
        "bbo_tree_edge_counts": (None, [vp, vp]),
        "bbo_tree_tie_depths": (None, [vp, vp]),
        "bbo_tree_split_counts": (None, [vp, vp]),
        "bbo_tree_compact": (None, [vp, i32]),
        "bbo_tree_mark_loaded": (None, [vp]),
        "bbo_tree_storage": (None, [vp, vp]),
        "bbo_tree_thaw_counts": (None, [vp, vp]),
        "bbo_tree_walk": (None, [vp, C.POINTER(i64), C.POINTER(i64), vp, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


class OracleEngine:
    def __init__(self, branching_factor, threshold, criterion, tolerance, tol_table, n_features, device=0):
        self.lib = oracle_lib()
        self.n_features = int(n_features)
        self.nbytes = self.n_features // 8
        tab = np.ascontiguousarray(tol_table, dtype=np.float64)
        self._h = self.lib.bbo_tree_create(int(branching_factor), float(threshold), int(criterion),
                                           float(tolerance), tab.ctypes.data if tab.size else None,
                                           tab.size, self.n_features)
        if not self._h:
            raise RuntimeError("Only n_features divisible by 8 is supported")

    def set_merge(self, criterion, tolerance, tol_table, threshold, branching_factor):
        tab = np.ascontiguousarray(tol_table, dtype=np.float64)
        self.lib.bbo_tree_set_merge(self._h, int(criterion), float(tolerance),
                                    tab.ctypes.data if tab.size else None, tab.size,
                                    float(threshold), int(branching_factor))

    def reset(self):
        self.lib.bbo_tree_reset(self._h)

    def fit_packed(self, rows, stream=None):
        if hasattr(rows, "cpu"):
            rows = rows.cpu().numpy()
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        out = np.empty(rows.shape[0], dtype=np.uint32)
        self.lib.bbo_tree_fit_packed(self._h, rows.ctypes.data, rows.shape[0], out.ctypes.data)
        return out

    def fit_buffers(self, bufs, stream=None):
        bufs = np.ascontiguousarray(bufs)
        if bufs.dtype.kind != "u":
            bufs = bufs.astype(np.uint64)
        out = np.empty(bufs.shape[0], dtype=np.uint32)
        rc = self.lib.bbo_tree_fit_buffers(self._h, bufs.ctypes.data, bufs.dtype.itemsize,
                                           bufs.shape[0], out.ctypes.data)
        assert rc == 0
        return out

    def leaf_count(self):
        return int(self.lib.bbo_tree_leaf_count(self._h))

    def export_leaves(self, ls_width=None):
        k = self.leaf_count()
        ids = np.empty(k, dtype=np.uint32)
        ns = np.empty(k, dtype=np.uint64)
        cents = np.empty((k, self.nbytes), dtype=np.uint8)
        ls32 = np.empty((k, self.n_features), dtype=np.uint32) if ls_width else None
        self.lib.bbo_tree_export_leaves(self._h, ids.ctypes.data, ns.ctypes.data, cents.ctypes.data,
                                        ls32.ctypes.data if ls32 is not None else None)
        ls = ls32.astype(_W[ls_width]) if ls32 is not None else None
        return ids, ns, cents, ls

    def gather_buffers(self, positions, width):
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        out = np.empty((pos.size, self.n_features + 1), dtype=_W[width])
        rc = self.lib.bbo_tree_gather_buffers(self._h, pos.ctypes.data, pos.size, int(width), out.ctypes.data)
        assert rc == 0, rc
        return out

    def stats(self):
        out = np.zeros(8, dtype=np.uint64)
        self.lib.bbo_tree_stats(self._h, out.ctypes.data)
        return out

    def edge_counts(self):
        r"""[merge decisions, those with a comparison of two equal values, best-row searches with a tied maximum > 0,
        those tied between different (inter, union) pairs], since create or reset."""
        out = np.zeros(4, dtype=np.uint64)
        self.lib.bbo_tree_edge_counts(self._h, out.ctypes.data)
        return [int(v) for v in out]

    def tie_depths(self):
        r"""edge_counts()[3] by the depth of the node searched: [depth 1 (the root), depth 2, ..., depth 8 and deeper]."""
        out = np.zeros(8, dtype=np.uint64)
        self.lib.bbo_tree_tie_depths(self._h, out.ctypes.data)
        return [int(v) for v in out]

    def split_counts(self):
        r"""name -> how many node splits met that condition since create or reset (SPLIT_COUNTS, bb_oracle.h)."""
        out = np.zeros(24, dtype=np.uint64)
        self.lib.bbo_tree_split_counts(self._h, out.ctypes.data)
        return {name: int(v) for name, v in zip(SPLIT_COUNTS, out)}

    def compact(self, seal):
        r"""The storage model's compaction (bbo_tree_compact): the tree itself does not change."""
        self.lib.bbo_tree_compact(self._h, int(seal))

    def reload(self):
        r"""The storage model's state after a save and bbh_tree_load_fd (bbo_tree_mark_loaded)."""
        self.lib.bbo_tree_mark_loaded(self._h)

    def storage(self):
        r"""name -> value of the storage model (STORAGE, bb_oracle.h)."""
        out = np.zeros(8, dtype=np.uint64)
        self.lib.bbo_tree_storage(self._h, out.ctypes.data)
        return {name: int(v) for name, v in zip(STORAGE, out)}

    def thaw_counts(self):
        r"""name -> how many thaws met that condition since create or reset (THAW_COUNTS, bb_oracle.h)."""
        out = np.zeros(24, dtype=np.uint64)
        self.lib.bbo_tree_thaw_counts(self._h, out.ctypes.data)
        return {name: int(v) for name, v in zip(THAW_COUNTS, out)}

    def walk(self, ls=True):
        r"""The whole tree in pre-order (the root first, then the subtrees of its rows in row order), as
        tree_image_format.Image.walk gives it: nodes (n, 4) int32 [depth, leaf flag, length, position in the leaf chain or
        -1], and per row n, id, pop, cent, ls.  ls=False: without the linear sums (rows x features uint64: 400 MB for a
        tree of 24 000 leaves at 2048 bits)."""
        n_nodes, n_rows = C.c_int64(-1), C.c_int64(-1)
        self.lib.bbo_tree_walk(self._h, C.byref(n_nodes), C.byref(n_rows), None, None, None, None, None, None)
        k, r = n_nodes.value, n_rows.value
        w = dict(nodes=np.empty((k, 4), np.int32), n=np.empty(r, np.uint64), id=np.empty(r, np.uint32), pop=np.empty(r, np.uint32),
                 cent=np.empty((r, self.nbytes), np.uint8))
        if ls:
            w["ls"] = np.empty((r, self.n_features), np.uint64)
        self.lib.bbo_tree_walk(self._h, C.byref(n_nodes), C.byref(n_rows),
                               *[w[key].ctypes.data if key in w else None for key in ("nodes", "n", "id", "pop", "cent", "ls")])
        assert (n_nodes.value, n_rows.value) == (k, r)
        return w

    def close(self):
        if self._h:
            self.lib.bbo_tree_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

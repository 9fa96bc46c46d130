r"""Edge cases of the tree engine (bblean_amd/csrc/bb_tree.hip) through the raw C ABI: what bblean_amd/_engine.py never passes -
strided and misaligned rows, device out_leaf on a side stream, buffer tables of every width from host and device, singleton
runs around the splitter's kMinRun, slabs that cut them, mixed multi-tree launches, positions in any order, 2^22 + 5 gathered
rows, refused calls.  Every case of tree_abi_cases.py (held against its conditions by test_tree_abi_cases.py) is replayed here
with ctypes on raw addresses, outputs pre-filled with sentinels, and everything the oracle's replay returned must be equal.

Left untested: the launch chunking of bbh_tree_export_leaves (the `ls_only` layout of gather()) - only a tree of more than
2^22 leaf BitFeatures reaches its second launch; the offsets it shares with the gather calls are checked through those."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import tree_abi_cases as T

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
SENT32 = 0xDEADBEEF
SENT8 = 0xA7
OK, INVALID, STATE = 0, 1, 5


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def ok(lib, rc):
    assert rc == 0, (rc, lib.bbh_last_error())


def refused(lib, rc, code=INVALID):
    assert rc == code, (rc, lib.bbh_last_error())
    assert lib.bbh_last_error(), "a refusal comes with a message"


def dev(torch, a: np.ndarray):
    r"""A device copy of a NumPy array, bit for bit (uint16 / 32 / 64 travel as int16 / 32 / 64)."""
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a).view(view) if view else np.ascontiguousarray(a)).cuda()


def host(t, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def at(x):
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def sentinel(shape, dtype) -> np.ndarray:
    r"""An output array filled with a sentinel, one element longer than asked for (the guard)."""
    n = int(np.prod(shape))
    return np.full(n + 1, SENT32 if np.dtype(dtype).itemsize >= 4 else SENT8, dtype)


def untouched(a: np.ndarray) -> bool:
    return bool((a == (SENT32 if a.dtype.itemsize >= 4 else SENT8)).all())


class Raw:
    r"""One bbh_tree handle with OracleEngine's methods (tree_abi_cases.run drives both), every call on raw addresses.
    `where`: inputs of the fits as host or device pointers; `out`: out_leaf host, device or None (NULL)."""

    def __init__(self, lib, torch, c, where="host", out="host"):
        self.lib, self.torch, self.F, self.nb, self.where, self.out = lib, torch, c["F"], c["F"] // 8, where, out
        tab = np.ascontiguousarray(c["table"], dtype=np.float64)
        self.h = C.c_void_p()
        ok(lib, lib.bbh_tree_create(C.byref(self.h), c["bf"], c["thr"], c["crit"], c["tol"], tab.ctypes.data if tab.size else None,
                                    tab.size, c["F"], 0))
        assert self.h.value

    def close(self):
        if self.h:
            ok(self.lib, self.lib.bbh_tree_destroy(self.h))
            self.h = None

    def _fit(self, call, n):
        o = sentinel(n, np.uint32)
        if self.out is None:
            ok(self.lib, call(None))
            return None
        if self.out == "device":
            d = dev(self.torch, o)
            ok(self.lib, call(d.data_ptr()))
            o = host(d, np.uint32)
        else:
            ok(self.lib, call(o.ctypes.data))
        assert o[n] == SENT32, "wrote past out_leaf"
        return o[:n].copy()

    def fit_packed(self, rows, stream=None):
        if self.where == "device":
            src = dev(self.torch, rows)
            stride = self.nb
        else:
            src = rows if rows.strides[1] == 1 else np.ascontiguousarray(rows)
            stride = src.strides[0]
        n = rows.shape[0]
        return self._fit(lambda o: self.lib.bbh_tree_fit_packed(self.h, at(src), n, stride, o, stream), n)

    def fit_buffers(self, bufs, stream=None):
        src = dev(self.torch, bufs) if self.where == "device" else np.ascontiguousarray(bufs)
        k = bufs.shape[0]
        return self._fit(lambda o: self.lib.bbh_tree_fit_buffers(self.h, at(src), bufs.dtype.itemsize, k, o, stream), k)

    def set_merge(self, criterion, tolerance, tol_table, threshold, branching_factor, expect=OK):
        tab = np.ascontiguousarray(tol_table, dtype=np.float64)
        rc = self.lib.bbh_tree_set_merge(self.h, criterion, tolerance, tab.ctypes.data if tab.size else None, tab.size, threshold,
                                         branching_factor)
        assert rc == expect, (rc, self.lib.bbh_last_error())
        assert expect == OK or self.lib.bbh_last_error(), "a refusal comes with a message"

    def reset(self):
        ok(self.lib, self.lib.bbh_tree_reset(self.h))

    def leaf_count(self):
        k = C.c_int64(-7)
        ok(self.lib, self.lib.bbh_tree_leaf_count(self.h, C.byref(k)))
        return k.value

    def export_leaves(self, ls_width=None):
        k = self.leaf_count()
        ids, ns = sentinel(k, np.uint32), sentinel(k, np.uint64)
        cents = sentinel(k * self.nb, np.uint8)
        ls = sentinel(k * self.F, T.W[ls_width]) if ls_width else None
        ok(self.lib, self.lib.bbh_tree_export_leaves(self.h, at(ids), at(ns), at(cents), at(ls), ls_width or 0))
        for a in (ids, ns, cents) + ((ls,) if ls is not None else ()):
            assert untouched(a[-1:]), "wrote past an output"
        return ids[:k], ns[:k], cents[:-1].reshape(k, self.nb), ls[:-1].reshape(k, self.F) if ls is not None else None

    def gather_buffers(self, positions, width):
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        out = sentinel(pos.size * (self.F + 1), T.W[width])
        ok(self.lib, self.lib.bbh_tree_gather_buffers(self.h, at(pos), pos.size, width, at(out)))
        assert untouched(out[-1:])
        return out[:-1].reshape(pos.size, self.F + 1)

    def gather_centroids(self, positions):
        pos = np.ascontiguousarray(positions, dtype=np.int64)
        out = sentinel(pos.size * self.nb, np.uint8)
        ok(self.lib, self.lib.bbh_tree_gather_centroids(self.h, at(pos), pos.size, at(out)))
        assert untouched(out[-1:])
        return out[:-1].reshape(pos.size, self.nb)

    def stats(self):
        out = np.zeros(8, np.uint64)
        ok(self.lib, self.lib.bbh_tree_stats(self.h, at(out)))
        return out

    def kernel_counts(self):
        out = np.zeros(8, np.uint64)
        ok(self.lib, self.lib.bbh_tree_kernel_counts(self.h, at(out)))
        return [int(v) for v in out]

    def compact(self, seal):
        ok(self.lib, self.lib.bbh_tree_compact(self.h, int(seal)))

    def memory(self):
        r"""bbh_tree_memory: [pool bytes, used bytes, cluster-feature bytes, peak, compactions, sealed and full nodes of the last
        one, thaws]."""
        out = np.zeros(8, np.uint64)
        ok(self.lib, self.lib.bbh_tree_memory(self.h, at(out)))
        return [int(v) for v in out]

    def reload(self):
        r"""Save the image, load it into a new handle (bbh_tree_load_fd), destroy the old handle and go on with the new one."""
        with tempfile.TemporaryFile() as f:
            written = C.c_uint64(0)
            ok(self.lib, self.lib.bbh_tree_save_fd(self.h, f.fileno(), 0, C.byref(written)))
            f.seek(0)
            new = C.c_void_p()
            ok(self.lib, self.lib.bbh_tree_load_fd(C.byref(new), f.fileno(), 0, 0))
            assert new.value and os.lseek(f.fileno(), 0, os.SEEK_CUR) == written.value, written.value
        ok(self.lib, self.lib.bbh_tree_destroy(self.h))
        self.h = new

    def save_image(self) -> bytes:
        r"""The tree's image (bbh_tree_save_fd into a temporary file); the tree stays as it was."""
        with tempfile.TemporaryFile() as f:
            written = C.c_uint64(0)
            ok(self.lib, self.lib.bbh_tree_save_fd(self.h, f.fileno(), 0, C.byref(written)))
            f.seek(0)
            image = f.read()
        assert len(image) == written.value, (len(image), written.value)
        return image


@functools.lru_cache(maxsize=None)
def oracle_runs(name):
    return T.replay(T.RUN_CFG, [("buffers", T.run_table(name))])


@functools.lru_cache(maxsize=None)
def oracle_tier(width):
    return T.replay(T.TIER_CFG, [("buffers", T.tier_table(width)[0])])


def hip_run(lib, torch, c, ops, positions=None, width=8, **how):
    eng = Raw(lib, torch, c, **how)
    try:
        return T.run(eng, ops, positions, width), eng.kernel_counts()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. bbh_tree_fit_buffers
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("how", ["host", "device", "host_slab64", "host_slab16"])
@pytest.mark.parametrize("name", list(T.RUN_TABLES))
def test_buffer_singleton_runs(lib, torch, monkeypatch, name, how):
    r"""Width-1 tables with singleton runs around kMinRun = 1024: the splitter packs the long runs and inserts them as
    fingerprints, out_leaf lands at out + lo.  From the host (one slab), from the device (k_gather_n_col, k_pack_singletons),
    and from the host in slabs of 1008 rows (they cut the long runs) and of 252 rows (no slab holds a run of 1024)."""
    if how.startswith("host_slab"):
        monkeypatch.setenv("BBHIP_SLAB_KB", how[len("host_slab"):])
    got, _ = hip_run(lib, torch, T.RUN_CFG, [("buffers", T.run_table(name))], where=how.split("_")[0])
    T.same(got, oracle_runs(name))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_buffer_widths_and_tier_promotions(lib, torch, where, width):
    r"""The same BitFeatures as uint8 / 16 / 32 / 64 tables, n_samples of 255, 256, 65535 and 65536 where they fit, and pairs
    (200 + 200, 40000 + 40000) whose merge promotes a leaf BitFeature that arrived as a buffer to the next tier."""
    tab, _ = T.tier_table(width)
    pos = np.arange(oracle_tier(width)["leaf_count"], dtype=np.int64)[::-1]
    got, _ = hip_run(lib, torch, T.TIER_CFG, [("buffers", tab)], pos, 8, where=where)
    want = dict(oracle_tier(width), gathered=T.snapshot_rows(oracle_tier(width))[pos])
    T.same(got, want)


def test_buffer_pool_growth_relaunches(lib, torch):
    r"""A first call of width 8: pregrow sizes the uint8 pool for width-1 tables only, the kernel stops on the exhausted pool,
    the host grows it and relaunches."""
    tab = T.pool_table()
    got, kc = hip_run(lib, torch, T.POOL_CFG, [("buffers", tab)])
    assert kc[7] > 0, kc
    T.same(got, T.replay(T.POOL_CFG, [("buffers", tab)]))


@pytest.mark.parametrize("where", ["host", "device"])
def test_buffer_n_samples_beyond_range_is_refused(lib, torch, where):
    r"""n_samples = 2^32 after ten valid rows: BBH_ERR_INVALID (the kernel stops in front of the row).  Nothing is asserted
    about the half-inserted tree; after a reset the handle is as good as new."""
    bad, good = T.range_tables()
    eng = Raw(lib, torch, T.RANGE_CFG, where=where)
    src = dev(torch, bad) if where == "device" else bad
    out = sentinel(11, np.uint32)
    refused(lib, lib.bbh_tree_fit_buffers(eng.h, at(src), 8, 11, at(out), None))
    assert b"n_samples" in lib.bbh_last_error()
    assert out[11] == SENT32
    eng.reset()
    T.same(T.run(eng, [("buffers", good)]), T.replay(T.RANGE_CFG, [("buffers", good)]))
    eng.close()


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import tree_abi_cases as T
import test_hip_tree_abi_edges as E
from bblean_amd import _lib
lib = _lib.load()
res = {{}}
for bf in (50, 254):
    for width in (1, 4):
        eng = E.Raw(lib, None, T.switch_cfg(bf), where="host")
        snap = T.run(eng, [("buffers", T.switch_table(width))])
        snap["out_leaf"] = snap["out_leaf"][0]
        snap["kc"] = np.array(eng.kernel_counts(), np.uint64)
        snap["leaf_count"] = np.array(snap["leaf_count"])
        eng.close()
        for key, v in snap.items():
            res["%d_%d_%s" % (bf, width, key)] = v
np.savez({out!r}, **res)
"""


@pytest.mark.parametrize("switch", T.SWITCHES)
def test_buffers_on_every_insertion_kernel(switch, tmp_path):
    r"""F = 2048, bf 50 and 254, a width-1 table (runs of 1500 and 500 singletons between buffers) and the same BitFeatures at
    width 4, under each kernel switch.  The switches are read once per process: one child process per switch."""
    script = _CHILD.format(repo=str(REPO), tests=str(REPO / "tests"), out=str(tmp_path / "out.npz"))
    env = dict(os.environ)
    if switch:
        env[switch] = "1"
    done = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    res = np.load(tmp_path / "out.npz")
    for bf in (50, 254):
        for width in (1, 4):
            want = T.replay(T.switch_cfg(bf), [("buffers", T.switch_table(width))])
            got = {key: res[f"{bf}_{width}_{key}"] for key in ("ids", "ns", "cents", "ls", "stats")}
            got["leaf_count"] = int(res[f"{bf}_{width}_leaf_count"])
            got["out_leaf"] = [res[f"{bf}_{width}_out_leaf"]]
            T.same(got, want)
            kc = [int(v) for v in res[f"{bf}_{width}_kc"]]
            what = (switch, bf, width, kc)
            assert kc[0] + kc[1] + kc[2] == 3000, what
            if switch == "BBHIP_NO_FAST":  # no steady-state kernel, and the pipelined one only runs beside it
                assert kc[:3] == [0, 0, 3000], what
            elif switch in ("BBHIP_NO_PIPE", "BBHIP_NO_SINGLETON_PATH") or width == 4:  # nothing packed, or no pipeline for it
                assert kc[:3] == [0, 3000, 0] and kc[3] == 0, what
            else:  # the long singleton run goes to the pipelined kernel as fingerprints, the buffers to the steady-state kernel
                assert kc[3] > 0 and kc[1] >= 1500 and kc[2] == 0, what


# ---------------------------------------------------------------------------------------------------------------------
# 2. bbh_tree_fit_packed
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("slabs", [1, 2, 3])
@pytest.mark.parametrize("extra", T.STRIDE_EXTRA)
def test_packed_strided_host_rows(lib, torch, monkeypatch, extra, slabs):
    r"""Host views of row stride nbytes + 1, + 4 and 2 * nbytes that end where their allocation ends, streamed in 1, 2 and 3
    slabs (the last one a single row): the result of the contiguous call and of the oracle.  That the staging copy reads
    (m - 1) * row_stride + nbytes bytes and no more is checked by reading HostSlabs::fetch and bbh_trees_fit_packed, not
    here: an over-read of a few bytes past a heap block shows in no result."""
    monkeypatch.setenv("BBHIP_SLAB_KB", str(T.STRIDE_SLAB_KB))
    rows = T.stride_rows(extra, slabs)
    base, view = T.strided_view(rows, 8 + extra)
    want = T.replay(T.STRIDE_CFG, [("packed", rows)])
    got, _ = hip_run(lib, torch, T.STRIDE_CFG, [("packed", view)])
    T.same(got, want)
    contiguous, _ = hip_run(lib, torch, T.STRIDE_CFG, [("packed", rows)])
    T.same(got, contiguous)
    assert (base.reshape(-1)[-8:] == rows[-1]).all()


@pytest.mark.parametrize("off,stride", T.MISALIGNED)
def test_packed_strided_and_misaligned_device_rows(lib, torch, off, stride):
    r"""Device rows that start 1, 4 or 16 bytes into an allocation, 260, 264 or 272 bytes apart (F = 2048, bf 50): rows that
    are not 16-byte aligned go to the complete kernel, aligned ones to the kernels that read them with 16-byte loads."""
    rows = T.misaligned_rows()
    n, nb = rows.shape
    flat = torch.full((off + n * stride,), SENT8, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:].as_strided((n, nb), (stride, 1))
    view.copy_(dev(torch, rows))
    eng = Raw(lib, torch, T.MISALIGNED_CFG)
    out = eng._fit(lambda o: lib.bbh_tree_fit_packed(eng.h, view.data_ptr(), n, stride, o, None), n)
    got = T.snapshot(eng)
    got["out_leaf"] = [out]
    kc = eng.kernel_counts()
    eng.close()
    T.same(got, T.replay(T.MISALIGNED_CFG, [("packed", rows)]))
    if (off | stride) % 16:
        assert kc[:3] == [0, 0, n], kc
    else:
        assert kc[2] == 0 and kc[0] + kc[1] == n, kc


def test_packed_device_out_leaf_on_a_side_stream(lib, torch):
    r"""Rows written on a non-blocking side stream, that stream passed as `stream`, out_leaf on the device: the call is
    synchronous, out_leaf is read right after it returns."""
    rows = T.misaligned_rows()
    n = rows.shape[0]
    pinned = torch.from_numpy(rows).pin_memory()
    side = torch.cuda.Stream()
    eng = Raw(lib, torch, T.MISALIGNED_CFG)
    d_out = dev(torch, sentinel(n, np.uint32))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_rows = torch.empty((n, rows.shape[1]), dtype=torch.uint8, device="cuda")
        d_rows.copy_(pinned, non_blocking=True)
    ok(lib, lib.bbh_tree_fit_packed(eng.h, d_rows.data_ptr(), n, rows.shape[1], d_out.data_ptr(), side.cuda_stream))
    out = host(d_out, np.uint32)
    assert out[n] == SENT32
    got = T.snapshot(eng)
    got["out_leaf"] = [out[:n]]
    eng.close()
    T.same(got, T.replay(T.MISALIGNED_CFG, [("packed", rows)]))


def test_empty_calls_change_nothing(lib, torch):
    rows = T.rows_near(1, 60, 64, k=10)
    eng = Raw(lib, torch, T.CHAIN_CFG)
    eng.fit_packed(rows)
    before = T.snapshot(eng)
    out = sentinel(4, np.uint32)
    d_out = dev(torch, out)
    for o in (out.ctypes.data, d_out.data_ptr(), None):
        ok(lib, lib.bbh_tree_fit_packed(eng.h, None, 0, 8, o, None))
        ok(lib, lib.bbh_tree_fit_buffers(eng.h, None, 1, 0, o, None))
    assert untouched(out) and untouched(host(d_out, np.uint32))
    ok(lib, lib.bbh_tree_gather_buffers(eng.h, None, 0, 1, None))
    ok(lib, lib.bbh_tree_gather_centroids(eng.h, None, 0, None))
    after = T.snapshot(eng)
    before["out_leaf"] = after["out_leaf"] = []
    T.same(after, before)
    eng.close()


def test_leaf_chain_cache_follows_every_fit(lib, torch):
    r"""leaf_count -> fit -> leaf_count -> export -> fit -> export on one handle: a stale chain would return the old leaves."""
    a, b, c = (T.rows_near(10 + i, 80, 64, k=20) for i in range(3))
    eng, ora = Raw(lib, torch, T.CHAIN_CFG), T.make_oracle(T.CHAIN_CFG)
    assert eng.leaf_count() == 0
    eng.fit_packed(a), ora.fit_packed(a)
    assert eng.leaf_count() == ora.leaf_count() > 0
    eng.fit_packed(b), ora.fit_packed(b)
    assert eng.leaf_count() == ora.leaf_count()
    first = T.snapshot(eng)
    T.same(dict(first, out_leaf=[]), dict(T.snapshot(ora), out_leaf=[]))
    eng.fit_buffers(T.tier_table(1)[0][:120]), ora.fit_buffers(T.tier_table(1)[0][:120])
    T.same(dict(T.snapshot(eng), out_leaf=[]), dict(T.snapshot(ora), out_leaf=[]))
    eng.fit_packed(c), ora.fit_packed(c)
    pos = np.arange(ora.leaf_count(), dtype=np.int64)
    second = T.snapshot(eng, pos, 8)
    T.same(dict(second, out_leaf=[]), dict(T.snapshot(ora, pos, 8), out_leaf=[]))
    assert second["leaf_count"] != first["leaf_count"]
    eng.close(), ora.close()


@pytest.mark.parametrize("bf,F", T.CORNERS)
def test_shape_corners(lib, torch, bf, F):
    r"""(bf, F) in {2, 1023} x {8, 8192}: all four run and equal the oracle (no corner is refused)."""
    c, rows = T.corner_case(bf, F)
    pos = np.array([0, 1], np.int64)
    got, _ = hip_run(lib, torch, c, [("packed", rows)], pos, 4)
    T.same(got, T.replay(c, [("packed", rows)], pos, 4))


@pytest.mark.parametrize("thr", [0.0, 1.0])
def test_threshold_extremes(lib, torch, thr):
    rows = T.threshold_rows()
    got, _ = hip_run(lib, torch, T.THRESHOLD_CASES[thr], [("packed", rows)])
    T.same(got, T.replay(T.THRESHOLD_CASES[thr], [("packed", rows)]))


@pytest.mark.parametrize("name", list(T.tol_cases()))
def test_tolerance_table_of_five_entries(lib, torch, name):
    r"""tol_len = 5 under both tolerance criteria, clusters that grow past five members (entries at or beyond tol_len count
    as 0), and tol_table = NULL."""
    c = T.tol_cases()[name]
    got, _ = hip_run(lib, torch, c, [("packed", T.tol_rows())])
    T.same(got, T.replay(c, [("packed", T.tol_rows())]))


# ---------------------------------------------------------------------------------------------------------------------
# 3. bbh_trees_fit_packed / bbh_trees_fit_buffers: mixed launches
# ---------------------------------------------------------------------------------------------------------------------

# residency of every tree's input and out_leaf in the one call (the tree named "empty" passes NULL rows and n = 0)
MIXED_PLAN = [("device", "device"), ("host", "host"), ("device", None), ("host", "host"), (None, None)]


def _mixed(lib, torch, trees, which, with_out):
    names = list(trees)
    engines = {}
    for name in names:
        c, before, _ = trees[name]
        engines[name] = Raw(lib, torch, c)
        T.run(engines[name], before)
    keep, ins, outs, counts, strides, widths = [], [], [], [], [], []
    for name, (where, out) in zip(names, MIXED_PLAN):
        c, _, data = trees[name]
        if data is None:
            ins.append(None), outs.append(None), counts.append(0), strides.append(c["F"] // 8), widths.append(1)
            continue
        if name.endswith("strided"):
            _, src = T.strided_view(data, data.shape[1] + 5)
        else:
            src = dev(torch, data) if where == "device" else data
        o = sentinel(data.shape[0], np.uint32) if out else None
        if out == "device":
            o = dev(torch, o)
        keep += [src, o]
        ins.append(at(src)), outs.append(at(o)), counts.append(data.shape[0])
        strides.append(src.strides[0] if isinstance(src, np.ndarray) else data.shape[1]), widths.append(data.dtype.itemsize)
    n = len(names)
    handles = (C.c_void_p * n)(*[engines[name].h.value for name in names])
    a_in, a_out = (C.c_void_p * n)(*ins), (C.c_void_p * n)(*outs)
    a_n, a_stride, a_width = (C.c_int64 * n)(*counts), (C.c_int64 * n)(*strides), (C.c_int32 * n)(*widths)
    p_out = C.addressof(a_out) if with_out else None
    if which == "packed":
        ok(lib, lib.bbh_trees_fit_packed(C.addressof(handles), n, C.addressof(a_in), C.addressof(a_n), C.addressof(a_stride), p_out, None))
    else:
        ok(lib, lib.bbh_trees_fit_buffers(C.addressof(handles), n, C.addressof(a_in), C.addressof(a_width), C.addressof(a_n), p_out, None))
    for name in names:
        c, before, data = trees[name]
        ops = before + ([(which, data)] if data is not None else [])
        want = T.replay(c, ops)
        got = T.snapshot(engines[name])
        T.same(dict(got, out_leaf=[]), dict(want, out_leaf=[]))
        engines[name].close()
        # the same handle sequence with single-tree calls
        single, _ = hip_run(lib, torch, c, ops)
        T.same(single, want)
    # out_leaf of the trees that asked for one
    it = iter(keep)
    for name in names:
        if trees[name][2] is None:
            continue
        _, o = next(it), next(it)
        if o is None:
            continue
        c, before, data = trees[name]
        want = T.replay(c, before + [(which, data)])["out_leaf"][-1]
        arr = o if isinstance(o, np.ndarray) else host(o, np.uint32)
        if with_out:
            assert (arr[:-1] == want).all() and arr[-1] == SENT32, name
        else:
            assert untouched(arr), name


@pytest.mark.parametrize("with_out", [True, False])
def test_mixed_launch_of_packed_rows(lib, torch, with_out):
    r"""One bbh_trees_fit_packed call over trees of (bf, F) = (50, 2048), (254, 2048), (5, 64), (17, 800), four criteria,
    one fitted / fresh / reset / empty (n = 0, NULL rows), host, device and strided host rows, out_leaf on the device, on the
    host, NULL - and the array out_leaf itself NULL."""
    _mixed(lib, torch, T.mixed_packed(), "packed", with_out)


@pytest.mark.parametrize("with_out", [True, False])
def test_mixed_launch_of_buffer_tables(lib, torch, with_out):
    r"""The same for bbh_trees_fit_buffers, widths 1, 2, 4 and 8 in one call."""
    _mixed(lib, torch, T.mixed_buffers(), "buffers", with_out)


# ---------------------------------------------------------------------------------------------------------------------
# 4. export / gather
# ---------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def gather_tree(lib, torch):
    eng = Raw(lib, torch, T.GATHER_CFG)
    T.run(eng, T.gather_ops())
    want = T.replay(T.GATHER_CFG, T.gather_ops())
    yield eng, want
    eng.close()


EXPORT_OUTPUTS = ["ids", "ns", "cents", "ls"]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("which", [("ids",), ("ns",), ("cents",), ("ls",), tuple(EXPORT_OUTPUTS), ()], ids=lambda w: "+".join(w) or "none")
def test_export_output_residency(lib, torch, gather_tree, which, where):
    eng, want = gather_tree
    k, F = want["leaf_count"], eng.F
    bufs = {"ids": sentinel(k, np.uint32), "ns": sentinel(k, np.uint64), "cents": sentinel(k * F // 8, np.uint8), "ls": sentinel(k * F, np.uint64)}
    given = {key: (dev(torch, bufs[key]) if where == "device" else bufs[key]) if key in which else None for key in EXPORT_OUTPUTS}
    ok(lib, lib.bbh_tree_export_leaves(eng.h, at(given["ids"]), at(given["ns"]), at(given["cents"]), at(given["ls"]), 8))
    for key in which:
        arr = given[key] if where == "host" else host(given[key], bufs[key].dtype)
        assert untouched(arr[-1:]), key
        assert (arr[:-1] == want[key].reshape(-1)).all(), key


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_export_widths_truncate_like_a_cast(lib, torch, gather_tree, width):
    eng, want = gather_tree
    _, _, _, ls = eng.export_leaves(ls_width=width)
    assert ls.dtype == T.W[width] and (ls == want["ls"].astype(T.W[width])).all()
    if width < 4:
        assert (ls.astype(np.uint64) != want["ls"]).any(), "some value does not fit"


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_gather_positions(lib, torch, gather_tree, width, where):
    r"""Reversed, shuffled, repeated positions, the first and last leaf only, m = 1: rows [linear_sum | n_samples] of `width`
    bytes (the low bits where a value does not fit), and the packed centroids of the same leaves."""
    eng, want = gather_tree
    ora = T.make_oracle(T.GATHER_CFG)
    T.run(ora, T.gather_ops())
    rows = T.snapshot_rows(want)
    for name, pos in T.position_sets(want["leaf_count"]).items():
        expect = ora.gather_buffers(pos, width)
        assert (expect == rows[pos].astype(T.W[width])).all()
        if where == "host":
            got, cents = eng.gather_buffers(pos, width), eng.gather_centroids(pos)
        else:
            d_out, d_cent = dev(torch, sentinel(expect.size, T.W[width])), dev(torch, sentinel(pos.size * eng.nb, np.uint8))
            ok(lib, lib.bbh_tree_gather_buffers(eng.h, at(pos), pos.size, width, d_out.data_ptr()))
            ok(lib, lib.bbh_tree_gather_centroids(eng.h, at(pos), pos.size, d_cent.data_ptr()))
            got, cents = host(d_out, T.W[width]), host(d_cent, np.uint8)
            assert untouched(got[-1:]) and untouched(cents[-1:])
            got, cents = got[:-1].reshape(expect.shape), cents[:-1].reshape(pos.size, eng.nb)
        assert (got == expect).all(), name
        assert (cents == want["cents"][pos]).all(), name
    ora.close()


def test_centroids_are_the_majority_bits(gather_tree):
    eng, want = gather_tree
    pos = np.arange(want["leaf_count"], dtype=np.int64)
    cents = eng.gather_centroids(pos)
    assert (cents == want["cents"]).all()
    many = want["ns"] > 1
    assert many.any() and (~many).any()
    majority = np.packbits(2 * want["ls"] >= want["ns"][:, None], axis=1)
    assert (cents[many] == majority[many]).all()
    assert (cents[~many] == np.packbits(want["ls"][~many].astype(bool), axis=1)).all()


def test_gather_launch_chunking(lib, torch):
    r"""gather() launches 2^22 rows at a time: 2^22 + 5 positions that cycle over ten leaves of several leaf nodes.  The rows
    of the second launch read d_nodes + lo and land at the lo * cols * width output offset."""
    eng = Raw(lib, torch, T.CHUNK_CFG)
    T.run(eng, T.chunk_ops())
    want = T.replay(T.CHUNK_CFG, T.chunk_ops())
    k = want["leaf_count"]
    assert eng.leaf_count() == k
    pos = np.arange(T.CHUNK_M, dtype=np.int64) % k
    rows = T.snapshot_rows(want).astype(np.uint8)
    got = eng.gather_buffers(pos, 1)
    assert got.shape == (T.CHUNK_M, 9)
    assert np.array_equal(got[-64:], rows[pos[-64:]]), "the second launch"
    assert np.array_equal(got, rows[pos])
    del got
    cents = eng.gather_centroids(pos)
    assert np.array_equal(cents[-64:], want["cents"][pos[-64:]]), "the second launch"
    assert np.array_equal(cents, want["cents"][pos])
    eng.close()


def _refuses_positions(lib, torch, eng, positions):
    pos = np.asarray(positions, dtype=np.int64)
    m, cols = pos.size, eng.F + 1
    out, cent = sentinel(m * cols, np.uint32), sentinel(m * eng.nb, np.uint8)
    d_out, d_cent = dev(torch, out), dev(torch, cent)
    for o, c in ((out.ctypes.data, cent.ctypes.data), (d_out.data_ptr(), d_cent.data_ptr())):
        refused(lib, lib.bbh_tree_gather_buffers(eng.h, at(pos), m, 4, o))
        refused(lib, lib.bbh_tree_gather_centroids(eng.h, at(pos), m, c))
    assert untouched(out) and untouched(cent) and untouched(host(d_out, np.uint32)) and untouched(host(d_cent, np.uint8))


def test_positions_out_of_range_are_refused_before_any_write(lib, torch, gather_tree):
    eng, want = gather_tree
    k = want["leaf_count"]
    _refuses_positions(lib, torch, eng, [0, 1, k])
    _refuses_positions(lib, torch, eng, [k - 1, -1, 0])
    _refuses_positions(lib, torch, eng, [k])


@pytest.mark.parametrize("state", ["never_fitted", "reset"])
def test_empty_trees_export_nothing(lib, torch, state):
    eng = Raw(lib, torch, T.GATHER_CFG)
    if state == "reset":
        T.run(eng, T.gather_ops())
        eng.reset()
    assert eng.leaf_count() == 0
    bufs = [sentinel(4, np.uint32), sentinel(4, np.uint64), sentinel(32, np.uint8), sentinel(256, np.uint64)]
    ok(lib, lib.bbh_tree_export_leaves(eng.h, *[at(b) for b in bufs], 8))
    assert all(untouched(b) for b in bufs)
    _refuses_positions(lib, torch, eng, [0])
    assert eng.stats()[:7].tolist() == [0, 0, 0, 0, 0, 1, 0], "one empty leaf root"
    eng.close()


def test_compaction_changes_no_result(lib, torch):
    ops = T.gather_ops()
    more = T.rows_near(95, 200, 64, k=30)
    eng = Raw(lib, torch, T.GATHER_CFG)
    pos = T.position_sets(T.replay(T.GATHER_CFG, ops)["leaf_count"])["shuffled"]
    before = T.run(eng, ops, pos, 8)
    T.same(before, T.replay(T.GATHER_CFG, ops, pos, 8))
    for seal in (1, 1, 0):  # (the first compaction records the lengths, the second seals the nodes that kept theirs)
        ok(lib, lib.bbh_tree_compact(eng.h, seal))
        T.same(dict(T.snapshot(eng, pos, 8), out_leaf=before["out_leaf"]), before)
        assert (eng.gather_centroids(pos) == before["cents"][pos]).all()
    ok(lib, lib.bbh_tree_compact(eng.h, 1))
    ok(lib, lib.bbh_tree_compact(eng.h, 1))
    out = eng.fit_packed(more)
    want = T.replay(T.GATHER_CFG, ops + [("packed", more)])
    T.same(dict(T.snapshot(eng), out_leaf=before["out_leaf"] + [out]), want)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. set_merge / reset
# ---------------------------------------------------------------------------------------------------------------------


def test_set_merge_between_two_fits(lib, torch):
    a, b = T.merge_rows(0), T.merge_rows(1)
    crit, tol, tab, thr = T.MERGE_NEW
    ops = [("packed", a), ("set_merge", crit, tol, tab, thr, T.MERGE_CFG["bf"]), ("packed", b),
           ("set_merge", T.TOL_RADIUS, 0.1, T.TOL_TABLE[:3], 0.5, T.MERGE_CFG["bf"]), ("packed", np.ascontiguousarray(a[::-1]))]
    got, _ = hip_run(lib, torch, T.MERGE_CFG, ops)
    T.same(got, T.replay(T.MERGE_CFG, ops))


@pytest.mark.parametrize("state", ["never_fitted", "reset"])
def test_branching_factor_change_on_an_empty_tree(lib, torch, state):
    a, b = T.merge_rows(0), T.merge_rows(1)
    c = T.MERGE_CFG
    change = ("set_merge", c["crit"], c["tol"], c["table"], c["thr"], 7)
    ops = ([("packed", a), ("reset",)] if state == "reset" else []) + [change, ("packed", b)]
    eng = Raw(lib, torch, c)
    if state == "reset":
        eng.fit_packed(a)
        assert eng.stats()[6] >= 3, "several levels"
        eng.reset()
    T.apply_op(eng, change)
    out = eng.fit_packed(b)
    want = T.replay(c, ops)
    T.same(dict(T.snapshot(eng), out_leaf=[out]), dict(want, out_leaf=want["out_leaf"][-1:]))
    T.same(dict(want, out_leaf=[]), dict(T.replay(T.cfg(7, c["thr"], 64, c["crit"], c["tol"], c["table"]), [("packed", b)]), out_leaf=[]))
    eng.close()


@pytest.mark.parametrize("bf,code", [(7, STATE), (1, INVALID), (1024, INVALID)])
def test_refused_set_merge_leaves_the_tree_as_it_was(lib, torch, bf, code):
    r"""A branching factor change on a non-empty tree (BBH_ERR_STATE) or out of range (BBH_ERR_INVALID), with a new criterion,
    tolerance, table and threshold in the same call: the following fit behaves as under the old settings - the oracle here
    never sees the refused call."""
    a, b = T.merge_rows(0), T.merge_rows(1)
    crit, tol, tab, thr = T.MERGE_NEW
    eng = Raw(lib, torch, T.MERGE_CFG)
    first = eng.fit_packed(a)
    eng.set_merge(crit, tol, tab, thr, bf, expect=code)
    second = eng.fit_packed(b)
    T.same(dict(T.snapshot(eng), out_leaf=[first, second]), T.replay(T.MERGE_CFG, [("packed", a), ("packed", b)]))
    eng.set_merge(6, tol, tab, thr, T.MERGE_CFG["bf"], expect=INVALID)
    eng.set_merge(-1, tol, tab, thr, T.MERGE_CFG["bf"], expect=INVALID)
    third = eng.fit_packed(a)
    T.same(dict(T.snapshot(eng), out_leaf=[first, second, third]), T.replay(T.MERGE_CFG, [("packed", a), ("packed", b), ("packed", a)]))
    eng.close()


def test_reset_restarts_ids_and_stats(lib, torch):
    a, b = T.merge_rows(0), T.merge_rows(1)
    ops = [("packed", a), ("buffers", T.tier_table(4)[0]), ("reset",), ("packed", b), ("reset",), ("reset",), ("buffers", T.tier_table(2)[0])]
    got, _ = hip_run(lib, torch, T.MERGE_CFG, ops)
    want = T.replay(T.MERGE_CFG, ops)
    T.same(got, want)
    assert int(want["out_leaf"][-1][0]) == 0, "ids restart"


# ---------------------------------------------------------------------------------------------------------------------
# 6. invalid calls
# ---------------------------------------------------------------------------------------------------------------------


def test_invalid_calls_are_refused_before_any_write(lib, torch):
    r"""Every call returns BBH_ERR_INVALID with a message, leaves every sentinel intact and the tree equal to the oracle's.
    (bbh_tree_destroy(NULL) is BBH_OK, like free(NULL).)"""
    c = T.CHAIN_CFG
    rows = T.rows_near(1, 60, 64, k=10)
    tab8, tab1 = T.tier_table(8)[0][:20], T.tier_table(1)[0][:20]
    eng = Raw(lib, torch, c)
    eng.fit_packed(rows)
    want = T.replay(c, [("packed", rows)])
    h, k = eng.h, want["leaf_count"]
    out32, out8, out64 = sentinel(4096, np.uint32), sentinel(4096, np.uint8), sentinel(4096, np.uint64)
    d_out32 = dev(torch, out32)
    pos = np.array([0, 1], np.int64)
    cnt, st = C.c_int64(-7), np.full(8, SENT32, np.uint64)
    d_rows, d_tab = dev(torch, rows), dev(torch, tab8)
    o32 = out32.ctypes.data
    L = lib
    calls = {
        # NULL handle
        "set_merge(NULL)": lambda: L.bbh_tree_set_merge(None, 0, 0.0, None, 0, 0.5, 4),
        "reset(NULL)": lambda: L.bbh_tree_reset(None),
        "fit_packed(NULL)": lambda: L.bbh_tree_fit_packed(None, at(rows), 60, 8, o32, None),
        "fit_buffers(NULL)": lambda: L.bbh_tree_fit_buffers(None, at(tab8), 8, 20, o32, None),
        "trees_fit_packed(NULL)": lambda: L.bbh_trees_fit_packed(None, 1, None, None, None, None, None),
        "trees_fit_buffers(NULL)": lambda: L.bbh_trees_fit_buffers(None, 1, None, None, None, None, None),
        "leaf_count(NULL)": lambda: L.bbh_tree_leaf_count(None, C.byref(cnt)),
        "leaf_count(out NULL)": lambda: L.bbh_tree_leaf_count(h, None),
        "export(NULL)": lambda: L.bbh_tree_export_leaves(None, o32, at(out64), at(out8), None, 0),
        "gather_buffers(NULL)": lambda: L.bbh_tree_gather_buffers(None, at(pos), 2, 4, o32),
        "gather_centroids(NULL)": lambda: L.bbh_tree_gather_centroids(None, at(pos), 2, at(out8)),
        "compact(NULL)": lambda: L.bbh_tree_compact(None, 1),
        "stats(NULL)": lambda: L.bbh_tree_stats(None, at(st)),
        "kernel_counts(NULL)": lambda: L.bbh_tree_kernel_counts(None, at(st)),
        # create
        "create(out NULL)": lambda: L.bbh_tree_create(None, 4, 0.5, 0, 0.05, None, 0, 64, 0),
        **{f"create(F={F})": (lambda F=F: _create_refused(L, 4, 0, F)) for F in (0, 4, 12, 8200)},
        **{f"create(crit={cr})": (lambda cr=cr: _create_refused(L, 4, cr, 64)) for cr in (-1, 6)},
        **{f"create(bf={bf})": (lambda bf=bf: _create_refused(L, bf, 0, 64)) for bf in (1, 1024)},
        **{f"set_merge(crit={cr})": (lambda cr=cr: L.bbh_tree_set_merge(h, cr, 0.0, None, 0, 0.9, 4)) for cr in (-1, 6)},
        # shapes
        "fit_packed(stride < nbytes)": lambda: L.bbh_tree_fit_packed(h, at(rows), 60, 7, o32, None),
        "fit_packed(n < 0)": lambda: L.bbh_tree_fit_packed(h, at(rows), -1, 8, o32, None),
        "fit_buffers(k < 0)": lambda: L.bbh_tree_fit_buffers(h, at(tab8), 8, -1, o32, None),
        **{f"fit_buffers(width={w})": (lambda w=w: L.bbh_tree_fit_buffers(h, at(tab8), w, 20, o32, None)) for w in (0, 3, 16)},
        **{f"gather_buffers(width={w})": (lambda w=w: L.bbh_tree_gather_buffers(h, at(pos), 2, w, o32)) for w in (0, 3, 16)},
        **{f"export(ls_width={w})": (lambda w=w: L.bbh_tree_export_leaves(h, o32, None, None, at(out64), w)) for w in (0, 3, 16)},
        "gather_buffers(positions NULL)": lambda: L.bbh_tree_gather_buffers(h, None, 2, 4, o32),
        "gather_buffers(out NULL)": lambda: L.bbh_tree_gather_buffers(h, at(pos), 2, 4, None),
        "gather_buffers(m < 0)": lambda: L.bbh_tree_gather_buffers(h, at(pos), -1, 4, o32),
        "gather_centroids(positions NULL)": lambda: L.bbh_tree_gather_centroids(h, None, 2, at(out8)),
        "gather_centroids(out NULL)": lambda: L.bbh_tree_gather_centroids(h, at(pos), 2, None),
        "gather_centroids(m < 0)": lambda: L.bbh_tree_gather_centroids(h, at(pos), -1, at(out8)),
        # NULL rows / bufs with a positive count
        "fit_packed(rows NULL)": lambda: L.bbh_tree_fit_packed(h, None, 60, 8, o32, None),
        "fit_packed(rows NULL, device out)": lambda: L.bbh_tree_fit_packed(h, None, 60, 8, d_out32.data_ptr(), None),
        "fit_buffers(bufs NULL)": lambda: L.bbh_tree_fit_buffers(h, None, 8, 20, o32, None),
        "fit_buffers(bufs NULL, width 1)": lambda: L.bbh_tree_fit_buffers(h, None, 1, 20, o32, None),
    }
    # the multi-tree calls: three slots, a NULL tree at index 0 / 2, NULL rows / bufs at index 1, the other slots valid
    for label, trees_, ins_p, ins_b in [("trees[0] NULL", (None, h.value, h.value), None, None), ("trees[2] NULL", (h.value, h.value, None), None, None),
                                        ("rows[1] NULL", (h.value,) * 3, (at(rows), None, d_rows.data_ptr()), (at(tab8), None, d_tab.data_ptr()))]:
        a_t = (C.c_void_p * 3)(*trees_)
        a_rows = (C.c_void_p * 3)(*(ins_p or (at(rows), d_rows.data_ptr(), at(rows))))
        a_bufs = (C.c_void_p * 3)(*(ins_b or (at(tab8), d_tab.data_ptr(), at(tab8))))
        a_n, a_k, a_s, a_w = (C.c_int64 * 3)(60, 60, 60), (C.c_int64 * 3)(20, 20, 20), (C.c_int64 * 3)(8, 8, 8), (C.c_int32 * 3)(8, 8, 8)
        a_o = (C.c_void_p * 3)(o32, d_out32.data_ptr(), None)
        arrays = (a_t, a_rows, a_bufs, a_n, a_k, a_s, a_w, a_o)
        calls[f"trees_fit_packed({label})"] = lambda A=arrays: L.bbh_trees_fit_packed(C.addressof(A[0]), 3, C.addressof(A[1]), C.addressof(A[3]), C.addressof(A[5]), C.addressof(A[7]), None)
        calls[f"trees_fit_buffers({label})"] = lambda A=arrays: L.bbh_trees_fit_buffers(C.addressof(A[0]), 3, C.addressof(A[2]), C.addressof(A[6]), C.addressof(A[4]), C.addressof(A[7]), None)
    one = (C.c_void_p * 1)(h.value)
    bad_n, bad_s, bad_w, some = (C.c_int64 * 1)(-1), (C.c_int64 * 1)(7), (C.c_int32 * 1)(3), (C.c_void_p * 1)(at(rows))
    good_n, good_s = (C.c_int64 * 1)(60), (C.c_int64 * 1)(8)
    adr = C.addressof
    calls["trees_fit_packed(n < 0)"] = lambda: L.bbh_trees_fit_packed(adr(one), 1, adr(some), adr(bad_n), adr(good_s), None, None)
    calls["trees_fit_packed(stride < nbytes)"] = lambda: L.bbh_trees_fit_packed(adr(one), 1, adr(some), adr(good_n), adr(bad_s), None, None)
    calls["trees_fit_buffers(width 3)"] = lambda: L.bbh_trees_fit_buffers(adr(one), 1, adr(some), adr(bad_w), adr(good_n), None, None)
    calls["trees_fit_packed(n_trees < 0)"] = lambda: L.bbh_trees_fit_packed(adr(one), -1, adr(some), adr(good_n), adr(good_s), None, None)
    assert tab1.dtype == np.uint8
    for label, call in calls.items():
        rc = call()
        assert rc == INVALID, (label, rc, lib.bbh_last_error())
        assert lib.bbh_last_error(), label
        assert untouched(out32) and untouched(out8) and untouched(out64) and untouched(st) and cnt.value == -7, label
    assert untouched(host(d_out32, np.uint32))
    ok(lib, lib.bbh_tree_destroy(None))
    T.same(dict(T.snapshot(eng), out_leaf=[]), dict(want, out_leaf=[]))
    assert eng.leaf_count() == k
    # and the handle still works
    more = T.rows_near(2, 60, 64, k=10)
    out = eng.fit_packed(more)
    after = T.replay(c, [("packed", rows), ("packed", more)])
    T.same(dict(T.snapshot(eng), out_leaf=[out]), dict(after, out_leaf=after["out_leaf"][-1:]))
    eng.close()


def _create_refused(lib, bf, crit, F):
    h = C.c_void_p(0x5EED)
    rc = lib.bbh_tree_create(C.byref(h), bf, 0.5, crit, 0.05, None, 0, F, 0)
    assert not h.value, "no handle comes back from a refused create"
    return rc

r"""bbh_tree_route_packed (bb_tree_route.inc) at the raw C ABI and through Python, against the NumPy reference of route_refs.py
(held against the oracle and against its cases' conditions by test_route_refs.py).  Every output must be EQUAL: the leaf id,
the merge decision, the intersection and the union of every query.

And the call must be read-only: around every route call the counters of bbh_tree_stats, bbh_tree_kernel_counts and
bbh_tree_memory and the bytes bbh_tree_save_fd writes are compared, on trees whose nodes are sealed (two compactions), thawed
back to full capacity (compact(0)) and loaded from an image.

Each test is a tree of a few hundred rows and at most a few thousand queries.  Measured on one MI355X: the whole file (89
tests) 4.9 s; the slowest, the Python surface with its save / load and pickle round trips, 1.2 s, every other under 0.2 s."""
from __future__ import annotations

import ctypes as C
import itertools
import pickle
import tempfile

import numpy as np
import pytest

import route_refs as R
import test_hip_tree_abi_edges as E
import tree_abi_cases as T
from test_hip_tree_abi_edges import INVALID, STATE, lib, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GRID_MAX = 256 * 8  # ROUTE_GRID_MAX of bb_tree_route.inc: one query per workgroup up to here, then a workgroup takes several
OUTS = (("leaf", np.uint32), ("accept", np.uint8), ("inter", np.uint32), ("union", np.uint32))


def build(lib, torch, c, ops, **how):
    eng = E.Raw(lib, torch, c, **how)
    for op in ops:
        T.apply_op(eng, op)
    return eng


def route(lib, torch, eng, rows, n=None, stride=None, where="host", out_where="host", outs=("leaf", "accept", "inter", "union"), stream=None,
          expect=0):
    r"""One bbh_tree_route_packed call on raw addresses; outputs pre-filled with sentinels, one element longer than n.
    -> name -> the n results (None for an output passed as NULL).  `expect` != 0: the call must be refused with that code and
    write nothing."""
    n = rows.shape[0] if n is None else n
    stride = (rows.strides[0] if rows is not None else 0) if stride is None else stride
    src = rows
    if rows is not None and where == "device":  # (contiguous rows; strided device rows have a test of their own)
        src = E.dev(torch, np.ascontiguousarray(rows))
    bufs, args = {}, []
    for name, dt in OUTS:
        if name not in outs:
            args.append(None)
            continue
        o = E.sentinel(max(n, 0), dt)
        bufs[name] = E.dev(torch, o) if out_where == "device" else o
        args.append(E.at(bufs[name]))
    rc = lib.bbh_tree_route_packed(eng.h if eng is not None else None, E.at(src), n, stride, *args, stream)
    if stream is not None:
        torch.cuda.synchronize()
    got = {name: (E.host(b, dt) if out_where == "device" else b) for (name, dt), b in ((od, bufs[od[0]]) for od in OUTS if od[0] in bufs)}
    if expect:
        E.refused(lib, rc, expect)
        assert all(E.untouched(a) for a in got.values()), "a refused call wrote to an output"
        return None
    E.ok(lib, rc)
    for name, a in got.items():
        assert E.untouched(a[max(n, 0):]), f"wrote past out_{name}"
    return {name: (got[name][:n].copy() if name in got else None) for name, _ in OUTS}


def same(got, want, who, idx=None):
    for name, _ in OUTS:
        if got.get(name) is None:
            continue
        w = want[name] if idx is None else want[name][idx]
        assert got[name].shape == w.shape, (who, name, got[name].shape, w.shape)
        d = got[name] != w
        assert not d.any(), f"{who}: out_{name} differs for {int(d.sum())} of {d.size} queries, first {int(np.argmax(d))}: {got[name][np.argmax(d)]} against {w[np.argmax(d)]}"


def state(eng):
    r"""Everything a read-only call must leave alone."""
    return dict(stats=[int(v) for v in eng.stats()], kc=eng.kernel_counts(), mem=eng.memory(), leaves=eng.leaf_count())


def unchanged(eng, before, image, who):
    after = state(eng)
    assert after == before, (who, "a route call changed the tree's counters", before, after)
    assert eng.save_image() == image, f"{who}: the bytes bbh_tree_save_fd writes changed over a route call"


@pytest.fixture(scope="module")
def depth_tree(lib, torch):  # noqa: F811
    c, ops, q = R.CASES["depth"]()
    eng = build(lib, torch, c, ops)
    yield eng, q, R.expected("depth")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the cases against the reference
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_equal_the_reference(lib, torch, name):  # noqa: F811
    r"""depth (four levels), every width x bf corner (8 .. 8192 bits, bf 2 .. 1023, a leaf root of 600 rows), node lengths 1, 4,
    5, bf, the tie cases, the six criteria on their thresholds, the four cluster-feature tiers: all four outputs equal, the
    tree untouched."""
    c, ops, q = R.CASES[name]()
    eng = build(lib, torch, c, ops)
    try:
        before, image = state(eng), eng.save_image()
        before = state(eng)  # (the save's staging buffers count in the peak)
        got = route(lib, torch, eng, q)
        same(got, R.expected(name), name)
        unchanged(eng, before, image, name)
        same(route(lib, torch, eng, q, where="device", out_where="device"), R.expected(name), name + " (device)")
    finally:
        eng.close()


@pytest.mark.parametrize("name", R.STORAGE_CASES)
def test_sealed_thawed_and_reloaded_trees(lib, torch, monkeypatch, name):  # noqa: F811
    r"""The same queries on the tree as fitted, after two sealing compactions (nodes at capacity below bf + 1, read where they
    lie: no thaw), after compact(0) and on the handle bbh_tree_load_fd returns: identical results, counters and thaw count
    unchanged, saved bytes unchanged by the route calls."""
    monkeypatch.delenv("BBHIP_TINY_POOLS", raising=False)
    monkeypatch.setenv("BBHIP_GC_MIN_MB", "1024")
    c, ops, q = R.storage_case(name)
    want = R.expected("depth" if name == "depth" else "storage_wide")
    eng = build(lib, torch, c, ops)
    try:
        same(route(lib, torch, eng, q), want, f"{name} as fitted")
        for i, op in enumerate(R.STORAGE_OPS):
            T.apply_op(eng, op)
            if i == 0:
                continue
            who = f"{name} after {R.STORAGE_OPS[:i + 1]}"
            image = eng.save_image()
            before = state(eng)
            if i == 1:
                assert before["mem"][5] > 0, (who, "the second compaction sealed nothing", before["mem"])
            same(route(lib, torch, eng, q), want, who)
            same(route(lib, torch, eng, q, where="device"), want, who + " (device rows)")
            unchanged(eng, before, image, who)
            assert eng.memory()[7] == before["mem"][7], (who, "a route call thawed a node")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# the ABI's edges
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("offset,extra", [(0, 1), (0, 4), (0, 32), (1, 0), (1, 3), (16, 16)])
def test_strided_and_odd_address_rows(lib, torch, depth_tree, where, offset, extra):  # noqa: F811
    r"""Rows `nbytes + extra` bytes apart in a buffer that ends with the last row, starting `offset` bytes into an allocation."""
    eng, q, want = depth_tree
    nb = q.shape[1]
    stride = nb + extra
    base = np.full(offset + (q.shape[0] - 1) * stride + nb, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(base[offset:], q.shape, (stride, 1))
    view[:] = q
    if where == "host":
        got = route(lib, torch, eng, view, stride=stride)
    else:
        d = E.dev(torch, base)
        args = [E.sentinel(q.shape[0], dt) for _, dt in OUTS]
        E.ok(lib, lib.bbh_tree_route_packed(eng.h, d.data_ptr() + offset, q.shape[0], stride, *[E.at(a) for a in args], None))
        got = {name: a[:-1] for (name, _), a in zip(OUTS, args)}
        assert all(E.untouched(a[-1:]) for a in args)
    same(got, want, f"{where} offset {offset} stride {stride}")


@pytest.mark.parametrize("where,out_where", [("host", "device"), ("device", "host"), ("device", "device")])
def test_host_and_device_pointers(lib, torch, depth_tree, where, out_where):  # noqa: F811
    eng, q, want = depth_tree
    same(route(lib, torch, eng, q, where=where, out_where=out_where), want, f"rows {where}, outputs {out_where}")


def test_mixed_output_residency(lib, torch, depth_tree):  # noqa: F811
    r"""out_leaf and out_inter on the device, out_accept and out_union on the host, in one call."""
    eng, q, want = depth_tree
    n = q.shape[0]
    leaf, inter = E.dev(torch, E.sentinel(n, np.uint32)), E.dev(torch, E.sentinel(n, np.uint32))
    acc, uni = E.sentinel(n, np.uint8), E.sentinel(n, np.uint32)
    E.ok(lib, lib.bbh_tree_route_packed(eng.h, E.at(q), n, q.shape[1], leaf.data_ptr(), E.at(acc), inter.data_ptr(), E.at(uni), None))
    got = dict(leaf=E.host(leaf, np.uint32), accept=acc, inter=E.host(inter, np.uint32), union=uni)
    assert all(E.untouched(a[n:]) for a in got.values())
    same({k: v[:n] for k, v in got.items()}, want, "mixed residency")


@pytest.mark.parametrize("outs", [s for r in range(5) for s in itertools.combinations([o for o, _ in OUTS], r)], ids=lambda s: "+".join(s) or "none")
def test_every_subset_of_outputs(lib, torch, depth_tree, outs):  # noqa: F811
    eng, q, want = depth_tree
    got = route(lib, torch, eng, q, outs=outs)
    assert [k for k, v in got.items() if v is not None] == [o for o, _ in OUTS if o in outs]
    same(got, want, f"outputs {outs}")


@pytest.mark.parametrize("n", [0, 1, 2, GRID_MAX - 1, GRID_MAX, GRID_MAX + 1, 3 * GRID_MAX + 7])
def test_query_counts_around_the_grid(lib, torch, depth_tree, n):  # noqa: F811
    r"""n = 0 (nothing happens, whatever the pointers), 1, and one below / at / one above the count at which workgroups start
    to take more than one query."""
    eng, q, want = depth_tree
    idx = np.arange(n) % q.shape[0]
    rows = np.ascontiguousarray(q[idx]) if n else np.zeros((0, q.shape[1]), np.uint8)
    if n == 0:
        assert route(lib, torch, eng, None, n=0, stride=q.shape[1]) is not None
        E.ok(lib, lib.bbh_tree_route_packed(eng.h, None, 0, q.shape[1], None, None, None, None, None))
        return
    same(route(lib, torch, eng, rows), want, f"n = {n}", idx)
    same(route(lib, torch, eng, rows, where="device", out_where="device"), want, f"n = {n} (device)", idx)


def test_permuted_queries_give_permuted_results(lib, torch, depth_tree):  # noqa: F811
    eng, q, want = depth_tree
    perm = np.random.default_rng(5).permutation(q.shape[0])
    same(route(lib, torch, eng, np.ascontiguousarray(q[perm])), want, "permuted", perm)


def test_host_rows_in_several_slabs(lib, torch, depth_tree, monkeypatch):  # noqa: F811
    r"""Host rows go through the slab streamer: 1 KiB slabs of 32 rows, 150 rows, the last slab short."""
    monkeypatch.setenv("BBHIP_SLAB_KB", "1")
    eng, q, want = depth_tree
    same(route(lib, torch, eng, q), want, "1 KiB slabs")
    same(route(lib, torch, eng, q, out_where="device"), want, "1 KiB slabs, device outputs")


def test_side_stream(lib, torch, depth_tree):  # noqa: F811
    eng, q, want = depth_tree
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = route(lib, torch, eng, q, where="device", out_where="device", stream=s.cuda_stream)
    same(got, want, "side stream")
    same(route(lib, torch, eng, q, stream=s.cuda_stream), want, "side stream, host pointers")


def test_refusals_write_nothing(lib, torch, depth_tree):  # noqa: F811
    eng, q, _ = depth_tree
    nb = q.shape[1]
    before = state(eng)
    route(lib, torch, None, q, expect=INVALID)                       # no tree
    route(lib, torch, eng, q, n=-1, expect=INVALID)                  # negative count
    route(lib, torch, eng, q, stride=nb - 1, expect=INVALID)         # rows closer together than a row is long
    route(lib, torch, eng, None, n=3, stride=nb, expect=INVALID)     # no rows
    assert state(eng) == before
    fresh = E.Raw(lib, torch, R.CASES["depth"]()[0])
    try:
        route(lib, torch, fresh, q, expect=STATE)                    # never received anything
        E.ok(lib, lib.bbh_tree_route_packed(fresh.h, None, 0, nb, None, None, None, None, None))
        fresh.fit_packed(q[:20])
        assert route(lib, torch, fresh, q[:5]) is not None
        fresh.reset()
        route(lib, torch, fresh, q, expect=STATE)                    # reset: nothing to route to
    finally:
        fresh.close()


def test_profile_record(lib, torch, depth_tree):  # noqa: F811
    eng, q, _ = depth_tree
    lib.bbh_profile_reset()
    lib.bbh_profile_enable(1)
    try:
        route(lib, torch, eng, q)
        route(lib, torch, eng, q[:7], where="device")
        n, ms, units = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
        E.ok(lib, lib.bbh_profile_get(b"tree_route", C.byref(n), C.byref(ms)))
        E.ok(lib, lib.bbh_profile_units(b"tree_route", C.byref(units)))
        assert (n.value, units.value) == (2, q.shape[0] + 7) and ms.value > 0.0, (n.value, units.value, ms.value)
    finally:
        lib.bbh_profile_enable(0)
        lib.bbh_profile_reset()


def test_merge_settings_are_the_trees_current_ones(lib, torch):  # noqa: F811
    r"""bbh_tree_set_merge after the fit: the route call decides with the new criterion, threshold and table."""
    c, ops, q = R.CASES["crit_diameter_256_bf5"]()
    c2, _, _ = R.CASES["crit_tol_radius_256_bf5"]()
    eng = build(lib, torch, c, ops)
    ora = R.build_oracle(c, ops)
    try:
        eng.set_merge(c2["crit"], c2["tol"], c2["table"], c2["thr"], c["bf"])
        same(route(lib, torch, eng, q), R.route(ora.walk(), dict(c2, bf=c["bf"]), q), "after set_merge")
    finally:
        eng.close()
        ora.close()


# ---------------------------------------------------------------------------------------------------------------------
# the consequence: insert the row alone into a copy of the tree
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["depth", "tiers"])
def test_inserting_the_row_alone_agrees(lib, torch, name):  # noqa: F811
    r"""For a dozen queries: a copy of the saved tree (bbh_tree_load_fd) takes that one row by bbh_tree_fit_packed.  Its merge
    counter rises iff out_accept, and its out_leaf is out_leaf when it does."""
    c, ops, q = R.CASES[name]()
    eng = build(lib, torch, c, ops)
    try:
        got = route(lib, torch, eng, q)
        pick = np.r_[np.flatnonzero(got["accept"] == 1)[:6], np.flatnonzero(got["accept"] == 0)[:6]]
        assert len(pick) == 12
        with tempfile.TemporaryFile() as f:
            written = C.c_uint64(0)
            E.ok(lib, lib.bbh_tree_save_fd(eng.h, f.fileno(), 0, C.byref(written)))
            for e in pick:
                f.seek(0)
                h = C.c_void_p()
                E.ok(lib, lib.bbh_tree_load_fd(C.byref(h), f.fileno(), 0, 0))
                try:
                    st0, st1, leaf = np.zeros(8, np.uint64), np.zeros(8, np.uint64), E.sentinel(1, np.uint32)
                    E.ok(lib, lib.bbh_tree_stats(h, E.at(st0)))
                    row = np.ascontiguousarray(q[e:e + 1])
                    E.ok(lib, lib.bbh_tree_fit_packed(h, E.at(row), 1, row.shape[1], E.at(leaf), None))
                    E.ok(lib, lib.bbh_tree_stats(h, E.at(st1)))
                    merged = int(st1[2]) - int(st0[2])
                    assert merged == int(got["accept"][e]), (name, int(e), merged, got["accept"][e])
                    if merged:
                        assert leaf[0] == got["leaf"][e], (name, int(e), leaf[0], got["leaf"][e])
                finally:
                    E.ok(lib, lib.bbh_tree_destroy(h))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# through Python
# ---------------------------------------------------------------------------------------------------------------------


def test_engine_and_model_against_the_reference_backed_model(lib, torch, tmp_path):  # noqa: F811
    r"""HipEngine.route_packed, BitBirch.route (both orders, host rows and a device tensor) and sklearn's predict_tree (after a
    fit, a save / load and a pickle round trip) against the same model on the oracle-backed engine whose route_packed is
    the reference."""
    from bblean_amd import BitBirch
    from bblean_amd.sklearn import BitBirch as SkBitBirch

    c, ops, q = R.CASES["depth"]()
    rows = ops[0][1]
    kw = dict(branching_factor=c["bf"], threshold=c["thr"], merge_criterion="diameter")
    hip = BitBirch(**kw).fit(rows)
    ref = BitBirch(**kw, _engine_factory=R.RefEngine).fit(rows)
    want = R.expected("depth")
    leaf, acc, inter, union = hip._engine.route_packed(q)
    same(dict(leaf=leaf, accept=acc, inter=inter, union=union), want, "HipEngine.route_packed")
    leaf, acc, inter, union = hip._engine.route_packed(torch.from_numpy(q).cuda())
    same(dict(leaf=leaf, accept=acc, inter=inter, union=union), want, "HipEngine.route_packed (device tensor)")
    for sort in (True, False):
        for x in (q, torch.from_numpy(q).cuda(), np.unpackbits(q, axis=1)):
            a = hip.route(x, input_is_packed=x.shape[1] == q.shape[1], sort=sort)
            b = ref.route(q, sort=sort)
            assert a[0].dtype == np.int64 and a[1].dtype == bool and a[2].dtype == np.float64
            assert all((u == v).all() for u, v in zip(a, b)), sort
        cents = np.array(hip.get_centroids(sort=sort))
        cl, _, sim = hip.route(q, sort=sort)
        i = np.unpackbits(cents[cl] & q, axis=1).sum(axis=1)
        u = np.unpackbits(cents[cl] | q, axis=1).sum(axis=1)
        assert (sim == i / np.maximum(u, 1)).all(), "sim is the similarity to get_centroids(sort)[cluster]"

    sk = SkBitBirch(threshold=c["thr"], branching_factor=c["bf"], merge_criterion="diameter").fit(rows)
    cl, acc, _ = ref.route(q, sort=True)
    labels = sk.predict_tree(q)
    assert (labels == cl + 1).all()
    lab2, acc2 = sk.predict_tree(q, novel=-1, return_accept=True)
    assert (acc2 == acc).all() and (lab2 == np.where(acc, cl + 1, -1)).all() and (~acc).any() and acc.any()
    dl, da = sk.predict_tree(torch.from_numpy(q).cuda(), novel=0, return_accept=True)
    assert dl.is_cuda and da.is_cuda and (dl.cpu().numpy() == np.where(acc, cl + 1, 0)).all() and (da.cpu().numpy() == acc).all()
    sk.save(tmp_path / "model.bb")
    for again in (SkBitBirch.load(tmp_path / "model.bb"), pickle.loads(pickle.dumps(sk))):
        assert (again.predict_tree(q, novel=-1) == lab2).all()

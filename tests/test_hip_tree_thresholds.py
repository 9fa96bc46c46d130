r"""Merge decisions ON the threshold and row choices ON a tie, on every default insertion kernel.  The float64 `>=` of the merge
criteria exists in four hand-written device copies (merge_accept and radius_compl in bb_tree.hip, the switch in
bb_tree_fast.inc, `decide` in bb_tree_pipe.inc, which does not even evaluate the reference's expression outside a 2^-48 band
around the threshold); the cases of tree_threshold_cases.py (held against their conditions by test_tree_threshold_cases.py)
decide thousands of merges at exact equality, one ulp to either side of it, inside, on the edge of and outside that band, and
choose rows among tied similarities of different (inter, union) pairs.  Everything goes through the raw C ABI (the `Raw`
wrapper of test_hip_tree_abi_edges.py) and everything observable must equal the oracle's replay: out_leaf of every element,
leaf ids, n_samples, centroids, linear sums and the seven counters.

The kernel switches are read once per process: the 2048-bit cases run in one child process per switch ("" - the pipelined
kernel takes the majority -, BBHIP_NO_PIPE - the steady-state kernel -, BBHIP_NO_FAST - the complete engine), which writes
what it saw to an .npz; this process compares with the oracle replays it caches.  bbh_tree_kernel_counts says where the
work went.

Left out on purpose: the systolic kernel (BBHIP_SYS).  It shares merge_accept with the complete engine, and DESIGN.md 6s
calls its hand-over not dependable yet."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_hip_tree_abi_edges as E
import tree_abi_cases as T
import tree_threshold_cases as H
from test_hip_tree_abi_edges import lib, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SWITCHES = ("", "BBHIP_NO_PIPE", "BBHIP_NO_FAST")
CHILD_TIMEOUT = {"": 300, "BBHIP_NO_PIPE": 300, "BBHIP_NO_FAST": 420}  # 88 fits of 24 000 rows and their exports; the complete engine is the slowest

_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import tree_abi_cases as T
import tree_threshold_cases as H
import test_hip_tree_abi_edges as E
from bblean_amd import _lib
lib = _lib.load()
res = {{}}
for i, case in enumerate(H.SWITCH_CASES):
    c, ops = H.build(*case)
    eng = E.Raw(lib, None, c, where="host")
    snap = H.compact(T.run(eng, ops))
    snap["kc"] = np.array(eng.kernel_counts(), np.uint64)
    eng.close()
    for j, o in enumerate(snap.pop("out_leaf")):
        res["%d_out_leaf_%d" % (i, j)] = o
    for key, v in snap.items():
        res["%d_%s" % (i, key)] = np.asarray(v)
np.savez({out!r}, **res)
"""


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    r"""switch -> the .npz of its child process, started when first asked for and once only.  After a child that did not end
    well no further one is started."""
    done = {}

    def get(switch):
        if switch not in done:
            bad = [s for s, v in done.items() if isinstance(v, str)]
            if bad:
                done[switch] = f"not started: the child process for {bad[0]!r} failed"
            else:
                out = tmp_path_factory.mktemp("thresholds") / "out.npz"
                script = _CHILD.format(repo=str(E.REPO), tests=str(E.REPO / "tests"), out=str(out))
                env = dict(os.environ)
                if switch:
                    env[switch] = "1"
                try:
                    run = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT[switch])
                    done[switch] = np.load(out) if run.returncode == 0 else f"exit status {run.returncode}: {run.stderr[-3000:]}"
                except subprocess.TimeoutExpired:
                    done[switch] = f"no result after {CHILD_TIMEOUT[switch]} s"
        if isinstance(done[switch], str):
            pytest.fail(f"child process for switch {switch!r}: {done[switch]}", pytrace=False)
        return done[switch]

    return get


def check(got, want):
    T.same(H.expand(got), H.expand(want))


def first_difference(got, want):
    r"""For the failure message: the first element whose out_leaf differs."""
    at = 0
    for a, b in zip(got["out_leaf"], want["out_leaf"]):
        if a.shape == b.shape and (a != b).any():
            return at + int(np.argmax(a != b))
        at += b.size
    return None


@pytest.mark.parametrize("case", H.SWITCH_CASES, ids=H.case_id)
@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
def test_on_edge_cases_on_every_insertion_kernel(children, switch, case):
    r"""The threshold ladders around q = fl(c / (c + 2 p)) (diameter, tolerance-diameter; grouped, shuffled, interleaved and
    mixed inputs), the tolerance tables that land old - tol on, under and over new, the families that cross the 255 -> 256
    member tier promotion on the edge, tolerance-legacy at tolerances that only rounding tells apart, and the block rows with
    their tied similarities: three fit_packed calls each, under each kernel switch."""
    res = children(switch)
    i = H.SWITCH_CASES.index(case)
    want = H.replay_named(*case)
    n_fits = len(want["out_leaf"])
    got = {key: res[f"{i}_{key}"] for key in ("ids", "ns", "cents", "stats", "ls_nz", "ls_val", "ls_shape")}
    got["leaf_count"] = int(res[f"{i}_leaf_count"])
    got["out_leaf"] = [res[f"{i}_out_leaf_{j}"] for j in range(n_fits)]
    kc = [int(v) for v in res[f"{i}_kc"]]
    n = sum(o.size for o in want["out_leaf"])
    print(f"{switch or 'default'} {H.case_id(case)}: kernel counts {kc}, edge counts {want['edge']}, first difference {first_difference(got, want)}")
    check(got, want)
    what = (switch, H.case_id(case), kc)
    assert kc[0] + kc[1] + kc[2] == n, what
    if switch == "BBHIP_NO_FAST":
        assert kc[:2] == [0, 0], what
    elif switch == "BBHIP_NO_PIPE" or H.case_criterion(case) == H.TOL_LEGACY:  # (the pipelined kernel has no tolerance-legacy)
        assert kc[0] == 0 and kc[2] * 10 < n, what
    else:
        assert kc[0] > kc[1] + kc[2], what  # the pipelined kernel inserted the majority


@pytest.mark.parametrize("case", H.RADIUS_CASES + [c + ("empty", True) for c in H.RADIUS_WIDE], ids=lambda c: "-".join(str(v) for v in c))
def test_radius_criteria_on_their_recurring_values(lib, torch, case):  # noqa: F811
    r"""radius and tolerance-radius (the complete engine, merge_accept and radius_compl): threshold = the value the criterion
    takes at the step to 2, 3, 5 and 9 members in every family, and one ulp to either side; 256 features at bf 5 and 17, and
    2048 features at bf 50 (radius_terms at full width)."""
    c, ops = H.build("radius", *case)
    got, kc = E.hip_run(lib, torch, c, ops)
    check(H.compact(got), H.replay_named("radius", *case))
    assert kc[:2] == [0, 0], kc


@pytest.mark.parametrize("bf,tab", H.TOLRAD_CASES + H.TOLRAD_WIDE)
def test_tolerance_radius_tables_on_under_and_over(lib, torch, bf, tab):  # noqa: F811
    r"""tolerance-radius, the second comparison: table entries that land old_rc - table[nT] on new_rc, one ulp under and one
    ulp over it, nT = tol_len - 1 and nT = tol_len, duplicate runs that grow beyond tol_len on reads of 0.0; 256 features at
    bf 5 and 17, 2048 at bf 50."""
    wide = (bf, tab) in H.TOLRAD_WIDE
    c, ops = H.build("tolrad", bf, tab, wide)
    got, kc = E.hip_run(lib, torch, c, ops)
    check(H.compact(got), H.replay_named("tolrad", bf, tab, wide))
    assert kc[:2] == [0, 0], kc


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("crit,bf", H.BUF_CASES)
def test_on_edge_decisions_between_buffers(lib, torch, crit, bf, width):  # noqa: F811
    r"""bbh_tree_fit_buffers: chunks of families as BitFeatures, so that the on-edge decisions have nS > 1 (tolerance-legacy's
    el.nS != 1 branch; at width 4 nS = 300: tier_for(nS) != 0), in two calls."""
    c, ops = H.build("buffers", crit, bf, width)
    got, _ = E.hip_run(lib, torch, c, ops)
    check(H.compact(got), H.replay_named("buffers", crit, bf, width))


def test_on_edge_decisions_across_pool_stops(lib, torch, monkeypatch):  # noqa: F811
    r"""BBHIP_TINY_POOLS=1: the kernels run out of nodes and cluster-feature slots every few elements, the host grows the pools
    and relaunches; the element in flight decides again, on the edge."""
    monkeypatch.setenv("BBHIP_TINY_POOLS", "1")
    c, ops = H.build("ladder", *H.TINY_CASE)
    got, kc = E.hip_run(lib, torch, c, ops)
    print("kernel counts", kc)
    assert kc[7] > 0, kc
    check(H.compact(got), H.replay_named("ladder", *H.TINY_CASE))


def test_three_family_trees_in_one_launch(lib, torch):  # noqa: F811
    r"""bbh_trees_fit_packed: three trees at bf 254, each with another fraction on its threshold, in one call; every tree
    against its own oracle replay."""
    engines, rows, outs = [], [], []
    for case in H.MULTI_CASES:
        c, ops = H.build("ladder", *case)
        engines.append(E.Raw(lib, torch, c))
        rows.append(np.ascontiguousarray(np.concatenate([op[1] for op in ops])))
        outs.append(E.sentinel(rows[-1].shape[0], np.uint32))
    n = len(engines)
    handles = (C.c_void_p * n)(*[e.h.value for e in engines])
    a_in, a_out = (C.c_void_p * n)(*[r.ctypes.data for r in rows]), (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    a_n, a_stride = (C.c_int64 * n)(*[r.shape[0] for r in rows]), (C.c_int64 * n)(*[r.shape[1] for r in rows])
    try:
        E.ok(lib, lib.bbh_trees_fit_packed(C.addressof(handles), n, C.addressof(a_in), C.addressof(a_n), C.addressof(a_stride), C.addressof(a_out), None))
        for case, eng, r, o in zip(H.MULTI_CASES, engines, rows, outs):
            want = H.expand(H.replay_named("ladder", *case))
            want["out_leaf"] = [np.concatenate(want["out_leaf"])]
            assert o[-1] == E.SENT32
            print(H.ladder_id(case), "kernel counts", eng.kernel_counts())
            T.same(dict(T.snapshot(eng), out_leaf=[o[:-1]]), want)
    finally:
        for eng in engines:
            eng.close()

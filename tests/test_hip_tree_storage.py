r"""The node storage of the tree engine ("Node storage" at the top of bb_tree.hip: blocks of 4 rows, gc_nodes with k_gc_size and
k_gc_move, thaw_node, the sealed trees bbh_tree_load_fd returns) on its edges.  The cases of tree_storage_cases.py (held
against their conditions by test_tree_storage_cases.py) go through the raw C ABI (the `Raw` wrapper of
test_hip_tree_abi_edges.py), with BBHIP_GC_MIN_MB=1024 and without BBHIP_TINY_POOLS, so that only the explicit compactions run,
and after EVERY operation - fit, compaction, reload, reset - everything must equal the oracle's replay:
  - out_leaf of every element, leaf ids, n_samples, centroids, linear sums and the seven counters (tree_abi_cases.same);
  - the tree image (bbh_tree_save_fd), walked in pre-order by tree_image_format.Image.walk, against OracleEngine.walk: the
    tracking rows, child links and the leaf chain as k_gc_move translated them and thaw_node re-pointed them (an image saved
    with the holes the thaws leave, too);
  - bbh_tree_memory against the oracle's storage model: [1] = used blocks * block bytes, [4] the compactions, [5] and [6] the
    cold and full nodes of the last one, [7] the thaws - exactly, wherever the complete engine alone inserts.

The shapes only the complete engine takes run in this process, once more with BBHIP_TINY_POOLS=1 and BBHIP_GC_MIN_MB=0
(automatic compactions interleave: the model's numbers do not apply, leaves and walk must still be the oracle's).  The
2048-bit cases at bf 50 and 254 - behind pipe_forward_cases.prefix(), and over grouped rows that give the tree to the
pipelined kernel's multi-level instance - run in one child process per kernel switch ("", BBHIP_NO_PIPE, BBHIP_NO_FAST).
The children are those of test_hip_tree_splits.py: a time limit each, no further child after one that ended badly, results
through an .npz.  Under the first two switches the steady-state and pipelined kernels hand an element that
meets a sealed node to the complete engine; the pipelined kernel's zero levels update tracking rows of sealed nodes in place,
which would make [7] fall short of the model's thaws - but in a tree of three levels the only zero level is the root, which is
never sealed (a fourth level takes some 45 000 rows at bf 50: DESIGN.md).  So [7] and the used blocks equal the model's under
all three switches, and that is asserted.  In every call the used blocks grow by (thaws + new nodes) * node_blocks(bf + 1):
no kernel reserves a block it does not use.

Left out on purpose: the systolic kernel (BBHIP_SYS), for the reason test_hip_tree_thresholds.py gives.

Measured on one MI355X: the whole file (86 tests) 58 s.  The slowest case, 7.0 s, is the first case of a switch, which runs
that switch's child process of six cases: 6.5 s a child.  The other kernel cases take 1.7 - 2.3 s each (the oracle's replay),
many_blocks 3.3 s, every other in-process case and the three-tree call under 0.6 s.  The child time limit is the 240 s that
test_hip_tree_splits.py gives a measured 2 - 6 s.  DESIGN.md, "Node-storage tests", has the mutants of the model and of
thaw_node that these cases catch."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import ctypes as C

import launch_trace_cases as L
import test_hip_tree_abi_edges as E
import tree_abi_cases as T
import tree_image_format as IMG
import tree_storage_cases as SC
from test_hip_tree_abi_edges import lib, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SWITCHES = ("", "BBHIP_NO_PIPE", "BBHIP_NO_FAST")
# At bf 254 the pipelined kernel takes 1 814 rows of the prefix and then stops on a tree shape it does not take (stop=9,
# STOP_PIPE_UNSUPPORTED, as in test_hip_tree_splits.py's HANDED_OVER): by default the steady-state kernel has the tree when the
# second tail comes, and must be the one that inserts and meets the sealed nodes.
HANDED_OVER = {254}
CHILD_TIMEOUT = 240  # six cases of 10 400 to 11 200 rows, five or six images each: measured 6.5 s (the margin of test_hip_tree_splits.py)


def same_tree(got_snap, image: bytes, want, who):
    r"""One operation's state against the oracle's: the leaf-level comparison, the image's invariants, the two walks."""
    walk = IMG.Image(bytearray(image)).walk()
    if len(want["walk"]["nodes"]) == 0:
        # a reset tree: the engine has its empty leaf root (and counts it) from the reset on, the oracle from the first insertion
        stats = want["stats"].copy()
        stats[5] = 1
        T.same(got_snap, dict(want, stats=stats))
        assert walk["nodes"].tolist() == [[1, 1, 0, 0]] and walk["n"].shape[0] == 0, (who, walk["nodes"])
        return
    T.same(got_snap, want)
    IMG.check_walk(want["walk"], f"{who}: oracle")
    IMG.check_walk(walk, f"{who}: image")
    IMG.same_walk(walk, want["walk"], f"{who}: image against oracle")


def same_storage(mem, want, c, who):
    r"""bbh_tree_memory against the storage model after one operation."""
    st = want["storage"]
    bb = IMG.block_bytes(IMG.row_bytes(c["F"]))
    print(who, "memory", mem[1] // bb, mem[4:8], "model", st)
    assert mem[1] == st["used_blocks"] * bb, (who, "used blocks", mem[1] / bb, st["used_blocks"])
    assert mem[4] == st["runs"] and mem[5] == st["cold"] and mem[6] == st["full"], (who, mem[4:7], st)
    assert mem[7] == st["thaws"], (who, "thaws", mem[7], st["thaws"])


def run_ops(eng, ops):
    r"""-> [(snapshot with the out_leaf of the fits so far, image, bbh_tree_memory)] after every operation."""
    outs, res = [], []
    for op in ops:
        outs.append(T.apply_op(eng, op))
        snap = T.snapshot(eng)
        snap["out_leaf"] = [o for o in outs if isinstance(o, np.ndarray)]
        mem = eng.memory()
        res.append((snap, eng.save_image(), mem))
        again = T.snapshot(eng)
        assert all((again[k] == snap[k]).all() for k in ("ids", "ns", "cents", "ls", "stats")), "saving an image changed the tree"
        after = eng.memory()  # ([3], the peak, counts the staging buffers of the save)
        assert after[:3] + after[4:] == mem[:3] + mem[4:], "saving an image changed the storage counters"
    return res


# (many_blocks with normal pools only: with tiny pools every few insertions would compact 350 MB of node pools)
IN_PROCESS = [(name, pools) for name in SC.CASES for pools in ("normal", "tiny") if (name, pools) != ("many_blocks", "tiny")]


@pytest.mark.parametrize("name,pools", IN_PROCESS, ids=lambda v: v)
def test_storage_cases_on_the_complete_engine(lib, torch, monkeypatch, name, pools):  # noqa: F811
    r"""Two sealing compactions or a reload, then rows that reach the first, the last and a middle leaf of the chain, leaves
    under a sealed parent, sealed leaves of every length mod 4 and on either side of "rounds up to full capacity" at bf 8, 50,
    254 and 1023, a thaw and a split on every level up to a new root, the half of a split that keeps its record, the three
    cluster-feature tiers, a reset, a compaction of more than 2^18 blocks: at 8 .. 8192 bits."""
    if pools == "tiny":
        monkeypatch.setenv("BBHIP_TINY_POOLS", "1")
        monkeypatch.setenv("BBHIP_GC_MIN_MB", "0")
    else:
        monkeypatch.delenv("BBHIP_TINY_POOLS", raising=False)
        monkeypatch.setenv("BBHIP_GC_MIN_MB", "1024")
    c, ops, _ = SC.build(name)
    want = SC.replay(name)
    eng = E.Raw(lib, torch, c)
    try:
        got = run_ops(eng, ops)
        kc = eng.kernel_counts()
    finally:
        eng.close()
    bb = IMG.block_bytes(IMG.row_bytes(c["F"]))
    for i, ((snap, image, mem), w) in enumerate(zip(got, want)):
        who = f"{name}, after operation {i} {ops[i][0]}"
        same_tree(snap, image, w, who)
        if pools == "normal":
            same_storage(mem, w, c, who)
    if pools == "normal":
        mem, st = got[-1][2], want[-1]["storage"]
        assert mem[5] == 0 and mem[1] == st["live"] * SC.node_blocks(c["bf"] + 1) * bb, (mem, st)
    assert kc[:2] == [0, 0], kc  # (no shape here is one the steady-state and pipelined kernels are built for)


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import tree_abi_cases as T
import tree_storage_cases as SC
import test_hip_tree_abi_edges as E
from bblean_amd import _lib
lib = _lib.load()
res = {{}}
for i, case in enumerate(SC.KERNEL_CASES):
    c, ops = SC.kernel_case(*case)
    eng = E.Raw(lib, None, c, where="host")
    for j, op in enumerate(ops):
        sys.stderr.write("[case %d op %d]\n" % (i, j)); sys.stderr.flush()
        out = T.apply_op(eng, op)
        snap = T.snapshot(eng)
        for key in ("ids", "ns", "cents", "stats"):
            res["%d_%d_%s" % (i, j, key)] = np.asarray(snap[key])
        if isinstance(out, np.ndarray):
            res["%d_%d_out_leaf" % (i, j)] = out
        # (as in test_hip_tree_splits.py: the sums of the one-member BitFeatures are their bits, checked here; the others travel)
        one = snap["ns"] == 1
        assert (snap["ls"][one] == np.unpackbits(snap["cents"][one], axis=1)).all(), "exported linear sum of a one-member BitFeature"
        res["%d_%d_ls_many" % (i, j)] = snap["ls"][~one]
        res["%d_%d_mem" % (i, j)] = np.array(eng.memory(), np.uint64)
        res["%d_%d_kc" % (i, j)] = np.array(eng.kernel_counts(), np.uint64)
        res["%d_%d_image" % (i, j)] = np.frombuffer(eng.save_image(), np.uint8)
    eng.close()
np.savez({out!r}, **res)
"""


def launch_lines(stderr: str) -> dict:
    r"""(case, operation) -> the parsed `[bbhip launch]` lines behind that marker."""
    by, key = {}, None
    for line in stderr.splitlines():
        if line.startswith("[case "):
            a = line.strip("[]\n").split()
            key = (int(a[1]), int(a[3]))
            by[key] = []
        elif line.startswith("[bbhip launch]"):
            m = L.LAUNCH.match(line)
            assert m is not None and key is not None, line
            by[key].append(dict(zip(L.FIELDS, [m.group(1)] + [int(v) if v.isdigit() else v for v in m.groups()[1:]])))
    return by


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    r"""switch -> (the .npz of its child process, its launch lines), started when first asked for and once only.  After a child that did not end
    well no further one is started."""
    done = {}

    def get(switch):
        if switch not in done:
            bad = [s for s, v in done.items() if isinstance(v, str)]
            if bad:
                done[switch] = f"not started: the child process for {bad[0]!r} failed"
            else:
                out = tmp_path_factory.mktemp("storage") / "out.npz"
                script = _CHILD.format(repo=str(E.REPO), tests=str(E.REPO / "tests"), out=str(out))
                env = dict(os.environ, BBHIP_GC_MIN_MB="1024", BBHIP_LAUNCH_LOG="1")
                for s in SWITCHES[1:] + ("BBHIP_TINY_POOLS",):
                    env.pop(s, None)
                if switch:
                    env[switch] = "1"
                try:
                    run = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
                    done[switch] = (np.load(out), launch_lines(run.stderr)) if run.returncode == 0 else f"exit status {run.returncode}: {run.stderr[-3000:]}"
                except subprocess.TimeoutExpired:
                    done[switch] = f"no result after {CHILD_TIMEOUT} s"
        if isinstance(done[switch], str):
            pytest.fail(f"child process for switch {switch!r}: {done[switch]}", pytrace=False)
        return done[switch]

    return get


@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.kernel_id)
@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
def test_sealed_nodes_on_every_insertion_kernel(children, switch, case):
    r"""Behind the prefix: a first tail, two sealing compactions or a reload, a second tail whose rows reach a sealed leaf-parent,
    sealed leaves under it once it is thawed, a sealed leaf without a spare row that is thawed, filled and split in the same
    call; then compact(0).  The same with grouped rows, whose tree the multi-level instance of the pipelined kernel takes: its
    fill_slot meets eight sealed leaf-parents (fill_sealed).  Under each kernel switch."""
    res, lines = children(switch)
    i = SC.KERNEL_CASES.index(case)
    bf, how, kind = case
    c, ops = SC.kernel_case(*case)
    want = SC.replay_kernel(*case)
    second = SC.second_fit(case)
    bb = IMG.block_bytes(IMG.row_bytes(c["F"]))
    full = SC.node_blocks(bf + 1)
    outs, prev = [], None
    for j, w in enumerate(want):
        who = f"{switch or 'default'} {SC.kernel_id(case)}, after operation {j} {ops[j][0]}"
        if f"{i}_{j}_out_leaf" in res:
            outs.append(res[f"{i}_{j}_out_leaf"])
        snap = {key: res[f"{i}_{j}_{key}"] for key in ("ids", "ns", "cents", "stats")}
        snap["leaf_count"] = int(snap["ids"].shape[0])
        snap["out_leaf"] = list(outs)
        one = snap["ns"] == 1
        snap["ls"] = np.empty((snap["ids"].shape[0], SC.S.F), np.uint64)
        snap["ls"][one] = np.unpackbits(snap["cents"][one], axis=1)
        snap["ls"][~one] = res[f"{i}_{j}_ls_many"]
        w = dict(w, ls=IMG.walk_leaves(w["walk"])["ls"])
        same_tree(snap, res[f"{i}_{j}_image"].tobytes(), w, who)
        mem, kc = [int(v) for v in res[f"{i}_{j}_mem"]], [int(v) for v in res[f"{i}_{j}_kc"]]
        cur = (mem, kc, int(snap["stats"][5]))
        # Exactly the model's numbers under every switch: the steady-state and pipelined kernels hand every element that meets a
        # sealed node to the complete engine, which thaws it, and reserve no block they do not use.  (The pipelined kernel's
        # zero levels, which would update a sealed node's tracking row in place and thaw less, are the root alone in trees
        # of three levels, and the root is never sealed.)
        print(who, "kernel counts", kc)
        same_storage(mem, w, c, who)
        if ops[j][0] == "packed" and prev is not None:  # (after a reload `prev` is the new handle's state already)
            # what thaw_node and split_node imply: every thaw and every new node takes one full-capacity reservation
            grown = (mem[1] - prev[0][1]) // bb
            assert grown == ((mem[7] - prev[0][7]) + (cur[2] - prev[2])) * full, (who, grown, mem[7] - prev[0][7], cur[2] - prev[2])
        if j == second:
            base_kc, base_thaws = prev[1], prev[0][7]
            assert mem[7] > base_thaws, (who, "no thaw in the call after the sealing", mem)
            if switch == "" and kind == "groups":
                # the multi-level instance (pipe_router_ml) has the tree: the single-level one asked for it (stop=11,
                # STOP_PIPE_NEEDS_ML) and it has not handed the tree back (stop=12) when the call's pipelined launches insert
                # (of the handle that takes the call: after a reload only the launches since)
                since = max([jj + 1 for jj in range(second) if ops[jj][0] == "reload"], default=0)
                stops = [ln["stop"] for jj in range(since, second + 1) for ln in lines.get((i, jj), []) if ln["stop"] in (11, 12)]
                piped = [ln["elems"] for ln in lines[(i, j)] if ln["engine"] == "pipe"]
                print(who, "launches (engine, elements, stop):", [(ln["engine"], ln["elems"], ln["stop"]) for ln in lines[(i, j)]])
                assert stops and stops[-1] == 11 and sum(piped) > 0 and kc[0] > base_kc[0], (who, stops, piped, kc, base_kc)
            elif switch == "" and bf in HANDED_OVER:
                assert kc[1] > base_kc[1], (who, "the steady-state kernel inserted nothing in the call after the sealing", kc, base_kc)
            elif switch == "":
                assert kc[0] > base_kc[0], (who, "the pipelined kernel inserted nothing in the call after the sealing", kc, base_kc)
            elif switch == "BBHIP_NO_PIPE":
                assert kc[1] > base_kc[1] and kc[0] == 0, (who, "the steady-state kernel inserted nothing in the call after the sealing", kc, base_kc)
            else:
                assert kc[:2] == [0, 0], kc
        prev = cur
    mem, st = [int(v) for v in res[f"{i}_{len(want) - 1}_mem"]], want[-1]["storage"]
    assert mem[5] == 0 and mem[1] == st["live"] * full * bb, (mem, st)


def test_one_call_over_a_sealed_a_reloaded_and_a_fresh_tree(lib, torch, monkeypatch):  # noqa: F811
    r"""bbh_trees_fit_packed over three handles: one sealed by two compactions, one returned by bbh_tree_load_fd, one that never
    received anything.  After the call each tree's out_leaf, leaves, image walk and bbh_tree_memory are those of its own
    oracle replay and storage model."""
    monkeypatch.delenv("BBHIP_TINY_POOLS", raising=False)
    monkeypatch.setenv("BBHIP_GC_MIN_MB", "1024")
    trees = SC.multi_tree()
    replays = SC.replay_multi_tree()
    engines, outs = [], []
    try:
        for name, c, before, rows in trees:
            eng = E.Raw(lib, torch, c)
            engines.append(eng)
            outs.append([o for o in (T.apply_op(eng, op) for op in before) if isinstance(o, np.ndarray)])
        n = len(trees)
        srcs = [np.ascontiguousarray(rows) for _, _, _, rows in trees]
        dsts = [E.sentinel(rows.shape[0], np.uint32) for rows in srcs]
        handles = (C.c_void_p * n)(*[eng.h.value for eng in engines])  # (the reloaded tree's handle is the new one)
        a_in, a_out = (C.c_void_p * n)(*[E.at(r) for r in srcs]), (C.c_void_p * n)(*[E.at(o) for o in dsts])
        a_n, a_stride = (C.c_int64 * n)(*[r.shape[0] for r in srcs]), (C.c_int64 * n)(*[r.strides[0] for r in srcs])
        E.ok(lib, lib.bbh_trees_fit_packed(C.addressof(handles), n, C.addressof(a_in), C.addressof(a_n), C.addressof(a_stride), C.addressof(a_out), None))
        for (name, c, before, rows), eng, out, dst in zip(trees, engines, outs, dsts):
            assert dst[-1] == E.SENT32, "wrote past out_leaf"
            snap = T.snapshot(eng)
            snap["out_leaf"] = out + [dst[:-1].copy()]
            want = replays[name][-1]
            same_tree(snap, eng.save_image(), want, f"multi_tree {name}")
            same_storage(eng.memory(), want, c, f"multi_tree {name}")
            assert eng.kernel_counts()[:2] == [0, 0]
    finally:
        for eng in engines:
            eng.close()

r"""The node split (split_node in bb_tree.hip: majority vote, two argmin steps, the strict row destination, the stable
partition, the tracking sums by difference, the leaf chain) on its edges, row by row.  The cases of tree_split_cases.py (held
against their conditions by test_tree_split_cases.py) go through the raw C ABI (the `Raw` wrapper of
test_hip_tree_abi_edges.py), and after EVERY fit call everything must equal the oracle's replay:
  - out_leaf of every element, leaf ids, n_samples, centroids, linear sums and the seven counters (tree_abi_cases.same);
  - the tree image (bbh_tree_save_fd), walked in pre-order by tree_image_format.Image.walk: structure, lengths, leaf-chain
    positions and every row's n_samples, id, popcount, centroid and linear sum - the tracking rows of the internal nodes
    included, which no leaf export shows;
  - the invariants of tree_image_format.walk_faults on the image's walk (a tracking row is the sum of its child's rows), so
    that a failure says which side broke what before the two are compared.

The shapes only the complete engine takes run in this process.  The 2048-bit cases at bf 50 and 254 run in one child process
per kernel switch ("" - behind pipe_forward_cases.prefix(), which hands the tree to the pipelined kernel -, BBHIP_NO_PIPE - the
steady-state kernel -, BBHIP_NO_FAST - the complete engine), as in test_hip_tree_thresholds.py: a time limit per child, no
further child after one that ended badly, results through an .npz.  The children run with BBHIP_LAUNCH_LOG=1 and the
`leaf_splits=` and `node_splits=` fields of the launch lines must add up to the oracle's counts and show that the kernel the
switch selects split leaves ITSELF in the tail's calls: a split that moved to another engine fails the test.

Left out on purpose: the systolic kernel (BBHIP_SYS), for the reason test_hip_tree_thresholds.py gives.

Measured on one MI355X: the whole file 22 s, the slowest case 3.4 s, a child process 2 - 6 s ("Node-split tests",
has the mutations of split_node that these cases catch)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

import launch_trace_cases as L
import test_hip_tree_abi_edges as E
import tree_abi_cases as T
import tree_image_format as IMG
import tree_split_cases as S
from test_hip_tree_abi_edges import lib, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SWITCHES = ("", "BBHIP_NO_PIPE", "BBHIP_NO_FAST")
ENGINE = {"": "pipe", "BBHIP_NO_PIPE": "fast", "BBHIP_NO_FAST": "complete"}
# Where the selected kernel need not have split a leaf itself.  Behind the prefix at bf 254, in the family and copy-run tails,
# the pipelined kernel stops on a tree shape it does not take (stop=9, STOP_PIPE_UNSUPPORTED, in the launch lines) and the
# host gives the steady-state kernel a stretch, in which the tails' leaves overflow (measured: pipelined kernel 1 814 and
# 1 826 rows of these runs, every split of the tail in the steady-state kernel's launches).  The pipelined kernel's own leaf
# splits at bf 254 are those of the block-row and zero-row tails: none with a uint16 row in the smaller half.
HANDED_OVER = {("", ("families", 254)), ("", ("tiers", 254))}
CHILD_TIMEOUT = 240  # six cases of at most 11 000 rows, three images each; measured 2 - 6 s


def same_after_fit(got_snap, image: bytes, want, who):
    r"""One fit call's state against the oracle's: the leaf-level comparison, the image's invariants, the two walks."""
    T.same(got_snap, want)
    walk = IMG.Image(bytearray(image)).walk()
    IMG.check_walk(want["walk"], f"{who}: oracle")
    IMG.check_walk(walk, f"{who}: image")
    IMG.same_walk(walk, want["walk"], f"{who}: image against oracle")


def run_with_images(eng, ops):
    r"""-> [(snapshot with the out_leaf of the calls so far, image)] after every operation."""
    outs, res = [], []
    for op in ops:
        outs.append(T.apply_op(eng, op))
        snap = T.snapshot(eng)
        snap["out_leaf"] = list(outs)
        res.append((snap, eng.save_image()))
        again = T.snapshot(eng)
        assert all((again[k] == snap[k]).all() for k in ("ids", "ns", "cents", "ls", "stats")), "saving an image changed the tree"
    return res


@pytest.mark.parametrize("name", list(S.CASES))
def test_split_cases_on_the_complete_engine(lib, torch, name):  # noqa: F811
    r"""Crafted root splits (majority ties at m = 4 .. 1024 and their twins one row away, duplicate and all-zero nodes, fp1 first
    and last), the second split of the same leaf with smaller halves of 15 .. 33 rows on either side, at 64 .. 8192 bits, every
    storage tier in the smaller half through bbh_tree_fit_buffers, block rows with tied similarities, lopsided and peeling
    rows that split internal nodes and the root."""
    c, ops = S.build(name)
    want, _ = S.replay(name)
    eng = E.Raw(lib, torch, c)
    try:
        got = run_with_images(eng, ops)
        kc = eng.kernel_counts()
    finally:
        eng.close()
    for i, ((snap, image), w) in enumerate(zip(got, want)):
        same_after_fit(snap, image, w, f"{name}, after fit {i}")
    print(name, "kernel counts", kc)
    if (c["bf"], c["F"]) not in ((50, S.F), (254, S.F)):  # (the shapes the steady-state and pipelined kernels are built for)
        assert kc[:2] == [0, 0], kc


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np
import tree_abi_cases as T
import tree_split_cases as S
import test_hip_tree_abi_edges as E
from bblean_amd import _lib
lib = _lib.load()
res = {{}}
for i, (name, bf) in enumerate(S.KERNEL_CASES):
    c, ops = S.kernel_case(name, bf, {prefixed!r})
    eng = E.Raw(lib, None, c, where="host")
    outs = []
    for j, op in enumerate(ops):
        sys.stderr.write("[case %d fit %d]\n" % (i, j)); sys.stderr.flush()
        outs.append(T.apply_op(eng, op))
        snap = T.snapshot(eng)
        for key in ("ids", "ns", "cents", "stats"):
            res["%d_%d_%s" % (i, j, key)] = np.asarray(snap[key])
        res["%d_%d_out_leaf" % (i, j)] = outs[-1]
        # the exported linear sums: a BitFeature of one member has its fingerprint's bits (its centroid row, which the parent
        # compares) - checked here, 160 MB a copy behind the prefix; the sums of all others travel
        one = snap["ns"] == 1
        assert (snap["ls"][one] == np.unpackbits(snap["cents"][one], axis=1)).all(), "exported linear sum of a one-member BitFeature"
        res["%d_%d_ls_many" % (i, j)] = snap["ls"][~one]
        res["%d_%d_image" % (i, j)] = np.frombuffer(eng.save_image(), np.uint8)
    res["%d_kc" % i] = np.array(eng.kernel_counts(), np.uint64)
    eng.close()
np.savez({out!r}, **res)
"""


def launch_lines(stderr: str) -> dict:
    r"""(case, fit) -> the parsed `[bbhip launch]` lines behind that marker."""
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
    r"""switch -> (the .npz of its child process, its launch lines), started when first asked for and once only.  After a child
    that did not end well no further one is started."""
    done = {}

    def get(switch):
        if switch not in done:
            bad = [s for s, v in done.items() if isinstance(v, str)]
            if bad:
                done[switch] = f"not started: the child process for {bad[0]!r} failed"
            else:
                out = tmp_path_factory.mktemp("splits") / "out.npz"
                script = _CHILD.format(repo=str(E.REPO), tests=str(E.REPO / "tests"), out=str(out), prefixed=switch == "")
                env = dict(os.environ, BBHIP_LAUNCH_LOG="1")
                for s in SWITCHES[1:]:
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


@pytest.mark.parametrize("case", S.KERNEL_CASES, ids=S.kernel_id)
@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
def test_split_tails_on_every_insertion_kernel(children, switch, case):
    r"""Block rows with tied similarities, families over a common core whose leaf splits again and again, the same with
    runs of exact copies (BitFeatures of 2 .. 255 and of 256 and more members in the halves of a split), and an all-zero
    BitFeature as row 0 of a leaf that splits (max(union, 1), fp1 == fp2, then fp1 the last row): in two fit_packed
    calls, under each kernel switch; by default behind the prefix that hands the tree to the pipelined kernel."""
    res, lines = children(switch)
    i = S.KERNEL_CASES.index(case)
    prefixed = switch == ""
    want, _ = S.replay_kernel(case[0], case[1], prefixed)
    outs = []
    for j, w in enumerate(want):
        outs.append(res[f"{i}_{j}_out_leaf"])
        snap = {key: res[f"{i}_{j}_{key}"] for key in ("ids", "ns", "cents", "stats")}
        snap["leaf_count"] = int(snap["ids"].shape[0])
        snap["out_leaf"] = list(outs)
        # the leaf export's linear sums: those of the one-member BitFeatures are their bits (the child checked that against the
        # centroids compared here), the others came along; against the oracle's leaves, which the replay keeps in its walk only
        one = snap["ns"] == 1
        snap["ls"] = np.empty((snap["ids"].shape[0], S.F), np.uint64)
        snap["ls"][one] = np.unpackbits(snap["cents"][one], axis=1)
        snap["ls"][~one] = res[f"{i}_{j}_ls_many"]
        w = dict(w, ls=IMG.walk_leaves(w["walk"])["ls"])
        same_after_fit(snap, res[f"{i}_{j}_image"].tobytes(), w, f"{switch or 'default'} {S.kernel_id(case)}, after fit {j}")
    # who split the leaves of the tail's calls
    kc = [int(v) for v in res[f"{i}_kc"]]
    tail_fits = range(1 if prefixed else 0, len(want))
    # (`leaf_splits=` is the launch's count of ALL splits, the oracle's stats[4]; `node_splits=` its count of new nodes,
    # stats[5]: one per split and one more per split of the root (the first root exists before the first launch).  A steady-state or pipelined launch
    # counts what its cold function, the complete engine, did inside it: the splits of internal nodes and of the root.)
    by_engine, new_nodes = {}, 0
    for j in tail_fits:
        for ln in lines[(i, j)]:
            by_engine[ln["engine"]] = by_engine.get(ln["engine"], 0) + ln["leaf_splits"]
            new_nodes += ln["node_splits"]
    before = int(want[0]["stats"][4]) if prefixed else 0
    assert new_nodes == int(want[-1]["stats"][5]) - (int(want[0]["stats"][5]) if prefixed else 1), (new_nodes, want[-1]["stats"])
    not_leaf = S.kernel_tail_counts(case[0], case[1], prefixed)["internal"]  # (the oracle: splits of the tail that split no leaf)
    print(f"{switch or 'default'} {S.kernel_id(case)}: kernel counts {kc}, leaf_splits of the tail by engine {by_engine}, the oracle's {int(want[-1]['stats'][4]) - before}")
    print("launches of the tail (engine, elements, leaf_splits, stop):", [(ln["engine"], ln["elems"], ln["leaf_splits"], ln["stop"]) for j in tail_fits for ln in lines[(i, j)]])
    assert sum(by_engine.values()) == int(want[-1]["stats"][4]) - before, by_engine
    if (switch, case) not in HANDED_OVER:
        assert by_engine.get(ENGINE[switch], 0) > not_leaf, (switch, by_engine, not_leaf)  # more than can be internal: a leaf split
    if switch == "BBHIP_NO_FAST":
        assert set(by_engine) == {"complete"} and kc[:2] == [0, 0], (by_engine, kc)
    elif switch == "BBHIP_NO_PIPE":
        assert "pipe" not in by_engine and kc[0] == 0, (by_engine, kc)

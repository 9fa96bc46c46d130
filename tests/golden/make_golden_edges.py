#!/usr/bin/env python3
r"""Generate tests/golden/edges.npz by running the REFERENCE itself on the tree edge-case families.

Runs only in the build container (needs the reference and oracle/_ref built by oracle/build_ref.sh), like make_golden.py.
The cases are those tests/edge_reference_cases.py lists: every case of tree_threshold_cases, tree_split_cases,
tree_storage_cases and tree_abi_cases that the reference's public BitBirch can express.  The rows come from the families'
own builders; the reference is run with the same fit calls (operations that do not change what the tree holds - the
storage model's compactions and reloads - are skipped), and what it computes is recorded:

    input_sha       sha256 of the rows of every fit call
    counts          clusters after every fit call
    numbers         [rows, clusters, nodes, walk rows, depth]
    assign_sha      get_assignments()                        (assign: the array itself for cases of at most INLINE_ROWS rows)
    members_sha     get_cluster_mol_ids(sort=False), flat
    cents_sha       get_centroids(sort=False)
    ns_sha, ls_sha  n_samples and linear sums of the leaf BitFeatures in chain order
    walk_*_sha      the pre-order walk of the node objects: per node [depth, leaf flag, length, chain position], per row
                    n_samples, the node's copy of the centroid, the linear sum
per case, one table per field over all cases in the file (edge_reference_cases.pack_fixture / fixture).

Arrays are kept as sha256 (edge_reference_cases.digests); linear sums are hashed from their non-zero entries, row by
row, and never held densely (24 000 leaves of 2 048 uint64 in a +1-ulp ladder case).

Usage:  python tests/golden/make_golden_edges.py                  write the fixture
        python tests/golden/make_golden_edges.py --explain CASE   run CASE on the reference and on the oracle here and print
                                                                  the first element, leaf or walk row that differs
        python tests/golden/make_golden_edges.py --check CASE...  regenerate these cases, compare with the committed file

Measured: 222 cases in 3 min (182 s) with the reference's C++ backend, a 24 000-row case 0.9 - 2.2 s, the slowest
(storage/many_blocks, branching factor 1023) 9 s; peak memory 0.8 GB; edges.npz 76 KB.
"""
from __future__ import annotations

import argparse
import resource
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
for p in (HERE, HERE.parent, HERE.parents[1]):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from _refimport import import_reference  # noqa: E402

import_reference(use_cpp=True)

from bblean import BitBirch  # noqa: E402

import edge_reference_cases as E  # noqa: E402

INLINE_ROWS = 1100  # assignments themselves for cases up to this many rows (the whole file stays far below sklearn.npz)


def _sparse(rows_ls):
    r"""An iterable of linear sums (one array per row) -> (counts, cols, vals), never dense."""
    counts, cols, vals = [], [], []
    for ls in rows_ls:
        ls = np.asarray(ls)
        nz = np.flatnonzero(ls)
        counts.append(nz.size)
        cols.append(nz.astype(np.uint32))
        vals.append(ls[nz].astype(np.uint64))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    return np.array(counts, np.uint32), cat(cols, np.uint32), cat(vals, np.uint64)


def reference_observables(c, ops):
    r"""The case on the reference's BitBirch -> the observables of edge_reference_cases, from its public getters and a walk
    of its node objects."""
    tree = BitBirch(**E.public_kwargs(c))
    counts = []
    for call in E.calls(ops):
        if call[0] == "fit":
            tree.fit(call[1], n_features=c["F"])
            counts.append(sum(len(leaf._subclusters) for leaf in tree._get_leaves()))
        else:
            tree.reset()
    nb = c["F"] // 8
    members = tree.get_cluster_mol_ids(sort=False)
    cents = tree.get_centroids(sort=False)
    leaves = list(tree._get_leaves())
    subs = [s for leaf in leaves for s in leaf._subclusters]
    obs = dict(counts=np.array(counts, np.int64), assign=np.asarray(tree.get_assignments()).astype(np.uint32),
               members=np.array([i for m in members for i in m], np.uint32),
               ns=np.array([s.n_samples for s in subs], np.uint64),
               cents=np.array(cents, np.uint8).reshape(len(cents), nb), ls=_sparse(s.linear_sum for s in subs))
    assert [len(m) for m in members] == obs["ns"].tolist()
    chain = {id(leaf): p for p, leaf in enumerate(leaves)}
    nodes, row_n, row_cent, row_subs = [], [], [], []

    def visit(node, depth):
        nodes.append([depth, int(node.is_leaf), len(node._subclusters), chain.get(id(node), -1)])
        cent = node.packed_centroids
        for i, sub in enumerate(node._subclusters):
            row_n.append(sub.n_samples)
            row_cent.append(np.array(cent[i], np.uint8))
            row_subs.append(sub)
        for sub in node._subclusters:
            if sub.child is not None:
                visit(sub.child, depth + 1)

    visit(tree._root, 1)
    obs.update(walk_nodes=np.array(nodes, np.int32).reshape(-1, 4), walk_n=np.array(row_n, np.uint64),
               walk_cent=np.array(row_cent, np.uint8).reshape(len(row_cent), nb), walk_ls=_sparse(s.linear_sum for s in row_subs))
    return obs


def record(cid):
    r"""-> the fixture's fields of one case."""
    c, ops = E.build(cid)
    assert E.why_not(c, ops) is None, (cid, E.why_not(c, ops))
    obs = reference_observables(c, ops)
    out = E.digests(obs)
    out["input_sha"] = np.frombuffer(bytes.fromhex(E.input_digest(ops)), np.uint8)
    if obs["assign"].size <= INLINE_ROWS:
        out["assign"] = obs["assign"]
    return out


def explain(cid):
    c, ops = E.build(cid)
    print(f"{cid}: {E.public_kwargs(c)}, {E.n_rows(ops)} rows in {sum(op[0] == 'packed' for op in ops)} fit calls")
    ref = reference_observables(c, ops)
    ora = E.oracle_observables(cid)
    print(f"reference: {ref['ns'].size} clusters, {len(ref['walk_nodes'])} nodes; oracle: {ora['ns'].size} clusters, {len(ora['walk_nodes'])} nodes")
    lines = E.first_difference(ora, ref)
    print("\n".join("oracle against reference, " + ln for ln in lines) if lines else "the oracle and the reference agree in every observable")
    if (HERE / "edges.npz").is_file() and cid in E.fixture():
        want = E.fixture()[cid]
        bad = [k for k, v in E.digests(ref).items() if not np.array_equal(v, want[k])]
        print("the committed fixture is " + (f"STALE in {bad}" if bad else "what the reference gives now"))
    return 1 if lines else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--explain", metavar="CASE")
    ap.add_argument("--check", metavar="CASE", nargs="+", help="regenerate these cases and compare them with the committed fixture (exit status 1: stale)")
    ap.add_argument("--only", metavar="PREFIX", help="(with nothing written) time the cases whose id starts with PREFIX")
    args = ap.parse_args()
    if args.explain:
        sys.exit(explain(args.explain))
    if args.check:
        stale = []
        for cid in args.check:
            got, want = record(cid), E.fixture()[cid]
            stale += [f"{cid}: {k}" for k in sorted(set(got) | set(want)) if k not in got or k not in want or not np.array_equal(got[k], want[k])]
        print("\n".join(["STALE: the reference gives something else now for"] + stale) if stale else f"{len(args.check)} cases regenerated: the fixture is current")
        sys.exit(1 if stale else 0)
    t0 = time.time()
    records, slowest = {}, (0.0, "")
    for cid in E.RECORDED:
        if args.only and not cid.startswith(args.only):
            continue
        t = time.time()
        records[cid] = record(cid)
        slowest = max(slowest, (time.time() - t, cid))
        print(f"  {cid}: {records[cid]['numbers'].tolist()} {time.time() - t:.1f} s", flush=True)
    print(f"{len(records)} cases in {time.time() - t0:.0f} s, slowest {slowest[1]} {slowest[0]:.1f} s, "
          f"peak {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6:.2f} GB")
    if not args.only:
        np.savez_compressed(HERE / "edges.npz", **E.pack_fixture(records))
        print(f"wrote {HERE / 'edges.npz'}: {(HERE / 'edges.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()

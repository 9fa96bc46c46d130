#!/usr/bin/env python3
r"""Routing fresh rows through a fitted tree (bbh_tree_route_packed) against the only way before: the
nearest centroid of the flat table (jt_assign_packed, what `predict` runs).  Results in profiles/route/.

Trees: the headline workload (bench.synth_fake_fps, threshold 0.3, branching factor 50) and the zipf workload at branching
factors 50 and 254, `--tree-rows` rows each.  Queries: 10^4, 10^5 and 10^6 fresh rows of the same generator under another
seed, resident on the device.  The two contenders alternate inside one process: one warm-up round, then `--repeats` rounds.

Timing: the library's own HIP events around its launches (bbh_profile_*: "tree_route" and "jt_assign"), so host-side
staging of the outputs is outside both.  The two answer different questions - the tree's own cluster against the globally
nearest centroid - so nothing is compared for equality; the share of queries whose routed cluster IS the nearest centroid
(same similarity) is reported as quality information.  Every step runs under its own time limit (SIGALRM with the default
action: a step that hangs ends the process).

    python tools/route_bench.py --out profiles/route/route_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import signal
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the workloads' generators)
from bblean_amd import BitBirch, _lib  # noqa: E402
from bblean_amd.similarity import jt_assign_packed  # noqa: E402

SIZES = (10_000, 100_000, 1_000_000)
TREES = (("fake", 50), ("zipf", 50), ("zipf", 254))
STEP_LIMIT = 300  # seconds


class step:
    r"""A time limit for the statements inside."""

    def __init__(self, seconds: int = STEP_LIMIT):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


def prof_ms(lib, name: str) -> float:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _lib.check(lib.bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return ms.value


def line_of(name: str, rounds: list[float], rows: int, extra: str = "") -> tuple[str, float]:
    med = statistics.median(rounds)
    spread = (max(rounds) - min(rounds)) / med * 100.0
    return f"    {name:22s} {med:10.3f} ms {rows / (med * 1e-3) / 1e6:10.3f} M rows/s  (spread {spread:4.1f} % of {len(rounds)} rounds){extra}", med


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tree-rows", type=int, default=1_000_000)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; trees of {args.tree_rows} 2048-bit rows (diameter merge); queries: fresh rows of the tree's "
             f"generator (seed 8 against 7), device-resident; median of {args.repeats} alternating rounds after 1 warm-up round; times by "
             "the library's HIP events (tree_route / jt_assign)"]
    print(lines[0], flush=True)
    for wname, bf in TREES:
        gen, thr, _ = bench.WORKLOADS[wname]
        with step(900):
            fps = gen(args.tree_rows, 7, dev)
            tree = BitBirch(branching_factor=bf, threshold=thr, merge_criterion="diameter").fit(fps)
            del fps
            order = tree._leaf_order(True)
            cents = tree._engine.gather_centroids(order, device_out=True)
            ids = tree._leaves()["ids"][order]
            pos_of_id = np.full(int(ids.max()) + 1, -1, np.int64)
            pos_of_id[ids] = np.arange(ids.size)
            st = [int(v) for v in tree._engine.stats()]
            queries = gen(max(args.sizes), 8, dev)
        K = int(cents.shape[0])
        head = (f"{wname}, branching factor {bf}, threshold {thr}: {K} clusters, {st[5]} nodes, depth {st[6]}, "
                f"{st[1] / max(st[0], 1):.1f} rows per node compare during the fit")
        lines.append(head)
        print(head, flush=True)
        for n in args.sizes:
            q = queries[:n].contiguous()
            r_rounds, a_rounds = [], []
            leaf = acc = inter = union = idx = ai = au = None
            for j in range(args.repeats + 1):
                with step():
                    _lib.check(lib.bbh_profile_reset())
                    leaf, acc, inter, union = tree._engine.route_packed(q)
                    r_ms = prof_ms(lib, "tree_route")
                    _lib.check(lib.bbh_profile_reset())
                    idx, ai, au = jt_assign_packed(q, cents, return_counts=True)
                    torch.cuda.synchronize()
                    a_ms = prof_ms(lib, "jt_assign")
                if j:
                    r_rounds.append(r_ms)
                    a_rounds.append(a_ms)
            idx, ai, au = idx.cpu().numpy(), ai.cpu().numpy().view(np.uint32).astype(np.int64), au.cpu().numpy().view(np.uint32).astype(np.int64)
            routed = pos_of_id[leaf.astype(np.int64)]
            assert (routed >= 0).all(), "a routed id that is no leaf"
            # the same similarity as the nearest centroid's (exact fractions): the routed cluster is A nearest centroid
            ri, ru = inter.astype(np.int64), np.maximum(union.astype(np.int64), 1)
            nearest = ri * np.maximum(au, 1) == ai * ru
            assert (ri * np.maximum(au, 1) <= ai * ru).all(), "a routed row more similar than the nearest centroid"
            lines.append(f"  {n} queries x {K} centroids ({n * K / 1e9:.2f} G pairs for the flat table)")
            t_r, m_r = line_of("tree_route", r_rounds, n, f"  accept {acc.mean() * 100:.1f} %")
            t_a, m_a = line_of("jt_assign (predict)", a_rounds, n, f"  {n * K / (statistics.median(a_rounds) * 1e-3) / 1e9:.1f} G pairs/s")
            lines += [t_r, t_a, f"    tree_route / jt_assign: {m_a / m_r:.1f} x the rows per second; routed cluster is a nearest centroid for "
                                f"{nearest.mean() * 100:.1f} % of the queries (the same index for {(routed == idx).mean() * 100:.1f} %)"]
            for ln in lines[-4:]:
                print(ln, flush=True)
        del tree, cents, queries
        torch.cuda.empty_cache()
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

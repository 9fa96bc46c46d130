#!/usr/bin/env python3
r"""Connected components at a radius on one MI355X against the only way before (results in
profiles/components/).

Two contenders, from device rows to labels on the host:
  (A) jt_radius_packed(c, c, r, exclude=arange) - the CSR of the threshold graph on the device - copied to the host, then
      scipy.sparse.csgraph.connected_components on it
  (B) jt_components_packed(c, r), its labels copied to the host
on 2048-bit random tables at three radii - sample quantiles of the table's distances that give about 1e-5, 1e-4 and 1e-3
hits per pair - and on the centroids of the 200 k-row and 1 M-row fits of the flagship workload at radius 1 - threshold.

Timing: wall clock between two device synchronisations, from the call to the host labels.  One process, two warm-up rounds,
then `--repeats` rounds in which the contenders alternate; the median is reported.  Before a rate is printed the two label
arrays are compared for equality.  Memory: the bytes each contender holds beside the table at its peak - on the device the
outputs of the call (torch's peak) plus the library's temporaries (from the shape, as include/bbhip.h documents them), on
the host the arrays it brings back.  Every step runs under its own time limit (SIGALRM with the default action: a step that
hangs ends the process) and the script stops at the first failing step.

    python tools/components_bench.py --out profiles/components/components_bench.txt
"""
from __future__ import annotations

import argparse
import signal
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.sparse import csr_matrix  # noqa: E402
from scipy.sparse.csgraph import connected_components  # noqa: E402

from bblean_amd.similarity import jt_components_packed, jt_dist_matrix_packed, jt_radius_packed  # noqa: E402

RATES = (1e-5, 1e-4, 1e-3)  # hits per pair the radii aim at
SIZES = (65536, 262144)     # rows of the random tables
SAMPLE = 4096               # rows of the sample the quantiles are taken from
STEP_LIMIT = 300            # seconds
EDGE_LIMIT = 1 << 30        # entries of the CSR beyond which (A) is left out (12 bytes each on the device, 12 on the host)


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


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base, out


def graph_way(c, radius: float):
    r"""(A) -> (labels, count, host bytes, library temporaries on the device, edges)."""
    n = int(c.shape[0])
    off, idx, dist = jt_radius_packed(c, c, radius, exclude=torch.arange(n, dtype=torch.int32, device=c.device))
    off_h, idx_h = off.cpu().numpy(), idx.cpu().numpy()
    del off, idx, dist
    count, labels = connected_components(csr_matrix((np.ones(len(idx_h), np.int8), idx_h, off_h), shape=(n, n)), directed=False)
    host = off_h.nbytes + idx_h.nbytes + len(idx_h) + labels.nbytes
    qblocks = (n + 255) // 256
    cus = torch.cuda.get_device_properties(c.device).multi_processor_count
    nsplit = max(1, min((4 * cus + qblocks - 1) // qblocks, (n + 63) // 64))  # the ranges of bbh_jt_radius
    return labels, count, host, 4 * n + 4 * nsplit * n + 4 * n, len(idx_h)


def components_way(c, radius: float):
    r"""(B) -> (labels, count, host bytes, library temporaries on the device)."""
    n = int(c.shape[0])
    labels_t, count = jt_components_packed(c, radius)
    labels = labels_t.cpu().numpy()
    return labels, count, labels.nbytes, 4 * n + 4 * n + 4 * n


def radii_of(c, rates) -> list[float]:
    r"""Realised distances at the sample quantiles `rates` (the head of the table against the rows after it)."""
    d = jt_dist_matrix_packed(c[:SAMPLE].contiguous(), c[SAMPLE:2 * SAMPLE].contiguous()).reshape(-1)
    out = [float(torch.kthvalue(d, max(1, int(r * d.numel()))).values) for r in rates]
    del d
    return out


def run(c, radius: float, args, lines: list[str], head: str) -> None:
    n = int(c.shape[0])
    pairs = n * (n - 1) / 2
    with step():
        ms_b, dev_b, (lab_b, count, host_b, tmp_b) = timed(lambda: components_way(c, radius))
    edges = 0
    contenders = {"(B) jt_components_packed": lambda: components_way(c, radius)}
    with step():
        ms_a, dev_a, res_a = timed(lambda: graph_way(c, radius)) if args.with_graph else (0.0, 0, None)
    if res_a is not None:
        lab_a, count_a, host_a, tmp_a, edges = res_a
        if not (count_a == count and lab_a.shape == lab_b.shape and bool((lab_a == lab_b).all())):
            raise SystemExit(f"the labels differ on {n} rows at {radius!r}: {count_a} and {count} components")
        if edges <= EDGE_LIMIT:
            contenders = {"(A) radius CSR + scipy": lambda: graph_way(c, radius), **contenders}
    head = f"{head}: {count} components" + (f", {edges} edges in the CSR, {edges / 2 / pairs:.2e} hits per pair" if res_a else "")
    for fn in contenders.values():  # warm-up 2
        with step():
            timed(fn)
    rounds = {name: [] for name in contenders}
    peak = {name: (0, 0) for name in contenders}
    for _ in range(args.repeats):
        for name, fn in contenders.items():
            with step():
                ms, dev, res = timed(fn)
            rounds[name].append(ms)
            peak[name] = (dev + res[3], res[2])
    lines.append(head)
    print(head, flush=True)
    med = {}
    for name in contenders:
        med[name] = statistics.median(rounds[name])
        spread = (max(rounds[name]) - min(rounds[name])) / med[name] * 100.0
        line = (f"    {name:26s} {med[name]:10.2f} ms {pairs / (med[name] * 1e-3) / 1e9:9.1f} G pairs/s  (spread {spread:4.1f} %)"
                f"  extra device {peak[name][0] / 2**20:9.1f} MiB, host {peak[name][1] / 2**20:9.1f} MiB")
        lines.append(line)
        print(line, flush=True)
    if len(med) == 2:
        a, b = (med[k] for k in contenders)
        line = f"    labels equal; time (A) / (B) = {a / b:.2f}"
        lines.append(line)
        print(line, flush=True)
    torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--tree-rows", type=int, nargs="*", default=[200_000, 1_000_000], help="rows of the fitted trees")
    ap.add_argument("--no-graph", dest="with_graph", action="store_false", help="leave contender (A) out")
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's rows by this (rehearsals)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines = [f"device: {torch.cuda.get_device_name(0)}; 2048-bit rows; wall clock from the call to the labels on the host, median "
             f"of {args.repeats} rounds after 2 warm-up rounds, the contenders alternating; pairs = n (n - 1) / 2; radii of the "
             "random tables: sample quantiles of their distances"]
    print(lines[0], flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in SIZES:
        n = max(2 * SAMPLE, n // args.scale)
        c = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device="cuda", generator=g)
        head = f"{n} random rows  ({n * (n - 1) / 2 / 1e9:.2f} G pairs)"
        lines.append(head)
        print(head, flush=True)
        with step():
            radii = radii_of(c, RATES)
        for radius in radii:
            run(c, radius, args, lines, f"  radius {radius!r}")
        del c
        torch.cuda.empty_cache()

    for rows in args.tree_rows:
        import bench  # the flagship workload's generator
        from bblean_amd import BitBirch

        thr = 0.3
        rows = max(1000, rows // args.scale)
        with step(600):
            fps = bench.synth_fake_fps(rows, 7, torch.device("cuda", 0))
            tree = BitBirch(branching_factor=50, threshold=thr, merge_criterion="diameter").fit(fps)
            cents = tree._engine.gather_centroids(tree._leaf_order(True), device_out=True)
            del fps, tree
        K = int(cents.shape[0])
        head = (f"{K} centroids of the {rows}-row tree (threshold {thr}, branching factor 50)  ({K * (K - 1) / 2 / 1e9:.2f} G pairs)")
        lines.append(head)
        print(head, flush=True)
        run(cents, 1.0 - thr, args, lines, f"  radius 1 - threshold = {1.0 - thr!r}")
        del cents
        torch.cuda.empty_cache()

    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

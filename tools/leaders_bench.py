#!/usr/bin/env python3
r"""Leader clustering at a radius on one MI355X against the only way before (results in
profiles/leaders/).

Two contenders, from device rows to labels on the host:
  (A) jt_radius_packed(c, c, r, exclude=arange) - the CSR of the threshold graph on the device - copied to the host, then
      the sequential sphere exclusion over the CSR (`csr_leaders` below)
  (B) jt_leaders_packed(c, r), its labels copied to the host
on the shapes of tools/components_bench.py: 2048-bit random tables at three radii (sample quantiles of the table's distances
that give about 1e-5, 1e-4 and 1e-3 hits per pair) and the centroids of the 200 k-row and 1 M-row fits of the flagship
workload at radius 1 - threshold, the 1 M-row fit's weighted by the clusters' sizes too.

Timing: wall clock between two device synchronisations, from the call to the host labels.  One process, two warm-up rounds,
then `--repeats` rounds in which the contenders alternate; the median is reported.  Before a rate is printed the two label
arrays are compared for equality.  After the timed rounds (B) runs once more with the library's profile on: rounds, the rows
that entered the tail (one stepping launch each), isolated rows and the milliseconds of every profile record.  Memory: the
bytes each contender holds beside the table at its peak - on the device the outputs of the call (torch's peak) plus the
library's temporaries (from the shape, as include/bbhip.h documents them), on the host the arrays it brings back or builds.

`--rule` adds the measurements behind the rule that starts the tail: (B) alone with BBHIP_LEADERS_ROUNDS unset and forced,
on the fitted trees' centroids, the random tables at their middle radius, a block model and the 32 764-row chain of
8 192-byte rows.

Every step runs under its own time limit (SIGALRM with the default action: a step that hangs ends the process) and the
script stops at the first failing step.

    python tools/leaders_bench.py --rule --out profiles/leaders/leaders_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes
import os
import signal
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bblean_amd import _lib  # noqa: E402
from bblean_amd.similarity import jt_dist_matrix_packed, jt_leaders_packed, jt_radius_packed  # noqa: E402

RATES = (1e-5, 1e-4, 1e-3)  # hits per pair the radii aim at
SIZES = (65536, 262144)     # rows of the random tables
SAMPLE = 4096               # rows of the sample the quantiles are taken from
STEP_LIMIT = 300            # seconds
EDGE_LIMIT = 1 << 30        # entries of the CSR beyond which (A) is left out
SWITCH = "BBHIP_LEADERS_ROUNDS"
RECORDS = ("jt_leaders/degree", "jt_leaders/round", "jt_leaders/step", "jt_leaders/assign", "jt_leaders")


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


def csr_leaders(off, idx, w):
    r"""The sequential sphere exclusion over a CSR on the host -> (labels, count, bytes built on the way)."""
    n = len(off) - 1
    cs = np.concatenate([np.zeros(1, np.int64), np.cumsum(w[idx], dtype=np.int64)])
    dens = w + cs[off[1:]] - cs[off[:-1]]
    order = np.lexsort((np.arange(n), -dens))
    centre = np.full(n, -1, np.int64)
    for p in order.tolist():
        if centre[p] >= 0:
            continue
        centre[p] = p
        nb = idx[off[p]:off[p + 1]]
        centre[nb[centre[nb] < 0]] = p
    is_c = centre == np.arange(n)
    rank = np.cumsum(is_c) - is_c
    return rank[centre], int(is_c.sum()), cs.nbytes + dens.nbytes + order.nbytes + centre.nbytes + rank.nbytes


def graph_way(c, radius: float, w):
    r"""(A) -> (labels, count, host bytes, library temporaries on the device, edges)."""
    n = int(c.shape[0])
    off, idx, dist = jt_radius_packed(c, c, radius, exclude=torch.arange(n, dtype=torch.int32, device=c.device))
    off_h, idx_h = off.cpu().numpy(), idx.cpu().numpy()
    del off, idx, dist
    wh = np.ones(n, np.int64) if w is None else w.cpu().numpy().astype(np.int64)
    labels, count, built = csr_leaders(off_h, idx_h, wh)
    host = off_h.nbytes + idx_h.nbytes + built + labels.nbytes
    qblocks = (n + 255) // 256
    cus = torch.cuda.get_device_properties(c.device).multi_processor_count
    nsplit = max(1, min((4 * cus + qblocks - 1) // qblocks, (n + 63) // 64))  # the ranges of bbh_jt_radius
    return labels, count, host, 4 * n + 4 * nsplit * n + 4 * n, len(idx_h)


def leaders_way(c, radius: float, w):
    r"""(B) -> (labels, count, host bytes, library temporaries on the device but for the working table)."""
    n = int(c.shape[0])
    labels_t, count = jt_leaders_packed(c, radius, weights=w)
    labels = labels_t.cpu().numpy()
    return labels, count, labels.nbytes + 12 * n, 20 * n


def profile_of(c, radius: float, w):
    r"""One call of (B) with the profile on -> (isolated rows, rounds, rows in the tail, {record: ms})."""
    lib = _lib.load()
    n = int(c.shape[0])
    lib.bbh_profile_enable(1)
    lib.bbh_profile_reset()
    try:
        _, _, dens = jt_leaders_packed(c, radius, weights=w, return_density=True)
        isolated = int((dens == (1 if w is None else w.to(torch.int64))).sum())
        if w is not None:  # (a row of weight w with neighbours of weight 0 only does not occur: cluster sizes are >= 1)
            assert int(w.min()) >= 1
        ms = {}
        cnt, t, u = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int64(0)
        for name in RECORDS:
            lib.bbh_profile_get(name.encode(), ctypes.byref(cnt), ctypes.byref(t))
            ms[name] = float(t.value)
            if name == "jt_leaders/round":
                rounds = int(cnt.value)
        lib.bbh_profile_units(b"jt_leaders/step", ctypes.byref(u))
    finally:
        lib.bbh_profile_reset()
        lib.bbh_profile_enable(0)
    return isolated, rounds, int(u.value), ms, n - isolated


def radii_of(c, rates) -> list[float]:
    r"""Realised distances at the sample quantiles `rates` (the head of the table against the rows after it)."""
    d = jt_dist_matrix_packed(c[:SAMPLE].contiguous(), c[SAMPLE:2 * SAMPLE].contiguous()).reshape(-1)
    out = [float(torch.kthvalue(d, max(1, int(r * d.numel()))).values) for r in rates]
    del d
    return out


def say(lines: list[str], line: str) -> None:
    lines.append(line)
    print(line, flush=True)


def run(c, radius: float, w, args, lines: list[str], head: str) -> None:
    n, nb = int(c.shape[0]), int(c.shape[1])
    pairs = n * (n - 1) / 2
    with step():
        ms_b, dev_b, (lab_b, count, host_b, tmp_b) = timed(lambda: leaders_way(c, radius, w))
    edges = 0
    contenders = {"(B) jt_leaders_packed": lambda: leaders_way(c, radius, w)}
    with step():
        ms_a, dev_a, res_a = timed(lambda: graph_way(c, radius, w)) if args.with_graph else (0.0, 0, None)
    if res_a is not None:
        lab_a, count_a, host_a, tmp_a, edges = res_a
        if not (count_a == count and lab_a.shape == lab_b.shape and bool((lab_a == lab_b).all())):
            raise SystemExit(f"the labels differ on {n} rows at {radius!r}: {count_a} and {count} clusters")
        if edges <= EDGE_LIMIT:
            contenders = {"(A) radius CSR + host loop": lambda: graph_way(c, radius, w), **contenders}
    with step():
        isolated, nrounds, tail, rec, active = profile_of(c, radius, w)
    wb = nb if nb > 256 else max(8, 1 << (nb - 1).bit_length())
    work = active * (wb + 32)  # the working table of (B): a copy of the rows with a neighbour and 32 bytes of bookkeeping each
    say(lines, f"{head}: {count} clusters" + (f", {edges} edges in the CSR, {edges / 2 / pairs:.2e} hits per pair" if res_a else ""))
    for fn in contenders.values():  # warm-up 2
        for _ in range(2):
            with step():
                timed(fn)
    rounds = {name: [] for name in contenders}
    peak = {name: (0, 0) for name in contenders}
    for _ in range(args.repeats):
        for name, fn in contenders.items():
            with step():
                ms, dev, res = timed(fn)
            rounds[name].append(ms)
            peak[name] = (dev + res[3] + (work if name.startswith("(B)") else 0), res[2] + (4 * active if name.startswith("(B)") else 0))
    med = {}
    for name in contenders:
        med[name] = statistics.median(rounds[name])
        spread = (max(rounds[name]) - min(rounds[name])) / med[name] * 100.0
        say(lines, f"    {name:26s} {med[name]:10.2f} ms {pairs / (med[name] * 1e-3) / 1e9:9.1f} G pairs/s  (spread {spread:4.1f} %)"
                   f"  extra device {peak[name][0] / 2**20:9.1f} MiB, host {peak[name][1] / 2**20:9.1f} MiB")
    if len(med) == 2:
        a, b = (med[k] for k in contenders)
        say(lines, f"    labels equal; time (A) / (B) = {a / b:.2f}")
    say(lines, f"    (B): {isolated} isolated rows, {active} ranked; {nrounds} rounds, {tail} rows entered the tail (one stepping launch each); "
               + ", ".join(f"{k} {v:.2f} ms" for k, v in rec.items()))
    torch.cuda.empty_cache()


def rule(c, radius: float, w, lines: list[str], head: str, forced=(0, 2, 4, 8, 16, 64), calls: int = 3) -> None:
    r"""(B) alone: the built-in rule against forced numbers of rounds; the labels must not move."""
    say(lines, head)
    ref = None
    for k in (None,) + tuple(forced):
        if k is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = str(k)
        try:
            with step(600):
                timed(lambda: leaders_way(c, radius, w))
                ts = [timed(lambda: leaders_way(c, radius, w)) for _ in range(calls)]
                isolated, nrounds, tail, rec, active = profile_of(c, radius, w)
        finally:
            os.environ.pop(SWITCH, None)
        labels = ts[-1][2][0]
        if ref is None:
            ref = labels
        elif not bool((labels == ref).all()):
            raise SystemExit(f"{head}: the labels depend on {SWITCH}={k}")
        say(lines, f"    {SWITCH}={'unset' if k is None else k:>5}: {statistics.median(t[0] for t in ts):10.2f} ms; {nrounds} rounds, {tail} rows "
                   f"entered the tail; " + ", ".join(f"{n.split('/')[-1]} {v:.2f}" for n, v in rec.items()) + " ms")
    torch.cuda.empty_cache()


def block_model(n: int, centres: int, flip: float, g) -> "torch.Tensor":
    r"""n 2048-bit rows, each one of `centres` random rows with every bit flipped with probability `flip`."""
    base = torch.randint(0, 2, (centres, 2048), dtype=torch.uint8, device="cuda", generator=g)
    which = torch.randint(0, centres, (n,), device="cuda", generator=g)
    bits = base[which] ^ (torch.rand((n, 2048), device="cuda", generator=g) < flip).to(torch.uint8)
    weights = (1 << torch.arange(7, -1, -1, device="cuda", dtype=torch.int32)).to(torch.uint8)
    return (bits.reshape(n, 256, 8) * weights).sum(-1).to(torch.uint8).contiguous()


def chain(n: int, nb: int) -> "torch.Tensor":
    r"""components_refs' chain pattern: row k has bits [2k, 2k + 8); neighbours are at 0.4, rows two apart at 2 / 3."""
    assert 2 * n + 6 <= nb * 8
    bits = torch.zeros((n, nb * 8), dtype=torch.uint8, device="cuda")
    k = torch.arange(n, device="cuda")
    for j in range(8):
        bits[k, 2 * k + j] = 1
    weights = (1 << torch.arange(7, -1, -1, device="cuda", dtype=torch.int32)).to(torch.uint8)
    return (bits.reshape(n, nb, 8) * weights).sum(-1).to(torch.uint8).contiguous()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--tree-rows", type=int, nargs="*", default=[200_000, 1_000_000], help="rows of the fitted trees")
    ap.add_argument("--no-graph", dest="with_graph", action="store_false", help="leave contender (A) out")
    ap.add_argument("--no-random", dest="with_random", action="store_false", help="leave the random tables out")
    ap.add_argument("--rule", action="store_true", help="add the measurements behind the rule that starts the tail")
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's rows by this (rehearsals)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lines: list[str] = []

    def flush() -> None:
        if args.out is not None:
            args.out.parent.mkdir(parents=True, exist_ok=True)
            args.out.write_text("\n".join(lines) + "\n")

    say(lines, f"device: {torch.cuda.get_device_name(0)}; 2048-bit rows; wall clock from the call to the labels on the host, median "
               f"of {args.repeats} rounds after 2 warm-up rounds, the contenders alternating; pairs = n (n - 1) / 2; radii of the "
               "random tables: sample quantiles of their distances")
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in SIZES if args.with_random else ():
        n = max(2 * SAMPLE, n // args.scale)
        c = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device="cuda", generator=g)
        say(lines, f"{n} random rows  ({n * (n - 1) / 2 / 1e9:.2f} G pairs)")
        with step():
            radii = radii_of(c, RATES)
        for radius in radii:
            run(c, radius, None, args, lines, f"  radius {radius!r}")
            flush()
        del c
        torch.cuda.empty_cache()

    tables = []
    for rows in args.tree_rows:
        import bench  # the flagship workload's generator
        from bblean_amd import BitBirch

        thr = 0.3
        rows = max(1000, rows // args.scale)
        with step(600):
            fps = bench.synth_fake_fps(rows, 7, torch.device("cuda", 0))
            tree = BitBirch(branching_factor=50, threshold=thr, merge_criterion="diameter").fit(fps)
            order = tree._leaf_order(True)
            cents = tree._engine.gather_centroids(order, device_out=True)
            sizes = torch.from_numpy(np.asarray(tree._leaves()["n"], dtype=np.int64)[order]).cuda()
            del fps, tree
        K = int(cents.shape[0])
        say(lines, f"{K} centroids of the {rows}-row tree (threshold {thr}, branching factor 50)  ({K * (K - 1) / 2 / 1e9:.2f} G pairs)")
        run(cents, 1.0 - thr, None, args, lines, f"  radius 1 - threshold = {1.0 - thr!r}, unweighted")
        flush()
        if rows == max(args.tree_rows) // args.scale or len(args.tree_rows) == 1:
            run(cents, 1.0 - thr, sizes, args, lines, f"  radius 1 - threshold = {1.0 - thr!r}, weighted by the clusters' sizes")
            flush()
        tables.append((f"{K} centroids of the {rows}-row tree at {1.0 - thr!r}, weighted", cents, 1.0 - thr, sizes))

    if args.rule:
        say(lines, f"the rule that starts the tail: (B) alone, median of 3 calls after one (the chain: one call after one), {SWITCH} unset (the built-in rule) and forced")
        for head, c, radius, w in tables:
            rule(c, radius, w, lines, "  " + head, forced=(2, 4, 8, 16, 64))
            flush()
        for n in SIZES:
            n = max(2 * SAMPLE, n // args.scale)
            c = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
            with step():
                radius = radii_of(c, RATES)[1]
            rule(c, radius, None, lines, f"  {n} random rows at {radius!r}", forced=(4, 16, 64), calls=1)
            flush()
            del c
        n = max(2000, 65536 // args.scale)
        rule(block_model(n, max(8, n // 40), 0.04, g), 0.14, None, lines, f"  block model: {n} rows around {max(8, n // 40)} centres, 4 % of the bits flipped, radius 0.14")
        flush()
        n = max(1000, 32764 // args.scale)
        rule(chain(n, 8192), 0.4, None, lines, f"  chain: {n} rows of 8192 bytes, ascending, radius 0.4", forced=(0, 8), calls=1)
    flush()


if __name__ == "__main__":
    main()

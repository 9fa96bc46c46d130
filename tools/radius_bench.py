#!/usr/bin/env python3
r"""Radius search on one MI355X against its neighbours (results in profiles/radius/).

For 2048-bit random device rows, each shape runs at three radii - sample quantiles of its distances that give about 1e-5,
1e-3 and 1e-1 hits per pair - through
  (a) bbh_jt_radius in one call (the capacity suffices: count pass, scans, fill pass) and in two calls (a pure count with
      capacity 0, then the call at the exact capacity: two count passes and one fill pass), reported separately
  (b) bbh_jt_assign, BBHIP_ASSIGN=bcnt: the same inner loop, once, without table lookup or output - the bare loop
  (c) the only way to the same answer without bbh_jt_radius: jt_dist_matrix_packed on device rows in query chunks whose
      float64 matrix fits `--chunk-gib`, then torch.nonzero(d <= r) on the device
and the centroids of the fitted 1 M-row tree run against themselves at radius 1 - threshold.

Timing: the library's own HIP events around its launches (bbh_profile_*; for bbh_jt_radius they enclose the host's look at
the total between the passes); the matrix path, which is partly torch's, between two torch events on the same stream.  One
process, two warm-up rounds, then `--repeats` rounds in which the contenders alternate; a small shape is called repeatedly
inside a round until the round holds about `--window` seconds of device work.  Before a rate is printed the results are
compared: offsets and indices of the one-call and two-call variants with each other and with the rows and columns of
torch.nonzero.  Every step runs under its own time limit (SIGALRM with the default action: a step that hangs ends the
process) and the script stops at the first failing step.

    python tools/radius_bench.py --out profiles/radius/radius_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import signal
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bblean_amd import _lib  # noqa: E402
from bblean_amd.similarity import jt_dist_matrix_packed  # noqa: E402

RATES = (1e-5, 1e-3, 1e-1)  # hits per pair the radii aim at
SHAPES = [(1 << 20, 1000), (16384, 16384), (4096, 1 << 18), (8192, 1 << 20)]  # profiles/topk/topk_bench.txt's
SAMPLE = 4096       # rows of each side in the sample the quantiles are taken from
STEP_LIMIT = 180    # seconds
FILL_LIMIT = 24 << 30  # bytes of (idx, inter, union) beyond which only the count is timed


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


class Bench:
    def __init__(self, q, c, chunk_bytes: int, exclude=None):
        self.lib = _lib.load()
        self.q, self.c, self.ex = q, c, exclude
        self.nq, self.nc = int(q.shape[0]), int(c.shape[0])
        self.st = torch.cuda.current_stream().cuda_stream
        self.off = torch.empty(self.nq + 1, dtype=torch.int64, device="cuda")
        self.total = np.zeros(1, np.int64)
        self.out = None
        self.chunk = max(1, min(self.nq, chunk_bytes // (8 * self.nc)))

    def call(self, radius: float, capacity: int) -> int:
        o = self.out
        fill = capacity > 0
        _lib.check(self.lib.bbh_jt_radius(self.q.data_ptr(), self.nq, 256, self.c.data_ptr(), self.nc, 256, radius,
                                          None if self.ex is None else self.ex.data_ptr(), capacity, self.off.data_ptr(),
                                          self.total.ctypes.data, o[0].data_ptr() if fill else None,
                                          o[1].data_ptr() if fill else None, o[2].data_ptr() if fill else None, self.st))
        return int(self.total[0])

    def room(self, total: int) -> None:
        self.out = None
        torch.cuda.empty_cache()
        self.out = torch.empty((3, max(1, total)), dtype=torch.int32, device="cuda")

    def count(self, radius: float, reps: int = 1):
        _lib.check(self.lib.bbh_profile_reset())
        for _ in range(reps):
            total = self.call(radius, 0)
        return prof_ms(self.lib, "jt_radius"), total

    def one_call(self, radius: float, total: int, reps: int = 1):
        _lib.check(self.lib.bbh_profile_reset())
        for _ in range(reps):
            assert self.call(radius, max(1, total)) == total
        return prof_ms(self.lib, "jt_radius"), (self.off, self.out[0][:total])

    def two_calls(self, radius: float, total: int, reps: int = 1):
        _lib.check(self.lib.bbh_profile_reset())
        for _ in range(reps):
            n = self.call(radius, 0)
            assert n == total and self.call(radius, max(1, n)) == n
        return prof_ms(self.lib, "jt_radius"), (self.off, self.out[0][:total])

    def assign(self, reps: int = 1):
        os.environ["BBHIP_ASSIGN"] = "bcnt"  # (the library reads it with getenv at every call)
        _lib.check(self.lib.bbh_profile_reset())
        idx = torch.empty(self.nq, dtype=torch.int32, device="cuda")
        for _ in range(reps):
            _lib.check(self.lib.bbh_jt_assign(self.q.data_ptr(), self.nq, 256, self.c.data_ptr(), self.nc, 256,
                                              idx.data_ptr(), None, None, self.st))
        os.environ.pop("BBHIP_ASSIGN", None)
        return prof_ms(self.lib, "jt_assign"), idx

    def matrix(self, radius: float, reps: int = 1, keep: bool = False):
        r"""The distance matrix chunk by chunk, then torch.nonzero; with `keep` the (rows, columns) of all chunks."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kept = []
        a.record()
        for _ in range(reps):
            for lo in range(0, self.nq, self.chunk):
                d = jt_dist_matrix_packed(self.q[lo:lo + self.chunk], self.c)
                hit = d <= radius
                if self.ex is not None:
                    hit[torch.arange(hit.shape[0], device="cuda"), self.ex[lo:lo + self.chunk].long()] = False
                nz = torch.nonzero(hit)
                del d, hit
                if keep:
                    kept.append((nz[:, 0] + lo, nz[:, 1]))
        b.record()
        b.synchronize()
        return a.elapsed_time(b), kept


def radii_of(q, c, rates) -> list[float]:
    r"""Realised distances at the sample quantiles `rates` (SAMPLE x SAMPLE pairs from the heads of both sides)."""
    d = jt_dist_matrix_packed(q[:SAMPLE].contiguous(), c[:SAMPLE].contiguous()).reshape(-1)
    out = [float(torch.kthvalue(d, max(1, int(r * d.numel()))).values) for r in rates]
    del d
    return out


def fmt(rounds: list[float], pairs: float, reps: int) -> tuple[str, float]:
    per_call = [r / reps for r in rounds]
    med = statistics.median(per_call)
    rate = pairs / (med * 1e-3) / 1e9
    spread = (max(per_call) - min(per_call)) / med * 100.0
    return f"{med:10.3f} ms {rate:9.1f} G pairs/s  (spread {spread:4.1f} %, {reps} calls/round)", rate


def run_radius(b: Bench, radius: float, with_matrix: bool, args, lines: list[str], head: str, assign_rate: float | None):
    nq, nc = b.nq, b.nc
    with step():
        total = b.count(radius)[1]
    fill = total * 12 <= FILL_LIMIT
    head = f"{head}: {total} hits, {total / (float(nq) * nc):.2e} per pair"
    contenders = {"radius count only": lambda r=1: b.count(radius, r)}
    if fill:
        with step():
            b.room(total)
        contenders["radius one call"] = lambda r=1: b.one_call(radius, total, r)
        contenders["radius two calls"] = lambda r=1: b.two_calls(radius, total, r)
        if with_matrix:
            contenders["matrix+nonzero"] = lambda r=1: b.matrix(radius, r)
    else:
        head += f"  (outputs of {total * 12 / 2**30:.0f} GiB: the count alone is timed)"
    reps = {}
    for name, fn in contenders.items():  # warm-up 1: correctness and the number of calls a round needs
        with step():
            ms, res = fn()
            torch.cuda.synchronize()
            reps[name] = max(1, min(2000, int(args.window * 1e3 / max(ms, 1e-3)) + 1))
    if fill:
        with step():
            off1, idx1 = (t.clone() for t in b.one_call(radius, total)[1])
            off2, idx2 = b.two_calls(radius, total)[1]
            torch.cuda.synchronize()
            if not (bool((off1 == off2).all()) and bool((idx1 == idx2).all())):
                raise SystemExit(f"one call and two calls differ on {nq} x {nc} at {radius}")
            if with_matrix:
                kept = b.matrix(radius, 1, keep=True)[1]
                rows = torch.cat([k[0] for k in kept])
                cols = torch.cat([k[1] for k in kept])
                counts = torch.bincount(rows, minlength=nq)
                if not (len(cols) == total and bool((cols == idx1).all())
                        and bool((torch.cumsum(counts, 0) == off1[1:]).all())):
                    raise SystemExit(f"matrix+nonzero differs from bbh_jt_radius on {nq} x {nc} at {radius}")
                del kept, rows, cols, counts
            del off1, idx1
    for name, fn in contenders.items():  # warm-up 2
        with step():
            fn(reps[name])
            torch.cuda.synchronize()
    rounds: dict[str, list[float]] = {n: [] for n in contenders}
    for _ in range(args.repeats):
        for name, fn in contenders.items():
            with step():
                rounds[name].append(fn(reps[name])[0])
                torch.cuda.synchronize()
    lines.append(head)
    print(head, flush=True)
    rates = {}
    for name in contenders:
        text, rates[name] = fmt(rounds[name], float(nq) * nc, reps[name])
        extra = "  offsets and indices equal to bbh_jt_radius" if name == "matrix+nonzero" else ""
        line = f"    {name:18s} {text}{extra}"
        lines.append(line)
        print(line, flush=True)
    parts = []
    if assign_rate is not None:
        parts += [f"assign/bcnt / {n} {assign_rate / rates[n]:.2f}" for n in rates if n.startswith("radius")]
    if "matrix+nonzero" in rates:
        parts += [f"{n} / matrix+nonzero {rates[n] / rates['matrix+nonzero']:.2f}" for n in ("radius one call", "radius two calls")]
    if parts:
        line = "    rate ratios: " + ", ".join(parts)
        lines.append(line)
        print(line, flush=True)
    b.out = None
    torch.cuda.empty_cache()


def run_assign(b: Bench, args, lines: list[str]) -> float:
    with step():
        ms = b.assign()[0]
        torch.cuda.synchronize()
    reps = max(1, min(2000, int(args.window * 1e3 / max(ms, 1e-3)) + 1))
    rounds = []
    for j in range(args.repeats + 1):
        with step():
            ms = b.assign(reps)[0]
            torch.cuda.synchronize()
        if j:  # the first round is the second warm-up
            rounds.append(ms)
    text, rate = fmt(rounds, float(b.nq) * b.nc, reps)
    line = f"  {'assign/bcnt':20s} {text}"
    lines.append(line)
    print(line, flush=True)
    return rate


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--chunk-gib", type=float, default=4.0, help="float64 distance matrix of one query chunk")
    ap.add_argument("--tree-rows", type=int, default=1_000_000, help="rows of the fitted tree (0 skips it)")
    ap.add_argument("--no-tree-matrix", action="store_true", help="leave matrix+nonzero out of the tree's centroid table")
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's sides by this (rehearsals)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    chunk_bytes = int(args.chunk_gib * 2**30)
    lines = [f"device: {torch.cuda.get_device_name(0)}; 2048-bit random rows; median of {args.repeats} rounds after 2 warm-up "
             "rounds; radius and assign by the library's HIP events, matrix+nonzero (jt_dist_matrix_packed in query chunks of "
             f"at most {args.chunk_gib:g} GiB, then torch.nonzero(d <= r)) between two device events; radii: sample quantiles of "
             "the shape's distances"]
    print(lines[0], flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for nq, nc in SHAPES:
        nq, nc = max(64, nq // args.scale), max(64, nc // args.scale)
        q = torch.randint(0, 256, (nq, 256), dtype=torch.uint8, device="cuda", generator=g)
        c = torch.randint(0, 256, (nc, 256), dtype=torch.uint8, device="cuda", generator=g)
        b = Bench(q, c, chunk_bytes)
        head = f"{nq} x {nc}  ({nq * nc / 1e9:.2f} G pairs, matrix {nq * nc * 8 / 2**30:.1f} GiB in chunks of {b.chunk} queries)"
        lines.append(head)
        print(head, flush=True)
        assign_rate = run_assign(b, args, lines)
        with step():
            radii = radii_of(q, c, RATES)
        for radius in radii:
            run_radius(b, radius, True, args, lines, f"  radius {radius!r}", assign_rate)
        del q, c, b
        torch.cuda.empty_cache()

    if args.tree_rows:
        import bench  # the flagship workload's generator
        from bblean_amd import BitBirch

        thr = 0.3
        with step(600):
            fps = bench.synth_fake_fps(args.tree_rows, 7, torch.device("cuda", 0))
            tree = BitBirch(branching_factor=50, threshold=thr, merge_criterion="diameter").fit(fps)
            cents = tree._engine.gather_centroids(tree._leaf_order(True), device_out=True)
            del fps
        K = int(cents.shape[0])
        ex = torch.arange(K, dtype=torch.int32, device="cuda")
        head = (f"{K} x {K}  ({K * K / 1e9:.2f} G pairs): the centroids of the {args.tree_rows}-row tree (threshold {thr}, branching "
                f"factor 50) against themselves, each without itself; the matrix would be {K * K * 8 / 2**40:.2f} TiB")
        lines.append(head)
        print(head, flush=True)
        run_radius(Bench(cents, cents, chunk_bytes, ex), 1.0 - thr, not args.no_tree_matrix,
                   args, lines, f"  radius 1 - threshold = {1.0 - thr!r}", None)

    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

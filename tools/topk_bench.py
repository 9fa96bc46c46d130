#!/usr/bin/env python3
r"""Top-k nearest rows on one MI355X against its neighbours (results in profiles/topk/).

For 2048-bit random device rows, each shape runs through
  (a) bbh_jt_topk at k = 1, 10 and 64
  (b) bbh_jt_assign, BBHIP_ASSIGN=bcnt: the same inner loop without a list - what selection costs
  (c) the only way to the same answer without bbh_jt_topk: jt_dist_matrix_packed on device rows, then
      torch.topk(..., largest=False) on the device (where the nq x nc float64 matrix fits)
and the centroids of the fitted 1 M-row tree run against themselves at k = 10.

Timing: the library's own HIP events around its launches (bbh_profile_*); the matrix path, which is partly torch's, between
two torch events on the same stream.  One process, two warm-up rounds, then `--repeats` rounds in which the contenders
alternate; a small shape is called repeatedly inside a round until the round holds about `--window` seconds of device work.
Before a rate is printed the indices are compared: top-k at k = 1 with assign, and the matrix path with top-k on every
query whose k + 1 smallest distances are distinct (torch.topk does not order ties), its distances on all of them.  Every
step runs under its own time limit (SIGALRM with the default action: a step that hangs ends the process) and the script
stops at the first failing step.

    python tools/topk_bench.py --out profiles/topk/topk_bench.txt
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

import torch  # noqa: E402

from bblean_amd import _lib  # noqa: E402
from bblean_amd.similarity import jt_dist_matrix_packed  # noqa: E402

KS = (1, 10, 64)
# (nq, nc, the matrix path runs)
SHAPES = [(1 << 20, 1000, True), (16384, 16384, True), (4096, 1 << 18, True), (8192, 1 << 20, False)]
STEP_LIMIT = 120  # seconds


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
    def __init__(self, q, c, exclude=None):
        self.lib = _lib.load()
        self.q, self.c, self.ex = q, c, exclude
        self.nq, self.nc = int(q.shape[0]), int(c.shape[0])
        self.st = torch.cuda.current_stream().cuda_stream
        self.out = {k: torch.empty((3, self.nq, k), dtype=torch.int32, device="cuda") for k in KS}

    def topk(self, k: int, reps: int = 1):
        lib, o = self.lib, self.out[k]
        _lib.check(lib.bbh_profile_reset())
        for _ in range(reps):
            _lib.check(lib.bbh_jt_topk(self.q.data_ptr(), self.nq, 256, self.c.data_ptr(), self.nc, 256, k,
                                       None if self.ex is None else self.ex.data_ptr(), o[0].data_ptr(), o[1].data_ptr(),
                                       o[2].data_ptr(), self.st))
        return prof_ms(lib, "jt_topk"), o

    def assign(self, reps: int = 1):
        lib, o = self.lib, self.out[1]
        os.environ["BBHIP_ASSIGN"] = "bcnt"  # (the library reads it with getenv at every call; a cached value would not see this)
        _lib.check(lib.bbh_profile_reset())
        idx = torch.empty(self.nq, dtype=torch.int32, device="cuda")
        for _ in range(reps):
            _lib.check(lib.bbh_jt_assign(self.q.data_ptr(), self.nq, 256, self.c.data_ptr(), self.nc, 256, idx.data_ptr(),
                                         None, None, self.st))
        os.environ.pop("BBHIP_ASSIGN", None)
        return prof_ms(lib, "jt_assign"), idx

    def matrix(self, k: int, reps: int = 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            d = jt_dist_matrix_packed(self.q, self.c)
            val, idx = torch.topk(d, k, dim=1, largest=False, sorted=True)
            del d
        b.record()
        b.synchronize()
        return a.elapsed_time(b), (idx, val)


def dist_of(o):
    i, u = o[1].double(), o[2].double()
    return torch.where(o[2] == 0, 0.0, (u - i) / u)


def fmt(rounds: list[float], pairs: float, reps: int) -> tuple[str, float, float]:
    per_call = [r / reps for r in rounds]
    med = statistics.median(per_call)
    rate = pairs / (med * 1e-3) / 1e9
    spread = (max(per_call) - min(per_call)) / med * 100.0
    return f"{med:10.3f} ms {rate:9.1f} G pairs/s  (spread {spread:4.1f} %, {reps} calls/round)", rate, spread


def run_shape(b: Bench, with_matrix: bool, ks, args, lines: list[str], head: str, with_assign: bool = True) -> None:
    nq, nc = b.nq, b.nc
    contenders = {}
    if with_assign:
        contenders["assign/bcnt"] = lambda r=1: b.assign(r)
    for k in ks:
        contenders[f"topk k={k}"] = lambda r=1, k=k: b.topk(k, r)
    if with_matrix:
        for k in ks:
            contenders[f"matrix+topk k={k}"] = lambda r=1, k=k: b.matrix(k, r)
    reps, checked = {}, {}
    for name, fn in contenders.items():  # warm-up 1: correctness and the number of calls a round needs
        with step():
            ms, res = fn()
            torch.cuda.synchronize()
            if name == "topk k=1" and with_assign:
                if not bool((res[0][:, 0] == b.assign()[1]).all()):
                    raise SystemExit(f"{name}: indices differ from assign on {nq} x {nc}")
            if name.startswith("matrix"):
                k = int(name.split("=")[1])
                o = b.topk(k)[1]
                torch.cuda.synchronize()
                idx, val = res
                if not bool((val == dist_of(o)).all()):
                    raise SystemExit(f"{name}: distances differ from top-k on {nq} x {nc}")
                if k + 1 <= nc:  # rows without a tie among the k + 1 smallest: the indices must be equal
                    d = jt_dist_matrix_packed(b.q, b.c)
                    v1 = torch.topk(d, k + 1, dim=1, largest=False, sorted=True)[0]
                    del d
                    clear = (v1[:, 1:] != v1[:, :-1]).all(dim=1)
                else:
                    clear = (val[:, 1:] != val[:, :-1]).all(dim=1) if k > 1 else torch.ones(nq, dtype=torch.bool, device="cuda")
                if not bool((idx[clear] == o[0][clear]).all()):
                    raise SystemExit(f"{name}: indices differ from top-k on {nq} x {nc}")
                checked[name] = int(clear.sum())
            reps[name] = max(1, min(2000, int(args.window * 1e3 / max(ms, 1e-3)) + 1))
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
    rates, spreads = {}, {}
    for name in contenders:
        text, rates[name], spreads[name] = fmt(rounds[name], float(nq) * nc, reps[name])
        extra = f"  indices equal on the {checked[name]} queries without ties, distances on all" if name in checked else ""
        line = f"  {name:18s} {text}{extra}"
        lines.append(line)
        print(line, flush=True)
    parts = []
    if with_assign:
        parts += [f"assign/bcnt / topk k={k} {rates['assign/bcnt'] / rates[f'topk k={k}']:.2f}" for k in ks]
    if with_matrix:
        parts += [f"topk / matrix+topk k={k} {rates[f'topk k={k}'] / rates[f'matrix+topk k={k}']:.2f}" for k in ks]
    if parts:
        line = "  rate ratios: " + ", ".join(parts)
        lines.append(line)
        print(line, flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--tree-rows", type=int, default=1_000_000, help="rows of the fitted tree (0 skips it)")
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's sides by this (rehearsals)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    lines = [f"device: {torch.cuda.get_device_name(0)}; 2048-bit random rows; median of {args.repeats} rounds after 2 warm-up "
             "rounds; top-k and assign by the library's HIP events, matrix+topk (jt_dist_matrix_packed, then torch.topk) "
             "between two device events"]
    print(lines[0], flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for nq, nc, with_matrix in SHAPES:
        nq, nc = max(64, nq // args.scale), max(64, nc // args.scale)
        q = torch.randint(0, 256, (nq, 256), dtype=torch.uint8, device="cuda", generator=g)
        c = torch.randint(0, 256, (nc, 256), dtype=torch.uint8, device="cuda", generator=g)
        head = f"{nq} x {nc}  ({nq * nc / 1e9:.2f} G pairs" + (f", matrix {nq * nc * 8 / 2**30:.1f} GiB)" if with_matrix else
                                                                f"; the matrix would be {nq * nc * 8 / 2**30:.0f} GiB: top-k alone)")
        run_shape(Bench(q, c), with_matrix, KS, args, lines, head)
        del q, c
        torch.cuda.empty_cache()

    if args.tree_rows:
        import bench  # the flagship workload's generator
        from bblean_amd import BitBirch

        with step(600):
            fps = bench.synth_fake_fps(args.tree_rows, 7, torch.device("cuda", 0))
            tree = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter").fit(fps)
            cents = tree._engine.gather_centroids(tree._leaf_order(True), device_out=True)
            del fps
        K = int(cents.shape[0])
        ex = torch.arange(K, dtype=torch.int32, device="cuda")
        head = (f"{K} x {K}  ({K * K / 1e9:.2f} G pairs): the centroids of the {args.tree_rows}-row tree (threshold 0.3, branching "
                f"factor 50) against themselves, each without itself; the matrix would be {K * K * 8 / 2**40:.2f} TiB")
        run_shape(Bench(cents, cents, ex), False, (10,), args, lines, head, with_assign=False)

    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

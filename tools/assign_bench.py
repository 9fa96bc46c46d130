#!/usr/bin/env python3
r"""A/B of the assignment kernels on one MI355X (results in profiles/predict/).

For 2048-bit random device rows, each shape runs through
  (a) bbh_jt_best_match          the batched node compare, the baseline (centroids in halves where nc > 2^20)
  (b) bbh_jt_assign, BBHIP_ASSIGN=bcnt   AND + popcount over a 2-D grid
  (c) bbh_jt_assign, BBHIP_ASSIGN=mfma   int8 matrix cores
and bbh_jt_dist_matrix runs against bbh_jt_best_match with its full similarity matrix.

Timing: the library's own HIP events around each launch (bbh_profile_*), one process, two warm-up rounds, then
`--repeats` rounds in which the kernels alternate; a small shape is called repeatedly inside a round until the round
holds at least `--window` seconds of device work per kernel.  The rate of a kernel is pairs / median round time.
Before any rate is printed the indices of (a), (b) and (c) are compared for equality (random rows, none all-zero, so
the two orderings agree).  The script stops at the first failing step.

    python tools/assign_bench.py --out profiles/predict/assign_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from bblean_amd import _lib  # noqa: E402

INT8_SPEC_PAIRS = 2.5e15 / 2048  # ~5 P int8 op/s dense = 2.5e15 multiply-adds/s; 2048 of them per pair
SHAPES = [(1 << 20, 1000), (1 << 20, 100_000), (8192, 1 << 20), (256, 50_000)]
LIMIT = 1 << 20  # bbh_jt_best_match refuses more centroid rows


def prof_ms(lib, name: str) -> float:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _lib.check(lib.bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return ms.value


class Bench:
    def __init__(self, q, c):
        self.lib = _lib.load()
        self.q, self.c = q, c
        self.nq, self.nc = int(q.shape[0]), int(c.shape[0])
        self.st = torch.cuda.current_stream().cuda_stream
        self.idx = torch.empty(self.nq, dtype=torch.int32, device="cuda")
        self.n = torch.empty(self.nq, dtype=torch.int32, device="cuda")
        self.u = torch.empty(self.nq, dtype=torch.int32, device="cuda")

    def best_match(self, reps: int = 1) -> tuple[float, torch.Tensor]:
        r"""(ms of device work, indices).  nc > 2^20: two halves, combined by exact cross-multiplication (untimed)."""
        lib = self.lib
        _lib.check(lib.bbh_profile_reset())
        halves = [(0, self.nc)] if self.nc <= LIMIT else [(0, self.nc // 2), (self.nc // 2, self.nc)]
        outs = []
        for _ in range(reps):
            outs = []
            for lo, hi in halves:
                i = torch.empty(self.nq, dtype=torch.int32, device="cuda")
                n = torch.empty_like(i)
                u = torch.empty_like(i)
                _lib.check(lib.bbh_jt_best_match(self.q.data_ptr(), self.nq, self.c[lo:hi].data_ptr(), hi - lo, 256,
                                                 i.data_ptr(), n.data_ptr(), u.data_ptr(), None, self.st))
                outs.append((i.long() + lo, n.long(), u.long()))
        ms = prof_ms(lib, "jt_best_match")
        i, n, u = outs[0]
        for i2, n2, u2 in outs[1:]:
            second = n2 * u > n * u2  # strict: ties stay with the lower half
            i, n, u = torch.where(second, i2, i), torch.where(second, n2, n), torch.where(second, u2, u)
        return ms, i.int()

    def assign(self, mode: str, reps: int = 1) -> tuple[float, torch.Tensor]:
        lib = self.lib
        os.environ["BBHIP_ASSIGN"] = mode
        _lib.check(lib.bbh_profile_reset())
        for _ in range(reps):
            _lib.check(lib.bbh_jt_assign(self.q.data_ptr(), self.nq, 256, self.c.data_ptr(), self.nc, 256,
                                         self.idx.data_ptr(), self.n.data_ptr(), self.u.data_ptr(), self.st))
        os.environ.pop("BBHIP_ASSIGN", None)
        return prof_ms(lib, "jt_assign"), self.idx.clone()


def fmt(rounds: list[float], pairs: float, reps: int) -> tuple[str, float]:
    per_call = [r / reps for r in rounds]
    med = statistics.median(per_call)
    rate = pairs / (med * 1e-3) / 1e9
    spread = (max(per_call) - min(per_call)) / med * 100.0
    return f"{med:10.3f} ms {rate:9.1f} G pairs/s  (spread {spread:4.1f} %, {reps} calls/round)", rate


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--skip-dist", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    lines = [f"device: {torch.cuda.get_device_name(0)}; 2048-bit random rows; median of {args.repeats} rounds after 2 warm-up rounds",
             f"int8 matrix-core ceiling by the spec: {INT8_SPEC_PAIRS / 1e9:.0f} G pairs/s"]
    print("\n".join(lines), flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for nq, nc in SHAPES:
        q = torch.randint(0, 256, (nq, 256), dtype=torch.uint8, device="cuda", generator=g)
        c = torch.randint(0, 256, (nc, 256), dtype=torch.uint8, device="cuda", generator=g)
        b = Bench(q, c)
        kernels = {"best_match": lambda r=1: b.best_match(r), "assign/bcnt": lambda r=1: b.assign("bcnt", r),
                   "assign/mfma": lambda r=1: b.assign("mfma", r)}
        reps, ref = {}, None
        for name, fn in kernels.items():  # warm-up 1: correctness and the number of calls a round needs
            ms, idx = fn()
            if ref is None:
                ref = idx
            if not bool((idx == ref).all()):
                raise SystemExit(f"{name}: indices differ from best_match on {nq} x {nc}")
            reps[name] = max(1, min(2000, int(args.window * 1e3 / max(ms, 1e-3)) + 1))
        for name, fn in kernels.items():  # warm-up 2
            fn(reps[name])
        rounds: dict[str, list[float]] = {k: [] for k in kernels}
        for _ in range(args.repeats):
            for name, fn in kernels.items():
                rounds[name].append(fn(reps[name])[0])
        head = f"{nq} x {nc}  ({nq * nc / 1e9:.2f} G pairs), indices of the three equal"
        lines.append(head)
        print(head, flush=True)
        rates = {}
        for name in kernels:
            text, rates[name] = fmt(rounds[name], float(nq) * nc, reps[name])
            extra = f"  = {rates[name] * 1e9 / INT8_SPEC_PAIRS * 100:.1f} % of the int8 spec rate" if name == "assign/mfma" else ""
            line = f"  {name:12s} {text}{extra}"
            lines.append(line)
            print(line, flush=True)
        line = (f"  ratios: bcnt / best_match {rates['assign/bcnt'] / rates['best_match']:.2f}, "
                f"mfma / bcnt {rates['assign/mfma'] / rates['assign/bcnt']:.2f}")
        lines.append(line)
        print(line, flush=True)
        del q, c, b, kernels
        torch.cuda.empty_cache()

    if not args.skip_dist:
        n = 16384
        q = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device="cuda", generator=g)
        c = torch.randint(0, 256, (n, 256), dtype=torch.uint8, device="cuda", generator=g)
        out = torch.empty((n, n), dtype=torch.float64, device="cuda")
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def dist() -> float:
            _lib.check(lib.bbh_profile_reset())
            _lib.check(lib.bbh_jt_dist_matrix(q.data_ptr(), n, 256, c.data_ptr(), n, 256, out.data_ptr(), st))
            return prof_ms(lib, "jt_dist_matrix")

        def sims() -> float:
            _lib.check(lib.bbh_profile_reset())
            _lib.check(lib.bbh_jt_best_match(q.data_ptr(), n, c.data_ptr(), n, 256, idx.data_ptr(), None, None,
                                             out.data_ptr(), st))
            return prof_ms(lib, "jt_best_match")

        sims(), dist(), sims(), dist()
        s_ms = out.sum().item()  # (touch the result)
        del s_ms
        r_d, r_s = [], []
        for _ in range(args.repeats):
            r_s.append(sims())
            r_d.append(dist())
        head = f"{n} x {n} full matrix (float64, {n * n * 8 / 2**30:.1f} GiB written)"
        lines.append(head)
        for name, r in (("best_match+sims", r_s), ("dist_matrix", r_d)):
            text, rate = fmt(r, float(n) * n, 1)
            lines.append(f"  {name:16s} {text}  = {rate * 8:.0f} GB/s of output")
        print("\n".join(lines[-3:]), flush=True)

    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

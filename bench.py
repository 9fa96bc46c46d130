#!/usr/bin/env python3
r"""Benchmark of the BitBIRCH insertion hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--n-fps M] [--workload fake|ecfp|rdkit] [--full]
                    [--dump-outputs DIR]

N = 1 (BASELINE.json configs[1]): one "step" = `BitBirch.fit` of the whole synthetic workload (1 M synthetic
2048-bit packed fingerprints, threshold 0.3, branching factor 50, diameter merge) into a fresh HBM-resident
tree, fingerprints already resident in HBM when the timed region starts.

N > 1 (the multiround path of configs[3]/[4]): one rank per GPU over RCCL; one "step" = the WHOLE
`run_multiround_distributed` job on N shards of M rows each (one shard per GPU, resident in HBM): round 1
(fit + full refinement per shard, no collective), the RCCL exchange of the leaf BitFeature tables to the
merging ranks, the merge round, the exchange to rank 0, the final sequential merge and the cluster labels.
Weak scaling: the per-GPU shard is fixed as N grows.  When WORLD_SIZE is not set, `--gpus N` re-executes
itself under `python -m torch.distributed.run` with N ranks; when it is set it must equal N.

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel (the tree insertion kernel;
algorithmic bytes = 264 B per inserted element) timed with HIP events on its launch
stream inside libbbhip during the timed steps.  A plain run does only what that line needs: it sets up, warms
up, times K steps and prints it.  `--full` adds everything else: the sub-records (end-to-end step, other
branching factors, workloads, sizes and paths), `k1_roofline` (the arr-vec Tanimoto kernel, 264 B per row,
that the north star's HBM target refers to) and `k2_valu`, `cpu_baseline` (the CPU oracle, a C restatement
of the reference path, kind "port") and `regressions` against the previous round's line.
`--dump-outputs DIR` writes what the last timed step computed (`tree_outputs`) as DIR/<name>.npy; the inputs
are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

PREVIOUS_ROUND = "r05"  # BENCH_<round>.json (the driver's line) + profiles/<round>/bench_line_final.json: what `regressions` compares this line with
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BYTES_PER_FP = 264  # 256 B row read once + 8 B label
_W8 = [128, 64, 32, 16, 8, 4, 2, 1]


def synth_fake_fps(n: int, seed: int, device):
    r"""S-fake(N, seed): same distribution as the reference's make_fake_fingerprints
    (fingerprints.py:70-108: popcount ~ rint(truncnorm(750, 400)) in [1, 2047], uniformly
    random bit positions), generated on the GPU in chunks.  Returns packed uint8 [n, 256]."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty((n, 256), dtype=torch.uint8, device=device)
    weights = torch.tensor(_W8, dtype=torch.int32, device=device)
    chunk = 50_000
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        pops = torch.empty(m, device=device)
        todo = torch.ones(m, dtype=torch.bool, device=device)
        while bool(todo.any()):
            draw = torch.randn(m, device=device, generator=g) * 400.0 + 750.0
            ok = (draw >= 1.0) & (draw <= 2047.0)
            take = todo & ok
            pops[take] = draw[take]
            todo &= ~ok
        pops = torch.round(pops).to(torch.int64)
        scores = torch.rand((m, 2048), device=device, generator=g)
        ranks = scores.argsort(dim=1).argsort(dim=1)
        bits = (ranks < pops[:, None]).to(torch.int32)
        out[lo : lo + m] = (bits.view(m, 256, 8) * weights).sum(dim=2).to(torch.uint8)
    return out


def _synth_planted(n: int, seed: int, device, pop_mean: float, pop_std: float, pop_lo: float, pop_hi: float,
                   noise: float, n_features: int = 2048):
    r"""Rows scattered around n/50 planted prototypes: `noise` of a prototype's bits dropped and as many
    random bits added (the distribution of tests/golden/cases.py sparse_ecfp_like / dense_rdkit_like)."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    k = max(n // 50, 1)
    pops = torch.clamp(torch.round(torch.randn(k, device=device, generator=g) * pop_std + pop_mean), pop_lo, pop_hi).to(torch.int64)
    weights = torch.tensor(_W8, dtype=torch.int32, device=device)
    protos = torch.empty((k, n_features // 8), dtype=torch.uint8, device=device)
    chunk = 50_000
    for lo in range(0, k, chunk):
        m = min(chunk, k - lo)
        ranks = torch.rand((m, n_features), device=device, generator=g).argsort(dim=1).argsort(dim=1)
        bits = (ranks < pops[lo:lo + m, None]).to(torch.int32)
        protos[lo:lo + m] = (bits.view(m, -1, 8) * weights).sum(dim=2).to(torch.uint8)
    out = torch.empty((n, n_features // 8), dtype=torch.uint8, device=device)
    shifts = torch.arange(7, -1, -1, device=device, dtype=torch.uint8)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        which = torch.randint(0, k, (m,), device=device, generator=g)
        pb = ((protos[which][:, :, None] >> shifts) & 1).bool().view(m, n_features)
        keep = torch.rand((m, n_features), device=device, generator=g) > noise
        add = torch.rand((m, n_features), device=device, generator=g) < (noise * pops[which].double() / n_features)[:, None]
        bits = ((pb & keep) | add).to(torch.int32)
        out[lo:lo + m] = (bits.view(m, -1, 8) * weights).sum(dim=2).to(torch.uint8)
    return out


def synth_ecfp(n: int, seed: int, device, n_features: int = 2048):
    r"""S-ecfp: sparse ECFP4-like rows, popcount ~ N(48, 12) clipped to [8, 160]."""
    return _synth_planted(n, seed, device, 48.0, 12.0, 8, 160, 0.15, n_features)


def synth_rdkit_like(n: int, seed: int, device, n_features: int = 2048):
    r"""S-rdkit-like (BASELINE configs[4]): dense rows, popcount ~ N(900, 250) clipped."""
    return _synth_planted(n, seed, device, 900.0, 250.0, 64, 1900, 0.12, n_features)


def synth_hier(n: int, seed: int, device, n_features: int = 2048):
    r"""Two-level planted families (tests/golden/cases.py clustered_hier, on the GPU): 12 super-prototypes at 50 % density,
    n/50 cluster prototypes (a super-prototype with 12 % of its bits toggled), rows = a cluster prototype with 4 % toggled.
    The tracking centroids of the INTERNAL tree levels stay informative: every level compares and routes for real."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    k = max(n // 50, 1)
    sup = torch.rand((12, n_features), device=device, generator=g) < 0.5
    protos = sup[torch.randint(0, 12, (k,), device=device, generator=g)] ^ (torch.rand((k, n_features), device=device, generator=g) < 0.12)
    weights = torch.tensor(_W8, dtype=torch.int32, device=device)
    out = torch.empty((n, n_features // 8), dtype=torch.uint8, device=device)
    for lo in range(0, n, 50_000):
        m = min(50_000, n - lo)
        which = torch.randint(0, k, (m,), device=device, generator=g)
        bits = (protos[which] ^ (torch.rand((m, n_features), device=device, generator=g) < 0.04)).to(torch.int32)
        out[lo:lo + m] = (bits.view(m, -1, 8) * weights).sum(dim=2).to(torch.uint8)
    return out


def synth_zipf(n: int, seed: int, device, n_features: int = 2048):
    r"""Rows with a realistic per-bit frequency profile: bit j of a random permutation of the positions is
    set with probability p_j = min(0.95, 4 / (j + 1)^0.85) - a Zipf-like tail, 11 bits above 50 % (the substructure bits most
    molecules share), ~60 bits per row - in n/50 planted prototypes; a row is its prototype with 10 % of its bits dropped and
    3 % as many drawn afresh from the same profile.  Unlike S-ecfp the common bits keep the tracking centroids of the tree's
    internal levels non-zero (a majority vote keeps what more than half of the members share), and rows of one prototype
    merge at threshold 0.3."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    rank = torch.randperm(n_features, device=device, generator=g).double()
    p = torch.clamp(4.0 / (rank + 1.0) ** 0.85, max=0.95).float()
    k = max(n // 50, 1)
    weights = torch.tensor(_W8, dtype=torch.int32, device=device)
    shifts = torch.arange(7, -1, -1, device=device, dtype=torch.uint8)
    protos = torch.empty((k, n_features // 8), dtype=torch.uint8, device=device)
    chunk = 50_000
    for lo in range(0, k, chunk):
        m = min(chunk, k - lo)
        bits = (torch.rand((m, n_features), device=device, generator=g) < p).to(torch.int32)
        protos[lo:lo + m] = (bits.view(m, -1, 8) * weights).sum(dim=2).to(torch.uint8)
    out = torch.empty((n, n_features // 8), dtype=torch.uint8, device=device)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        which = torch.randint(0, k, (m,), device=device, generator=g)
        pb = ((protos[which][:, :, None] >> shifts) & 1).bool().view(m, n_features)
        keep = torch.rand((m, n_features), device=device, generator=g) > 0.10
        add = torch.rand((m, n_features), device=device, generator=g) < 0.03 * p
        bits = ((pb & keep) | add).to(torch.int32)
        out[lo:lo + m] = (bits.view(m, -1, 8) * weights).sum(dim=2).to(torch.uint8)
    return out


WORKLOADS = {
    # name: (generator, threshold, description)
    "fake": (synth_fake_fps, 0.3, "make_fake_fingerprints popcount distribution"),
    "ecfp": (synth_ecfp, 0.3, "S-ecfp sparse ECFP4-like rows around n/50 planted prototypes"),
    "rdkit": (synth_rdkit_like, 0.6, "S-rdkit-like dense rows (popcount ~N(900,250)) around n/50 planted prototypes"),
    "hier": (synth_hier, 0.6, "two-level planted families (clustered_hier): informative internal tree levels"),
    "zipf": (synth_zipf, 0.3, "Zipf-like per-bit frequencies (11 bits above 50 %), n/50 planted prototypes that merge at 0.3"),
}


def kernel_src_sha() -> str:
    r"""sha256 over the device sources of libbbhip.so: what a PMC measurement has to match to describe this build
    (the GPU box has no .git; tools/profile_bench.sh stores the same hash next to its counters)."""
    import hashlib

    h = hashlib.sha256()
    for f in sorted((REPO / "bblean_amd" / "csrc").glob("*")):
        if f.suffix in (".hip", ".inc", ".h"):
            h.update(f.name.encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:16]


def _cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(fps_host, bf: int, thr: float) -> dict:
    from oracle_engine import OracleEngine

    import numpy as np

    sample = fps_host.shape[0]
    eng = OracleEngine(bf, thr, 0, 0.0, np.zeros(0), 2048)
    t0 = time.perf_counter()
    eng.fit_packed(fps_host)
    dt = time.perf_counter() - t0
    eng.close()
    return {
        "value": sample / dt,
        "unit": "fingerprints/s",
        "cores": 1,
        "kind": "port",
        "cpu_model": _cpu_model(),
        "nproc": os.cpu_count(),
        "sample": f"oracle (C restatement of the reference path; the algorithm is sequential: 1 thread) fit of "
                  f"{sample} fingerprints of the same workload, {dt:.1f} s on one host core",
    }


def _cpu_round1(args_):
    r"""One shard of the CPU multiround baseline's first round (fit + full refinement), in a pool worker."""
    path, start, end, bf, thr = args_
    import numpy as np
    from oracle_engine import OracleEngine

    from bblean_amd import BitBirch

    t = BitBirch(branching_factor=bf, threshold=thr, merge_criterion="diameter", _engine_factory=OracleEngine)
    t.fit(Path(path), reinsert_indices=range(start, end))
    t.delete_internal_nodes()
    bufs, mols = t._refine_tables(Path(path), initial_mol=start)
    t.reset()
    t.set_merge("tolerance-diameter", tolerance=0.05, threshold=thr)
    for name in bufs:
        t._fit_buffers(bufs[name], mols[name])
    t.delete_internal_nodes()
    bufs, mols = t._bf_tables(t._leaf_order(True))
    return {k: np.asarray(v) for k, v in bufs.items()}, {k: (v.counts, v.flat) for k, v in mols.items()}


def _cpu_round2(args_):
    r"""One batch of the CPU multiround baseline's merge round, in a pool worker."""
    batch, common = args_
    import numpy as np
    from oracle_engine import OracleEngine

    from bblean_amd.bitbirch import _IndexLists
    from bblean_amd.multiround import _merge_rounds

    tree = _merge_rounds([[(t, _IndexLists(*i)) for t, i in batch]], engine_factory=OracleEngine, **common)[0]
    bufs, mols = tree._bf_tables(tree._leaf_order(True))
    return {k: np.asarray(v) for k, v in bufs.items()}, {k: (v.counts, v.flat) for k, v in mols.items()}


def cpu_multiround_baseline(files: list[Path], bf: int, thr: float, bin_size: int = 10) -> dict:
    r"""the N-process multiround CPU baseline - round 1 in a process pool of
    min(shards, host cores) workers (the reference's `mp.Pool`, multiround.py:419-422), merge rounds in one
    process each like the reference; the C oracle engine under this repo's host logic."""
    import multiprocessing as mp

    import numpy as np
    from oracle_engine import OracleEngine

    from bblean_amd.bitbirch import _IndexLists
    from bblean_amd.multiround import _files_range_tuples, _merge_rounds
    from bblean_amd.utils import batched

    infos = _files_range_tuples(files)
    nproc = max(1, min(len(files), os.cpu_count() or 1))
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(nproc) as pool:
        r1 = pool.map(_cpu_round1, [(str(f), s, e, bf, thr) for _, f, s, e in infos])
    t1 = time.perf_counter()
    entries = []
    for (lab, _, _, _), (bufs, mols) in zip(infos, r1):
        for name in bufs:
            entries.append((f"label-{lab}-{name.replace('8', '08')}", name, bufs[name], _IndexLists(*mols[name])))
    entries.sort(key=lambda e: e[0])
    common = dict(branching_factor=bf, tolerance=0.05, device=0, threshold=thr, criterion="tolerance-diameter")
    batches = [sorted(b, key=lambda e: int(e[1][4:]), reverse=True) for b in batched(entries, bin_size)]
    # the reference runs the batches of a merge round in a process pool as well (multiround.py:443-455)
    nproc2 = max(1, min(len(batches), os.cpu_count() or 1))
    with mp.get_context("fork").Pool(nproc2) as pool:
        r2 = pool.map(_cpu_round2, [([(t, (i.counts, i.flat)) for _, _, t, i in b], common) for b in batches])
    z = len(str(len(batches)))
    entries = []
    for b, (bufs, mols) in enumerate(r2):
        for name in bufs:
            entries.append((f"label-{str(b).zfill(z)}-{name.replace('8', '08')}", name, bufs[name], _IndexLists(*mols[name])))
    entries.sort(key=lambda e: e[0])
    t2 = time.perf_counter()
    final = _merge_rounds([[(t, i) for _, _, t, i in entries]], engine_factory=OracleEngine, **common)[0]
    k = len(final._leaves()["ids"])
    t3 = time.perf_counter()
    rows = infos[-1][3]
    return {"value": rows / (t3 - t0), "unit": "fingerprints/s", "kind": "port", "cores": nproc, "nproc": os.cpu_count(),
            "cpu_model": _cpu_model(), "rows": rows, "files": len(files), "clusters": k,
            "rounds_s": {"round-1": round(t1 - t0, 3), "round-2": round(t2 - t1, 3), "round-3": round(t3 - t2, 3)},
            "sample": f"{rows} rows of the same workload in {len(files)} shard files; round 1 in {nproc} processes, the "
                      f"merge round's {len(batches)} batches in {nproc2} processes (the reference's pools, multiround.py:419-455), "
                      "the final merge in one"}


def regressions(out: dict, prev_files: list, tolerance: float = 0.05) -> dict:
    r"""Every GPU throughput of this line next to the same entry of the previous round: the DRIVER's line
    (`BENCH_rNN.json:parsed`, measured by the judge's harness) where it has the entry, the builder's committed full line
    (`profiles/rNN/bench_line_final.json`) for the sub-records the driver's file does not keep.  Entries more than
    `tolerance` worse are listed - and when the entry carries its repeats (`<name>_repeats`), only if at least two of three
    are worse (a guard that fires on box noise every round is ignored the round it is right).  The
    file-based multiround is compared on its summed kernel time (`kernel_fingerprints_per_s`), not on wall time with the
    box's file system inside.  CPU baselines are not compared: they move with the host."""
    names = {"fingerprints_per_s", "gpu_fingerprints_per_s", "kernel_fingerprints_per_s", "achieved", "value", "elements_per_s"}
    prev: dict = {}
    used = []

    def merge(dst, src):
        for k, v in src.items():
            if isinstance(v, dict) and isinstance(dst.get(k), dict):
                merge(dst[k], v)
            else:
                dst[k] = v

    for f in prev_files:  # (later files override earlier ones)
        try:
            rec = json.loads(Path(f).read_text())
            rec = rec.get("parsed", rec) if isinstance(rec, dict) else {}
            if isinstance(rec, dict) and rec:
                merge(prev, rec)
                used.append(str(Path(f).relative_to(REPO)) if Path(f).is_relative_to(REPO) else str(f))
        except Exception:
            continue
    if not prev:
        return {"against": [str(f) for f in prev_files], "error": "no previous line readable"}

    def walk(a, b, path, acc):
        if isinstance(a, dict) and isinstance(b, dict):
            for k in a:
                if k in b and "cpu" not in k and k not in ("projected_8gpu", "traffic_source", "plan", "regressions"):
                    walk(a[k], b[k], path + [k], acc)
                    if k in names and isinstance(a.get(k + "_repeats"), list):
                        acc[-1] = acc[-1] + (a[k + "_repeats"],)
        elif path and path[-1] in names and isinstance(a, (int, float)) and isinstance(b, (int, float)) and b > 0:
            acc.append((".".join(path), float(a), float(b)))

    pairs: list = []
    walk(out, prev, [], pairs)
    worse, better = {}, {}
    for item in pairs:
        k, a, b = item[:3]
        reps = item[3] if len(item) > 3 else None
        if a < (1.0 - tolerance) * b:
            if reps is not None and sum(1 for r in reps if r < (1.0 - tolerance) * b) < 2:
                continue
            worse[k] = {"now": a, "before": b, "ratio": round(a / b, 3), "repeats": reps}
        elif a > (1.0 + tolerance) * b:
            better[k] = round(a / b, 3)
    return {"against": used, "compared": len(pairs), "tolerance": tolerance, "worse": worse, "better": better}


# --- sizing of the N > 1 job --------------------------------------------------------------
# One step of the multiround job costs, per row of a shard: round 1 (fit + full refinement on the shard's own GPU) and,
# for EVERY shard of the job, two sequential passes on the merging rank (merge round + final merge: the reference's
# Amdahl shape, multiround.py:443-470).  Rates measured on one MI355X at bf 254 on S-ecfp rows
# (profiles/r05/bench_line_distributed_one_rank.json: 11.6 / 6.8 / 6.0 s for one shard of 2 M rows).
PLAN_ROUND1_S_PER_ROW = 5.8e-6
PLAN_MERGE_S_PER_ROW = 6.4e-6
PLAN_BUDGET_S = 1200.0      # (warmup + steps) x step must fit this (the driver allows 1 800 s per run)
PLAN_REF_WORLD = 8          # the shard is sized for the largest job the driver runs, so that every N times EQUAL work per GPU
PLAN_MAX_ROWS = 2_000_000
PLAN_STATED_ROWS = 12_500_000  # BASELINE configs[3]: 100 M rows in 8 shards


def plan_step_seconds(world: int, rows: int, scale: float = 1.0) -> float:
    return scale * rows * (PLAN_ROUND1_S_PER_ROW + world * PLAN_MERGE_S_PER_ROW)


def plan_rows_per_shard(steps: int, warmup: int, world: int = PLAN_REF_WORLD, scale: float = 1.0, cap: int = PLAN_MAX_ROWS) -> int:
    r"""Rows per shard such that (warmup + steps) steps of the `world`-rank job fit PLAN_BUDGET_S, in multiples of 50 000."""
    per_row = scale * (PLAN_ROUND1_S_PER_ROW + world * PLAN_MERGE_S_PER_ROW) * max(steps + warmup, 1)
    rows = int(PLAN_BUDGET_S / per_row)
    return max(50_000, min(cap, rows // 50_000 * 50_000))


def plan_multi(world: int, steps: int, warmup: int, n_fps: int | None = None) -> dict:
    rows = n_fps if n_fps is not None else plan_rows_per_shard(steps, warmup, max(world, PLAN_REF_WORLD))
    step = plan_step_seconds(world, rows)
    return {"world": world, "steps": steps, "warmup": warmup, "rows_per_shard": rows, "rows_per_shard_stated": PLAN_STATED_ROWS,
            "sized_for_world": max(world, PLAN_REF_WORLD), "overridden_by_n_fps": n_fps is not None,
            "projected_step_s": round(step, 2), "projected_wall_s": round((steps + warmup) * step, 1), "budget_s": PLAN_BUDGET_S,
            "model": {"round1_s_per_row": PLAN_ROUND1_S_PER_ROW, "merge_s_per_row_and_shard": PLAN_MERGE_S_PER_ROW}}


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _longest(lib, name: bytes) -> tuple[float, int]:
    ms, units = C.c_double(0.0), C.c_int64(0)
    lib.bbh_profile_longest(name, C.byref(ms), C.byref(units))
    return float(ms.value), int(units.value)


def _profile(lib, name: bytes) -> tuple[int, float, int]:
    launches, total_ms, units = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
    lib.bbh_profile_get(name, C.byref(launches), C.byref(total_ms))
    lib.bbh_profile_units(name, C.byref(units))
    return int(launches.value), float(total_ms.value), int(units.value)


def parse() -> argparse.Namespace:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-fps", type=int, default=None,
                    help="rows per GPU (default 1 000 000 at N=1; at N>1 sized so that (warmup + steps) steps of the 8-GPU job fit "
                         "20 minutes, at most 2 000 000 - `--dry-run` prints the plan; BASELINE configs[3] states 12 500 000)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None,
                    help="default: fake at N=1 (BASELINE configs[1]), ecfp at N>1 (configs[3])")
    ap.add_argument("--bf", type=int, default=None, help="default: 50 at N=1 (configs[1]), 254 at N>1 (the CLI default, configs[3])")
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--cpu-sample", type=int, default=None, help="rows of the CPU baseline (default: all)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--k1-rows", type=int, default=8_000_000)
    ap.add_argument("--shards", type=int, default=512)
    ap.add_argument("--multiround-files", type=int, default=64, help="0 skips the file-based multiround run")
    ap.add_argument("--no-extras", action="store_true", help="skip the sub-records (bf 254, other workloads, config 3, bf 1000, one-rank distributed)")
    ap.add_argument("--config3-rows", type=int, default=10_000_000, help="rows of the config-3 sub-record (0 skips it)")
    ap.add_argument("--dry-run", action="store_true", help="print the plan of the N > 1 job (rows per shard, projected wall time) and exit")
    ap.add_argument("--distributed", action="store_true",
                    help="time the one-rank-per-GPU multiround path even at N=1 (what N>1 always times)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: sub-records, other kernels' rooflines, CPU baselines, the regression "
                         "record (without it a run sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def _sample_rows(a, cap: int, seed: int):
    r"""`a` and None when it has at most `cap` rows, else a fixed seeded sample of `cap` of its rows (in row order) and
    their row numbers."""
    import numpy as np

    if a.shape[0] <= cap:
        return a, None
    idx = np.sort(np.random.default_rng(seed).choice(a.shape[0], cap, replace=False))
    return a[idx], idx


def tree_outputs(assignments, centroids=None) -> dict:
    r"""What a caller of the timed path receives from the fitted tree, as float64 arrays: `assignments` = the cluster label
    (1..K, largest cluster first) of every fingerprint (`get_assignments`), `cluster_sizes` = the size of cluster k at
    k - 1, and - when the centroids are given (`get_centroids`, packed) - `centroids` of a seeded sample of the clusters
    beside `centroids_clusters`, their labels.  An array longer than its cap is a fixed seeded sample of its rows, written
    with `<name>_rows`, the row numbers taken: at most 57 MB in all."""
    import numpy as np

    labels = np.asarray(assignments).astype(np.int64)
    out = {}
    a, rows = _sample_rows(labels, 2_000_000, 1)
    out["assignments"] = a.astype(np.float64)
    if rows is not None:
        out["assignments_rows"] = rows.astype(np.float64)
    sizes, rows = _sample_rows(np.bincount(labels)[1:], 1_000_000, 2)
    out["cluster_sizes"] = sizes.astype(np.float64)
    if rows is not None:
        out["cluster_sizes_rows"] = rows.astype(np.float64)
    if centroids is not None and len(centroids):
        k = len(centroids)
        pick = np.arange(k) if k <= 4096 else np.sort(np.random.default_rng(3).choice(k, 4096, replace=False))
        out["centroids"] = np.stack([np.asarray(centroids[i]) for i in pick]).astype(np.float64)
        out["centroids_clusters"] = (pick + 1).astype(np.float64)
    return out


def write_outputs(directory: str, arrays: dict) -> None:
    import numpy as np

    total = sum(int(a.nbytes) for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes of outputs, the limit is {DUMP_LIMIT_BYTES}")
    d = Path(directory)
    d.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"--dump-outputs: {name} is {a.dtype}, not float32 / float64")
        np.save(d / f"{name}.npy", a)


_JSON_FD = 1


def _emit(out: dict) -> None:
    os.write(_JSON_FD, (json.dumps(out) + "\n").encode())


def main() -> None:
    args = parse()
    if args.dry_run:
        print(json.dumps(plan_multi(args.gpus, args.steps, args.warmup, args.n_fps)))
        return
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and (args.gpus > 1 or args.distributed):
        # `python bench.py --gpus N` run bare: N ranks of this same script, one per GPU
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), str(Path(__file__).resolve())] + sys.argv[1:]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.run(cmd, env=env).returncode)
    # stdout carries ONE JSON line: everything else any library prints there (RCCL's version banner, through the C library's
    # buffer, flushed at exit) goes to stderr - file descriptor 1 is pointed at stderr for the rest of the process and the
    # line is written to the saved descriptor
    global _JSON_FD
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)
    world = int(env_world or "1")
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                 f"(python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...)")
    multi = not (world == 1 and not args.distributed)
    if args.workload is None:
        args.workload = "ecfp" if multi else "fake"
    if args.bf is None:
        args.bf = 254 if multi else 50
    if args.threshold is None:
        args.threshold = WORKLOADS[args.workload][1]
    args.n_fps_given = args.n_fps is not None
    if args.n_fps is None:
        args.n_fps = plan_multi(world, args.steps, args.warmup)["rows_per_shard"] if multi else 1_000_000
    if world == 1 and not args.distributed:
        single_gpu(args)
    else:
        multi_gpu(args, world)


# ------------------------------------------------------------------------------------------------------
def multi_gpu(args: argparse.Namespace, world: int) -> None:
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist.init_process_group("nccl", device_id=dev)

    from bblean_amd import _lib
    from bblean_amd.multiround import ShardRows, run_multiround_distributed

    lib = _lib.load()
    n = args.n_fps
    gen = WORKLOADS[args.workload][0]
    plan = plan_multi(world, args.steps, args.warmup, n if args.n_fps_given else None)
    shard = gen(n, 1000 + rank, dev)  # this rank's shard, resident in HBM
    torch.cuda.synchronize()

    state: dict = {}

    def one_step(rows: int) -> None:
        inputs = [ShardRows(rows) for _ in range(world)]
        inputs[rank] = shard[:rows]
        tree, timer = run_multiround_distributed(inputs, None, branching_factor=args.bf, threshold=args.threshold,
                                                 device=local_rank, return_tree=True)
        if tree is not None:  # rank 0: the labels are part of "clustered"
            state["labels"] = tree.get_assignments()
            state["clusters"] = len(tree._leaves()["ids"])
        state["timer"] = timer

    def barrier() -> None:
        dist.barrier()
        torch.cuda.synchronize()

    def timed(rows: int) -> float:
        barrier()
        t_ = time.perf_counter()
        one_step(rows)
        barrier()
        tt_ = torch.tensor([time.perf_counter() - t_], dtype=torch.float64, device=dev)
        dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
        return float(tt_.item())

    # A measured step on the first rows of every shard (the same rows the CPU baseline below is timed on): it calibrates the
    # plan - if (warmup + steps) steps at the planned size would not fit the budget on THIS box, the shard shrinks (every rank
    # computes the same number from the all-reduced time) - and it is the GPU figure on the CPU baseline's sample.
    n_cal = min(n, 100_000)
    timed(n_cal)  # (first call: library load, RCCL communicator, pools)
    t_cal = timed(n_cal)
    scale = t_cal / plan_step_seconds(world, n_cal)
    plan["calibration"] = {"rows_per_shard": n_cal, "step_s": round(t_cal, 3), "fingerprints_per_s": world * n_cal / t_cal,
                           "measured_over_model": round(scale, 3)}
    # (small shards are dearer per row than the model's large ones: the projection from them is an upper bound)
    projected = (args.warmup + args.steps) * plan_step_seconds(world, n, min(scale, 3.0))
    if projected > 1.25 * PLAN_BUDGET_S and not args.n_fps_given:
        n = max(50_000, int(n * PLAN_BUDGET_S / projected) // 50_000 * 50_000)
        plan["shrunk_to"] = n
    plan["rows_per_shard_run"] = n
    for _ in range(args.warmup):
        one_step(n)
    lib.bbh_profile_enable(1)
    lib.bbh_profile_reset()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step(n)
    barrier()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    launches, total_ms, units = _profile(lib, b"tree_insert")
    lib.bbh_profile_enable(0)
    timer = state["timer"]
    # per-round maxima over the ranks and the bytes every rank put on / took off the links (last step)
    names = sorted(k for k in timer.timings if k != "total")
    tt = torch.tensor([timer.timings[k] for k in names] + [timer.timings["total"]], dtype=torch.float64, device=dev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    ex = torch.tensor([[timer.exchange.get(k, {}).get("sent", 0), timer.exchange.get(k, {}).get("received", 0)] for k in names],
                      dtype=torch.int64, device=dev)
    ex_all = [torch.zeros_like(ex) for _ in range(world)]
    dist.all_gather(ex_all, ex)
    if rank == 0 and args.dump_outputs:
        write_outputs(args.dump_outputs, tree_outputs(state["labels"]))
    cpu_mr = None
    if rank == 0 and args.full and not args.no_cpu:
        # the same job on this host's cores: one shard file per rank with this rank's generator seeds, the oracle engine
        # under the file-based multiround host code (round 1 and the merge round's batches in process pools)
        import tempfile

        import numpy as np

        # (a bounded sample: the first 100 000 rows of every rank's shard - 10-30 s of host work; the whole job's merge rounds are
        # sequential on the CPU too and would take ten minutes at 2 M rows per shard)
        msamp = n_cal
        with tempfile.TemporaryDirectory() as d:
            shard_files = []  # (NOT `names`: that is the list of round names the JSON line is keyed by below)
            for r in range(world):
                f = Path(d) / f"fps.{r:05d}.npy"
                np.save(f, gen(n, 1000 + r, dev)[:msamp].cpu().numpy())
                shard_files.append(f)
            cpu_mr = cpu_multiround_baseline(shard_files, args.bf, args.threshold)
    if rank == 0:
        avg_ms = total_ms / max(launches, 1)
        achieved = BYTES_PER_FP * (units / max(launches, 1)) / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
        labels = state.get("labels")
        out = {
            "metric": "fingerprints/sec clustered (2048-bit, thr=%.2g)" % args.threshold,
            "value": world * args.steps * n / elapsed,
            "unit": "fingerprints/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {
                "workload": f"BASELINE configs[3] (multiround, one shard per GPU) at {n} rows per shard (stated: 12 500 000 per shard = "
                            f"--n-fps 12500000; tools/config45.py runs that size on one GPU): multiround over {world} GPUs: {world} shards x {n} synthetic 2048-bit packed fingerprints "
                            f"({WORKLOADS[args.workload][2]}), one shard per GPU resident in HBM, threshold={args.threshold}, "
                            f"branching_factor={args.bf}, reference defaults otherwise (diameter, full refinement, one merge "
                            "round in bins of 10, tolerance-diameter merges); timed region = run_multiround_distributed "
                            "(round 1, RCCL exchange of the BitFeature tables to the merging ranks, merge round, exchange to "
                            "rank 0, final merge) + cluster labels",
                "rows_per_shard": n,
                "rows_per_shard_stated": PLAN_STATED_ROWS,
                "plan": plan,
                "clusters": state.get("clusters"),
                "labelled": None if labels is None else int(labels.size),
                "rccl_ranks": dist.get_world_size(),
                "backend": dist.get_backend(),
                "rounds_s_max_over_ranks": {k: round(float(v), 4) for k, v in zip(names + ["total"], tt.tolist())},
                "exchange_bytes_per_rank": {k: {"sent": [int(e[i, 0]) for e in ex_all], "received": [int(e[i, 1]) for e in ex_all]}
                                            for i, k in enumerate(names) if k != "round-1"},
            },
            "roofline": {
                "kernel": "k_tree_pipe / k_tree_fast / k_tree_insert on rank 0 (all launches of the timed steps)",
                "bound": "hbm",
                "limiter": "dependency chain of the sequential algorithm, not bandwidth",
                "traffic_source": None,
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": None,
                "launches": launches,
                "avg_launch_ms": avg_ms,
                "elements_per_launch": units / max(launches, 1),
                "note": "latency/dependency-bound sequential insertion; 264 algorithmic bytes per inserted element",
            },
        }
        if args.full:
            out["cpu_baseline"] = cpu_mr
        if cpu_mr is not None:
            # like for like: the GPU job on the very rows the CPU baseline was timed on - small trees on both sides;
            # `value` above is the job at `rows_per_shard`, whose per-row cost differs (larger trees), so no ratio is formed from it
            cpu_mr["gpu_on_same_sample"] = {"rows_per_shard": n_cal, "fingerprints_per_s": world * n_cal / t_cal,
                                            "gpu_over_cpu": (world * n_cal / t_cal) / cpu_mr["value"] if cpu_mr.get("value") else None}
        _emit(out)
    dist.barrier()
    dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------
def workgroups_busy(others) -> dict:
    out = {"headline_kernel": 1, "compute_units": 256}
    for key, rec in (others or {}).items():
        so = rec.get("systolic_opt_in") if isinstance(rec, dict) else None
        if so and "workgroups" in so:
            out[f"systolic_opt_in_{key}"] = {"workgroups_resident": so["workgroups"], "parallel_workgroups": so["parallel_workgroups"],
                                             "identical_to_default_path": so["identical_to_default_path"]}
    return out


def systolic_record(BitBirch, rows, default_tree, bf: int, thr: float, device: int, n: int) -> dict:
    r"""The same rows through the opt-in level-systolic kernel (`BBHIP_SYS=1`: ONE tree over many workgroups,
    bblean_amd/csrc/bb_tree_sys.inc), checked against the tree the default path has just built from them: labels and engine
    counters must be identical, or the record says so instead of quoting a rate.  Opt-in because its hand-over between
    workgroups is not dependable on adversarial shapes yet (profiles/r06/sys_stability.txt); the kernel returns an error rather
    than a result when its own checks fail, and that is reported here as `error`."""
    import torch

    prev = os.environ.get("BBHIP_SYS")
    os.environ["BBHIP_SYS"] = "1"
    try:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st = BitBirch(branching_factor=bf, threshold=thr, merge_criterion="diameter", device=device).fit(rows)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        sc = [int(v) for v in st._engine.sys_counts()]
        same = bool((st.get_assignments() == default_tree.get_assignments()).all()) and \
            [int(v) for v in st._engine.stats()[:7]] == [int(v) for v in default_tree._engine.stats()[:7]]
        rec = {"identical_to_default_path": same, "seconds": dt, "elements_in_systolic_kernel": sc[0], "launches": sc[1],
               "relaunches_after_root_splits": sc[2], "workgroups": sc[3],
               # cycles spent on elements (not waiting), summed over the launches: all workgroups, the root's owner, the busiest
               # other workgroup; `parallel_workgroups` = all / the busier of the two = how many workgroups' worth of work ran
               # beside the critical one
               "busy_cycles": {"all": sc[4], "root_owner": sc[5], "busiest_other": sc[6]},
               "parallel_workgroups": sc[4] / max(sc[5], sc[6], 1)}
        if same:
            rec["fingerprints_per_s"] = n / dt
        del st
        return rec
    except Exception as exc:  # the kernel's own checks gave up: no result, no rate
        return {"error": str(exc)[:300]}
    finally:
        if prev is None:
            os.environ.pop("BBHIP_SYS", None)
        else:
            os.environ["BBHIP_SYS"] = prev


def single_gpu_full(args: argparse.Namespace, n: int, fps, one_step, lib, dev, local_rank: int) -> dict:
    r"""`--full`: everything of the N = 1 line beyond the headline - the end-to-end step, the sub-records (other branching
    factors, workloads, sizes and paths), the arr-vec and batched-compare kernels' own runs and the one-core CPU baselines."""
    import numpy as np
    import torch

    from bblean_amd import BitBirch, _lib

    # fit + labels: the labels (get_assignments, reference bitbirch.py:1002-1047) on top of the timed fit
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    t_e2e = one_step()
    labels = t_e2e.get_assignments()
    e2e = time.perf_counter() - t1
    del t_e2e, labels

    # bf 254 is the default of `bb run` / `bb multiround` (BASELINE configs 3-5): the same rows into one tree at bf 254
    bf254 = None
    if args.bf != 254 and not args.no_extras:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t254 = BitBirch(branching_factor=254, threshold=args.threshold, merge_criterion="diameter", device=local_rank).fit(fps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        bf254 = {"branching_factor": 254, "seconds": dt, "fingerprints_per_s": n / dt, "stats": [int(v) for v in t254._engine.stats()[:7]]}
        del t254

    # the other generators at the same size and branching factor(s): S-ecfp (configs 3 / 4), S-rdkit-like (config 5) and the
    # workload whose INTERNAL levels stay informative (planted two-level families) - one fit each, with which kernel did it
    others = None
    if not args.no_extras:
        others = {}
        for wname in ("ecfp", "rdkit", "hier", "zipf"):
            if wname == args.workload:
                continue
            wgen, wthr, _ = WORKLOADS[wname]
            wf = wgen(n, 1000, dev)
            torch.cuda.synchronize()
            for wbf in ((args.bf,) if wname in ("ecfp", "rdkit") else (args.bf, 254)):
                t1 = time.perf_counter()
                wt = BitBirch(branching_factor=wbf, threshold=wthr, merge_criterion="diameter", device=local_rank).fit(wf)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                wk = wt._engine.kernel_counts()
                wst = [int(v) for v in wt._engine.stats()[:7]]
                rec = {"rows": n, "threshold": wthr, "branching_factor": wbf, "seconds": dt, "fingerprints_per_s": n / dt,
                       "elements_by_kernel": {"pipe": int(wk[0]), "fast": int(wk[1]), "complete": int(wk[2])},
                       "unsupported_shape_stops": int(wk[6]), "stats": wst,
                       # (of the insertions: how many merged into an existing BitFeature; how many ended as clusters of one)
                       "merge_fraction": wst[2] / max(wst[2] + wst[3], 1)}
                if not args.no_cpu:
                    # the same workload through the C oracle on one host core (a bounded sample: the first 200 k rows)
                    msamp = min(n, 200_000)
                    cb = cpu_baseline(wf[:msamp].cpu().numpy(), wbf, wthr)
                    rec["cpu_baseline"] = {"value": cb["value"], "unit": cb["unit"], "cores": 1, "kind": "port", "rows": msamp}
                    rec["gpu_over_cpu_core"] = rec["fingerprints_per_s"] / cb["value"]
                if wname in ("hier", "zipf"):
                    rec["systolic_opt_in"] = systolic_record(BitBirch, wf, wt, wbf, wthr, local_rank, n)
                others[f"{wname}_bf{wbf}"] = rec
                del wt
            del wf
        # the headline workload drawn with other seeds: informative levels above the leaf-parents come and go,
        # the tree then moves between the two instances of the pipelined kernel - the headline's seed never does in 1 M rows
        if args.workload == "fake":
            seeds = {}
            for sd in (5000, 5001, 123456):
                wf = WORKLOADS["fake"][0](n, sd, dev)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                wt = BitBirch(branching_factor=args.bf, threshold=args.threshold, merge_criterion="diameter", device=local_rank).fit(wf)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t1
                wk = wt._engine.kernel_counts()
                seeds[str(sd)] = {"fingerprints_per_s": n / dt, "pipelined_kernel_launches": int(wk[3])}
                del wt, wf
            others["headline_other_seeds"] = seeds

    # BASELINE configs[2] in one run: S-ecfp, 10 M rows, the CLI's branching factor 254, `bb run --refine-num 1`
    # (fit -> set_merge(tolerance-diameter, 0.05) -> refine_inplace(n_largest=1) -> labels; cli.py:1067-1092)
    config3 = None
    if not args.no_extras and args.config3_rows > 0:
        try:
            sys.path.insert(0, str(REPO / "tools"))
            from props import check_clustering, column_sums

            c3 = synth_ecfp(args.config3_rows, 7, dev)
            c3_want = column_sums(c3)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            ct = BitBirch(branching_factor=254, threshold=0.3, merge_criterion="diameter", device=local_rank).fit(c3)
            t2 = time.perf_counter()
            k_fit = int(ct._engine.stats()[7])
            ct.set_merge("tolerance-diameter", tolerance=0.05, threshold=0.3)
            ct.refine_inplace(c3, n_largest=1)
            t3 = time.perf_counter()
            clab = ct.get_assignments()
            t4 = time.perf_counter()
            config3 = {"rows": args.config3_rows, "branching_factor": 254, "fit_s": t2 - t1, "refine_s": t3 - t2, "labels_s": t4 - t3,
                       "fingerprints_per_s": args.config3_rows / (t4 - t1), "leaf_bitfeatures_after_fit": k_fit, "clusters": int(clab.max())}
            # (outside the clock) the size-independent properties at this size: the clusters partition 0..n-1, sizes / labels
            # agree, the final cluster features' column sums are those of all fingerprints (tools/props.py)
            try:
                cs = check_clustering(ct, args.config3_rows, c3_want, clab)
                config3["checked"] = {"partition": True, "column_sums": True, **cs}
            except AssertionError as exc:
                config3["checked"] = {"failed": repr(exc)[:200]}
            mem3 = ct._engine.memory()
            config3["memory"] = {"node_pools_gb": int(mem3[0]) / 1e9, "node_pools_used_gb": int(mem3[1]) / 1e9, "cf_pools_gb": int(mem3[2]) / 1e9,
                                 "compactions": int(mem3[4]), "sealed_nodes": int(mem3[5]), "thawed": int(mem3[7])}
            del ct, clab, c3
        except Exception as exc:  # the sub-record must not take the headline down with it
            config3 = {"error": repr(exc)[:200]}
        torch.cuda.empty_cache()

    # A merge round in isolation (reference multiround.py:240-264, :284-312): the round-1 table of a
    # 1 M-row S-ecfp shard (fit + full refinement at the CLI's bf 254 -> leaf BitFeatures, sorted by size, singletons as a
    # packed tail) inserted into a fresh tree with the merge rounds' criterion (tolerance-diameter, tol 0.05) - what rounds 2
    # and 3 of a multiround job do with every table they receive; the C oracle on the first 200 k rows' table beside it
    merge_round = None
    if not args.no_extras:
        try:
            mr_n = min(n, 1_000_000)
            mr_fps = synth_ecfp(mr_n, 11, dev)

            def round1_tables(rows, factory=None):
                kw = {} if factory is None else {"_engine_factory": factory}
                t = BitBirch(branching_factor=254, threshold=0.3, merge_criterion="diameter", device=local_rank, **kw).fit(rows)
                t.set_merge("tolerance-diameter", tolerance=0.05, threshold=0.3)
                t.refine_inplace(rows, n_largest=1)
                return t._bf_tables(t._leaf_order(True), device=factory is None)

            def insert_tables(bufs, mols, factory=None):
                kw = {} if factory is None else {"_engine_factory": factory}
                t = BitBirch(branching_factor=254, threshold=0.3, merge_criterion="tolerance-diameter", tolerance=0.05, device=local_rank, **kw)
                k_in = 0
                t0_ = time.perf_counter()
                for name in bufs:
                    t._fit_buffers(bufs[name], reinsert_index_seqs=mols[name])
                    k_in += len(mols[name].counts)
                if factory is None:
                    torch.cuda.synchronize()
                return k_in, time.perf_counter() - t0_, t

            bufs, mols = round1_tables(mr_fps)
            torch.cuda.synchronize()
            k_in, dt, mt = insert_tables(bufs, mols)
            wk = mt._engine.kernel_counts()
            merge_round = {"rows": mr_n, "bitfeatures_inserted": k_in, "seconds": dt, "elements_per_s": k_in / dt, "us_per_element": 1e6 * dt / k_in,
                           "elements_by_kernel": {"pipe": int(wk[0]), "fast": int(wk[1]), "complete": int(wk[2])},
                           "note": "round-1 table of a 1 M-row S-ecfp shard (bf 254, CLI defaults) inserted into a fresh tree with tolerance-diameter"}
            del bufs, mols, mt
            if not args.no_cpu:
                from oracle_engine import OracleEngine

                hs = mr_fps[:200_000].cpu().numpy()
                ob, om = round1_tables(hs, OracleEngine)
                k_o, dt_o, ot = insert_tables(ob, om, OracleEngine)
                merge_round["cpu_baseline"] = {"value": k_o / dt_o, "unit": "elements/s", "cores": 1, "kind": "port", "bitfeatures_inserted": k_o,
                                               "sample": "the same on the first 200 000 rows through the C oracle, one host core"}
                merge_round["gpu_over_cpu_core"] = merge_round["elements_per_s"] / (k_o / dt_o)
                del ob, om, ot
            del mr_fps
        except Exception as exc:  # the sub-record must not take the headline down with it
            merge_round = {"error": repr(exc)[:300]}
        torch.cuda.empty_cache()

    # bf 1000 (what the reference's user guide recommends for 100-200 M molecules, docs/src/user-guide/parameters.rst:95-98):
    # a sample through the GPU engine and through the C oracle on one host core, side by side
    bf1000 = None
    cpu254 = None
    if not args.no_extras and not args.no_cpu:
        from oracle_engine import OracleEngine

        m1000 = min(n, 200_000)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        bt = BitBirch(branching_factor=1000, threshold=args.threshold, merge_criterion="diameter", device=local_rank).fit(fps[:m1000])
        torch.cuda.synchronize()
        g_dt = time.perf_counter() - t1
        del bt
        hs = fps[:m1000].cpu().numpy()
        eng = OracleEngine(1000, args.threshold, 0, 0.0, np.zeros(0), 2048)
        t1 = time.perf_counter()
        eng.fit_packed(hs)
        c_dt = time.perf_counter() - t1
        eng.close()
        bf1000 = {"rows": m1000, "gpu_fingerprints_per_s": m1000 / g_dt, "cpu_oracle_1core_fingerprints_per_s": m1000 / c_dt,
                  "gpu_over_cpu_core": c_dt / g_dt}
        m254 = min(n, 300_000)
        eng = OracleEngine(254, args.threshold, 0, 0.0, np.zeros(0), 2048)
        t1 = time.perf_counter()
        eng.fit_packed(fps[:m254].cpu().numpy())
        c_dt = time.perf_counter() - t1
        eng.close()
        cpu254 = {"value": m254 / c_dt, "unit": "fingerprints/s", "cores": 1, "kind": "port", "branching_factor": 254,
                  "sample": f"oracle fit of the first {m254} rows of the workload at bf 254, {c_dt:.1f} s on one host core"}

    # K1 (arr-vec Tanimoto): the HBM-bound kernel, on an array larger than the 256 MiB
    # Infinity Cache so that the rate is an HBM rate (the 1 M-row workload itself is 256 MB)
    from bblean_amd.similarity import _jt_sim_arr_vec_packed

    k1_rows = max(n, args.k1_rows)
    reps_fill = (k1_rows + n - 1) // n
    big = fps.repeat(reps_fill, 1)[:k1_rows].contiguous() if reps_fill > 1 else fps
    vec = fps[0].clone()
    for _ in range(3):
        _jt_sim_arr_vec_packed(big, vec)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 10
    k1_runs = []
    for _ in range(3):  # (three repeats: the regression guard lists an entry only when two of three are worse)
        e0.record()
        for _ in range(reps):
            _jt_sim_arr_vec_packed(big, vec)
        e1.record()
        torch.cuda.synchronize()
        k1_runs.append(e0.elapsed_time(e1) / reps)
    k1_ms = sorted(k1_runs)[1]
    k1_gbs = BYTES_PER_FP * k1_rows / (k1_ms * 1e-3) / 1e9
    k1_repeats = [BYTES_PER_FP * k1_rows / (m_ * 1e-3) / 1e9 for m_ in k1_runs]
    # K2 (batched descent step: every query row against all centroids of a node, exact first-argmax):
    # VALU-bound - 2 ops (AND, BCNT) per query dword and centroid row on 256 CUs x 64 lanes
    nq2, nc2 = min(k1_rows, 4_000_000), args.bf + 1  # enough queries to hide the launch tail
    cents = fps[:nc2].contiguous()
    i_o = torch.empty(nq2, dtype=torch.int32, device=dev)
    n_o = torch.empty(nq2, dtype=torch.int32, device=dev)
    u_o = torch.empty(nq2, dtype=torch.int32, device=dev)

    def k2() -> None:
        _lib.check(lib.bbh_jt_best_match(big.data_ptr(), nq2, cents.data_ptr(), nc2, 256, i_o.data_ptr(), n_o.data_ptr(),
                                         u_o.data_ptr(), None, None))

    for _ in range(2):
        k2()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(5):
        k2()
    e1.record()
    torch.cuda.synchronize()
    k2_ms = e0.elapsed_time(e1) / 5
    k2_laneops = nq2 * nc2 * 128 / (k2_ms * 1e-3)  # 64 dwords x (AND + BCNT) per pair
    k2_peak = 256 * 64 * 2.4e9  # CUs x lanes x clock: one VALU op per lane and clock

    del big

    # independent trees in one launch (multiround round 1 with many shards on this GPU)
    shard_stats = None
    if args.shards > 1:
        from bblean_amd import fit_concurrently

        per = n // args.shards
        parts = [fps[i * per:(i + 1) * per] for i in range(args.shards)]
        best = None
        for _ in range(2):
            trees = [BitBirch(branching_factor=args.bf, threshold=args.threshold, device=local_rank)
                     for _ in range(args.shards)]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fit_concurrently(trees, parts, reinsert_indices=[range(i * per, (i + 1) * per) for i in range(args.shards)])
            dt = time.perf_counter() - t1
            best = dt if best is None else min(best, dt)
            del trees
        shard_stats = {"shards": args.shards, "rows_per_shard": per, "seconds": best,
                       "fingerprints_per_s": args.shards * per / best,
                       "note": "multiround round 1 (reference multiround.py:401-422) with this many input files: "
                               "one workgroup per shard tree, one kernel launch; results equal per-shard fit"}

    # the reference's answer for large sets, `bb multiround` (multiround.py:333-484), on this one GPU:
    # the same rows as shard files; all shards of round 1 and all batches of the merge round share
    # kernel launches, the final merge is one sequential tree
    mr_stats = None
    cpu_mr = None
    if args.multiround_files > 1:
        import tempfile

        from bblean_amd.multiround import run_multiround_bitbirch

        host = fps.cpu().numpy()
        per = n // args.multiround_files
        shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None  # (memory-backed: the box's disk is not the subject)
        with tempfile.TemporaryDirectory(dir=shm) as d:
            names = []
            for i in range(args.multiround_files):
                f = Path(d) / f"fps.{i:05d}.npy"
                np.save(f, host[i * per:(i + 1) * per])
                names.append(f)
            out_dir = Path(d) / "out"
            out_dir.mkdir()
            lib.bbh_profile_enable(1)
            lib.bbh_profile_reset()
            t1 = time.perf_counter()
            timer = run_multiround_bitbirch(names, out_dir, branching_factor=args.bf, threshold=args.threshold,
                                            num_initial_processes=1, device=local_rank)
            dt = time.perf_counter() - t1
            _, mr_kernel_ms, _ = _profile(lib, b"tree_insert")
            lib.bbh_profile_enable(0)
            mr_stats = {"files": args.multiround_files, "rows": per * args.multiround_files, "seconds": dt,
                        "wall_fingerprints_per_s": per * args.multiround_files / dt,
                        # what the regression guard compares: the summed HIP-event time of the tree kernels' launches; the rest of
                        # the wall time is the reference's file formats (.npy tables, pickled member lists) on whatever the box offers
                        "kernel_s": mr_kernel_ms * 1e-3, "io_and_host_s": dt - mr_kernel_ms * 1e-3,
                        "kernel_fingerprints_per_s": per * args.multiround_files / (mr_kernel_ms * 1e-3) if mr_kernel_ms > 0 else None,
                        "files_on": "/dev/shm" if shm else "tmp",
                        "rounds_s": {k: round(v, 3) for k, v in timer.timings.items()},
                        "note": "file-compatible multiround with the reference's defaults (full refinement, one merge "
                                "round in bins of 10, tolerance-diameter merges); files on tmpfs/disk inside the timing"}
            if not args.no_cpu:
                # the SAME files as the GPU leg (1 M rows: about 15 s on the host's cores)
                cpu_mr = cpu_multiround_baseline(names, args.bf, args.threshold)
        del host

    # (last: a live RCCL communicator slows the many-tree launch measured above by 2x)
    # the rank path (what --gpus N times) on this one GPU: 8 shards of n / 8 rows resident in HBM through
    # run_multiround_distributed with one RCCL rank (round 1, table "exchange" on the device, merge round, final merge, labels)
    dist_one = None
    scale_anchor = None
    if not args.no_extras:
        try:
            import torch.distributed as dist

            from bblean_amd.multiround import run_multiround_distributed

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
            # (RCCL prints its version banner on stdout when the first communicator comes up: keep stdout to the ONE JSON line)
            sys.stdout.flush()
            saved_fd = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
                dist.barrier()
            finally:
                try:  # (the banner sits in the C library's stdout buffer - fully buffered when stdout is a file - until flushed)
                    import ctypes
                    ctypes.CDLL(None).fflush(None)
                except Exception:
                    pass
                os.dup2(saved_fd, 1)
                os.close(saved_fd)
            # (a) SCALE anchor: the `--gpus N` job with ONE shard on ONE RCCL rank - same generator, branching
            # factor, rows per shard (sized by plan_multi for this --steps / --warmup, as every N is), CLI defaults - so that the
            # driver's 1 -> N curve compares equal work per GPU; the `--gpus 1` headline above is a different job (one tree, bf 50).
            plan = plan_multi(1, args.steps, args.warmup)
            a_rows = plan["rows_per_shard"]
            a_gen, a_thr, _ = WORKLOADS["ecfp"]
            a_shard = a_gen(a_rows, 1000, dev)
            torch.cuda.synchronize()
            run_multiround_distributed([a_shard[:100_000]], None, branching_factor=254, threshold=a_thr, device=local_rank, return_tree=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            atree, atimer = run_multiround_distributed([a_shard], None, branching_factor=254, threshold=a_thr, device=local_rank,
                                                       return_tree=True)
            alabels = atree.get_assignments()
            a_dt = time.perf_counter() - t1
            scale_anchor = {"value": a_rows / a_dt, "unit": "fingerprints/s", "n_gpus": 1, "rccl_ranks": 1, "seconds": a_dt,
                            "rows_per_shard": a_rows, "workload": "ecfp", "branching_factor": 254, "threshold": a_thr,
                            "clusters": int(alabels.max()), "rounds_s": {k: round(float(v), 3) for k, v in atimer.timings.items()},
                            "plan": plan,
                            "note": "the job `bench.py --gpus N` times (BASELINE configs[3] shape: multiround, one S-ecfp shard per GPU, "
                                    "bf 254, CLI defaults, labels included) with N = 1: the like-for-like 1-GPU point of the scaling curve"}
            del atree, alabels, a_shard
            # (b) the rank path on the HEADLINE rows: 8 shards of n / 8 rows resident in HBM, one RCCL rank
            per = n // 8
            parts = [fps[i * per:(i + 1) * per] for i in range(8)]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dtree, dtimer = run_multiround_distributed(parts, None, branching_factor=args.bf, threshold=args.threshold,
                                                       device=local_rank, return_tree=True)
            dlabels = dtree.get_assignments()
            dt = time.perf_counter() - t1
            dist_one = {"shards": 8, "rows": 8 * per, "seconds": dt, "fingerprints_per_s": 8 * per / dt, "rccl_ranks": 1,
                        "clusters": int(dlabels.max()), "rounds_s": {k: round(float(v), 3) for k, v in dtimer.timings.items()}}
            # What 8 ranks would make of the same job, as a PROJECTION (nothing here ran on 8 GPUs): only round 1 shards
            # (one shard per rank); with 8 tables per dtype the merge round is one or two batches and the final merge one
            # sequential tree (the reference's shape, multiround.py:443-470), so they stay what they are on one rank.
            r_ = dtimer.timings
            proj = r_["round-1"] / 8.0 + sum(v for k, v in r_.items() if k not in ("round-1", "total"))
            dist_one["projected_8gpu"] = {"seconds": proj, "fingerprints_per_s": 8 * per / proj,
                                          "note": "projection from this one-rank run: round-1 / 8 + the merge rounds as measured; "
                                                  "exchange over xGMI and the labels not included; NOT a measurement"}
            del dtree, dlabels
            dist.destroy_process_group()
        except Exception as exc:  # the sub-record must not take the headline down with it
            dist_one = {"error": repr(exc)[:200]}

    return {
        "end_to_end": {
            "seconds": e2e, "fingerprints_per_s": n / e2e,
            "note": "one extra step: BitBirch.fit + get_assignments() (leaf export, member lists, labels 1..K)",
        },
        "k1_roofline": {
            "kernel": "k_arr_vec<16,true> (arr-vec Tanimoto, 264 B/row)",
            "bound": "hbm",
            "achieved": k1_gbs,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": k1_gbs / HBM_PEAK_GBS,
            "rows": k1_rows,
            "avg_launch_ms": k1_ms,
            "achieved_repeats": k1_repeats,
        },
        "k2_valu": {
            "kernel": "k_best_match<64> (batched node compare, exact first-argmax)",
            "bound": "valu",
            "achieved": k2_laneops / 1e12,
            "peak": k2_peak / 1e12,
            "unit": "T lane-ops/s",
            "frac": k2_laneops / k2_peak,
            "queries": nq2, "centroids": nc2, "avg_launch_ms": k2_ms,
        },
        "bf254": bf254,
        "other_workloads": others,
        "config3": config3,
        "merge_round": merge_round,
        "bf1000": bf1000,
        "cpu_baseline_bf254": cpu254,
        "scale_anchor": scale_anchor,
        "distributed_one_rank": dist_one,
        "concurrent_shards": shard_stats,
        "multiround_one_gpu": mr_stats,
        "cpu_multiround_baseline": cpu_mr,
    }



def single_gpu(args: argparse.Namespace) -> None:
    import torch

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    from bblean_amd import BitBirch, _lib

    lib = _lib.load()
    n = args.n_fps
    gen = WORKLOADS[args.workload][0]
    fps = gen(n, 1000, dev)  # resident in HBM
    torch.cuda.synchronize()

    def one_step() -> BitBirch:
        tree = BitBirch(branching_factor=args.bf, threshold=args.threshold, merge_criterion="diameter",
                        device=local_rank)
        tree.fit(fps)
        return tree

    for _ in range(args.warmup):
        one_step()
    lib.bbh_profile_enable(1)
    lib.bbh_profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tree = None
    for _ in range(args.steps):
        tree = one_step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # every tree-kernel launch of the timed steps, the pipelined kernel's launches among them, and the one dominant launch
    # (a fit is: a probe of the pipelined kernel on the empty tree, 8 192 elements of k_tree_fast, then ONE long launch)
    all_launches, all_ms, all_units = _profile(lib, b"tree_insert")
    k_launches, total_ms, units = _profile(lib, b"tree_insert/pipe")
    dom_ms, dom_units = _longest(lib, b"tree_insert")
    by_kernel = {name: dict(zip(("launches", "ms", "elements"), _profile(lib, b"tree_insert/" + name.encode())))
                 for name in ("pipe", "fast", "complete")}
    lib.bbh_profile_enable(0)
    if units == 0:  # (a workload the pipelined kernel never took: the record is then about whatever did the work)
        k_launches, total_ms, units = all_launches, all_ms, all_units
    k_launches = max(k_launches, 1)
    avg_ms = total_ms / k_launches
    achieved = BYTES_PER_FP * units / (total_ms * 1e-3) / 1e9 if total_ms > 0 else 0.0
    kc = tree._engine.kernel_counts()

    n_clusters = tree._engine.leaf_count()
    if args.dump_outputs:
        write_outputs(args.dump_outputs, tree_outputs(tree.get_assignments(), tree.get_centroids()))
    full = single_gpu_full(args, n, fps, one_step, lib, dev, local_rank) if args.full else {}

    # HBM traffic of the tree kernel: NOT measured in this run - PMC counters need rocprofv3 (separate passes,
    # tools/profile_bench.sh); the committed measurement is only quoted when it was taken on this very kernel source
    traffic, traffic_source = None, None
    pmc = REPO / "profiles" / "pmc_latest.json"
    src_sha = kernel_src_sha()
    if pmc.is_file():
        try:
            rec = json.loads(pmc.read_text())
            traffic_source = {"file": "profiles/pmc_latest.json", "kernel_src_sha": rec.get("kernel_src_sha"),
                              "this_build_src_sha": src_sha, "n_fps": rec.get("n_fps")}
            if int(rec.get("n_fps", -1)) == n and rec.get("kernel_src_sha") == src_sha:
                # FETCH_SIZE/WRITE_SIZE are in KB; FETCH_SIZE reads 1/2 on gfx950 (MI355X_MICROARCH.md).  Per FIT: the profiled
                # command runs `fits` fits (tools/profile_bench.sh: one timed step + the end-to-end step), each of them one long
                # launch of the pipelined kernel (the dominant launch `achieved` is about) next to a 5 us probe and the first
                # 8 192 elements on k_tree_fast - dividing by all tree-kernel launches read as a third of the truth
                traffic = (2.0 * rec["tree_fetch_kb_total"] + rec["tree_write_kb_total"]) * 1024.0 / max(int(rec.get("fits", 2)), 1)
        except Exception:
            traffic = None
    out = {
        "metric": "fingerprints/sec clustered (2048-bit, thr=%.2g)" % args.threshold,
        "value": args.steps * n / elapsed,
        "unit": "fingerprints/s",
        "n_gpus": 1,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {
            "workload": f"{n} synthetic 2048-bit packed fingerprints ({WORKLOADS[args.workload][2]}), "
                        f"threshold={args.threshold}, branching_factor={args.bf}, "
                        "merge=diameter, BitBirch.fit into a fresh HBM-resident tree, inputs resident in HBM",
            "clusters": n_clusters,
        },
        "roofline": {
            "kernel": "k_tree_pipe (the pipelined tree insertion kernel; k_tree_fast / the complete engine for the stretches it hands over)",
            "bound": "hbm",
            "limiter": "dependency chain of the sequential algorithm (instruction issue of two specialised waves), not bandwidth",
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_per_element": None if traffic is None else traffic / n,
            "traffic_note": "HBM bytes (FETCH_SIZE x 2 + WRITE_SIZE, separate PMC passes) per FIT = per dominant launch; 264 B x elements algorithmic",
            "traffic_source": traffic_source,
            "launches": k_launches,
            "avg_launch_ms": avg_ms,
            "elements_per_launch": units / k_launches,
            "dominant_launch": {"ms": dom_ms, "elements": dom_units,
                                "achieved_GBps": BYTES_PER_FP * dom_units / (dom_ms * 1e-3) / 1e9 if dom_ms > 0 else 0.0},
            # how much of the chip the tree kernels keep busy: the headline's pipelined kernel is ONE workgroup of 256 CUs by
            # construction (a single tree's insertions are one dependency chain); the opt-in level-systolic kernel spreads one
            # tree over its levels' owners (other_workloads.*.systolic_opt_in)
            "workgroups_busy": workgroups_busy(full.get("other_workloads")),
            "by_kernel": by_kernel,
            "last_fit_elements_by_kernel": {"pipe": int(kc[0]), "fast": int(kc[1]), "complete": int(kc[2]),
                                            "unsupported_shape_stops": int(kc[6])},
            "note": "latency/dependency-bound sequential insertion; 264 algorithmic bytes per fingerprint; `achieved` = the "
                    "pipelined kernel's elements x 264 B / its summed launch time (HIP events on the launch stream); "
                    "`dominant_launch` = the single longest tree-kernel launch of the timed steps",
        },
    }
    if args.full:
        out.update(full)
        if not args.no_cpu:
            sample = n if args.cpu_sample is None else min(args.cpu_sample, n)
            out["cpu_baseline"] = cpu_baseline(fps[:sample].cpu().numpy(), args.bf, args.threshold)
        else:
            out["cpu_baseline"] = None
        if args.workload == "fake" and n == 1_000_000 and args.bf == 50:
            out["regressions"] = regressions(out, [REPO / "profiles" / PREVIOUS_ROUND / "bench_line_final.json",
                                                   REPO / f"BENCH_{PREVIOUS_ROUND}.json"])
    _emit(out)


if __name__ == "__main__":
    main()

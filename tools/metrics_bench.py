#!/usr/bin/env python3
r"""Per-cluster against segmented evaluation of the clustering indices on one MI355X (results in
profiles/metrics/).

"Segmented" is what `jt_isim_chi` / `jt_dbi` do with `tree.cluster_sets(fps)`: `bbh_cluster_stats_segments` and
`bbh_dbi_worst_ratios`, a fixed number of launches.  "Per cluster" is the same build with `_segmented=False`: library
calls per cluster and, for DBI, the k x k similarity matrix and a k^2 Python loop.  One process, a warm-up of both first,
then the two alternate inside every repeat.  Wall times are host clocks around synchronised calls; kernel times are the
library's HIP events (`bbh_profile_get`).

  CHI and DBI (centrals="centroid") on trees (bf 50, threshold 0.3) fitted on 3 000 and 200 000 fake fingerprints,
  CHI alone on `--rows` (1 000 000) fingerprints.

Where the per-cluster path would run for many minutes (or cannot hold its matrix) it is timed on a random subset of the
clusters and the line says so: CHI's cost is per cluster and is scaled to all of them ("extrapolated"); DBI's is
quadratic and is reported for the subset only.

    python tools/metrics_bench.py --out profiles/metrics/metrics_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import statistics
import sys
import time
import warnings
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bblean_amd import BitBirch, _lib, make_fake_fingerprints  # noqa: E402
from bblean_amd.metrics import ClusterSets, jt_dbi, jt_isim_chi  # noqa: E402

LINES: list[str] = []
KERNELS = ("cluster_stats_seg", "cluster_stats_seg/small", "cluster_stats_seg/large", "dbi_pairs", "jt_arr_vec")


def say(line: str) -> None:
    LINES.append(line)
    print(line, flush=True)


def prof(lib, name: str) -> float:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _lib.check(lib.bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return float(ms.value)


def timed(fn):  # type: ignore[no-untyped-def]
    r"""(host s, device-event s, result) of one synchronised call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b) * 1e-3, out


def med(v: list[float]) -> str:
    m = statistics.median(v)
    return f"{m * 1e3:10.2f} ms (spread {(max(v) - min(v)) / m * 100:5.1f} %, {len(v)} repeats)"


def subset(sets: ClusterSets, pick: np.ndarray) -> ClusterSets:
    o = sets.offsets
    sizes = np.diff(o)[pick]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mem = np.concatenate([sets.members[o[g]:o[g + 1]] for g in pick])
    return ClusterSets(sets.fps, off, mem, sets.n_features)


def tree_case(lib, fps: np.ndarray, repeats: int, old_sample: int | None, with_dbi: bool) -> None:
    n = len(fps)
    tree = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter")
    t_fit = timed(lambda: tree.fit(fps))[0]
    sets = tree.cluster_sets(fps)
    dev_sets = tree.cluster_sets(torch.from_numpy(fps).cuda())
    k, sizes = len(sets), sets.sizes
    say(f"{n} rows: fit {t_fit:.2f} s, {k} clusters, largest {int(sizes.max())}, {int((sizes < 2).sum())} singletons")
    part = sets if old_sample is None or old_sample >= k else subset(sets, np.sort(np.random.default_rng(0).choice(k, old_sample, replace=False)))
    scale = k / len(part)
    for name, fn in (("jt_isim_chi", jt_isim_chi), ("jt_dbi", jt_dbi)):
        if name == "jt_dbi" and not with_dbi:
            say("  jt_dbi: not measured at this size")
            continue
        new, old = fn(sets), fn(part, _segmented=False)  # warm-up of both
        if part is sets:
            assert new == old or (np.isnan(new) and np.isnan(old)), (name, new, old)
        assert fn(dev_sets) == new or np.isnan(new)
        t_old, t_new, t_dev, e_dev, kern = [], [], [], [], {w: [] for w in KERNELS}
        for _ in range(repeats):
            t_old.append(timed(lambda: fn(part, _segmented=False))[0])
            _lib.check(lib.bbh_profile_reset())
            t_new.append(timed(lambda: fn(sets))[0])
            for w in KERNELS:
                kern[w].append(prof(lib, w))
            h, e, _ = timed(lambda: fn(dev_sets))
            t_dev.append(h)
            e_dev.append(e)
        say(f"  {name} = {new!r}")
        if part is sets:
            say(f"    per cluster (host rows)          {med(t_old)}")
        elif name == "jt_isim_chi":
            say(f"    per cluster (host rows)          {med([t * scale for t in t_old])}  [{len(part)} random clusters timed, "
                f"x {scale:.2f}: extrapolated, the cost is per cluster]")
        else:
            say(f"    per cluster (host rows)          {med(t_old)}  [{len(part)} random clusters ONLY: the cost is quadratic, "
                f"and all {k} need a k x k float64 matrix of {k * k * 8 / 1e9:.1f} GB; not extrapolated]")
        say(f"    segmented (host rows)            {med(t_new)}")
        say(f"    segmented (device rows)          {med(t_dev)}; between device events {statistics.median(e_dev) * 1e3:.2f} ms")
        say("    kernels of the host-rows call: " + ", ".join(f"{w} {statistics.median(v):.3f} ms" for w, v in kern.items()))
        if part is sets or name == "jt_isim_chi":
            say(f"    per cluster / segmented (host rows) = {statistics.median(t_old) * scale / statistics.median(t_new):.1f}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    warnings.simplefilter("ignore", RuntimeWarning)
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    say(f"device: {torch.cuda.get_device_name(0)}; make_fake_fingerprints(seed=7), 2048 bits; the two paths alternate in every repeat")
    tree_case(lib, np.array(make_fake_fingerprints(3000, seed=7), dtype=np.uint8), args.repeats, None, True)
    tree_case(lib, np.array(make_fake_fingerprints(200_000, seed=7), dtype=np.uint8), args.repeats, 2000, True)
    if args.rows > 200_000:
        tree_case(lib, np.array(make_fake_fingerprints(args.rows, seed=7), dtype=np.uint8), args.repeats, 2000, False)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
r"""Old against new medoid / complementary-iSIM paths on one MI355X (results in profiles/medoids/).

"New" is the segmented kernel call (`bbh_compl_isim_segments`) that packed uint8 input takes; "old" is the per-row
host loop, which stays reachable as `input_is_packed=False` on pre-unpacked rows.  One process, a warm-up of both
first, then old and new alternate inside every repeat.  Wall times are host clocks around synchronised calls; kernel
times are the library's HIP events (`bbh_profile_get("compl_isim_seg")`).

  (i)   BitBirch.get_medoids on a tree (bf 50, threshold 0.3) fitted on 3 000, 200 000 and 1 000 000 fake fingerprints
  (ii)  jt_compl_isim of ONE set of 100 000 and of 1 000 000 rows

Where the old path would run for many minutes it is timed on a part and the line says "extrapolated".
`--parent DIR` names a directory that holds the parent commit's `bblean_amd` package (with the built library in it):
its `get_medoids` runs in a child process at the 200 000-row size and must return the same bytes.

    python tools/medoid_bench.py --out profiles/medoids/medoid_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bblean_amd import BitBirch, _lib, make_fake_fingerprints  # noqa: E402
from bblean_amd.similarity import jt_compl_isim, jt_compl_isim_segments, jt_isim_medoid  # noqa: E402

HBM_GBS = 8000.0
LINES: list[str] = []


def say(line: str) -> None:
    LINES.append(line)
    print(line, flush=True)


def prof(lib, name: str) -> tuple[int, float]:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _lib.check(lib.bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    return int(n.value), float(ms.value)


def timed(fn):  # type: ignore[no-untyped-def]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def new_call(lib, fn):  # type: ignore[no-untyped-def]
    r"""(wall s, kernel ms, small ms, large ms, result) of one call of the new path."""
    _lib.check(lib.bbh_profile_reset())
    wall, out = timed(fn)
    return wall, prof(lib, "compl_isim_seg")[1], prof(lib, "compl_isim_seg/small")[1], prof(lib, "compl_isim_seg/large")[1], out


def spread(v: list[float]) -> str:
    med = statistics.median(v)
    return f"{med * 1e3:10.2f} ms (spread {(max(v) - min(v)) / med * 100:5.1f} %, {len(v)} repeats)"


def tree_case(lib, fps: np.ndarray, repeats: int, old_sample: int | None, parent: Path | None) -> None:
    n = len(fps)
    tree = BitBirch(branching_factor=50, threshold=0.3, merge_criterion="diameter")
    t_fit, _ = timed(lambda: tree.fit(fps))
    members = tree.get_cluster_mol_ids()
    sizes = np.array([len(m) for m in members])
    rows3 = int(sizes[sizes >= 3].sum())
    say(f"get_medoids, {n} rows: fit {t_fit:.2f} s, {len(members)} clusters, {int((sizes >= 3).sum())} of >= 3 rows holding "
        f"{rows3} rows, largest {int(sizes.max())}")
    bits = np.unpackbits(fps, axis=1) if old_sample is None else None

    def old():  # type: ignore[no-untyped-def]
        if bits is not None:
            return tree.get_medoids(bits, input_is_packed=False)
        pick = np.random.default_rng(0).choice(len(members), old_sample, replace=False)
        for g in pick:  # the loop of the old path on a random sample of the clusters, unpacking included
            jt_isim_medoid(np.unpackbits(fps[members[g]], axis=1), input_is_packed=False, pack=False)
        return None

    def new():  # type: ignore[no-untyped-def]
        return tree.get_medoids(fps)

    dev = torch.from_numpy(fps).cuda()
    ref_old, ref_new = old(), new()  # warm-up of both
    if ref_old is not None:
        assert np.array_equal(ref_old, ref_new), "old and new medoids differ"
    assert np.array_equal(tree.get_medoids(dev).cpu().numpy(), ref_new)
    t_old, t_new, t_dev, k_new, k_small, k_large = [], [], [], [], [], []
    for _ in range(repeats):
        t_old.append(timed(old)[0])
        w, k, ks, kl, _ = new_call(lib, new)
        t_new.append(w)
        k_new.append(k)
        k_small.append(ks)
        k_large.append(kl)
        t_dev.append(new_call(lib, lambda: tree.get_medoids(dev))[0])
    scale = 1.0 if old_sample is None else len(members) / old_sample
    tag = "" if old_sample is None else f"  [{old_sample} random clusters timed, x {scale:.2f}: extrapolated]"
    old_med = statistics.median(t_old) * scale
    say(f"  old (unpacked rows, host loop)   {spread([t * scale for t in t_old])}{tag}")
    say(f"  new (host rows)                  {spread(t_new)}")
    say(f"  new (device rows)                {spread(t_dev)}")
    kms = statistics.median(k_new)
    nbytes = 2.0 * rows3 * 256 + 8.0 * (n + len(members) + 1)
    say(f"  new kernels {kms:8.3f} ms (small {statistics.median(k_small):.3f}, large {statistics.median(k_large):.3f}); "
        f"{nbytes / 1e6:.1f} MB read = {nbytes / (kms * 1e-3) / 1e9:.1f} GB/s of {HBM_GBS:.0f}; "
        f"host share of the host-rows call {100 * (1 - kms * 1e-3 / statistics.median(t_new)):.1f} %")
    say(f"  old / new (host rows) = {old_med / statistics.median(t_new):.1f}, old / new (device rows) = "
        f"{old_med / statistics.median(t_dev):.1f}")
    if parent is not None:
        code = ("import sys, time, hashlib, numpy as np; sys.path.insert(0, sys.argv[1]); import bblean_amd; "
                "from bblean_amd import BitBirch, make_fake_fingerprints; "
                "assert str(bblean_amd.__file__).startswith(sys.argv[1]); "
                "fps = np.array(make_fake_fingerprints(int(sys.argv[2]), seed=7), dtype=np.uint8); "
                "t = BitBirch(branching_factor=50, threshold=0.3, merge_criterion='diameter').fit(fps); "
                "t0 = time.perf_counter(); m = t.get_medoids(fps); "
                "print(time.perf_counter() - t0, hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest())")
        env = dict(os.environ, PYTHONPATH="")
        child = subprocess.run([sys.executable, "-c", code, str(parent.resolve()), str(n)], capture_output=True, text=True,
                               timeout=900, env=env)
        if child.returncode != 0:
            raise SystemExit("the parent package's child process failed:\n" + child.stderr[-2000:])
        out = child.stdout.split()
        same = out[1] == hashlib.sha256(np.ascontiguousarray(ref_new).tobytes()).hexdigest()
        say(f"  parent commit's get_medoids (packed input, child process): {float(out[0]):.2f} s, medoids "
            f"{'identical to' if same else 'DIFFERENT from'} the new path's")
        assert same


def one_set_case(lib, fps: np.ndarray, repeats: int, old_rows: int | None) -> None:
    n = len(fps)
    dev = torch.from_numpy(fps).cuda()
    off = np.array([0, n], dtype=np.int64)
    say(f"jt_compl_isim, one set of {n} rows")

    def old():  # type: ignore[no-untyped-def]
        return jt_compl_isim(np.unpackbits(fps[: old_rows or n], axis=1), input_is_packed=False)

    ref_new = jt_compl_isim(fps)
    if old_rows is None:
        assert np.array_equal(old(), ref_new), "old and new values differ"
    assert np.array_equal(jt_compl_isim_segments(dev, off)[1].cpu().numpy(), ref_new)
    t_old, t_new, t_dev, k_new = [], [], [], []
    for _ in range(repeats):
        if old_rows is None or not t_old:
            t_old.append(timed(old)[0])
        w, k, _, _, _ = new_call(lib, lambda: jt_compl_isim(fps))
        t_new.append(w)
        w, k, _, _, _ = new_call(lib, lambda: jt_compl_isim_segments(dev, off))
        t_dev.append(w)
        k_new.append(k)
    scale = 1.0 if old_rows is None else n / old_rows
    tag = "" if old_rows is None else f"  [a set of {old_rows} rows timed, x {scale:.1f}: extrapolated, the cost is per row]"
    say(f"  old (unpacked rows, call per row) {spread([t * scale for t in t_old])}{tag}")
    say(f"  new (host rows, staging included) {spread(t_new)}")
    say(f"  new (device rows)                 {spread(t_dev)}")
    kms = statistics.median(k_new)
    nbytes = 2.0 * n * 256
    planes = int(n).bit_length()
    say(f"  new kernels {kms:8.3f} ms; {nbytes / 1e6:.1f} MB read = {nbytes / (kms * 1e-3) / 1e9:.1f} GB/s of {HBM_GBS:.0f}; "
        f"{planes} planes = {planes * 64 * 2 * n / (kms * 1e-3) / 1e12:.2f} T lane-operations/s in the AND + popcount passes")
    say(f"  old / new (host rows) = {statistics.median(t_old) * scale / statistics.median(t_new):.1f}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    lib = _lib.load()
    _lib.check(lib.bbh_profile_enable(1))
    say(f"device: {torch.cuda.get_device_name(0)}; make_fake_fingerprints(seed=7), 2048 bits; old and new alternate in every repeat")
    fps = np.array(make_fake_fingerprints(args.rows, seed=7), dtype=np.uint8)
    tree_case(lib, fps[:3000], args.repeats, None, None)
    tree_case(lib, np.array(make_fake_fingerprints(200_000, seed=7), dtype=np.uint8), 2, None, args.parent)
    tree_case(lib, fps, 3, 50_000, None)
    one_set_case(lib, fps[:100_000], 2, None)
    one_set_case(lib, fps, 3, 100_000)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

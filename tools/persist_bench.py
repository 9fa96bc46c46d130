#!/usr/bin/env python3
r"""Saving, loading and resuming a fitted tree on one MI355X (results in profiles/persist/).

Two trees: the 1 M-row headline (S-fake, bf 50, threshold 0.3, diameter) and a bf 254 S-ecfp tree (1 M sparse rows,
threshold 0.3).  For each, in ONE process, after a warm-up of every step at the full size:

  * image bytes against what the tree uses in HBM: `bbh_tree_memory` [1] (used node bytes) + used cluster-feature bytes
  * `BitBirch.save` / `BitBirch.load`: wall time (a host clock around the call; the file lies in a temporary directory,
    i.e. the page cache), and the device part from the library's profile records "tree_image/save" / "tree_image/load"
  * refitting the same rows (resident in HBM) in the same process - what a load replaces
  * fitting 200 000 further rows into the loaded tree (every node sealed) against the same rows into the never-saved
    tree, alternating inside every repeat

Every repeat does: refit -> continue (never-saved) -> load -> continue (loaded), so the two continuations and the two ways
to get the tree alternate.  Medians and the min-max spread over the repeats are reported; the profile records are taken
in repeats of their own (events on the null stream serialise the call).

    python tools/persist_bench.py --out profiles/persist/persist_bench.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import struct
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "tests" / "golden")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bblean_amd import BitBirch, _lib, make_fake_fingerprints  # noqa: E402
from bblean_amd.bitbirch import _TREE_FILE_MAGIC  # noqa: E402
from cases import fake_chunks, sparse_ecfp_words  # noqa: E402

LINES: list[str] = []


def say(line: str = "") -> None:
    LINES.append(line)
    print(line, flush=True)


def timed(fn):  # type: ignore[no-untyped-def]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def prof(lib, name: str) -> tuple[int, float, int]:
    n, ms, u = C.c_int64(0), C.c_double(0.0), C.c_int64(0)
    _lib.check(lib.bbh_profile_get(name.encode(), C.byref(n), C.byref(ms)))
    _lib.check(lib.bbh_profile_units(name.encode(), C.byref(u)))
    return int(n.value), float(ms.value), int(u.value)


def image_span(path: Path) -> tuple[int, int]:
    r"""(offset, bytes) of the engine image in a tree file: walk the container (INTEGRATION.md "Tree files") from its
    start - magic, version, JSON header, length-prefixed arrays, then the image behind its length word."""
    with open(path, "rb") as f:
        assert f.read(len(_TREE_FILE_MAGIC)) == _TREE_FILE_MAGIC
        _, n_json = struct.unpack("<II", f.read(8))
        header = json.loads(f.read(n_json))
        for _ in header["arrays"]:
            (n,) = struct.unpack("<Q", f.read(8))
            f.seek(n, 1)
        (n_image,) = struct.unpack("<Q", f.read(8))
        at = f.tell()
        assert f.read(8) == b"BBHTREE\0" and at + n_image == path.stat().st_size
    return at, n_image


def spread(v: list[float], unit: str = "s", scale: float = 1.0) -> str:
    return f"{statistics.median(v) * scale:.3f} {unit} (min {min(v) * scale:.3f}, max {max(v) * scale:.3f}, n={len(v)})"


def run(name: str, rows: np.ndarray, more: np.ndarray, kw: dict, repeats: int, tmp: Path, lib) -> None:
    say(f"== {name}: {len(rows):,} rows, then {len(more):,} further rows; {kw}")
    d_rows, d_more = torch.from_numpy(rows).cuda(), torch.from_numpy(more).cuda()
    path = tmp / "tree.bbt"
    t_refit, t_save, t_load, t_cont_plain, t_cont_loaded = [], [], [], [], []
    ref_assign = None
    for rep in range(repeats + 1):  # repeat 0 is the warm-up of every step at the full size
        dt, plain = timed(lambda: BitBirch(**kw).fit(d_rows))
        ds, _ = timed(lambda: plain.save(path))
        if rep == 0:
            mem = plain._engine.memory()
            image = path.stat().st_size
            at, n_image = image_span(path)
            with open(path, "rb") as f:
                f.seek(at + 24)
                h = np.frombuffer(f.read(40), dtype="<u4")  # bf, F, crit, tol_len, ng, rb, n_blocks, n8, n16, n32
            F, n8, n16, n32 = int(h[1]), int(h[7]), int(h[8]), int(h[9])
            used_cf = n8 * F + n16 * F * 2 + n32 * F * 4
            say(f"   file {image:,} bytes, of which engine image {n_image:,}; tree in HBM: used node bytes {int(mem[1]):,} + used "
                f"cluster-feature bytes {used_cf:,} = {int(mem[1]) + used_cf:,} (pool capacity {int(mem[0]) + int(mem[2]):,}); "
                f"image / used = {n_image / (int(mem[1]) + used_cf):.3f}")
        dc, _ = timed(lambda: plain.fit(d_more))
        dl, loaded = timed(lambda: BitBirch.load(path))
        thawed = int(loaded._engine.memory()[7])  # (stats[7] travels in the image: thaws of the tree's earlier life)
        dcl, _ = timed(lambda: loaded.fit(d_more))
        thawed = int(loaded._engine.memory()[7]) - thawed
        a, b = plain.get_assignments(), loaded.get_assignments()
        assert (a == b).all(), "the loaded tree went on differently"
        if ref_assign is None:
            ref_assign = a
        assert (a == ref_assign).all()
        if rep:
            t_refit.append(dt); t_save.append(ds); t_load.append(dl); t_cont_plain.append(dc); t_cont_loaded.append(dcl)
        del plain, loaded
    say(f"   refit of the same rows (device-resident): {spread(t_refit)}")
    say(f"   save: {spread(t_save)}")
    say(f"   load: {spread(t_load)}   -> refit / load = {statistics.median(t_refit) / statistics.median(t_load):.2f}")
    n_more = len(more)
    say(f"   {n_more:,} further rows into the never-saved tree: {spread(t_cont_plain)} = {n_more / statistics.median(t_cont_plain):,.0f} rows/s")
    say(f"   {n_more:,} further rows into the loaded tree:      {spread(t_cont_loaded)} = {n_more / statistics.median(t_cont_loaded):,.0f} rows/s "
        f"({thawed:,} sealed nodes thawed by these rows)")
    lo, hi = min(t_cont_plain), max(t_cont_plain)
    say(f"   loaded / never-saved (medians) = {statistics.median(t_cont_loaded) / statistics.median(t_cont_plain):.3f}; run-to-run spread of the "
        f"never-saved tree: {lo / statistics.median(t_cont_plain):.3f} .. {hi / statistics.median(t_cont_plain):.3f} of its median")
    # the device part of save / load, from the profile records, in repeats of their own
    tree = BitBirch(**kw).fit(d_rows)
    ks, kl = [], []
    _lib.check(lib.bbh_profile_enable(1))
    for _ in range(3):
        _lib.check(lib.bbh_profile_reset())
        tree.save(path)
        n_s, ms_s, u_s = prof(lib, "tree_image/save")
        _lib.check(lib.bbh_profile_reset())
        back = BitBirch.load(path)
        n_l, ms_l, u_l = prof(lib, "tree_image/load")
        ks.append(ms_s / 1e3); kl.append(ms_l / 1e3)
        del back
    _lib.check(lib.bbh_profile_enable(0))
    say(f"   device part (profile records, {n_s} / {n_l} ranges, units {u_s:,} / {u_l:,} bytes): save {spread(ks, 'ms', 1e3)}, load {spread(kl, 'ms', 1e3)}")
    say()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--more", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "persist_bench.py measures on the GPU"
    lib = _lib.load()
    say(f"persist_bench: {torch.cuda.get_device_name(0)}, rows {args.rows:,} + {args.more:,}, {args.repeats} repeats after one warm-up")
    say()
    with tempfile.TemporaryDirectory() as d:
        fake = fake_chunks(args.rows + args.more, 1000, make_fake_fingerprints)
        run("headline S-fake, bf 50", fake[:args.rows], fake[args.rows:], dict(branching_factor=50, threshold=0.3, merge_criterion="diameter"),
            args.repeats, Path(d), lib)
        del fake
        ecfp = sparse_ecfp_words(args.rows + args.more, 2048, 3003)
        run("S-ecfp, bf 254", ecfp[:args.rows], ecfp[args.rows:], dict(branching_factor=254, threshold=0.3, merge_criterion="diameter"),
            args.repeats, Path(d), lib)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
r"""Golden values of the complementary iSIM and the medoid (reference bblean/_py_similarity.py:65-117) produced by
running the REFERENCE in the build container.  Data only: offsets, members, float64 values, positions.  The input
rows are NOT stored: `medoid_cases` rebuilds them from the seeds, here and in the tests.

    python tests/golden/make_golden_medoids.py   ->  tests/golden/medoids.npz

The archive is written with fixed member timestamps, so the same inputs give the same bytes.
"""
from __future__ import annotations

import io
import sys
import warnings
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from _refimport import import_reference  # noqa: E402

import_reference(use_cpp=False)

from bblean.bitbirch import BitBirch  # noqa: E402
from bblean.fingerprints import make_fake_fingerprints  # noqa: E402
from bblean.similarity import jt_compl_isim, jt_isim_medoid  # noqa: E402

import medoid_cases as mc  # noqa: E402


def write_npz(path: Path, arrays: dict[str, np.ndarray]) -> None:
    r"""np.savez_compressed with a fixed timestamp on every member (NumPy stamps the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def reference_sets(rows: np.ndarray, offsets: np.ndarray, members: np.ndarray) -> tuple[np.ndarray, np.ndarray, int, int]:
    compl = np.empty(len(members), dtype=np.float64)
    med = np.zeros(len(offsets) - 1, dtype=np.int64)
    big, tied = 0, 0
    for g in range(len(offsets) - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        sel = rows[members[lo:hi]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            v = jt_compl_isim(sel)
        compl[lo:hi] = v
        med[g] = jt_isim_medoid(sel)[0]
        if hi - lo >= 3:
            big += 1
            tied += int((v == v.min()).sum() > 1)
    return compl, med, big, tied


def main() -> None:
    out: dict[str, np.ndarray] = {}
    # the clusters of a fitted tree
    rows = mc.tree_rows(make_fake_fingerprints)
    tree = BitBirch(branching_factor=mc.TREE["bf"], threshold=mc.TREE["thr"], merge_criterion="diameter")
    tree.fit(rows)
    ids = tree.get_cluster_mol_ids()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in ids])]).astype(np.int64)
    members = np.array([i for c in ids for i in c], dtype=np.int64)
    compl, med, n_big, n_tied = reference_sets(rows, offsets, members)
    print(f"tree: {len(ids)} sets, {n_big} with >= 3 rows, {n_tied} of them with a tied minimum")
    out["tree_offsets"], out["tree_members"], out["tree_compl"], out["tree_medoid"] = offsets, members, compl, med
    total_big, total_tied = n_big, n_tied

    # hand-made sets
    rows = mc.hand_rows(make_fake_fingerprints)
    offsets, members = mc.hand_index()
    compl, med, n_big, n_tied = reference_sets(rows, offsets, members)
    print(f"hand: {len(offsets) - 1} sets, {n_big} with >= 3 rows, {n_tied} of them with a tied minimum")
    assert med[5] == 0, med  # [a, a, b, b, c]
    assert (compl[offsets[3]:offsets[4]] == 1.0).all()  # all-zero rows
    out["hand_offsets"], out["hand_members"], out["hand_compl"], out["hand_medoid"] = offsets, members, compl, med
    total_big += n_big
    total_tied += n_tied

    # one large set with repeated rows: the value of a row depends on its bits only
    distinct, draw = mc.big_rows(make_fake_fingerprints)
    v = jt_compl_isim(distinct[draw])
    per_row = np.full(len(distinct), np.nan)
    per_row[draw] = v
    assert np.array_equal(per_row[draw], v), "equal rows must have equal values"
    out["big_compl_distinct"] = per_row
    out["big_medoid"] = np.array([jt_isim_medoid(distinct[draw])[0]], dtype=np.int64)
    assert out["big_medoid"][0] == int(np.argmin(v))
    total_big += 1
    total_tied += int((v == v.min()).sum() > 1)
    print(f"big: {len(draw)} rows, {int(np.isfinite(per_row).sum())} distinct rows drawn, medoid at {out['big_medoid'][0]}")

    # a fixture without sets of >= 3 rows, or without ties, would pass a kernel that is wrong there
    assert total_big >= 500, total_big
    assert total_tied >= 5, total_tied
    # the restatement the CPU test pins must agree before anything is written
    for name, r in (("tree", mc.tree_rows(make_fake_fingerprints)), ("hand", mc.hand_rows(make_fake_fingerprints))):
        m2, c2 = mc.compl_isim_segments(r, out[name + "_offsets"], out[name + "_members"])
        assert np.array_equal(m2, out[name + "_medoid"]), name
        assert np.array_equal(c2, out[name + "_compl"], equal_nan=True), name
    path = HERE / "medoids.npz"
    write_npz(path, out)
    print("wrote", path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 684 * 1024


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
r"""Golden values of the clustering metrics (reference bblean/metrics.py) on clusterings of a few hundred clusters,
produced by running the REFERENCE on the CPU.  Data only: seeds, sizes, member indices, float64 results.

    python tests/golden/make_golden_metrics_segments.py   ->  tests/golden/metrics_segments.npz

Case 0: 202 clusters over 6 000 fake fingerprints - one of 2 100 rows, some of 1 and 2 rows, and two clusters that are
copies of one row (identical centroids and medoids, no scatter: the reference divides 0 by 0 there).  CHI, DBI on centroids
and on medoids; and DBI on centroids once more with a 203rd cluster that repeats cluster 7 (identical centroids with
scatter: a division by zero, the index is inf).
Case 1: 60 clusters of 2 rows and more over 1 500 fingerprints; adds Dunn, and every index on unpacked input too.
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from _refimport import import_reference  # noqa: E402

import_reference(use_cpp=True)

from bblean.fingerprints import make_fake_fingerprints, unpack_fingerprints  # noqa: E402
from bblean.metrics import jt_dbi, jt_isim_chi, jt_isim_dunn  # noqa: E402

TWIN_OF = 7


def case0_members(rng: np.random.Generator, n: int) -> list[np.ndarray]:
    sizes = [2100, 1, 2, 1, 2] + rng.integers(3, 31, 195).tolist()
    perm = rng.permutation(n)
    cuts = np.cumsum(sizes)
    assert cuts[-1] + 1 <= n
    members = np.split(perm[: cuts[-1]], cuts[:-1])
    row = int(perm[cuts[-1]])
    return members + [np.full(3, row), np.full(4, row)]


def case1_members(rng: np.random.Generator, n: int) -> list[np.ndarray]:
    sizes = [2, 2, 3] + rng.integers(2, 45, 57).tolist()
    perm = rng.permutation(n)
    cuts = np.cumsum(sizes)
    assert cuts[-1] <= n
    return np.split(perm[: cuts[-1]], cuts[:-1])


def main() -> None:
    out: dict[str, np.ndarray] = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        seed, n = 31337, 6000
        fps = make_fake_fingerprints(n, seed=seed, pack=True)
        members = case0_members(np.random.default_rng(seed), n)
        clusters = [fps[m] for m in members]
        vals = [jt_isim_chi(clusters), jt_dbi(clusters), jt_dbi(clusters, centrals="medoid"),
                jt_dbi(clusters + [clusters[TWIN_OF]])]
        out["c0_case"] = np.array([seed, n, TWIN_OF], dtype=np.int64)
        out["c0_sizes"] = np.array([len(m) for m in members], dtype=np.int64)
        out["c0_members"] = np.concatenate(members).astype(np.int64)
        out["c0_values"] = np.array(vals, dtype=np.float64)
        print(len(members), vals)

        seed, n = 2718, 1500
        fps = make_fake_fingerprints(n, seed=seed, pack=True)
        members = case1_members(np.random.default_rng(seed), n)
        clusters = [fps[m] for m in members]
        unpacked = [unpack_fingerprints(c) for c in clusters]
        vals = [jt_isim_chi(clusters), jt_dbi(clusters), jt_dbi(clusters, centrals="medoid"), jt_isim_dunn(clusters),
                jt_isim_chi(unpacked, input_is_packed=False), jt_dbi(unpacked, input_is_packed=False),
                jt_dbi(unpacked, centrals="medoid", input_is_packed=False), jt_isim_dunn(unpacked, input_is_packed=False)]
        out["c1_case"] = np.array([seed, n], dtype=np.int64)
        out["c1_sizes"] = np.array([len(m) for m in members], dtype=np.int64)
        out["c1_members"] = np.concatenate(members).astype(np.int64)
        out["c1_values"] = np.array(vals, dtype=np.float64)
        print(len(members), vals)
    np.savez_compressed(HERE / "metrics_segments.npz", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
r"""Golden values of the scikit-learn face (reference bblean/sklearn.py: fit / predict / transform) produced by
running the REFERENCE (pure-Python backend) with scikit-learn in the build container.  Data only: packed
centroids, labels, distances.  The input rows are NOT stored: `sklearn_cases.rows` rebuilds them from the seeds,
here and in the tests.

    python tests/golden/make_golden_sklearn.py   ->  tests/golden/sklearn.npz

The archive is written with fixed member timestamps, so the same inputs give the same bytes.
"""
from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from _refimport import import_reference  # noqa: E402

import_reference(use_cpp=False)

from bblean.fingerprints import make_fake_fingerprints, pack_fingerprints  # noqa: E402
from bblean.sklearn import BitBirch, UnpackedBitBirch  # noqa: E402

from sklearn_cases import CASES, N_DIST_ROWS, rows  # noqa: E402


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


def main() -> None:
    out: dict[str, np.ndarray] = {}
    for name, case in CASES.items():
        fit_x, qry_x = rows(case, make_fake_fingerprints)
        cls = BitBirch if case["packed"] else UnpackedBitBirch
        est = cls(threshold=case["thr"], branching_factor=case["bf"]).fit(fit_x)
        centers = np.asarray(est.subcluster_centers_)
        k = centers.shape[0]
        assert k == case["K"], (name, k)
        assert est._n_features_out == k
        assert (est.subcluster_labels_ == np.arange(1, k + 1)).all()
        prefix = cls.__name__.lower()
        assert list(est.get_feature_names_out()[:2]) == [prefix + "0", prefix + "1"]
        labels = est.predict(qry_x)
        dist = est.transform(qry_x)
        assert labels.dtype == np.int64 and dist.dtype == np.float64 and dist.shape == (len(qry_x), k)
        assert (labels == np.argmin(dist, axis=1) + 1).all()
        q_unpacked = np.unpackbits(qry_x, axis=1) if case["packed"] else qry_x
        zero_q = np.flatnonzero(q_unpacked.sum(axis=1) == 0)
        zero_c = np.flatnonzero(centers.sum(axis=1) == 0)
        tied = int(((dist == dist.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        print(f"case {name}: K = {k}, {len(qry_x)} queries, {tied} with a tied minimum, "
              f"{zero_q.size} all-zero queries, {zero_c.size} all-zero centroids")
        if name == "B":
            # a fixture without ties would pass a kernel with the wrong tie-break; one without an all-zero pair would
            # pass a kernel that ranks an empty union as similarity 0
            assert tied >= 25, tied
            assert zero_c.size >= 1 and zero_q.size >= 1
            assert all(labels[q] - 1 in zero_c for q in zero_q), (labels[zero_q], zero_c)
        keep = np.unique(np.concatenate([np.arange(N_DIST_ROWS), zero_q]))
        out[f"{name}_centroids"] = pack_fingerprints(centers.astype(np.uint8))
        out[f"{name}_fit_labels"] = np.asarray(est.labels_).astype(np.uint64)
        out[f"{name}_labels"] = labels
        out[f"{name}_dist_rows"] = keep.astype(np.int64)
        out[f"{name}_dist"] = dist[keep]
        out[f"{name}_tied"] = np.array([tied], dtype=np.int64)
    write_npz(HERE / "sklearn.npz", out)
    print("wrote", HERE / "sklearn.npz", (HERE / "sklearn.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

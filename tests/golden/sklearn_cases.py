r"""The four cases of tests/golden/sklearn.npz (data only; shared by the generator, which runs the reference, and
the tests, which run this package - both rebuild the rows from the seeds with their own `make_fake_fingerprints`,
which give the same arrays bit for bit)."""
from __future__ import annotations

import numpy as np

N_DIST_ROWS = 16  # `transform` rows kept per case: the first 16 queries plus every all-zero query
ZEROED = (5, 700, 1499)  # rows of cases B-D that are set to all zeros: 5 and 700 are fitted, 1499 is a query

CASES = {
    "A": dict(kind="fake", n=3000, seed=7, n_fit=2000, thr=0.3, bf=50, K=793, packed=True, nbits=2048),
    "B": dict(kind="rng", n=1500, seed=64, n_fit=1000, thr=0.5, bf=50, K=997, packed=True, nbits=64),
    "C": dict(kind="rng", n=1500, seed=128, n_fit=1000, thr=0.4, bf=50, K=999, packed=True, nbits=128),
    "D": dict(kind="fake", n=1500, seed=11, n_fit=1000, thr=0.65, bf=50, K=991, packed=False, nbits=2048),
}


def rows(case: dict, make_fake_fingerprints) -> tuple[np.ndarray, np.ndarray]:  # type: ignore[no-untyped-def]
    r"""(rows to fit, query rows) of a case: packed uint8 rows, or unpacked 0/1 uint8 rows for case D."""
    if case["kind"] == "fake":
        x = make_fake_fingerprints(case["n"], seed=case["seed"], pack=case["packed"])
        x = np.array(x, dtype=np.uint8)
        if case["n"] == 3000:  # case A: two all-zero queries appended
            x = np.concatenate([x, np.zeros((2, x.shape[1]), np.uint8)])
        else:
            x[list(ZEROED)] = 0
    else:
        bits = (np.random.default_rng(case["seed"]).random((case["n"], case["nbits"])) < 0.25).astype(np.uint8)
        bits[list(ZEROED)] = 0
        x = np.packbits(bits, axis=1)
    return x[: case["n_fit"]], x[case["n_fit"]:]

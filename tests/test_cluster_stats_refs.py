r"""The NumPy references of tests/cluster_stats_refs.py against the C oracle, set by set and pair by pair, on cases
test_hip_cluster_stats_edges.py uses on the GPU.  No GPU needed: a reference that is wrong fails here."""
from __future__ import annotations

import warnings

import numpy as np
import pytest

import cluster_stats_refs as cs
import kernel_refs as R
from oracle_engine import oracle_lib


def o_set(sub: np.ndarray, nf: int, central: np.ndarray | None):
    r"""One set through the oracle: add_rows of the unpacked rows, centroid_from_sum, jt_isim_from_sum, arr-vec."""
    lib = oracle_lib()
    m, nb = sub.shape
    un = np.ascontiguousarray(np.unpackbits(sub, axis=1)[:, :nf])
    ls = np.empty(nf, np.uint64)
    lib.bbo_add_rows(un.ctypes.data, m, nf, ls.ctypes.data)
    cen = np.empty(nf // 8, np.uint8)
    lib.bbo_centroid_from_sum(ls.ctypes.data, nf, m, 1, cen.ctypes.data)
    isim = lib.bbo_isim_from_sum(ls.ctypes.data, nf, m)
    c = cen if central is None else central
    sim = np.empty(m)
    lib.bbo_jt_arr_vec(sub.ctypes.data, m, nb, c.ctypes.data, None, sim.ctypes.data, None, None)
    return cen, isim, 1 - sim, ls


def check_against_oracle(rows, off, mem, nf, ref, centrals=None):
    cents, isim, dist, sums = ref
    nb = nf // 8
    for g in range(len(off) - 1):
        b, e = int(off[g]), int(off[g + 1])
        sub = np.ascontiguousarray((rows[mem[b:e]] if mem is not None else rows[b:e])[:, :nb])
        cen, i, d, ls = o_set(sub, nf, None if centrals is None else np.ascontiguousarray(centrals[g, :nb]))
        assert (cen == cents[g]).all() and (ls == sums[g]).all(), g
        assert R.bits(np.array([i]))[0] == R.bits(isim[g:g + 1])[0] or (np.isnan(i) and np.isnan(isim[g])), g
        assert (R.bits(d) == R.bits(dist[b:e])).all(), g


def test_ref_small_mix_and_given_centrals():
    rows, off, ref = cs.small_mix()
    check_against_oracle(rows, off, None, 128, ref)
    assert np.isnan(ref[1][0]) and not np.isnan(ref[1][1:]).any()
    centrals = R.density_rows(np.random.default_rng(3), len(off) - 1, 16, 0.1, 0.9)
    check_against_oracle(rows, off, None, 128, cs.ref_cluster_stats(rows, off, centrals=centrals), centrals)


def test_ref_mix_first_sets_and_weighted_set():
    rows, off, mem, ref = cs.mix_case()
    k = len(cs.MIX_SIZES)
    first = list(range(9)) + [k - 1]  # up to 2047 rows, and the 70 001 members
    for g in first:
        o = off[g:g + 2] - off[g]
        sub_ref = tuple(x[g:g + 1] if x.ndim == 2 or len(x) == k else x[off[g]:off[g + 1]] for x in ref)
        check_against_oracle(rows, o, mem[off[g]:off[g + 1]], cs.MIX_NB * 8, sub_ref)


@pytest.mark.parametrize("nb", [1, 3, 260])
def test_ref_widths(nb):
    buf, nbytes, stride, nf, off, ref = cs.width_case(nb, True)
    assert buf[:, nb:].all()  # garbage behind the features
    check_against_oracle(np.ascontiguousarray(buf[:, :nb]), off, None, nf, ref)
    plain = cs.width_case(nb, False)
    assert all((R.bits(a) == R.bits(b)).all() if a.dtype == np.float64 else (a == b).all()
               for a, b in zip(ref, plain[5]) if not np.isnan(a.astype(np.float64)).any())


@pytest.mark.parametrize("m", cs.TIE_MS)
def test_ref_majority_ties(m):
    rows, counts = cs.tie_rows(m)
    cents, _, _, sums = cs.ref_cluster_stats(rows, cs.offsets_of([m]))
    assert (sums[0] == counts).all()
    want = (2 * counts >= m) if m > 1 else counts > 0
    assert (np.unpackbits(cents[0]) == want).all()
    near = {m // 2, m // 2 - 1} if m % 2 == 0 else {(m + 1) // 2, (m - 1) // 2}
    assert near & set(counts.tolist()) == {c for c in near if c >= 0}
    check_against_oracle(rows, cs.offsets_of([m]), None, 64, cs.ref_cluster_stats(rows, cs.offsets_of([m])))


def loop_worst_ratios(cents, scatter):
    r"""metrics.py:149-158 as written, similarities from the oracle's arr-vec."""
    lib = oracle_lib()
    k, nb = cents.shape
    out = np.zeros(k)
    for i in range(k):
        sim = np.empty(k)
        lib.bbo_jt_arr_vec(cents.ctypes.data, k, nb, cents[i].ctypes.data, None, sim.ctypes.data, None, None)
        max_d = 0.0
        for j in range(k):
            if i == j:
                continue
            mij = 1 - sim[j].item()
            max_d = max(max_d, (scatter[i] + scatter[j]) / mij)
        out[i] = max_d
    return out


@pytest.mark.parametrize("k,nb", [(1, 3), (2, 1), (3, 260), (cs.DBI_TILE + 1, 16)])
def test_ref_worst_ratios(k, nb):
    cents, scatter = cs.dbi_case(k, nb)
    worst, flags = cs.ref_worst_ratios(cents, scatter)
    assert (R.bits(worst) == R.bits(loop_worst_ratios(cents, scatter))).all() and not flags.any()


def test_ref_worst_ratios_divisions_by_zero():
    cents, scatter = cs.dbi_case(6, 8)
    cents[4] = cents[1]          # identical, with scatter: inf, two ordered pairs
    cents[5] = cents[2]          # identical, without: 0 / 0 is skipped
    scatter[2] = scatter[5] = 0.0
    worst, flags = cs.ref_worst_ratios(cents, scatter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert (R.bits(worst) == R.bits(loop_worst_ratios(cents, scatter))).all()
    assert flags.tolist() == [2, 2] and np.isinf(worst[[1, 4]]).all() and np.isfinite(worst[[0, 2, 3, 5]]).all()

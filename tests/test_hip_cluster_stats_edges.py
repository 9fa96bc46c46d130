r"""Edge cases of the cluster statistics kernels (bblean_amd/csrc/bb_cluster_stats.hip) through the raw C ABI,
`bbh_cluster_stats_segments` and `bbh_dbi_worst_ratios`, against the references of cluster_stats_refs.py.  Everything
observable is compared bit for bit (float64 as bit patterns, so NaN positions and signs of zero count).  Output buffers are
longer than the call may write and pre-filled with sentinels."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import cluster_stats_refs as cs
import kernel_refs as R

pytestmark = pytest.mark.gpu

PAD = 5
SENT_F64 = -12345.5
SENT_U8 = 0xA5
SENT_U64 = 0xDEADBEEFDEADBEEF
SENT_U32 = 0xCAFEF00D
INVALID = 1  # BBH_ERR_INVALID
NAMES = ("centroids", "isim", "dist", "sums")


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def at(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def buffers(k, nf, total, want=NAMES):
    out = {
        "centroids": np.full(k * (nf // 8) + PAD, SENT_U8, np.uint8),
        "isim": np.full(k + PAD, SENT_F64),
        "dist": np.full(total + PAD, SENT_F64),
        "sums": np.full(k * nf + PAD, SENT_U64, np.uint64),
    }
    return {w: v for w, v in out.items() if w in want}


def untouched(bufs, start=None):
    sent = {"centroids": SENT_U8, "isim": SENT_F64, "dist": SENT_F64, "sums": SENT_U64}
    return all((b[(start or {}).get(w, 0):] == sent[w]).all() for w, b in bufs.items())


def call(lib, rows, n_rows, nbytes, stride, mem, off, k, nf, bufs, centrals=None, c_stride=0, stream=None):
    return lib.bbh_cluster_stats_segments(at(rows), n_rows, nbytes, stride, at(mem), at(off), k, nf, at(centrals), c_stride,
                                          *(at(bufs.get(w)) for w in NAMES), stream)


def same(lib, rc, bufs, ref, k, nf, total, what=""):
    assert rc == 0, (what, rc, lib.bbh_last_error())
    ends = {"centroids": k * (nf // 8), "isim": k, "dist": total, "sums": k * nf}
    assert untouched(bufs, ends), (what, "written behind the end")
    for w, want in zip(NAMES, ref):
        if w not in bufs:
            continue
        got, want = bufs[w][:ends[w]], want.reshape(-1)
        if want.dtype == np.float64:
            got, want = R.bits(got), R.bits(want)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, w, bad[:10], bufs[w][bad[:5]], ref[NAMES.index(w)].reshape(-1)[bad[:5]])


def run_host(lib, rows, nbytes, stride, mem, off, nf, ref, what="", centrals=None, c_stride=0, want=NAMES):
    k, total = len(off) - 1, int(off[-1])
    bufs = buffers(k, nf, total, want)
    rc = call(lib, rows, len(rows), nbytes, stride, mem, off, k, nf, bufs, centrals, c_stride)
    same(lib, rc, bufs, ref, k, nf, total, what)


# ---------------------------------------------------------------------------------------------------------------------
# set sizes, ties, special rows, widths
# ---------------------------------------------------------------------------------------------------------------------


def test_mixed_set_sizes_in_one_call(lib):
    r"""1 .. 65 rows, both sides of the one-wave limit, the chunk edges of the large path and 70 001 members over 48 rows
    (17 planes), in one call; members unordered and with repeats."""
    rows, off, mem, ref = cs.mix_case()
    sizes = np.diff(off)
    assert (sizes <= cs.SMALL_MAX).sum() == 9 and (sizes > cs.SMALL_MAX).sum() == 5
    assert (np.diff(mem[:3000]) < 0).any() and len(np.unique(mem[off[8]:off[9]])) < sizes[8]
    run_host(lib, rows, cs.MIX_NB, cs.MIX_NB, mem, off, cs.MIX_NB * 8, ref, "mix")


@pytest.mark.parametrize("m", cs.TIE_MS)
def test_majority_ties(lib, m):
    r"""Columns at exactly m / 2 (set) and m / 2 - 1 (clear), (m + 1) / 2 and (m - 1) / 2 for odd m, on both paths."""
    rows, counts = cs.tie_rows(m)
    off = cs.offsets_of([m])
    ref = cs.ref_cluster_stats(rows, off)
    assert (np.unpackbits(ref[0][0]) == (2 * counts >= m)).all()
    run_host(lib, rows, 8, 8, None, off, 64, ref, m)


@pytest.mark.parametrize("m", [1, 5, 2100])
def test_zero_and_identical_rows(lib, m):
    r"""An all-zero set: zero centroid, distances 1.0, iSIM 1.0.  A set of identical rows: distances 0.0."""
    rng = np.random.default_rng(m)
    one = R.density_rows(rng, 1, 32, 0.3, 0.5)
    rows = np.concatenate([np.zeros((m, 32), np.uint8), np.repeat(one, m, axis=0)])
    off = cs.offsets_of([m, m])
    ref = cs.ref_cluster_stats(rows, off)
    assert not ref[0][0].any() and (ref[2][:m] == 1.0).all() and (ref[2][m:] == 0.0).all() and (ref[0][1] == one[0]).all()
    assert (ref[1][0] == 1.0) if m >= 2 else np.isnan(ref[1]).all()
    run_host(lib, rows, 32, 32, None, off, 256, ref, m)


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("nb", cs.WIDTHS)
def test_widths(lib, nb, padded):
    r"""One word, a word's part, the last width of one word per lane and the first of two, the last width in registers
    and the widths beyond; padded: n_features < nbytes * 8 with garbage behind, and row_stride > nbytes."""
    buf, nbytes, stride, nf, off, ref = cs.width_case(nb, padded)
    assert (np.diff(off) > cs.SMALL_MAX).any() and (np.diff(off) <= cs.SMALL_MAX).any()
    run_host(lib, buf, nbytes, stride, None, off, nf, ref, (nb, padded))


# ---------------------------------------------------------------------------------------------------------------------
# centrals, outputs, residency, alignment
# ---------------------------------------------------------------------------------------------------------------------


def test_given_centrals(lib):
    r"""The computed centroids handed back as centrals give the same distances; other centrals give the reference's; both
    with a stride of their own."""
    rows, off, ref = cs.small_mix()
    k = len(off) - 1
    table = np.full((k, 19), 0xFF, np.uint8)
    table[:, :16] = ref[0]
    run_host(lib, rows, 16, 16, None, off, 128, ref, "own centroids", table, 19)
    table[:, :16] = R.density_rows(np.random.default_rng(4), k, 16, 0.1, 0.9)
    ref2 = cs.ref_cluster_stats(rows, off, centrals=table)
    assert (R.bits(ref2[2]) != R.bits(ref[2])).any() and (ref2[0] == ref[0]).all()
    run_host(lib, rows, 16, 16, None, off, 128, ref2, "other centrals", table, 19)
    run_host(lib, rows, 16, 16, None, off, 128, ref2, "distances alone", table, 19, want=("dist",))


@pytest.mark.parametrize("want", [c for n in range(5) for c in itertools.combinations(NAMES, n)])
def test_every_subset_of_outputs(lib, want):
    rows, off, ref = cs.small_mix()
    run_host(lib, rows, 16, 16, None, off, 128, ref, want, want=want)


@pytest.mark.parametrize("dev_rows,dev_off,dev_mem", list(itertools.product([False, True], repeat=3)))
def test_mixed_residency(lib, torch, dev_rows, dev_off, dev_mem):
    rows, off, mem, ref = cs.mix_case()
    k = 9  # the sets of up to 2047 rows and one large set keep this quick
    off, mem = np.ascontiguousarray(off[:k + 2]), np.ascontiguousarray(mem[:off[k + 1]])
    ref = (ref[0][:k + 1], ref[1][:k + 1], ref[2][:off[-1]], ref[3][:k + 1])
    put = lambda a, on_dev: torch.from_numpy(a).cuda() if on_dev else a  # noqa: E731
    a_rows, a_off, a_mem = put(rows, dev_rows), put(off, dev_off), put(mem, dev_mem)
    bufs = buffers(k + 1, 512, int(off[-1]))
    rc = call(lib, a_rows, len(rows), 64, 64, a_mem, a_off, k + 1, 512, bufs)
    same(lib, rc, bufs, ref, k + 1, 512, int(off[-1]), (dev_rows, dev_off, dev_mem))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift", [0, 1, 4])
def test_device_outputs_on_side_stream_and_misaligned_bases(lib, torch, shift):
    r"""Rows, centrals and the centroid output at device addresses 1 and 4 bytes off a 16-byte boundary; inputs produced
    on a non-blocking side stream, the call enqueued on it, every output in device memory."""
    rows, off, ref = cs.small_mix()
    k, total = len(off) - 1, int(off[-1])
    src = torch.from_numpy(rows).cuda().reshape(-1)
    flat = torch.zeros(rows.size + 16, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    host = buffers(k, 128, total)
    dev = {w: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).cuda() for w, v in host.items()}
    cent = torch.full((k * 16 + PAD + 16,), SENT_U8, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        flat[shift:shift + rows.size].copy_(src ^ 0xFF).bitwise_xor_(0xFF)
        rc = lib.bbh_cluster_stats_segments(flat.data_ptr() + shift, len(rows), 16, 16, None, at(off), k, 128, None, 0,
                                            cent.data_ptr() + shift, dev["isim"].data_ptr(), dev["dist"].data_ptr(),
                                            dev["sums"].data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    got = {"centroids": cent[shift:shift + k * 16 + PAD].cpu().numpy(), "isim": dev["isim"].cpu().numpy(),
           "dist": dev["dist"].cpu().numpy(), "sums": dev["sums"].cpu().numpy().view(np.uint64)}
    assert (cent[:shift].cpu().numpy() == SENT_U8).all()
    same(lib, 0, got, ref, k, 128, total, shift)
    # the same centroids as misaligned, strided device centrals
    table = torch.zeros(k * 21 + 16, dtype=torch.uint8, device="cuda")
    view = table[shift:shift + k * 21].reshape(k, 21)
    view[:, :16] = torch.from_numpy(ref[0]).cuda()
    bufs = buffers(k, 128, total, ("dist",))
    rc = call(lib, flat.data_ptr() + shift, len(rows), 16, 16, None, off, k, 128, bufs, view, 21)
    same(lib, rc, bufs, ref, k, 128, total, ("centrals", shift))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------

GOOD = dict(rows=True, n_rows=50, nb=16, stride=16, members=None, offsets=[0, 10, 30, 50], k=3, nf=128, centrals=False,
            c_stride=0)
REFUSALS = {
    "NULL rows": (dict(rows=False), "need rows"),
    "NULL offsets": (dict(offsets=None), "need rows"),
    "k = 0": (dict(k=0), "need rows"),
    "n_rows = 0": (dict(n_rows=0), "need rows"),
    "row_stride < nbytes": (dict(stride=15), "need rows"),
    "n_features = 0": (dict(nf=0), "divisible by 8"),
    "n_features = 12": (dict(nf=12), "divisible by 8"),
    "n_features wider than the row": (dict(nf=16 * 8 + 8), "divisible by 8"),
    "offsets[0] = 1": (dict(offsets=[1, 10, 30, 50]), "start at 0"),
    "decreasing offsets": (dict(offsets=[0, 30, 10, 50]), "decrease"),
    "empty set in the middle": (dict(offsets=[0, 10, 10, 50]), "is empty"),
    "offsets[k] > n_rows": (dict(offsets=[0, 10, 30, 51]), "offsets name"),
    "members holding -1": (dict(members=-1), "not a row"),
    "members holding n_rows": (dict(members=50), "not a row"),
    "2^31 rows": (dict(offsets=[0, 1 << 31], k=1), "2^63"),
    "2^26 rows of 2^11 features": (dict(offsets=[0, 1 << 26], k=1, nb=256, stride=256, nf=2048), "2^63"),
    "centrals closer than a row": (dict(centrals=True, c_stride=15), "centrals_stride"),
    "a stride without centrals": (dict(c_stride=16), "centrals_stride"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID with the message of the check that is meant, before any launch, outputs untouched."""
    change, message = REFUSALS[name]
    a = dict(GOOD, **change)
    rows = np.ones((50, 256), np.uint8)
    off = None if a["offsets"] is None else np.array(a["offsets"], dtype=np.int64)
    mem = None
    if a["members"] is not None:
        mem = np.arange(50, dtype=np.int64)
        mem[17] = a["members"]
    cen = np.ones((3, 16), np.uint8) if a["centrals"] else None
    bufs = buffers(3, 128, 50)
    rc = call(lib, rows if a["rows"] else None, a["n_rows"], a["nb"], a["stride"], mem, off, a["k"], a["nf"], bufs, cen,
              a["c_stride"])
    assert rc == INVALID, (name, rc)
    assert message in lib.bbh_last_error().decode(), (name, lib.bbh_last_error())
    assert untouched(bufs), name


def test_device_members_are_checked(lib, torch):
    rows, off, ref = cs.small_mix()
    mem = torch.arange(int(off[-1]), dtype=torch.int64, device="cuda")
    mem[100] = len(rows)
    bufs = buffers(len(off) - 1, 128, int(off[-1]))
    rc = call(lib, rows, len(rows), 16, 16, mem, off, len(off) - 1, 128, bufs)
    assert rc == INVALID and b"not a row" in lib.bbh_last_error() and untouched(bufs)


def test_refusal_table_starts_from_a_valid_call(lib):
    rows = np.ones((50, 256), np.uint8)
    bufs = buffers(3, 128, 50)
    rc = call(lib, rows, 50, 16, 16, np.arange(50, dtype=np.int64), np.array(GOOD["offsets"], dtype=np.int64), 3, 128, bufs,
              np.ones((3, 16), np.uint8), 16)
    assert rc == 0 and not untouched({"dist": bufs["dist"][:50]}) and (bufs["sums"][:3 * 128].reshape(3, 128)[:, 7] == [10, 20, 20]).all()


# ---------------------------------------------------------------------------------------------------------------------
# bbh_dbi_worst_ratios
# ---------------------------------------------------------------------------------------------------------------------


def dbi(lib, cents, k, nb, stride, scatter, flags=True, stream=None):
    worst = np.full(max(k, 0) + PAD, SENT_F64)
    fl = np.full(2 + PAD, SENT_U32, np.uint32) if flags else None
    rc = lib.bbh_dbi_worst_ratios(at(cents), k, nb, stride, at(scatter), at(worst), at(fl), stream)
    return rc, worst, fl


def dbi_same(lib, got, ref, what=""):
    (rc, worst, fl), (want, wflags) = got, ref
    k = len(want)
    assert rc == 0, (what, rc, lib.bbh_last_error())
    assert (worst[k:] == SENT_F64).all() and (fl is None or (fl[2:] == SENT_U32).all()), (what, "written behind the end")
    bad = np.flatnonzero(R.bits(worst[:k]) != R.bits(want))
    assert bad.size == 0, (what, bad[:10], worst[bad[:5]], want[bad[:5]])
    assert fl is None or fl[:2].tolist() == wflags.tolist(), (what, fl[:2], wflags)


@pytest.mark.parametrize("nb", cs.DBI_WIDTHS)
@pytest.mark.parametrize("k", cs.DBI_KS)
def test_dbi_shapes(lib, k, nb):
    r"""1, 2 and 3 centrals, the tile and its neighbours, and several tiles (the j tiles go to more than one workgroup of a
    tile i as soon as there are two), at one word's part, 64 and 65 words and two turns of the word loop."""
    cents, scatter = cs.dbi_case(k, nb)
    ref = cs.ref_worst_ratios(cents, scatter)
    assert k == 1 or (ref[0] > 0).all()
    dbi_same(lib, dbi(lib, cents, k, nb, nb, scatter), ref, (k, nb))


def test_dbi_identical_and_zero_centrals(lib):
    r"""Identical centrals with scatter: inf and flags[0]; without: the pair is skipped and flags[1] counts it; all-zero
    centrals are at distance 1.  The pairs sit in one tile and across tiles; without out_flags the values are the same."""
    k = cs.DBI_TILE + 9
    cents, scatter = cs.dbi_case(k, 32, seed=1)
    cents[k - 2] = cents[3]
    cents[k - 1] = cents[5] = cents[6]
    scatter[[5, 6, k - 1]] = 0.0
    cents[10] = cents[11] = 0
    ref = cs.ref_worst_ratios(cents, scatter)
    assert ref[1].tolist() == [2, 6] and np.isinf(ref[0][[3, k - 2]]).all() and np.isfinite(ref[0][[5, 6, 10, 11]]).all()
    dbi_same(lib, dbi(lib, cents, k, 32, 32, scatter), ref, "flags")
    dbi_same(lib, dbi(lib, cents, k, 32, 32, scatter, flags=False), ref, "no flags")
    zeros = np.zeros((3, 8), np.uint8)
    sc = np.array([0.25, 0.5, 0.0])
    ref = cs.ref_worst_ratios(zeros, sc)
    assert ref[0].tolist() == [0.75, 0.75, 0.5]
    dbi_same(lib, dbi(lib, zeros, 3, 8, 8, sc), ref, "zeros")
    pair = np.full((2, 8), 0x5A, np.uint8)
    dbi_same(lib, dbi(lib, pair, 2, 8, 8, np.zeros(2)), (np.zeros(2), np.array([0, 2], np.uint32)), "0 / 0 alone")


@pytest.mark.parametrize("shift", [1, 4])
def test_dbi_strided_misaligned_device_centrals(lib, torch, shift):
    k, nb, stride = cs.DBI_TILE + 3, 37, 41
    cents, scatter = cs.dbi_case(k, nb)
    ref = cs.ref_worst_ratios(cents, scatter)
    table = torch.full((k * stride + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    assert table.data_ptr() % 16 == 0
    table[shift:shift + k * stride].reshape(k, stride)[:, :nb] = torch.from_numpy(cents).cuda()
    sc = torch.from_numpy(scatter).cuda()
    dbi_same(lib, dbi(lib, table.data_ptr() + shift, k, nb, stride, sc), ref, shift)
    torch.cuda.synchronize()


def test_dbi_refusals(lib):
    cents, scatter = cs.dbi_case(4, 8)
    for args in [(None, 4, 8, 8, scatter), (cents, 0, 8, 8, scatter), (cents, 4, 8, 7, scatter), (cents, 4, 0, 8, scatter),
                 (cents, 4, 8, 8, None)]:
        rc, worst, fl = dbi(lib, *args)
        assert rc == INVALID and (worst == SENT_F64).all() and (fl == SENT_U32).all(), args[1:4]
    assert lib.bbh_dbi_worst_ratios(at(cents), 4, 8, 8, at(scatter), None, None, None) == INVALID

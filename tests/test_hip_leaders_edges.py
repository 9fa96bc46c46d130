r"""Edge cases of the leader-clustering kernels (bblean_amd/csrc/bb_leaders.hip) through the raw C ABI, `bbh_jt_leaders`:
every case of tests/leaders_refs.py (the families of components_refs.py, block models at the wave, tile and range edges,
the monotone path, the late better centre, a member next to a lower-priority centre, the flips, zero weights, identical and
all-zero rows) x {no weights, weights} x {ties low, ties high} against leaders_refs.exact_leaders (held against the round
formulation and the defining properties by test_leaders_refs.py), each called twice; host pointers, device pointers, a side
stream, every subset of the four outputs, a table one byte off its alignment, every width, the refusals, and the paths:
BBHIP_LEADERS_ROUNDS at 0, 1, 2 and unset give identical outputs and the profile records show which path ran.  Every
comparison is == on integers; every output buffer is a few elements longer than the call may write and pre-filled with
sentinels.

Left untested: the cap of 65 535 table ranges and row counts near 2^31 (the argument check of n = 2^31 is here)."""
from __future__ import annotations

import ctypes
import itertools
import os

import numpy as np
import pytest

import components_refs as C
import leaders_refs as L

pytestmark = pytest.mark.gpu

PAD = 7
SENT32 = -7
SENT64 = -0x0123456789ABCDEF
INVALID = 1  # BBH_ERR_INVALID
TIES_HIGH = 1  # BBH_LEADERS_TIES_HIGH
SWITCH = "BBHIP_LEADERS_ROUNDS"

NAMES = [name for name, _, _, _ in L.all_cases()]
VARIANTS = [(weighted, ties_high) for weighted in (False, True) for ties_high in (False, True)]


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(autouse=True)
def switch_unset(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)


def at(x):
    r"""Address of a host array, a device tensor, an address or None."""
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run(lib, rows, n, nb, radius, weights=None, flags=0, centre=True, label=True, count=True, density=True, stream=None):
    r"""bbh_jt_leaders with host outputs of n + PAD sentinels -> (rc, centre | None, label | None, count | None, density | None)."""
    room = max(n, 0) + PAD
    ocen = np.full(room, SENT32, np.int32) if centre else None
    olab = np.full(room, SENT32, np.int32) if label else None
    ocnt = np.full(1 + PAD, SENT64, np.int64) if count else None
    oden = np.full(room, SENT64, np.int64) if density else None
    rc = lib.bbh_jt_leaders(at(rows), n, nb, radius, at(weights), flags, at(ocen), at(olab), at(ocnt), at(oden), stream)
    return rc, ocen, olab, ocnt, oden


def untouched(*arrays):
    sent = {np.dtype(np.int32): SENT32, np.dtype(np.int64): SENT64}
    return all((a == sent[a.dtype]).all() for a in arrays if a is not None)


def assert_leaders(lib, got, want, n, what=""):
    rc, ocen, olab, ocnt, oden = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    if ocen is not None:
        bad = np.flatnonzero(ocen[:n] != want[0])
        assert bad.size == 0 and untouched(ocen[n:]), (what, "centre", bad[:5], ocen[bad[:5]], want[0][bad[:5]])
    if olab is not None:
        bad = np.flatnonzero(olab[:n] != want[1])
        assert bad.size == 0 and untouched(olab[n:]), (what, "label", bad[:5], olab[bad[:5]], want[1][bad[:5]])
    if ocnt is not None:
        assert ocnt[0] == want[2] and untouched(ocnt[1:]), (what, "count", int(ocnt[0]), want[2])
    if oden is not None:
        bad = np.flatnonzero(oden[:n].view(np.uint64) != want[3])
        assert bad.size == 0 and untouched(oden[n:]), (what, "density", bad[:5], oden[bad[:5]], want[3][bad[:5]])


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("name", NAMES)
def test_case(lib, name):
    r"""Host pointers, all outputs, with and without weights, both tie orders, against the reference; a second call gives
    the same bytes."""
    rows, radius, w = L.case(name)
    n, nb = rows.shape
    for weighted, ties_high in VARIANTS:
        want = L.expected(name, weighted, ties_high)
        args = dict(weights=w if weighted else None, flags=TIES_HIGH if ties_high else 0)
        first = run(lib, rows, n, nb, radius, **args)
        assert_leaders(lib, first, want, n, what=(name, weighted, ties_high))
        again = run(lib, rows, n, nb, radius, **args)
        assert again[0] == 0 and same_bytes(first, again), (name, weighted, ties_high, "second call")


SUBSET_CASES = ["chain permuted 0.4", "block 0.14", "width 100 " + repr(C.width_radii(100)[1]), L.LATE]


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_every_subset_of_the_outputs(lib, name):
    rows, radius, w = L.case(name)
    n, nb = rows.shape
    want = L.expected(name, True, False)
    for centre, label, count, density in itertools.product((True, False), repeat=4):
        if not (centre or label or count or density):
            continue
        got = run(lib, rows, n, nb, radius, weights=w, centre=centre, label=label, count=count, density=density)
        assert [g is None for g in got[1:]] == [not centre, not label, not count, not density]
        assert_leaders(lib, got, want, n, what=(name, centre, label, count, density))


@pytest.mark.parametrize("name", SUBSET_CASES + ["star hub 511 " + repr(C.STAR_R), "bridge C at 256", L.MONOTONE])
def test_device_pointers_on_a_side_stream(lib, torch, name):
    r"""The rows produced on a torch side stream, the call enqueued on that stream, every operand and output in device
    memory (weights and count too), compared after synchronising that stream; device rows with host outputs on the null
    stream."""
    rows, radius, w = L.case(name)
    n, nb = rows.shape
    want = L.expected(name, True, True)
    src = torch.from_numpy(rows.copy()).cuda()
    dw = torch.from_numpy(w.view(np.int32).copy()).cuda()
    drows = torch.zeros_like(src)
    ocen = torch.full((n + PAD,), SENT32, dtype=torch.int32, device="cuda")
    olab = torch.full((n + PAD,), SENT32, dtype=torch.int32, device="cuda")
    ocnt = torch.full((1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    oden = torch.full((n + PAD,), SENT64, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        drows.copy_(src ^ 0xFF).bitwise_xor_(0xFF)
        rc = lib.bbh_jt_leaders(drows.data_ptr(), n, nb, radius, dw.data_ptr(), TIES_HIGH, ocen.data_ptr(), olab.data_ptr(),
                                ocnt.data_ptr(), oden.data_ptr(), s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    assert_leaders(lib, (0, ocen.cpu().numpy(), olab.cpu().numpy(), ocnt.cpu().numpy(), oden.cpu().numpy()), want, n, what=name)
    assert_leaders(lib, run(lib, drows, n, nb, radius, weights=dw, flags=TIES_HIGH), want, n, what=(name, "device rows, host outputs"))
    assert_leaders(lib, run(lib, drows, n, nb, radius, weights=w, flags=TIES_HIGH), want, n, what=(name, "device rows, host weights"))


@pytest.mark.parametrize("name", ["chain permuted 0.4", "block 0.14", "bridge C at 255", "width 8 " + repr(C.width_radii(8)[1]),
                                  "small block 257"])
def test_one_byte_off_takes_the_generic_degree_kernel(lib, torch, name):
    r"""The same table at an address one byte past a 4-aligned one: the degree pass runs k_ld_pairs_generic (the division)
    instead of k_ld_pairs (the table), identical bytes."""
    rows, radius, w = L.case(name)
    n, nb = rows.shape
    assert nb in C.FAST_WIDTHS
    want = L.expected(name, True, False)
    flat = torch.zeros(n * nb + 8, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    flat[1:1 + n * nb] = torch.from_numpy(rows.copy()).cuda().reshape(-1)
    aligned = run(lib, torch.from_numpy(rows.copy()).cuda(), n, nb, radius, weights=w)
    off = run(lib, flat.data_ptr() + 1, n, nb, radius, weights=w)
    assert_leaders(lib, aligned, want, n, what=(name, "aligned"))
    assert_leaders(lib, off, want, n, what=(name, "one byte off"))
    assert same_bytes(aligned, off)


def test_every_width_is_here():
    r"""(test_case walks them: the six instantiated widths, narrower ones that are padded, and wave-per-row widths)"""
    for nb in (1, 3, 8, 16, 24, 32, 64, 100, 128, 256, 257, 1024, 8192):
        assert sum(name.startswith(f"width {nb} ") for name in NAMES) >= 2


def test_no_rows(lib):
    r"""n == 0: BBH_OK, the count 0 and nothing else written; without a count output nothing at all."""
    rows = np.ones((4, 16), np.uint8)
    rc, ocen, olab, ocnt, oden = run(lib, rows, 0, 16, 0.5)
    assert rc == 0 and ocnt[0] == 0 and untouched(ocnt[1:], ocen, olab, oden)
    rc, ocen, olab, ocnt, oden = run(lib, rows, 0, 16, 0.5, count=False)
    assert rc == 0 and untouched(ocen, olab, oden)


# (n, nbytes, radius, flags, rows, outputs)
REFUSED = {
    "NaN radius": (4, 16, float("nan"), 0, True, True),
    "n < 0": (-1, 16, 0.5, 0, True, True),
    "n = 2^31": (1 << 31, 16, 0.5, 0, True, True),
    "nbytes = 0": (4, 0, 0.5, 0, True, True),
    "nbytes < 0": (4, -16, 0.5, 0, True, True),
    "no rows": (4, 16, 0.5, 0, False, True),
    "all outputs NULL": (4, 16, 0.5, 0, True, False),
    "flag bit 1": (4, 16, 0.5, 2, True, True),
    "flag bit 31": (4, 16, 0.5, 1 | (1 << 31), True, True),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID before anything is launched, every output untouched."""
    n, nb, radius, flags, with_rows, outputs = REFUSED[name]
    rows = np.ones((4, 16), np.uint8)
    ocen, olab = np.full(4 + PAD, SENT32, np.int32), np.full(4 + PAD, SENT32, np.int32)
    ocnt, oden = np.full(1 + PAD, SENT64, np.int64), np.full(4 + PAD, SENT64, np.int64)
    args = (at(ocen), at(olab), at(ocnt), at(oden)) if outputs else (None, None, None, None)
    assert lib.bbh_jt_leaders(at(rows) if with_rows else None, n, nb, radius, None, flags, *args, None) == INVALID, name
    assert untouched(ocen, olab, ocnt, oden) and lib.bbh_last_error(), name


def records(lib, name):
    launches, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
    assert lib.bbh_profile_get(name.encode(), ctypes.byref(launches), ctypes.byref(ms)) == 0
    return int(launches.value)


def units(lib, name):
    u = ctypes.c_int64(0)
    assert lib.bbh_profile_units(name.encode(), ctypes.byref(u)) == 0
    return int(u.value)


def profiled(lib, name, weighted, ties_high):
    r"""One call with the profile on -> (outputs, records of rounds, records of the tail)."""
    rows, radius, w = L.case(name)
    n, nb = rows.shape
    assert lib.bbh_profile_enable(1) == 0 and lib.bbh_profile_reset() == 0
    try:
        got = run(lib, rows, n, nb, radius, weights=w if weighted else None, flags=TIES_HIGH if ties_high else 0)
        out = got, records(lib, "jt_leaders/round"), records(lib, "jt_leaders/step")
        assert records(lib, "jt_leaders/degree") == 1 and records(lib, "jt_leaders/assign") == 1
        assert records(lib, "jt_leaders") == 2 + out[1] + out[2]
    finally:
        lib.bbh_profile_reset()
        lib.bbh_profile_enable(0)
    return out


# (case, weighted, ties high): each needs more than two rounds, so that the tail has rows left after 0, 1 and 2 of them
PATH_CASES = [(L.MONOTONE, False, False), ("block 0.13", True, True), (L.LATE, False, False)]


@pytest.mark.parametrize("name,weighted,ties_high", PATH_CASES)
def test_the_switch_changes_the_path_and_nothing_else(lib, monkeypatch, name, weighted, ties_high):
    r"""BBHIP_LEADERS_ROUNDS = k: k rounds, then the tail over exactly the rows the round formulation of leaders_refs has
    left; the outputs are those of the built-in rule, byte for byte."""
    rows, radius, w = L.case(name)
    n = len(rows)
    want = L.expected(name, weighted, ties_high)
    monkeypatch.delenv(SWITCH, raising=False)
    unset, _, _ = profiled(lib, name, weighted, ties_high)
    assert_leaders(lib, unset, want, n, what=(name, "unset"))
    for k in (0, 1, 2):
        trace = {}
        L.leaders_by_rounds(rows, radius, w if weighted else None, ties_high, cap=k, trace=trace)
        monkeypatch.setenv(SWITCH, str(k))
        assert lib.bbh_profile_enable(1) == 0 and lib.bbh_profile_reset() == 0
        try:
            got = run(lib, rows, n, rows.shape[1], radius, weights=w if weighted else None, flags=TIES_HIGH if ties_high else 0)
            rounds, steps = records(lib, "jt_leaders/round"), records(lib, "jt_leaders/step")
            stepped = units(lib, "jt_leaders/step")
        finally:
            lib.bbh_profile_reset()
            lib.bbh_profile_enable(0)
        assert_leaders(lib, got, want, n, what=(name, k))
        assert same_bytes(got, unset), (name, k)
        assert rounds == k and steps == 1 and stepped == trace["steps"] > 0, (name, k, rounds, steps, stepped, trace["steps"])


def test_the_built_in_rule(lib):
    r"""Unset: the block model finishes in its rounds with no stepping launch, the monotone path steps."""
    for name in ("block 0.13", "block 0.14", "block 0.15"):
        _, rounds, steps = profiled(lib, name, False, False)
        assert 1 <= rounds <= 5 and steps == 0, (name, rounds, steps)
    rows, radius, _ = L.case(L.MONOTONE)
    assert lib.bbh_profile_enable(1) == 0 and lib.bbh_profile_reset() == 0
    try:
        got = run(lib, rows, len(rows), rows.shape[1], radius)
        assert_leaders(lib, got, L.expected(L.MONOTONE, False, False), len(rows))
        assert 1 <= records(lib, "jt_leaders/round") <= 4 and records(lib, "jt_leaders/step") == 1
        assert units(lib, "jt_leaders/step") > 400  # the positions stepped through
    finally:
        lib.bbh_profile_reset()
        lib.bbh_profile_enable(0)

r"""Edge cases of the connected-components kernels (bblean_amd/csrc/bb_components.hip) through the raw C ABI,
`bbh_jt_components`: every case of tests/components_refs.py (chains in three orders, stars, bridges, a block model, radii on,
just below and just above realised distances at both kernels, degenerate tables and radii, every width) against
components_refs.exact_components (held against scipy by test_components_refs.py), each called twice; host pointers, device
pointers, a side stream, every subset of the outputs, the generic kernel on a table one byte off, and the refusals.  Every
comparison is == on integers; every output buffer is a few elements longer than the call may write and pre-filled with
sentinels.

Left untested: the cap of 65 535 table ranges and row counts near 2^31 (the argument check of n = 2^31 is here)."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import components_refs as C

pytestmark = pytest.mark.gpu

PAD = 7
SENT32 = -7
SENT64 = -0x0123456789ABCDEF
INVALID = 1  # BBH_ERR_INVALID

CASES = {name: (rows, r) for name, rows, r in C.all_cases()}


@pytest.fixture(scope="module")
def lib():
    from bblean_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def at(x):
    r"""Address of a host array, a device tensor, an address or None."""
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def run(lib, rows, n, nb, radius, root=True, label=True, count=True, stream=None):
    r"""bbh_jt_components with host outputs of n + PAD sentinels -> (rc, root | None, label | None, count | None)."""
    room = max(n, 0) + PAD
    oroot = np.full(room, SENT32, np.int32) if root else None
    olab = np.full(room, SENT32, np.int32) if label else None
    ocnt = np.full(1 + PAD, SENT64, np.int64) if count else None
    rc = lib.bbh_jt_components(at(rows), n, nb, radius, at(oroot), at(olab), at(ocnt), stream)
    return rc, oroot, olab, ocnt


def untouched(*arrays):
    sent = {np.dtype(np.int32): SENT32, np.dtype(np.int64): SENT64}
    return all((a == sent[a.dtype]).all() for a in arrays if a is not None)


def assert_components(lib, got, want, n, what=""):
    rc, oroot, olab, ocnt = got
    assert rc == 0, (what, rc, lib.bbh_last_error())
    if oroot is not None:
        bad = np.flatnonzero(oroot[:n] != want[0])
        assert bad.size == 0 and untouched(oroot[n:]), (what, "root", bad[:5], oroot[bad[:5]], want[0][bad[:5]])
    if olab is not None:
        bad = np.flatnonzero(olab[:n] != want[1])
        assert bad.size == 0 and untouched(olab[n:]), (what, "label", bad[:5], olab[bad[:5]], want[1][bad[:5]])
    if ocnt is not None:
        assert ocnt[0] == want[2] and untouched(ocnt[1:]), (what, "count", int(ocnt[0]), want[2])


@pytest.mark.parametrize("name", list(CASES))
def test_case(lib, name):
    r"""Host pointers, all outputs, against the reference; a second call gives the same bytes."""
    rows, radius = CASES[name]
    n, nb = rows.shape
    want = C.expected(name)
    first = run(lib, rows, n, nb, radius)
    assert_components(lib, first, want, n, what=name)
    again = run(lib, rows, n, nb, radius)
    assert again[0] == 0 and all((a == b).all() for a, b in zip(first[1:], again[1:])), (name, "second call")


SUBSET_CASES = ["chain permuted 0.4", "block 0.14", "width 100 " + repr(C.width_radii(100)[1])]


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_every_subset_of_the_outputs(lib, name):
    rows, radius = CASES[name]
    n, nb = rows.shape
    want = C.expected(name)
    for root, label, count in itertools.product((True, False), repeat=3):
        if not (root or label or count):
            continue
        got = run(lib, rows, n, nb, radius, root=root, label=label, count=count)
        assert (got[1] is None) == (not root) and (got[2] is None) == (not label) and (got[3] is None) == (not count)
        assert_components(lib, got, want, n, what=(name, root, label, count))


@pytest.mark.parametrize("name", SUBSET_CASES + ["star hub 511 " + repr(C.STAR_R), "bridge C at 256"])
def test_device_pointers_on_a_side_stream(lib, torch, name):
    r"""The rows produced on a torch side stream, the call enqueued on that stream, every operand and output in device
    memory (the count too), compared after synchronising that stream; device rows with host outputs on the null stream."""
    rows, radius = CASES[name]
    n, nb = rows.shape
    want = C.expected(name)
    src = torch.from_numpy(rows).cuda()
    drows = torch.zeros_like(src)
    oroot = torch.full((n + PAD,), SENT32, dtype=torch.int32, device="cuda")
    olab = torch.full((n + PAD,), SENT32, dtype=torch.int32, device="cuda")
    ocnt = torch.full((1 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        drows.copy_(src ^ 0xFF).bitwise_xor_(0xFF)
        rc = lib.bbh_jt_components(drows.data_ptr(), n, nb, radius, oroot.data_ptr(), olab.data_ptr(), ocnt.data_ptr(),
                                   s.cuda_stream)
        assert rc == 0, lib.bbh_last_error()
    s.synchronize()
    assert_components(lib, (0, oroot.cpu().numpy(), olab.cpu().numpy(), ocnt.cpu().numpy()), want, n, what=name)
    assert_components(lib, run(lib, drows, n, nb, radius), want, n, what=(name, "device rows, host outputs"))


@pytest.mark.parametrize("name", ["chain permuted 0.4", "block 0.14", "bridge C at 255", "width 8 " + repr(C.width_radii(8)[1])])
def test_one_byte_off_takes_the_generic_kernel(lib, torch, name):
    r"""The same table at an address one byte past a 4-aligned one: k_cc_pairs_generic (the division) instead of k_cc_pairs
    (the table), identical bytes."""
    rows, radius = CASES[name]
    n, nb = rows.shape
    assert nb in C.FAST_WIDTHS
    want = C.expected(name)
    flat = torch.zeros(n * nb + 8, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 4 == 0
    flat[1:1 + n * nb] = torch.from_numpy(rows).cuda().reshape(-1)
    aligned = run(lib, torch.from_numpy(rows).cuda(), n, nb, radius)
    off = run(lib, flat.data_ptr() + 1, n, nb, radius)
    assert_components(lib, aligned, want, n, what=(name, "aligned"))
    assert_components(lib, off, want, n, what=(name, "one byte off"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(aligned[1:], off[1:]))


def test_no_rows(lib):
    r"""n == 0: BBH_OK, the count 0 and nothing else written; without a count output nothing at all."""
    rows = np.ones((4, 16), np.uint8)
    rc, oroot, olab, ocnt = run(lib, rows, 0, 16, 0.5)
    assert rc == 0 and ocnt[0] == 0 and untouched(ocnt[1:], oroot, olab)
    rc, oroot, olab, ocnt = run(lib, rows, 0, 16, 0.5, count=False)
    assert rc == 0 and untouched(oroot, olab)


# (n, nbytes, radius, outputs)
REFUSED = {
    "NaN radius": (4, 16, float("nan"), True),
    "n < 0": (-1, 16, 0.5, True),
    "n = 2^31": (1 << 31, 16, 0.5, True),
    "nbytes = 0": (4, 0, 0.5, True),
    "nbytes < 0": (4, -16, 0.5, True),
    "all outputs NULL": (4, 16, 0.5, False),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals(lib, name):
    r"""Argument checks: BBH_ERR_INVALID before anything is launched, every output untouched."""
    n, nb, radius, outputs = REFUSED[name]
    rows = np.ones((4, 16), np.uint8)
    oroot, olab = np.full(4 + PAD, SENT32, np.int32), np.full(4 + PAD, SENT32, np.int32)
    ocnt = np.full(1 + PAD, SENT64, np.int64)
    args = (at(oroot), at(olab), at(ocnt)) if outputs else (None, None, None)
    assert lib.bbh_jt_components(at(rows), n, nb, radius, *args, None) == INVALID, name
    assert untouched(oroot, olab, ocnt) and lib.bbh_last_error(), name

r"""CPU: the dword-level helpers of the pipelined kernel's packed merge path (bblean_amd/csrc/bb_pipe_bytes.h).

The leaf engine takes the majority vote of a merged BitFeature four uint8 sums at a time, gathers the flags into the centroid's
bit order with one multiply, and spreads the element's bits to 0 / 1 bytes with another.  The header is plain integer code:
tests/pipe_bytes_main.cpp includes it and is built here for the host, then walks

- the 4-byte vote over every pair of neighbouring byte values x every threshold 1 .. 128 (a borrow between bytes would show),
- the expansion and the gather over all 2^8 nibble pairs,
- the composed dword against `centroid_dword31` (the kernel's former loop, one `alignbit` per feature) on random counters."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
_CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

CHECKS = ["vote4_exhaustive", "expand_all_nibble_pairs", "gather_all_nibble_pairs", "dword_against_centroid_dword31"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if _CXX is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("pipe_bytes") / "pipe_bytes_main"
    built = subprocess.run([_CXX, "-std=c++17", "-O2", "-Wall", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                            str(HERE / "pipe_bytes_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)


def test_all_checks_ran(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr.strip() == "", report.stderr
    assert sorted(ln.split()[1] for ln in report.stdout.splitlines()) == sorted(CHECKS), report.stdout


@pytest.mark.parametrize("name", CHECKS)
def test_pipe_bytes(report, name):
    lines = [ln for ln in report.stdout.splitlines() if ln.split()[1:2] == [name]]
    assert lines == [f"PASS {name}"], report.stdout + report.stderr

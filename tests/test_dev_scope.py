r"""CPU: `bb::DevScope` (bblean_amd/csrc/bb_common.h), the owner of one call's device and pinned blocks.

Its job is the exit paths that need a failing HIP call - an allocation that fails halfway, a stream that reports an error -
so it is tested where those can be made to happen: tests/dev_scope_main.cpp includes the header, fakes the six symbols the
scope uses (blocks from malloc, a log of the calls, switches that make the n-th allocation or the synchronisation fail) and
is built here without the HIP runtime, under the address and undefined-behaviour sanitizers: with g++, and with the clang++
of the ROCm installation where there is one - the library is compiled by clang, and the two order the evaluation of a call's
arguments differently."""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
_GXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
_ROCM_CLANG = ROCM / "llvm" / "bin" / "clang++"
COMPILERS = ([_GXX] if _GXX else []) + ([str(_ROCM_CLANG)] if _ROCM_CLANG.exists() else [])

CHECKS = [
    "alloc_1_fails", "alloc_2_fails", "alloc_3_fails", "alloc_4_fails",  # BBH_ERR_HIP, nothing live afterwards
    "early_return_syncs_before_free",          # a get, no sync(): one synchronise, then the free
    "sync_then_frees_only",                    # after sync(): frees only; pinned -> hipHostFree, device -> dev_free
    "get_after_sync_syncs_again",
    "failing_sync_in_destructor_still_frees",
    "sync_reports_stream_error",               # BBH_ERR_HIP, and the blocks still go
    "empty_scope_calls_nothing",
    "sync_without_blocks",
]


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: Path(c).name if c else "none")
def report(request, tmp_path_factory):
    if request.param is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("dev_scope") / "dev_scope_main"
    cmd = [request.param, "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM / 'include'}", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", "-O1", str(HERE / "dev_scope_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def test_sanitizers_report_nothing(report):
    assert report.returncode == 0, report.stdout + report.stderr
    assert report.stderr.strip() == "", report.stderr  # (ASan / UBSan write to stderr; leaks are reported at exit)
    assert sorted(ln.split()[1] for ln in report.stdout.splitlines()) == sorted(CHECKS), report.stdout


@pytest.mark.parametrize("name", CHECKS)
def test_dev_scope(report, name):
    lines = [ln for ln in report.stdout.splitlines() if ln.split()[1:2] == [name]]
    assert lines == [f"PASS {name}"], report.stdout + report.stderr

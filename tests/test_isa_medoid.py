r"""Compile-time guards on the segmented complementary-iSIM kernels (no GPU needed: hipcc cross-compiles gfx950), the
ones tests/test_isa_assign.py applies to the assignment kernels: bb_medoid.hip's device code is compiled to assembly with
the Makefile's flags; every kernel must have a private segment of zero bytes, no scratch instruction and no call; the
row kernels count bits with v_bcnt_u32_b32; the small-set kernel leaves room for two workgroups per compute unit."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "bblean_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_medoid_kernels_isa(tmp_path):
    out = tmp_path / "bb_medoid.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function",
           "--cuda-device-only", "-S", str(CSRC / "bb_medoid.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    assert "bb_medoid.hip" in (CSRC / "Makefile").read_text()

    def body_of(name):
        start = text.index(name + ":")
        return text[start:text.index(".Lfunc_end", start)]

    def lds_of(name):
        m = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)
        assert m is not None, name
        return int(m.group(1))

    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    assert len(kernels) >= 8, kernels
    assert all("k_seg_" in k for k in kernels), kernels
    for name in kernels:
        body = body_of(name)
        scratch = [ln.strip() for ln in body.splitlines() if ln.strip().startswith(("scratch_", "buffer_load", "buffer_store"))]
        assert not scratch, (name, scratch[:5])
        m = re.search(r"\.set " + re.escape(name) + r"\.private_seg_size, (\d+)", text)
        assert m is not None and int(m.group(1)) == 0, (name, m.group(0) if m else None)
        assert "s_swappc_b64" not in body, name
        assert lds_of(name) <= 80 * 1024, name

    small = [k for k in kernels if "k_seg_small" in k]
    rows = [k for k in kernels if "k_seg_rows" in k]
    assert len(small) == 2 and len(rows) >= 3, (small, rows)
    for name in small + rows:
        assert "v_bcnt_u32_b32" in body_of(name), name
    for name in small:  # two workgroups share a compute unit's 160 KiB
        assert lds_of(name) <= 80 * 1024, name

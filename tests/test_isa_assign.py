r"""Compile-time guards on the assignment kernels (no GPU needed: hipcc cross-compiles gfx950), the ones
tests/test_isa_guards.py applies to the tree kernels: bb_assign.hip's device code is compiled to assembly with the
Makefile's flags; the matrix-core kernel must contain int8 MFMAs, no scratch instruction, a private segment of zero
bytes and no call."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "bblean_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_assign_kernels_isa(tmp_path):
    out = tmp_path / "bb_assign.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function",
           "--cuda-device-only", "-S", str(CSRC / "bb_assign.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()

    def body_of(name):
        start = text.index(name + ":")
        return text[start:text.index(".Lfunc_end", start)]

    def guards(name):
        body = body_of(name)
        scratch = [ln.strip() for ln in body.splitlines() if ln.strip().startswith(("scratch_", "buffer_load", "buffer_store"))]
        assert not scratch, (name, scratch[:5])
        m = re.search(r"\.set " + re.escape(name) + r"\.private_seg_size, (\d+)", text)
        assert m is not None and int(m.group(1)) == 0, (name, m.group(0) if m else None)
        assert "s_swappc_b64" not in body, name
        return body

    mfma = re.findall(r"^(_ZN\S*k_assign_mfma\S*):", text, re.M)
    assert len(mfma) == 1, mfma
    body = guards(mfma[0])
    ops = re.findall(r"\bv_mfma_i32_\w+_i8\b", body)
    assert len(ops) >= 64 and set(ops) == {"v_mfma_i32_16x16x64_i8"}, sorted(set(ops))
    # operands come from LDS in 16-byte reads, the expansion goes there in 16-byte writes
    assert "ds_read_b128" in body and "ds_write_b128" in body
    m = re.search(r"\.amdhsa_kernel " + re.escape(mfma[0]) + r"\n(?:.*\n)*?\s*\.amdhsa_group_segment_fixed_size (\d+)", text)
    assert m is not None and int(m.group(1)) <= 80 * 1024, m  # two workgroups fit a CU's 160 KiB of LDS
    others = re.findall(r"^(_ZN\S*(?:k_assign_bcnt|k_assign_generic|k_assign_combine|k_jaccard_dist)\S*):", text, re.M)
    assert len(others) >= 15, others
    for name in others:
        guards(name)

"""Guards on the SHIPPED device code (the in-tree libc2m_hip.so, disassembled): hardware lessons that a source edit can
silently undo.  No GPU needed; skipped when the ROCm llvm-objdump is not installed."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "c2-matching_amd", "csrc", "libc2m_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    if not os.path.exists(OBJDUMP):
        pytest.skip("ROCm llvm-objdump not installed")
    if not os.path.exists(LIB):
        pytest.fail("libc2m_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    d = tmp_path_factory.mktemp("bundles")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
    objs = sorted(f for f in os.listdir(d) if "amdgcn-amd-amdhsa--gfx950" in f)
    assert objs, "no gfx950 code objects in the library"
    text = []
    for f in objs:
        out = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", f], cwd=d, check=True, capture_output=True, text=True).stdout
        text.append(out)
    return "\n".join(text)


def test_library_is_gfx950_only_and_has_matrix_kernels(disassembly):
    assert "v_mfma_f32_32x32x16_f16" in disassembly and "v_mfma_f32_32x32x2_f32" in disassembly


def test_no_128_bit_buffer_store_with_a_register_soffset(disassembly):
    """gfx950: `buffer_store_dwordx4 v[a:a+3], voff, s[..], sN offen` followed within two issue slots by a VALU write of
    v[a:a+3] stores the NEW value in lanes 12..15 / 28..31 of each half -- hipcc pads that hazard only for the immediate-
    soffset form (found twice: DESIGN.md 6.2 (round 4), 6.9 (round 5)).  The library keeps every wide buffer store on the
    immediate / zero soffset form; this test fails if an edit re-introduces the register form."""
    pat = re.compile(r"buffer_store_dwordx[34]\s+v\[\d+:\d+\],\s*\S+,\s*s\[\d+:\d+\],\s*(\S+)")
    wide = [m.group(1) for m in pat.finditer(disassembly)]
    assert len(wide) > 100        # the channels-last epilogues are there
    reg = [s for s in wide if re.fullmatch(r"(s\d+|m0|vcc_lo|vcc_hi|ttmp\d+)", s)]
    assert not reg, f"{len(reg)} wide buffer stores with a register soffset: {sorted(set(reg))[:8]}"


def test_no_measurement_scaffolding_in_the_shipped_library(tmp_path):
    """The timing-only ablation variants and A/B knobs of rounds 3 to 6 are gone (their numbers live on in DESIGN.md and profiles/):
    the library names none of their switches, and its code object holds the 38 product instantiations of conv3x3_split_kernel
    -- 3 flavours x 2 cout widths x 6 output modes + 2 bf16-source kernels -- and nothing else of that name."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("ROCm llvm-objdump not installed")
    if not os.path.exists(LIB):
        pytest.fail("libc2m_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    for name in (b"C2M_SPLIT_ABL", b"C2M_CONV_ABL", b"C2M_CORR_PF", b"C2M_SPLIT_TRACE", b"C2M_DCN_BWD_GROUPED",
                 b"C2M_CORR_DEDUP", b"C2M_CORR_DEAD_TILES"):
        assert name not in blob, f"{name.decode()} is back in libc2m_hip.so"
    shutil.copy(LIB, tmp_path / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    objs = sorted(f for f in os.listdir(tmp_path) if "amdgcn-amd-amdhsa--gfx950" in f)
    assert objs, "no gfx950 code objects in the library"
    kernels = set()
    for f in objs:
        out = subprocess.run([OBJDUMP, "-t", f], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            cols = line.split()
            if len(cols) >= 4 and "F" in cols[1:-1] and ".text" in line and "conv3x3_split_kernel" in cols[-1]:
                kernels.add(cols[-1])
    assert len(kernels) == 38, f"{len(kernels)} conv3x3_split_kernel functions in the code object: {sorted(kernels)}"

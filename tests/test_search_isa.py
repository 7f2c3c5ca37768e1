"""CPU-only check of the gfx950 code of csrc/search.hip, compiled with the Makefile's flags: every kernel keeps its registers (no scratch, no spilled
VGPRs), every instantiation of the score kernel forms its product on the fp32-input 32x32x2 MFMA, and its register count fits the occupancy DESIGN.md
states for it (one 256-thread block per CU = one wave per SIMD: the whole 512-entry file)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechclip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def search_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "search.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "search.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*(?:search|topk_merge)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    return text, kernels


def test_every_instantiation_is_there(search_asm):
    _, kernels = search_asm
    assert sum("search_kernel" in k for k in kernels) == 4, sorted(kernels)        # (query tiles per wave, list capacity) = (1, 16) (1, 128) (2, 16) (2, 64)
    assert sum("topk_merge_kernel" in k for k in kernels) == 1
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(search_asm):
    text, kernels = search_asm
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) >= len(kernels) and all(int(v) == 0 for v in spills)
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))


def test_scores_run_on_the_fp32_input_mfma_within_one_wave_per_simd(search_asm):
    text, kernels = search_asm
    for name, body in kernels.items():
        if "search_kernel" in name:
            assert "v_mfma_f32_32x32x2_f32" in body or "v_mfma_f32_16x16x4_f32" in body, name
    counts = re.findall(r"\.name:\s+(\S*search_kernel\S*).*?\.vgpr_count:\s+(\d+)", text, re.S)
    assert len(counts) == 4
    for name, n in counts:
        assert int(n) <= 512, (name, n)

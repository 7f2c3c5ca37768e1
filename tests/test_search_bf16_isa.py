"""CPU-only check of the gfx950 code of csrc/search_bf16.hip, compiled with the Makefile's flags: every instantiation of the bf16 score kernel is there,
keeps its registers (no scratch, no spilled VGPRs), forms its product on the bf16-input 32x32x16 MFMA and reads its fragments 16 bytes at a time, and its
register count fits the occupancy DESIGN.md states for it (one 256-thread block per CU = one wave per SIMD: the whole 512-entry file)."""
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
    out = tmp_path_factory.mktemp("isa") / "search_bf16.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "search_bf16.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*search_bf16_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    return text, kernels


def test_every_instantiation_is_there_and_nothing_else(search_asm):
    text, kernels = search_asm
    assert len(kernels) == 4, sorted(kernels)                  # (query tiles per wave, list capacity) = (1, 16) (1, 128) (2, 16) (2, 64), as search.hip
    for wq, kl in ((1, 16), (1, 128), (2, 16), (2, 64)):
        assert any(f"search_bf16_kernelILi{wq}ELi{kl}EE" in k for k in kernels), (wq, kl)
    assert len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 4      # the merge kernel is search.hip's: no second copy here
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(search_asm):
    text, kernels = search_asm
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) == len(kernels) and all(int(v) == 0 for v in spills)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(sizes) == len(kernels) and all(int(v) == 0 for v in sizes)
    for body in kernels.values():
        assert "scratch_" not in body


def test_scores_run_on_the_bf16_mfma_within_one_wave_per_simd(search_asm):
    text, kernels = search_asm
    for name, body in kernels.items():
        assert "v_mfma_f32_32x32x16_bf16" in body, name
        assert not re.search(r"v_mfma_f32_\w+_f32\b", body), name              # no fp32-input product left in
        assert "ds_read_b128" in body and "ds_write_b128" in body, name        # one 16-byte read per lane and k-group, 16-byte stage stores
    counts = re.findall(r"\.name:\s+(\S*search_bf16_kernel\S*).*?\.vgpr_count:\s+(\d+)", text, re.S)
    assert len(counts) == 4
    for name, n in counts:
        assert int(n) <= 512, (name, n)
    lds = [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert len(lds) == 4 and max(lds) <= 160 * 1024

"""CPU-only check of the gfx950 code of csrc/vq_modes.hip, compiled with the Makefile's flags: every kernel keeps its registers (no scratch, no spilled
VGPRs) and every instantiation of the fused soft-embed kernel (E tile 64 .. 512, with and without noise) forms its product on the bf16 16x16x32 MFMA."""
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
def vq_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "vq_modes.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "vq_modes.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*vq_\w+_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    return text, kernels


def test_every_instantiation_is_there(vq_asm):
    _, kernels = vq_asm
    assert sum("vq_soft_embed_kernel" in k for k in kernels) == 12, sorted(kernels)          # E tile / 64 in {1, 2, 3, 4, 6, 8} x noise
    for kind, n in (("gumbel_noise", 1), ("noisy_argmax", 2), ("row_stats", 2), ("probs", 2), ("mode_bwd", 2), ("soft_table", 1), ("soft_finish", 1)):
        assert sum(f"vq_{kind}_kernel" in k for k in kernels) == n, kind
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(vq_asm):
    text, kernels = vq_asm
    for name, body in kernels.items():
        assert "scratch_" not in body, name
    assert not re.search(r"ScratchSize:\s*[1-9]", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) >= len(kernels) and all(int(v) == 0 for v in spills)
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))


def test_soft_embed_runs_on_the_bf16_16x16x32_mfma_with_two_waves_per_simd(vq_asm):
    text, kernels = vq_asm
    for name, body in kernels.items():
        if "vq_soft_embed_kernel" in name:
            assert "v_mfma_f32_16x16x32_bf16" in body, name
    # 512 threads per block = two waves per SIMD: each must fit half of the 512-entry register file
    for m in re.finditer(r"\.name:\s+(\S*vq_soft_embed_kernel\S*).*?\.vgpr_count:\s+(\d+)", text, re.S):
        assert int(m.group(2)) <= 256, (m.group(1), m.group(2))

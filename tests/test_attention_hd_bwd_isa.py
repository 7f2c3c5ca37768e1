"""CPU-only check of the gfx950 code of csrc/attention_hd_bwd.hip, compiled with the Makefile's flags: every kernel instantiation (head_dim 64 / 96 / 128;
statistics, dK / dV and dQ sweeps, each with and without dropout) keeps its registers (no scratch, no spilled VGPRs) and recomputes S / dP on the bf16
16x16x32 MFMA."""
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
def bwd_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "attention_hd_bwd.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "attention_hd_bwd.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*attn_hd_bwd_(?:stats|dq|dkv)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)              # the whole body up to the function's end label: a kernel with early returns ends more than once
    return text, kernels


def test_every_instantiation_is_there(bwd_asm):
    _, kernels = bwd_asm
    assert len(kernels) == 18, sorted(kernels)              # head_dim {64, 96, 128} x {stats, dkv, dq} x dropout
    for kind in ("stats", "dkv", "dq"):
        assert sum(f"attn_hd_bwd_{kind}_kernel" in k for k in kernels) == 6, kind
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(bwd_asm):
    text, kernels = bwd_asm
    for name, body in kernels.items():
        assert "scratch_" not in body, name
    assert not re.search(r"ScratchSize:\s*[1-9]", text)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) >= len(kernels) and all(int(v) == 0 for v in spills)
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))


def test_scores_are_recomputed_on_the_bf16_16x16x32_mfma(bwd_asm):
    _, kernels = bwd_asm
    for name, body in kernels.items():
        assert "v_mfma_f32_16x16x32_bf16" in body, name

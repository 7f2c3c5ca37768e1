"""CPU-only check of the gfx950 code of csrc/search_rescore.hip, compiled with the Makefile's flags: the kernel keeps its registers (no scratch, no spilled
VGPRs), its score loop is a fused multiply-add with no separate multiply or add of floats anywhere in the kernel, subnormals are kept, and the gather
runs on 16-byte loads through LDS."""
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
    assert not re.search(r"^EXTRA_search_rescore\s*=", text, re.M)            # no flags of its own: in particular no fast-math
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def rescore_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "search_rescore.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    assert not any("fast" in f for f in flags)
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "search_rescore.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w*search_rescore_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)}
    return text, kernels


def test_one_kernel_no_scratch_and_no_spilled_registers(rescore_asm):
    text, kernels = rescore_asm
    assert len(kernels) == 1 and all("s_endpgm" in body for body in kernels.values())
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)
    assert len(spills) == 1 and int(spills[0]) == 0
    assert [int(v) for v in re.findall(r"\.sgpr_spill_count:\s+(\d+)", text)] == [0]
    assert [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)] == [0]
    assert "scratch_" not in next(iter(kernels.values()))
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= 256     # two blocks' waves per SIMD


def test_the_score_loop_is_a_fused_multiply_add_and_keeps_subnormals(rescore_asm):
    text, kernels = rescore_asm
    body = next(iter(kernels.values()))
    fused = len(re.findall(r"\bv_(?:fmac|fma)_f32(?:_e32|_e64)?\b", body))
    assert fused >= 64 + 4                                                    # a whole 64-element stage unrolled + the tail loop's unit of four
    for op in ("v_mul_f32", "v_add_f32", "v_mac_f32", "v_mad_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_mfma"):
        assert op not in body, op                                             # nothing that rounds a product apart from its sum, nothing that pairs two chains
    assert re.search(r"\.amdhsa_float_denorm_mode_32\s+3\b", text)            # fp32 subnormals: neither flushed on input nor on output


def test_the_gather_is_sixteen_byte_loads_staged_through_lds_without_atomics(rescore_asm):
    _, kernels = rescore_asm
    body = next(iter(kernels.values()))
    assert "global_load_dwordx4" in body and "ds_write_b128" in body and "ds_read_b128" in body
    assert "atomic" not in body

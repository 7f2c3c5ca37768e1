"""CPU-only checks of the fused attention backward's gfx950 code (csrc/attention_bwd.hip, the one kernel set behind sc_attention_bwd_packed and
sc_attention_hd_bwd, compiled with the Makefile's flags): every instantiation (head_dim 64 / 96 / 128; statistics, dK / dV and dQ sweeps, two forms each)
runs on v_mfma_f32_16x16x32_bf16, uses no scratch and spills nothing, contains no memory atomics (every output element has one writer: the determinism
claim), and no packed fp32 add fed by two LDS-crossbar shuffles (the construct profiles/r06_vit_layernorm_nondeterminism.txt traced run-to-run
differences to)."""
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
    assert os.path.exists(HIPCC), f"{HIPCC} not found: the ISA checks need the ROCm compiler"
    out = tmp_path_factory.mktemp("isa") / "attention_bwd.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "attention_bwd.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*attn_bwd_(?:stats|dq|dkv)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)              # the whole body up to the function's end label: a kernel with early returns ends more than once
    return text, kernels


def test_every_instantiation_is_there(bwd_asm):
    _, kernels = bwd_asm
    assert len(kernels) == 18, sorted(kernels)              # head_dim {64, 96, 128} x {stats, dkv, dq} x {delta source | dropout}
    for kind in ("stats", "dkv", "dq"):
        assert sum(f"attn_bwd_{kind}_kernel" in k for k in kernels) == 6, kind
    for body in kernels.values():
        assert "s_endpgm" in body


def test_kernels_run_on_the_mfma_without_scratch_or_spills(bwd_asm):
    text, kernels = bwd_asm
    for name, body in kernels.items():
        assert "v_mfma_f32_16x16x32_bf16" in body, name
        assert "scratch_" not in body and "buffer_store" not in body, name
        if "stats" not in name:
            assert "ds_read_b64_tr_b16" in body, name      # the transposed operands come out of the row-major LDS tiles
    assert not re.search(r"ScratchSize:\s*[1-9]", text)
    for key in ("vgpr_spill_count", "sgpr_spill_count"):
        vals = re.findall(rf"\.{key}:\s+(\d+)", text)
        assert len(vals) == len(kernels) and all(int(v) == 0 for v in vals), key
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))


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


def test_kernels_have_no_memory_atomics(bwd_asm):
    _, kernels = bwd_asm
    for name, body in kernels.items():
        assert not re.search(r"\b(global|buffer|flat|ds)_atomic_\w+|\bds_(add|pk_add)_\w+", body), name


def test_no_packed_fp32_add_fed_by_two_crossbar_shuffles(bwd_asm):
    """For every v_pk_add_f32: the last writers of its two source register pairs are not both ds_bpermute_b32.  (The row reductions of the pre-pass use
    v_permlane16_swap / v_permlane32_swap, so no ds_bpermute_b32 is expected at all.)"""
    _, kernels = bwd_asm

    def regs(tok):
        m = re.match(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.match(r"v(\d+)$", tok)
        return {int(m.group(1))} if m else set()
    for name, body in kernels.items():
        last = {}
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            op, _, rest = line.partition(" ")
            toks = [t.strip() for t in rest.split(",")]
            if op == "v_pk_add_f32" and len(toks) >= 3:
                srcs = [{last.get(r) for r in regs(t)} for t in toks[1:3]]
                assert not all(s == {"ds_bpermute_b32"} for s in srcs), (name, line)
            if toks and toks[0].startswith("v"):
                for r in regs(toks[0]):
                    last[r] = op
        assert "ds_bpermute_b32" not in body, name
        if "stats" in name:
            assert "v_permlane32_swap" in body and "v_permlane16_swap" in body, name

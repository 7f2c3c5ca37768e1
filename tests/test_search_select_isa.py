"""CPU-only check of the gfx950 code of csrc/search_select.hip, compiled with the Makefile's flags: the eight instantiations of the score kernel by subset
(the four (WQ, list capacity) pairs of the other search entries, for both operand formats) and the mask-packing kernel are there and nothing else is, every
kernel keeps its registers (no scratch, no spilled VGPRs), the fp32 kernels form their product on the fp32-input MFMA and the bf16 kernels on
v_mfma_f32_32x32x16_bf16, and registers and LDS fit one block per CU -- the live-tile walk lives in registers, and the group code per query row is the only
LDS beside what the kernels by item hold.  This file looks only for what must be present."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechclip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PAIRS = ((1, 16), (1, 128), (2, 16), (2, 64))
STAGE = {"F32Rows": 68 * 4, "Bf16Rows": 72 * 2}                               # bytes per stage row


def lds_bytes(fmt, wq, kl):
    """Declared LDS: two stage images + list and buffer (8 bytes per slot) + slot counter, skip code and group code per query row."""
    bq, cb = 64 * wq, 16 if (wq, kl) == (2, 64) else 32
    return (bq + 128) * STAGE[fmt] + bq * kl * 8 + bq * cb * 8 + bq * 12


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def select_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "search_select.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "search_select.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*(?:search_select|pack_row_mask)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), private=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return text, kernels, meta


def test_the_eight_instantiations_are_there_and_nothing_else(select_asm):
    text, kernels, meta = select_asm
    assert len(kernels) == 9 and len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 9, sorted(kernels)
    assert sum("pack_row_mask_kernel" in k for k in kernels) == 1
    for fmt in ("F32Rows", "Bf16Rows"):
        for wq, kl in PAIRS:
            assert sum(f"search_select_kernelIN11search_core{len(fmt)}{fmt}ELi{wq}ELi{kl}EE" in k for k in kernels) == 1, (fmt, wq, kl)
    assert set(meta) == set(kernels)
    assert not any("search_kernel" in k or "search_items_kernel" in k for k in kernels)      # a name of their own
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(select_asm):
    _, kernels, meta = select_asm
    for name, m in meta.items():
        assert m["spill"] == 0 and m["private"] == 0, (name, m)
    for body in kernels.values():
        assert "scratch_" not in body


def test_each_format_runs_on_its_mfma_within_one_block_per_cu(select_asm):
    _, kernels, meta = select_asm
    for name, body in kernels.items():
        if "F32Rows" in name:
            assert "v_mfma_f32_32x32x2_f32" in body, name
        elif "Bf16Rows" in name:
            assert "v_mfma_f32_32x32x16_bf16" in body, name
        if "search_select_kernel" in name:
            assert "ds_read_b128" in body and "ds_write_b128" in body, name
        assert meta[name]["vgpr"] <= 512 and meta[name]["lds"] <= 160 * 1024, (name, meta[name])


def test_lds_sizes_are_those_of_the_kernels_by_item_plus_a_group_code_per_query_row(select_asm):
    _, kernels, meta = select_asm
    for fmt in ("F32Rows", "Bf16Rows"):
        for wq, kl in PAIRS:
            name = next(k for k in kernels if f"{fmt}ELi{wq}ELi{kl}EE" in k)
            assert 0 <= meta[name]["lds"] - lds_bytes(fmt, wq, kl) <= 512, (name, meta[name]["lds"], lds_bytes(fmt, wq, kl))
    assert lds_bytes("F32Rows", 2, 64) == 153088                              # the widest: 149.5 KB of 160
    assert meta[next(k for k in kernels if "pack_row_mask_kernel" in k)]["lds"] == 0

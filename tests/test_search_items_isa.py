"""CPU-only check of the gfx950 code of csrc/search_items.hip, compiled with the Makefile's flags: the chosen instantiations of the id-aware score kernel
are there for both operand formats (the four (WQ, list capacity) pairs of the plain kernels: item codes are read from global memory, so the LDS sizes carry
over), every kernel keeps its registers (no scratch, no spilled VGPRs), the fp32 kernels form their product on the fp32-input MFMA and the bf16 kernels on
v_mfma_f32_32x32x16_bf16 only, and registers and LDS fit one block per CU.  search.hip and search_bf16.hip still assemble to their pinned kernel counts."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechclip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PAIRS = ((1, 16), (1, 128), (2, 16), (2, 64))
# declared LDS of an instantiation: two stage images + list (8 bytes per slot) + buffer (8 bytes per slot) + slot counter and skip code per query row; hipcc
# allots up to 512 bytes beside the declared arrays (256 today, in the plain kernels too)
STAGE = {"F32Rows": 68 * 4, "Bf16Rows": 72 * 2}                               # bytes per stage row


def lds_bytes(fmt, wq, kl):
    bq, cb = 64 * wq, 16 if (wq, kl) == (2, 64) else 32
    return (bq + 128) * STAGE[fmt] + bq * kl * 8 + bq * cb * 8 + bq * 8


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def assemble(tmp, name):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp / (name + ".s")
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", str(out)], check=True, cwd=CSRC)
    return out.read_text()


@pytest.fixture(scope="module")
def items_asm(tmp_path_factory):
    text = assemble(tmp_path_factory.mktemp("isa"), "search_items")
    kernels = {}
    for m in re.finditer(r"^(_Z\w*(?:search_items|topk_merge_items)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), private=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return text, kernels, meta


def test_the_chosen_instantiations_are_there_and_nothing_else(items_asm):
    text, kernels, meta = items_asm
    assert len(kernels) == 9 and len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 9, sorted(kernels)
    assert sum("topk_merge_items_kernel" in k for k in kernels) == 1
    for fmt in ("F32Rows", "Bf16Rows"):
        for wq, kl in PAIRS:
            assert sum(f"search_items_kernelIN11search_core{len(fmt)}{fmt}ELi{wq}ELi{kl}EE" in k for k in kernels) == 1, (fmt, wq, kl)
    assert set(meta) == set(kernels)
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(items_asm):
    _, kernels, meta = items_asm
    for name, m in meta.items():
        assert m["spill"] == 0 and m["private"] == 0, (name, m)
    for body in kernels.values():
        assert "scratch_" not in body


def test_each_format_runs_on_its_mfma_within_one_block_per_cu(items_asm):
    _, kernels, meta = items_asm
    for name, body in kernels.items():
        if "F32Rows" in name:
            assert "v_mfma_f32_32x32x2_f32" in body and "bf16" not in " ".join(re.findall(r"v_mfma\w+", body)), name
        elif "Bf16Rows" in name:
            assert "v_mfma_f32_32x32x16_bf16" in body and not re.search(r"v_mfma_f32_\w+_f32\b", body), name
        else:
            assert "v_mfma" not in body, name
        if "search_items_kernel" in name:
            assert "ds_read_b128" in body and "ds_write_b128" in body, name
        assert meta[name]["vgpr"] <= 512 and meta[name]["lds"] <= 160 * 1024, (name, meta[name])


def test_lds_sizes_are_the_stated_arithmetic(items_asm):
    """the plain kernels' LDS plus one skip code per query row -- no third field in list or buffer."""
    _, kernels, meta = items_asm
    for fmt in ("F32Rows", "Bf16Rows"):
        for wq, kl in PAIRS:
            name = next(k for k in kernels if f"{fmt}ELi{wq}ELi{kl}EE" in k)
            assert 0 <= meta[name]["lds"] - lds_bytes(fmt, wq, kl) <= 512, (name, meta[name]["lds"], lds_bytes(fmt, wq, kl))
    assert lds_bytes("F32Rows", 2, 64) == 152576 and lds_bytes("Bf16Rows", 1, 16) == 52736      # the widest: 149 KB of 160; the single-query path: two blocks per CU
    merge = next(k for k in kernels if "topk_merge_items_kernel" in k)
    assert 16 * 1024 <= meta[merge]["lds"] <= 16 * 1024 + 128             # the dead bitmap: one bit per candidate, L <= 1024 * 128


@pytest.mark.parametrize("name,score,total", [("search", "search_kernel", 5), ("search_bf16", "search_bf16_kernel", 4)])
def test_the_plain_files_keep_their_kernels(tmp_path, name, score, total):
    text = assemble(tmp_path, name)
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert len(names) == total and sum(score in n for n in names) == 4 and sum("topk_merge_kernel" in n for n in names) == total - 4, names
    assert not any("items" in n for n in names)

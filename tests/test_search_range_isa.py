"""CPU-only check of the gfx950 code of csrc/search_range.hip, compiled with the Makefile's flags: the count and the fill kernel are there for both operand
formats and both query-tile widths and nothing else is, every kernel keeps its registers (no scratch, no spilled VGPRs), each format forms its product on
its own MFMA, and no kernel holds an atomic of any kind: a hit's place comes from ballots, popcounts and one LDS table."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechclip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
STAGE = {"F32Rows": 68 * 4, "Bf16Rows": 72 * 2}                               # bytes per stage row (search_rows.h)


def lds_bytes(fmt, wq, fill):
    """two stage images + threshold and skip code per query row + fill: two [rows][4] count tables and an int64 position per row / count: two counts per row"""
    bq = 64 * wq
    return (bq + 128) * STAGE[fmt] + bq * 8 + (bq * 40 if fill else bq * 8)


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def range_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "search_range.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "search_range.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*range_(?:count|fill)_kernel\w*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
                         text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), private=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    return text, kernels, meta


def test_every_instantiation_is_there_and_nothing_else(range_asm):
    text, kernels, meta = range_asm
    assert len(kernels) == 8 and len(re.findall(r"^\s*\.amdhsa_kernel\s", text, re.M)) == 8, sorted(kernels)
    for fmt in ("F32Rows", "Bf16Rows"):
        for kind in ("17range_fill_kernel", "18range_count_kernel"):
            for wq in (1, 2):
                assert sum(f"{kind}IN11search_core{len(fmt)}{fmt}ELi{wq}EE" in k for k in kernels) == 1, (fmt, kind, wq)
    assert set(meta) == set(kernels) and not any("search_kernel" in k for k in kernels)      # tests/test_search_isa.py counts that name in search.hip
    for body in kernels.values():
        assert "s_endpgm" in body


def test_no_scratch_and_no_spilled_registers(range_asm):
    _, kernels, meta = range_asm
    for name, m in meta.items():
        assert m["spill"] == 0 and m["private"] == 0, (name, m)
    for body in kernels.values():
        assert "scratch_" not in body


def test_each_format_runs_on_its_mfma_without_atomics_within_one_block_per_cu(range_asm):
    _, kernels, meta = range_asm
    for name, body in kernels.items():
        if "F32Rows" in name:
            assert "v_mfma_f32_32x32x2_f32" in body and "bf16" not in " ".join(re.findall(r"v_mfma\w+", body)), name
        else:
            assert "Bf16Rows" in name and "v_mfma_f32_32x32x16_bf16" in body and not re.search(r"v_mfma_f32_\w+_f32\b", body), name
        assert "ds_read_b128" in body and "ds_write_b128" in body, name
        assert not re.search(r"\b(?:ds|global|flat|buffer)_(?:atomic|add|inc|dec|cmpst|cmpswap)\w*", body), name      # no LDS and no global atomics
        assert "s_bcnt1_i32_b32" in body or "v_bcnt_u32_b32" in body, name                                             # popcounts of the ballots
        assert meta[name]["vgpr"] <= 512, (name, meta[name])
        fill, wq = "range_fill_kernel" in name, 2 if "ELi2EE" in name else 1
        want = lds_bytes("F32Rows" if "F32Rows" in name else "Bf16Rows", wq, fill)
        assert 0 <= meta[name]["lds"] - want <= 512, (name, meta[name]["lds"], want)                                   # two blocks per CU fit the 160 KB
        if fill:
            assert "global_store_dword" in body and "global_store_dwordx2" in body, name                             # score and position of a hit

"""CPU-only check of the gfx950 code of csrc/train_vit.hip, compiled with the Makefile's flags: the kernels of sc_quickgelu_bwd_bf16 and sc_vit_embed_bwd keep
their registers (private segment size 0: no scratch).  Nothing else is inspected."""
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
def vit_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "train_vit.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "train_vit.hip"), "-o", str(out)], check=True, cwd=CSRC)
    return out.read_text()


def test_the_new_kernels_compile_without_scratch(vit_asm):
    sizes = dict(re.findall(r"\.name:\s+(\S+_kernel\S*).*?\.private_segment_fixed_size:\s+(\d+)", vit_asm, re.S))
    for kernel in ("quickgelu_bwd_bf16_kernel", "vit_embed_bwd_kernel", "vit_embed_bwd_finish_kernel"):
        hits = [n for n in sizes if kernel in n]
        assert len(hits) == 1, (kernel, sorted(sizes))
    assert len(sizes) == 3 and all(int(v) == 0 for v in sizes.values()), sizes

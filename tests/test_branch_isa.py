"""CPU-only checks of the multi-layer parallel branch: the new attention kernel's gfx950 code (no scratch, no spills, no LDS-crossbar shuffles
feeding packed-fp32 arithmetic: the construct profiles/r06_vit_layernorm_nondeterminism.txt traced run-to-run differences to), and the
module surface (any depth, either LayerNorm order, the reference's state-dict keys)."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speechclip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.+)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


@pytest.fixture(scope="module")
def hd_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "attention_hd.s"
    flags = [f for f in _makefile_flags() if f != "-fPIC"]
    subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "attention_hd.hip"), "-o", str(out)], check=True, cwd=CSRC)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_Z\w*attn_hd_fwd_kernel\w*):[^\n]*\n(.*?)^\s*s_endpgm", text, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    return text, kernels


def test_attention_hd_kernels_have_no_scratch_or_spills(hd_asm):
    text, kernels = hd_asm
    assert len(kernels) == 12, sorted(kernels)              # head_dim {64, 96, 128} x dropout x fp32 out
    for name, body in kernels.items():
        assert "scratch_" not in body and "buffer_store" not in body, name
    assert not re.search(r"ScratchSize:\s*[1-9]", text)
    for key in ("vgpr_spill_count", "sgpr_spill_count"):
        assert all(int(v) == 0 for v in re.findall(rf"\.{key}:\s+(\d+)", text)), key
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text))


def test_attention_hd_kernels_use_no_lds_crossbar_shuffles_before_packed_fp32(hd_asm):
    """No v_pk_{add,mul,fma}_f32 fed by ds_bpermute_b32 results: the kernels exchange row statistics with v_permlane32_swap (VALU) only,
    so no ds_bpermute_b32 appears at all."""
    _, kernels = hd_asm
    for name, body in kernels.items():
        assert "ds_bpermute_b32" not in body, name
        assert "v_permlane32_swap" in body, name


def test_branch_builds_any_depth_and_order_with_reference_keys():
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    m = TransformerEncoder(n_layers=3, norm_first=True)
    assert m.stacked and len(m.model.layers) == 3
    ref_layer = torch.nn.TransformerEncoderLayer(768, 8, 3072, 0.1, "gelu", 1e-5, batch_first=True, norm_first=True)
    ref = torch.nn.TransformerEncoder(ref_layer, 3, torch.nn.LayerNorm(768, eps=1e-5), enable_nested_tensor=False)
    want = {"model." + k: tuple(v.shape) for k, v in ref.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    m.load_state_dict({"model." + k: v for k, v in ref.state_dict().items()})
    for hd_ok in ((1024, 8), (512, 8), (768, 8)):
        TransformerEncoder(n_layers=2, d_model=hd_ok[0], nhead=hd_ok[1], dim_feedforward=64)
    with pytest.raises(NotImplementedError, match=r"\{64, 96, 128\}"):
        TransformerEncoder(n_layers=2, d_model=768, nhead=16)
    with pytest.raises(NotImplementedError):
        TransformerEncoder(n_layers=2, activation="relu")
    with pytest.raises(NotImplementedError):
        TransformerEncoder(n_layers=2, batch_first=False)
    assert not TransformerEncoder(n_layers=1, d_model=768, nhead=12).stacked      # the one-layer post-LN head keeps any head dim


def test_attention_hd_rejects_unsupported_head_dims_with_a_message():
    import ctypes
    from speechclip_amd import _lib
    L = _lib.lib()
    rc = L.sc_attention_hd_fwd(None, None, None, None, None, 1, 1, 8, 8, 80, 0, 240, 0, 240, 0, 80, ctypes.c_float(1.0), ctypes.c_float(0.0), 0, 0, None)
    assert rc < 0 and b"head_dim=80" in L.sc_last_error()

"""sc_attention_hd_fwd: the MFMA flash attention for head_dim 64 / 96 / 128 (full-row layers of a parallel branch deeper than one layer) against
fp64 torch on the same bf16 operands: key lengths at and around the 64-key tile edges, L = 1, L not a multiple of 16, the CLS-row form
(Tq = 1, strided query, fp32 out) and dropout with the mask restated on the host."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ref(qkv, B, L, H, hd, klens, mask=None):
    """fp64 softmax(q k^T / sqrt(hd)) v per (b, h) over keys < klens[b]; `mask` [B, H, L, L] multiplies the probabilities (dropout)."""
    D = H * hd
    x = qkv.double().view(B, L, 3, H, hd)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    valid = torch.arange(L)[None, :] < torch.as_tensor(klens)[:, None]
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p * mask.double()
    return (p @ v).permute(0, 2, 1, 3).reshape(B, L, D)


def _run(B, L, H, hd, klens, seed=0, drop_p=0.0, drop_seed=0):
    from speechclip_amd import ops
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * L, 3 * H * hd, generator=g).to(BF)
    kl = torch.tensor(klens, dtype=torch.int32)
    out = ops.attention_hd_qkv(qkv.cuda(), B, L, H, kl.cuda(), drop_p=drop_p, seed=drop_seed)
    return qkv, kl, out.float().cpu().view(B, L, H * hd)


@pytest.mark.parametrize("hd", [64, 96, 128])
@pytest.mark.parametrize("L,lens", [(1, [1, 1]), (63, [63, 1, 62]), (64, [64, 63, 1]), (65, [65, 64, 2]), (129, [129, 65, 128]),
                                    (200, [200, 13, 127]), (500, [500, 437, 64, 65])])
def test_attention_hd_matches_fp64(hd, L, lens):
    H = 2 if hd != 64 else 3
    B = len(lens)
    qkv, kl, out = _run(B, L, H, hd, lens, seed=L + hd)
    want = _ref(qkv, B, L, H, hd, lens)
    err = (out.double() - want).abs().max().item()
    assert err < 2e-2, (hd, L, lens, err)
    assert torch.isfinite(out).all()


def test_attention_hd_cls_row_form_fp32_out():
    """Tq = 1: the per-utterance query of the branch's last layer (query rows [B, D], K / V of [B, Lq] rows of [k | v]), fp32 output."""
    from speechclip_amd import ops
    B, L, H, hd = 5, 301, 8, 96
    D = H * hd
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, D, generator=g).to(BF)
    kv = torch.randn(B * L, 2 * D, generator=g).to(BF)
    lens = [301, 1, 64, 65, 200]
    kl = torch.tensor(lens, dtype=torch.int32).cuda()
    kvc = kv.cuda()
    out = ops.attention_hd(q.cuda(), kvc, kvc[:, D:], B, H, 1, L, hd, (D, D), (L * 2 * D, 2 * D), kl, out_f32=True).cpu().view(B, D)
    qkv = torch.zeros(B, L, 3 * D, dtype=BF)
    qkv[:, 0, :D] = q
    qkv[:, :, D:] = kv.view(B, L, 2 * D)
    want = _ref(qkv.view(B * L, 3 * D), B, L, H, hd, lens)[:, 0]
    assert (out.double() - want).abs().max().item() < 1e-2


def test_attention_hd_is_deterministic_and_keys_past_the_length_do_not_matter():
    from speechclip_amd import ops
    B, L, H, hd = 3, 300, 8, 128
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B * L, 3 * H * hd, generator=g).to(BF).cuda()
    kl = torch.tensor([300, 150, 77], dtype=torch.int32).cuda()
    a = ops.attention_hd_qkv(qkv, B, L, H, kl)
    assert torch.equal(a, ops.attention_hd_qkv(qkv, B, L, H, kl))
    x = qkv.view(B, L, 3, H * hd).clone()
    x[1, 150:, 1:] = float("nan")            # k / v rows past utterance 1's length
    x[2, 77:, 1:] = 1e4
    b_ = ops.attention_hd_qkv(x.view(B * L, -1), B, L, H, kl)
    assert torch.equal(a.view(B, L, -1)[:, :77], b_.view(B, L, -1)[:, :77])


def _keep_attn(seed, B, H, T, p):
    """csrc/common.h hash_pair restated (as tests/test_dropout_gpu.py): pair index ((b*H + h)*T + query) * ceil(T/2) + key/2, 16 bits per key."""
    def h32(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
        x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
        x ^= x >> np.uint64(16)
        return x
    rows = np.arange(B * H * T, dtype=np.uint64)[:, None]
    keys = np.arange(T, dtype=np.uint64)[None, :]
    pair = (rows * np.uint64((T + 1) // 2) + (keys >> np.uint64(1))) & np.uint64(0xffffffff)
    h = h32(((pair * np.uint64(0x9E3779B1)) + np.uint64(seed & 0xffffffff)) & np.uint64(0xffffffff))
    bits = np.where((keys & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xffff))
    return torch.from_numpy((bits >= np.uint64(int(p * 65536.0))).astype(np.float32)).view(B, H, T, T)


@pytest.mark.parametrize("hd", [96, 128])
def test_attention_hd_dropout_mask_restated_on_host(hd):
    B, L, H, p, seed = 2, 131, 2, 0.1, 4242
    lens = [131, 70]
    qkv, kl, out = _run(B, L, H, hd, lens, seed=11, drop_p=p, drop_seed=seed)
    mask = _keep_attn(seed, B, H, L, p) / (1 - p)
    want = _ref(qkv, B, L, H, hd, lens, mask)
    assert (out.double() - want).abs().max().item() < 2e-2
    no_drop = _ref(qkv, B, L, H, hd, lens)
    assert (out.double() - no_drop).abs().max().item() > 5e-2          # the mask is really applied


def test_attention_hd_argument_errors_and_head_dim_64_entry_unchanged():
    from speechclip_amd import _lib
    L = _lib.lib()
    rc = L.sc_attention_hd_fwd(None, None, None, None, None, 1, 1, 8, 8, 80, 0, 240, 0, 240, 0, 80, ctypes.c_float(1.0), ctypes.c_float(0.0), 0, 0, None)
    assert rc < 0 and b"head_dim=80" in L.sc_last_error()
    rc = L.sc_attention_fwd(None, None, None, None, None, 1, 1, 8, 96, 8, 8, ctypes.c_float(1.0), 0, None)
    assert rc < 0 and b"head_dim" in L.sc_last_error()

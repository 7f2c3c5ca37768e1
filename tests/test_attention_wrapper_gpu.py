"""ops.attention is the one attention-forward wrapper (uniform / packed rows, with / without probability dropout): it must reach the C entry that
ops.attention_dropout / ops.attention_packed reach, with the same arguments, and refuse what no entry serves."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, T, H = 2, 70, 2            # one 64-key tile plus a partial second one
KLENS = [70, 37]              # the second utterance ends inside the first tile


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(70)
    qkv = (0.5 * torch.randn(B * T, 3 * H * 64, generator=g)).to(BF).cuda()
    kl = torch.tensor(KLENS, dtype=torch.int32).cuda()
    off = torch.tensor([0, T, 2 * T], dtype=torch.int32).cuda()          # uniform offsets: the same rows through the packed entry
    return qkv, kl, off


def _entry(name, qkv, kl, *tail):
    """The C entry itself, with the argument list the three wrappers used to pass."""
    from speechclip_amd._lib import check, lib, stream
    D = H * 64
    out = torch.empty(qkv.shape[0], D, device=qkv.device, dtype=BF)
    check(getattr(lib(), name)(qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr(), kl.data_ptr(), *tail, stream()), name)
    return out


def test_drop_routes_to_the_dropout_entry(case):
    from speechclip_amd import ops
    qkv, kl, _ = case
    D = H * 64
    got = ops.attention(qkv, B, T, H, kl, drop=(0.1, 7))
    assert torch.equal(got, ops.attention_dropout(qkv, B, T, H, kl, 0.1, 7))
    assert torch.equal(got, _entry("sc_attention_fwd_dropout", qkv, kl, B, H, T, 64, 3 * D, D, 0.125, 0, 0.1, 7))
    assert not torch.equal(got, ops.attention(qkv, B, T, H, kl))          # the mask was applied


@pytest.mark.parametrize("drop", [None, (0.1, 7)])
def test_row_off_routes_to_the_packed_entry(case, drop):
    from speechclip_amd import ops
    qkv, kl, off = case
    got = ops.attention(qkv, B, T, H, kl, row_off_i32=off, drop=drop)
    p, seed = drop if drop else (0.0, 0)
    assert torch.equal(got, ops.attention_packed(qkv, B, T, H, kl, off, drop_p=p, seed=seed))
    D = H * 64
    assert torch.equal(got, _entry("sc_attention_fwd_packed", qkv, kl, off.data_ptr(), B, H, T, B * T, 64, 3 * D, D, 0.125, p, seed, 0))
    # ragged rows: utterance 1 owns 37 rows only
    rows = torch.cat([qkv[:T], qkv[T:T + 37]]).contiguous()
    off2 = torch.tensor([0, T, T + 37], dtype=torch.int32).cuda()
    got = ops.attention(rows, B, T, H, kl, row_off_i32=off2, drop=drop)
    assert got.shape == (T + 37, H * 64)
    assert torch.equal(got, ops.attention_packed(rows, B, T, H, kl, off2, drop_p=p, seed=seed))


def test_unserved_combinations_raise(case):
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    qkv, kl, off = case
    for kw in (dict(scale=0.1, row_off_i32=off), dict(causal=True, row_off_i32=off), dict(scale=0.1, drop=(0.1, 7)), dict(causal=True, drop=(0.1, 7))):
        with pytest.raises(SpeechClipHipError):
            ops.attention(qkv, B, T, H, kl, **kw)
    with pytest.raises(SpeechClipHipError):
        ops.attention(qkv.to(torch.float16), B, T, H, kl, drop=(0.1, 7))

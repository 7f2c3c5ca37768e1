"""Fused attention backward over packed rows (sc_attention_bwd_packed) and sc_pack_rows, the adjoint of sc_unpack_rows.

The kernel is compared with torch autograd in fp64 on the CPU over the same bf16-rounded operands, per utterance: ragged row offsets (lengths 1, 63, 64,
65 and a full Tmax among them), the uniform layout beside the existing image-based backward, the dropout form against the mask read back from the forward,
the row_off and the uniform addressing of the same rows bit for bit, NaN on the rows that take no part, run-to-run bitwise equality, and the memory it
takes (no L x L image)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cos(a, b):
    return F.cosine_similarity(a.double().reshape(1, -1), b.double().reshape(1, -1)).item()


def _reference(qkv, dO, rows, klens, H, masks=None, drop_p=0.0):
    """fp64 autograd of softmax(Q K^T / 8) V per utterance and head over its klen valid rows (queries and keys); masks[b][h]: kept set [klen, klen] of a
    forward with attention dropout.  Returns dqkv fp64 [total, 3*H*64] (zeros on the rows that take no part)."""
    d = H * 64
    out = torch.zeros(qkv.shape[0], 3 * d, dtype=torch.float64)
    off = 0
    for b, (n, kl) in enumerate(zip(rows, klens)):
        if kl > 0:
            x = qkv[off:off + kl].double().clone().requires_grad_(True)
            xx = x.view(kl, 3, H, 64)
            q, k, v = xx[:, 0].transpose(0, 1), xx[:, 1].transpose(0, 1), xx[:, 2].transpose(0, 1)           # [H, kl, 64]
            p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1)
            if masks is not None:
                p = p * torch.stack([masks[b][h] for h in range(H)]).double() / (1.0 - drop_p)
            o = (p @ v).transpose(0, 1).reshape(kl, d)
            o.backward(dO[off:off + kl].double())
            out[off:off + kl] = x.grad
        off += n
    return out


def _check(got, ref, rows, klens, H, what):
    """Bound 1 of the issue, per utterance and per operand on the valid rows; exact zeros on the masked rows."""
    d = H * 64
    got = got.double().cpu()
    off = 0
    for b, (n, kl) in enumerate(zip(rows, klens)):
        for name, c0 in (("dq", 0), ("dk", d), ("dv", 2 * d)):
            gv, rv = got[off:off + kl, c0:c0 + d], ref[off:off + kl, c0:c0 + d]
            if kl > 0:
                cos, err, bound = _cos(gv, rv), (gv - rv).abs().max().item(), 3e-2 * rv.abs().max().item() + 1e-3
                print(f"{what} utt {b} rows {n} klen {kl} {name}: cosine {cos:.6f} max|err| {err:.3e} bound {bound:.3e}")
                if rv.abs().max().item() < 1e-12:          # one valid key: softmax of a single score, dq = dk = 0 analytically -- the cosine of a zero vector is undefined
                    assert err < bound, (what, b, name, err, bound)
                    continue
                assert cos > 0.999 and err < bound, (what, b, name, cos, err, bound)
            assert bool((got[off + kl:off + n, c0:c0 + d] == 0).all()), (what, b, name, "masked rows must be exactly 0")
        off += n


def _inputs(rows, H, seed):
    g = _g(seed)
    total, d = sum(rows), H * 64
    qkv = torch.randn(total, 3 * d, generator=g).to(BF)
    dO = torch.randn(total, d, generator=g).to(BF)
    off = [0]
    for n in rows:
        off.append(off[-1] + n)
    return qkv, dO, torch.tensor(off, dtype=torch.int32)


ROWS = [2, 64, 65, 66, 131, 40, 1]
KLENS = [1, 63, 64, 65, 131, 30, 1]          # 131 = Tmax: a full-length utterance; the others leave a halo row (or more) masked


@pytest.mark.parametrize("H", [2, 12])
def test_packed_backward_vs_fp64_autograd(H):
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    qkv, dO, off = _inputs(ROWS, H, 100 + H)
    B, Tmax = len(ROWS), max(ROWS)
    kl = torch.tensor(KLENS, dtype=torch.int32).cuda()
    att = ops.attention_packed(qkv.cuda(), B, Tmax, H, kl, off.cuda())
    got = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda())
    assert got.shape == (sum(ROWS), 3 * H * 64) and got.dtype == BF
    _check(got, _reference(qkv, dO, ROWS, KLENS, H), ROWS, KLENS, H, f"packed H={H}")


@pytest.mark.parametrize("B,T,H,lens", [(3, 70, 2, [70, 33, 7]), (2, 500, 12, [500, 321])])
def test_uniform_layout_beside_the_image_backward(B, T, H, lens):
    """row_off = NULL: the same operands through the new kernel and through train_hubert.attention_bwd; both meet the fp64 bound (they round differently,
    so they are not compared with each other).  Padded query rows carry dO = 0, as in a training step, so both treat them alike."""
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd, attention_bwd_packed
    qkv, dO, _ = _inputs([T] * B, H, 7 * T + H)
    for b, n in enumerate(lens):
        dO[b * T + n:(b + 1) * T] = 0
    d, Lp = H * 64, -(-T // 64) * 64
    kl = torch.tensor(lens, dtype=torch.int32).cuda()
    qkv_slack = torch.zeros(B * T + (Lp - T), 3 * d, dtype=BF)
    qkv_slack[:B * T] = qkv
    att = ops.attention(qkv.cuda(), B, T, H, kl)
    ref = _reference(qkv, dO, [T] * B, lens, H)
    new = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, T, H, kl, None)
    _check(new, ref, [T] * B, lens, H, "uniform, fused")
    old = attention_bwd(qkv_slack.cuda(), att, dO.cuda(), B, T, H, kl).double().cpu()
    for b, n in enumerate(lens):          # the image form leaves dq of padded query rows to its (zero) dO and writes key rows >= klen as zeros
        for c0 in (0, d, 2 * d):
            gv, rv = old[b * T:b * T + n, c0:c0 + d], ref[b * T:b * T + n, c0:c0 + d]
            assert _cos(gv, rv) > 0.999 and (gv - rv).abs().max().item() < 3e-2 * rv.abs().max().item() + 1e-3, ("image form", b, c0)


def test_row_off_and_uniform_layouts_agree():
    """Equal-length rows addressed through row_off and as the uniform layout (row_off = NULL) are the same units: without dropout the same bits.  (With
    dropout the two layouts index the forward's mask differently by contract and are not compared.)"""
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    rows, klens, H = [70, 70, 70], [70, 33, 64], 2
    qkv, dO, off = _inputs(rows, H, 71)
    assert off.tolist() == [0, 70, 140, 210]
    kl = torch.tensor(klens, dtype=torch.int32).cuda()
    att = ops.attention(qkv.cuda(), 3, 70, H, kl)
    uniform = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), 3, 70, H, kl, None)
    packed = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), 3, 70, H, kl, off.cuda())
    assert torch.equal(packed, uniform) and bool(uniform.float().abs().sum() > 0)


def test_rows_that_take_no_part_may_hold_anything():
    """Rows >= klens[b] of every utterance (q | k | v, dO and the forward's output) are zeroed on load: NaN there changes no bit of the result, and every
    row of it is finite.  att comes from the clean qkv: the packed forward still requires a finite V."""
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    H = 2
    qkv, dO, off = _inputs(ROWS, H, 9)
    B, Tmax = len(ROWS), max(ROWS)
    kl = torch.tensor(KLENS, dtype=torch.int32).cuda()
    att = ops.attention_packed(qkv.cuda(), B, Tmax, H, kl, off.cuda())
    clean = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda())
    qkv2, dO2, att2 = qkv.clone(), dO.clone(), att.cpu().clone()
    for b, k in enumerate(KLENS):
        for x in (qkv2, dO2, att2):
            x[int(off[b]) + k:int(off[b + 1])] = float("nan")
    assert bool(torch.isnan(qkv2.float()).any()) and bool(torch.isnan(att2.float()).any())
    got = attention_bwd_packed(qkv2.cuda(), att2.cuda(), dO2.cuda(), B, Tmax, H, kl, off.cuda())
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, clean)


def _recover_masks(qkv, rows, klens, H, off, drop_p, seed, packed):
    """The kept set of the forward's attention dropout: v is replaced by one-hot columns (key j -> unit vector j mod 64, one 64-key chunk at a time), so the
    output row of query i IS its probability row; an entry the dropped forward zeroed is a dropped key."""
    from speechclip_amd import ops
    B, Tmax, d = len(rows), max(rows), H * 64
    kl = torch.tensor(klens, dtype=torch.int32).cuda()
    masks = [[torch.zeros(k, k, dtype=torch.bool) for _ in range(H)] for k in klens]
    for c in range(-(-max(klens) // 64)):
        probe = qkv.clone()
        probe[:, 2 * d:] = 0
        o = 0
        for n in rows:
            for j in range(64 * c, min(n, 64 * c + 64)):
                probe[o + j, 2 * d + (j - 64 * c)::64] = 1.0           # every head's column (j mod 64)
            o += n
        if packed:
            plain = ops.attention_packed(probe.cuda(), B, Tmax, H, kl, off.cuda())
            dropped = ops.attention_packed(probe.cuda(), B, Tmax, H, kl, off.cuda(), drop_p=drop_p, seed=seed)
        else:
            plain = ops.attention(probe.cuda(), B, Tmax, H, kl)
            dropped = ops.attention_dropout(probe.cuda(), B, Tmax, H, kl, drop_p, seed)
        plain, dropped = plain.float().cpu(), dropped.float().cpu()
        o = 0
        for b, (n, k) in enumerate(zip(rows, klens)):
            hi = min(k, 64 * c + 64)
            for h in range(H):
                if hi > 64 * c:
                    assert bool((plain[o:o + k, h * 64:h * 64 + hi - 64 * c] > 0).all())
                    masks[b][h][:, 64 * c:hi] = dropped[o:o + k, h * 64:h * 64 + hi - 64 * c] > 0
            o += n
    return masks


@pytest.mark.parametrize("packed", [True, False])
def test_dropout_mask_is_the_forwards(packed):
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    H, drop_p, seed = 2, 0.25, 1234567
    rows = [38, 65, 101, 20] if packed else [70, 70, 70]
    klens = [37, 64, 100, 20] if packed else [70, 33, 64]
    qkv, dO, off = _inputs(rows, H, 55)
    B, Tmax = len(rows), max(rows)
    kl = torch.tensor(klens, dtype=torch.int32).cuda()
    masks = _recover_masks(qkv, rows, klens, H, off, drop_p, seed, packed)
    kept = sum(m.sum().item() for mb in masks for m in mb) / sum(m.numel() for mb in masks for m in mb)
    assert 0.70 < kept < 0.80, kept
    if packed:
        att = ops.attention_packed(qkv.cuda(), B, Tmax, H, kl, off.cuda(), drop_p=drop_p, seed=seed)
    else:
        att = ops.attention_dropout(qkv.cuda(), B, Tmax, H, kl, drop_p, seed)
    got = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda() if packed else None, (drop_p, seed))
    _check(got, _reference(qkv, dO, rows, klens, H, masks, drop_p), rows, klens, H, f"dropout packed={packed}")
    plain = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda() if packed else None)
    assert not torch.equal(plain, got)


@pytest.mark.parametrize("drop", [None, (0.1, 77)])
def test_two_calls_are_bitwise_equal(drop):
    from speechclip_amd import ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    H = 12
    qkv, dO, off = _inputs(ROWS, H, 3)
    B, Tmax = len(ROWS), max(ROWS)
    kl = torch.tensor(KLENS, dtype=torch.int32).cuda()
    att = ops.attention_packed(qkv.cuda(), B, Tmax, H, kl, off.cuda(), drop_p=drop[0] if drop else 0.0, seed=drop[1] if drop else 0)
    a = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda(), drop)
    b = attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, Tmax, H, kl, off.cuda(), drop)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())


def test_no_image_sized_temporary():
    """B = 8, H = 12, Tmax = 499 full lengths: the op's peak memory above its inputs and its output stays below ONE [B*H, Lp, Lp] bf16 image, and is exactly
    the statistics workspace the library asks for."""
    from speechclip_amd import _lib, ops
    from speechclip_amd.train_hubert import attention_bwd_packed
    B, H, T = 8, 12, 499
    qkv, dO, _ = _inputs([T] * B, H, 11)
    qkv, dO = qkv.cuda(), dO.cuda()
    kl = torch.full((B,), T, dtype=torch.int32).cuda()
    att = ops.attention(qkv, B, T, H, kl)
    attention_bwd_packed(qkv, att, dO, B, T, H, kl, None)           # warm: library load, kernel code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = attention_bwd_packed(qkv, att, dO, B, T, H, kl, None)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - out.numel() * 2
    image = B * H * 512 * 512 * 2
    ws = _lib.lib().sc_attention_bwd_packed_workspace_bytes(B * T, H)
    print("peak above inputs and output:", extra, "bytes; workspace:", ws, "; one image:", image)
    assert ws == 2 * 4 * B * T * H
    assert extra < image
    assert ws <= extra < ws + 512           # the caching allocator rounds a block up to 512 bytes


def test_head_dim_other_than_64_is_an_error():
    import ctypes
    from speechclip_amd import _lib
    L = _lib.lib()
    rc = L.sc_attention_bwd_packed(None, None, None, 0, None, None, 0, None, None, 1, 1, 8, 8, 80, ctypes.c_float(1.0), ctypes.c_float(0.0), 0, None, None, None,
                                   0, None, None)
    assert rc < 0 and b"head_dim=80" in L.sc_last_error()


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_pack_rows_is_the_adjoint_of_unpack_rows(dtype):
    from speechclip_amd import ops
    g = _g(21)
    rows = [5, 1, 9, 3, 7]
    off = [0]
    for n in rows:
        off.append(off[-1] + n)
    B, T, D, n = len(rows), 8, 64, 3           # T = 8 < 9: one utterance is cut by the padded length as well
    off_d = torch.tensor(off, dtype=torch.int32).cuda()
    x = torch.randn(n, off[-1], D, generator=g).to(dtype).cuda()
    y = torch.randn(n, B, T, D, generator=g).to(dtype).cuda()
    back = ops.pack_rows(ops.unpack_rows(x, off_d, B, T, halo=1), off_d, off[-1], halo=1)
    want = x.clone()
    for b, r in enumerate(rows):
        want[:, off[b] + min(r - 1, T):off[b + 1]] = 0              # the halo row (and rows beyond the padded length)
    assert torch.equal(back, want)
    lhs = (ops.unpack_rows(x, off_d, B, T, halo=1).double().cpu() * y.double().cpu()).sum().item()
    rhs = (x.double().cpu() * ops.pack_rows(y, off_d, off[-1], halo=1).double().cpu()).sum().item()
    assert abs(lhs - rhs) <= 1e-9 * max(1.0, abs(lhs)), (lhs, rhs)
    one = ops.pack_rows(y[0].contiguous(), off_d, off[-1])          # 3-D input, halo = 0
    assert one.shape == (off[-1], D) and torch.equal(one[off[2]:off[2] + 8], y[0, 2]) and bool((one[off[2] + 8:off[3]] == 0).all())

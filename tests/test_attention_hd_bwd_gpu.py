"""sc_attention_hd_bwd: the fused attention backward for head_dim 64 / 96 / 128 in sc_attention_hd_fwd's strided layout (Tq == Tk, and Tq == 1: the CLS
query of a branch's last layer).

The kernel is compared with torch autograd in fp64 on the CPU over the same bf16-rounded operands, per utterance and per operand, with the bound of
tests/test_attn_bwd_packed_gpu.py::_check (cosine > 0.999, max|err| < 3e-2 * max|ref| + 1e-3, its zero-gradient case for one valid key, exact zeros on the
rows that take no part): lengths 1, 63, 64, 65, a partial tile and a full T = 131; the dropout form against the forward's mask restated on the host;
head_dim 64 beside sc_attention_bwd_packed; run-to-run bitwise equality; the combinations the entry refuses; the memory it takes (no Tq x Tk image)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KLENS = [131, 1, 63, 64, 65, 30]          # a full length, one key, a 64-key tile edge from both sides, a partial tile
B, H, T = 6, 2, 131


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cos(a, b):
    return F.cosine_similarity(a.double().reshape(1, -1), b.double().reshape(1, -1)).item()


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


# ---- the forward's attention-dropout mask, restated (csrc/common.h hash32 / hash_pair; sc_attention_hd_fwd's pair index)
def _hash32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def _keep(seed, b, h, nH, queries, Tk, p):
    """kept set [len(queries), Tk] of (b, h): pair index ((b*H + h)*Tk + query) * ceil(Tk / 2) + key / 2, one hash per key pair (even key: the low 16 bits),
    kept iff the 16 bits >= p * 2^16."""
    rows = ((b * nH + h) * Tk + np.asarray(queries, dtype=np.uint64)).reshape(-1, 1)
    keys = np.arange(Tk, dtype=np.uint64)[None, :]
    pair = (rows * np.uint64((Tk + 1) // 2) + (keys >> np.uint64(1))) & np.uint64(0xffffffff)
    hsh = _hash32(((pair * np.uint64(0x9E3779B1)) + np.uint64(seed & 0xffffffff)) & np.uint64(0xffffffff))
    bits = np.where((keys & np.uint64(1)) == 1, hsh >> np.uint64(16), hsh & np.uint64(0xffff))
    return torch.from_numpy((bits >= np.uint64(min(65535, int(p * 65536.0)))).astype(np.float64))


def _reference(q, k, v, dO, klens, nH, hd, drop=None):
    """fp64 autograd of softmax(Q K^T / sqrt(hd)) V per utterance and head.  q / dO [B, Tq, D], k / v [B, Tk, D]; the queries that take part are t < min(klen, Tq),
    the keys j < klen.  drop = (p, seed): the probabilities are multiplied by the forward's kept set / (1 - p).  -> dq [B, Tq, D], dk, dv [B, Tk, D] (fp64, zeros
    on the rows that take no part)."""
    nB, Tq, D = q.shape
    Tk = k.shape[1]
    dq, dk, dv = torch.zeros(nB, Tq, D, dtype=torch.float64), torch.zeros(nB, Tk, D, dtype=torch.float64), torch.zeros(nB, Tk, D, dtype=torch.float64)
    for b, kl in enumerate(klens):
        nq = min(kl, Tq)
        if nq == 0:
            continue
        qb = q[b, :nq].double().clone().requires_grad_(True)
        kb = k[b, :kl].double().clone().requires_grad_(True)
        vb = v[b, :kl].double().clone().requires_grad_(True)
        qh, kh, vh = (x.view(-1, nH, hd).transpose(0, 1) for x in (qb, kb, vb))
        p = torch.softmax((qh @ kh.transpose(-1, -2)) * hd ** -0.5, -1)
        if drop is not None:
            keep = torch.stack([_keep(drop[1], b, h, nH, np.arange(nq), Tk, drop[0])[:, :kl] for h in range(nH)])
            p = p * keep / (1.0 - drop[0])
        o = (p @ vh).transpose(0, 1).reshape(nq, D)
        o.backward(dO[b, :nq].double())
        dq[b, :nq], dk[b, :kl], dv[b, :kl] = qb.grad, kb.grad, vb.grad
    return dq, dk, dv


def _check(got, ref, klens, what):
    """got / ref: (dq, dk, dv), each [B, rows, D]; per utterance and per operand on the rows that take part, exact zeros elsewhere."""
    for name, g_, r_ in zip(("dq", "dk", "dv"), got, ref):
        g_ = g_.double().cpu()
        assert g_.shape == r_.shape, (what, name, g_.shape, r_.shape)
        for b, kl in enumerate(klens):
            n = min(kl, g_.shape[1])
            gv, rv = g_[b, :n], r_[b, :n]
            if n > 0:
                cos, err, bound = _cos(gv, rv), (gv - rv).abs().max().item(), 3e-2 * rv.abs().max().item() + 1e-3
                print(f"{what} utt {b} klen {kl} {name}: cosine {cos:.6f} max|err| {err:.3e} bound {bound:.3e}")
                if rv.abs().max().item() < 1e-12:          # one valid key: dq = dk = 0 analytically, and the cosine of a zero vector is undefined
                    assert err < bound, (what, b, name, err, bound)
                else:
                    assert cos > 0.999 and err < bound, (what, b, name, cos, err, bound)
            assert bool((g_[b, n:] == 0).all()), (what, b, name, "rows that take no part must be exactly 0")


def _full_inputs(hd, seed, nB=B, nH=H, nT=T):
    g, D = _g(seed), nH * hd
    return torch.randn(nB * nT, 3 * D, generator=g).to(BF), torch.randn(nB * nT, D, generator=g).to(BF)


def _full_run(qkv, dO, klens, nB, nT, nH, drop=(0.0, 0)):
    from speechclip_amd import ops
    kl = _i32(klens)
    att = ops.attention_hd_qkv(qkv.cuda(), nB, nT, nH, kl, drop_p=drop[0], seed=drop[1])
    return ops.attention_hd_qkv_bwd(qkv.cuda(), att, dO.cuda(), nB, nT, nH, kl, drop_p=drop[0], seed=drop[1])


def _split(dqkv, nB, nT, D):
    x = dqkv.view(nB, nT, 3 * D)
    return x[..., :D], x[..., D:2 * D], x[..., 2 * D:]


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_full_rows_vs_fp64_autograd(hd):
    D = H * hd
    qkv, dO = _full_inputs(hd, 100 + hd)
    got = _full_run(qkv, dO, KLENS, B, T, H)
    assert got.shape == (B * T, 3 * D) and got.dtype == BF
    q, k, v = _split(qkv, B, T, D)
    _check(_split(got, B, T, D), _reference(q, k, v, dO.view(B, T, D), KLENS, H, hd), KLENS, f"full rows hd={hd}")


def _cls_inputs(hd, seed):
    g, D = _g(seed), H * hd
    return torch.randn(B, D, generator=g).to(BF), torch.randn(B * T, 2 * D, generator=g).to(BF), torch.randn(B, D, generator=g).to(BF)


def _cls_run(q, kv, dO, hd, klens, drop=(0.0, 0)):
    from speechclip_amd import ops
    D, kl = H * hd, _i32(klens)
    qc, kvc = q.cuda(), kv.cuda()
    qs, ks = (D, D), (T * 2 * D, 2 * D)
    O = ops.attention_hd(qc, kvc, kvc[:, D:], B, H, 1, T, hd, qs, ks, kl, drop_p=drop[0], seed=drop[1])
    return ops.attention_hd_bwd(qc, kvc, kvc[:, D:], O, dO.cuda().view(B, 1, D), B, H, 1, T, hd, qs, ks, kl, drop_p=drop[0], seed=drop[1])


@pytest.mark.parametrize("hd", [64, 96, 128])
def test_cls_query_form_vs_fp64_autograd(hd):
    """Tq = 1: q from its own [B, D] buffer, k | v from a [B*Tk, 2D] buffer with strides (Tk*2D, 2D)."""
    D = H * hd
    q, kv, dO = _cls_inputs(hd, 200 + hd)
    dq, dk, dv = _cls_run(q, kv, dO, hd, KLENS)
    assert dq.shape == (B, 1, D) and dk.shape == (B, T, D) and dv.shape == (B, T, D)
    kv3 = kv.view(B, T, 2 * D)
    ref = _reference(q.view(B, 1, D), kv3[..., :D], kv3[..., D:], dO.view(B, 1, D), KLENS, H, hd)
    _check((dq, dk, dv), ref, KLENS, f"Tq=1 hd={hd}")
    for b, kl in enumerate(KLENS):
        assert bool((dk[b, kl:] == 0).all()) and bool((dv[b, kl:] == 0).all())


def test_zero_length_utterance_and_null_klens():
    """klens[b] = 0: nothing takes part, every row of that utterance is written as zeros; klens = NULL means Tk; values outside [0, Tk] are clamped."""
    from speechclip_amd import ops
    hd, nB, nT = 96, 3, 70
    D = H * hd
    qkv, dO = _full_inputs(hd, 5, nB, H, nT)
    q, k, v = _split(qkv, nB, nT, D)
    got = _full_run(qkv, dO, [0, 70, 40], nB, nT, H)
    _check(_split(got, nB, nT, D), _reference(q, k, v, dO.view(nB, nT, D), [0, 70, 40], H, hd), [0, 70, 40], "klen 0")
    att = ops.attention_hd_qkv(qkv.cuda(), nB, nT, H)
    full = ops.attention_hd_qkv_bwd(qkv.cuda(), att, dO.cuda(), nB, nT, H)
    _check(_split(full, nB, nT, D), _reference(q, k, v, dO.view(nB, nT, D), [70, 70, 70], H, hd), [70, 70, 70], "klens NULL")
    clamped = ops.attention_hd_qkv_bwd(qkv.cuda(), att, dO.cuda(), nB, nT, H, _i32([999, 70, 71]))
    assert torch.equal(clamped, full)


def test_rows_that_take_no_part_may_hold_anything():
    """K / V rows >= klens[b] and Q / dO rows of queries that take no part are zeroed on load: NaN there changes nothing (full rows and Tq = 1)."""
    hd = 96
    D = H * hd
    qkv, dO = _full_inputs(hd, 9)
    clean = _full_run(qkv, dO, KLENS, B, T, H)
    qkv2, dO2 = qkv.clone(), dO.clone()
    for b, kl in enumerate(KLENS):
        qkv2[b * T + kl:(b + 1) * T] = float("nan")
        dO2[b * T + kl:(b + 1) * T] = float("nan")
    assert torch.equal(_full_run(qkv2, dO2, KLENS, B, T, H), clean)
    q, kv, d1 = _cls_inputs(hd, 10)
    a = _cls_run(q, kv, d1, hd, KLENS)
    kv2 = kv.clone()
    for b, kl in enumerate(KLENS):
        kv2[b * T + kl:(b + 1) * T] = float("nan")
    for x, y in zip(a, _cls_run(q, kv2, d1, hd, KLENS)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("hd", [96, 128])
def test_dropout_regenerates_the_forwards_mask(hd):
    """The same lengths, the single key included: there the kept probability is 1 / (1 - p), dq = dk = 0 analytically, and the bound is its absolute 1e-3."""
    D, drop = H * hd, (0.1, 424242)
    qkv, dO = _full_inputs(hd, 300 + hd)
    q, k, v = _split(qkv, B, T, D)
    kept = torch.cat([_keep(drop[1], b, h, H, np.arange(T), T, drop[0]).reshape(-1) for b in range(B) for h in range(H)]).mean().item()
    assert 0.88 < kept < 0.92, kept
    # the restated mask IS the forward's: the dropped forward against fp64 with that mask (the forward's own 2e-2 bound)
    from speechclip_amd import ops
    att = ops.attention_hd_qkv(qkv.cuda(), B, T, H, _i32(KLENS), drop_p=drop[0], seed=drop[1]).float().cpu().view(B, T, D)
    for b, kl in enumerate(KLENS):
        qh, kh, vh = (x[b, :kl].double().view(kl, H, hd).transpose(0, 1) for x in (q, k, v))
        p = torch.softmax((qh @ kh.transpose(-1, -2)) * hd ** -0.5, -1)
        p = p * torch.stack([_keep(drop[1], b, h, H, np.arange(kl), T, drop[0])[:, :kl] for h in range(H)]) / (1.0 - drop[0])
        assert (att[b, :kl].double() - (p @ vh).transpose(0, 1).reshape(kl, D)).abs().max().item() < 2e-2, b
    got = _full_run(qkv, dO, KLENS, B, T, H, drop)
    _check(_split(got, B, T, D), _reference(q, k, v, dO.view(B, T, D), KLENS, H, hd, drop), KLENS, f"dropout hd={hd}")
    other = _full_run(qkv, dO, KLENS, B, T, H, (drop[0], drop[1] + 1))
    assert not torch.equal(other, got)
    # Tq = 1 with the same rate
    qc, kv, d1 = _cls_inputs(hd, 400 + hd)
    kv3 = kv.view(B, T, 2 * D)
    _check(_cls_run(qc, kv, d1, hd, KLENS, drop), _reference(qc.view(B, 1, D), kv3[..., :D], kv3[..., D:], d1.view(B, 1, D), KLENS, H, hd, drop), KLENS,
           f"dropout Tq=1 hd={hd}")


def test_head_dim_64_beside_the_packed_kernel():
    """The uniform layout through sc_attention_bwd_packed and through sc_attention_hd_bwd: both meet the fp64 bound, and -- one kernel set behind both
    entries, without dropout the same statistics kernel -- they return bitwise equal dqkv."""
    from speechclip_amd import ops
    hd, D = 64, H * 64
    qkv, dO = _full_inputs(hd, 64)
    q, k, v = _split(qkv, B, T, D)
    ref = _reference(q, k, v, dO.view(B, T, D), KLENS, H, hd)
    kl = _i32(KLENS)
    att = ops.attention_hd_qkv(qkv.cuda(), B, T, H, kl)
    hd_out = ops.attention_hd_qkv_bwd(qkv.cuda(), att, dO.cuda(), B, T, H, kl)
    packed_out = ops.attention_bwd_packed(qkv.cuda(), att, dO.cuda(), B, T, H, kl, None)
    _check(_split(hd_out, B, T, D), ref, KLENS, "hd 64, sc_attention_hd_bwd")
    _check(_split(packed_out, B, T, D), ref, KLENS, "hd 64, sc_attention_bwd_packed")
    assert torch.equal(hd_out, packed_out)


@pytest.mark.parametrize("drop", [(0.0, 0), (0.1, 77)])
def test_two_runs_are_bitwise_equal(drop):
    qkv, dO = _full_inputs(128, 3)
    a, b = _full_run(qkv, dO, KLENS, B, T, H, drop), _full_run(qkv, dO, KLENS, B, T, H, drop)
    assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all())
    q, kv, d1 = _cls_inputs(96, 4)
    for x, y in zip(_cls_run(q, kv, d1, 96, KLENS, drop), _cls_run(q, kv, d1, 96, KLENS, drop)):
        assert torch.equal(x, y)


def test_unserved_combinations_raise():
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    z = lambda *s: torch.zeros(*s, dtype=BF).cuda()      # noqa: E731
    with pytest.raises(SpeechClipHipError, match="head_dim=80"):
        ops.attention_hd_bwd(z(8, 160), z(8, 160), z(8, 160), z(1, 8, 160), z(1, 8, 160), 1, 2, 8, 8, 80, (8 * 160, 160), (8 * 160, 160))
    with pytest.raises(SpeechClipHipError, match="Tq=7 Tk=40"):
        ops.attention_hd_bwd(z(7, 192), z(40, 192), z(40, 192), z(1, 7, 192), z(1, 7, 192), 1, 2, 7, 40, 96, (7 * 192, 192), (40 * 192, 192))
    with pytest.raises(SpeechClipHipError):          # no CPU fallback
        c = torch.zeros(8, 192, dtype=BF)
        ops.attention_hd_bwd(c, c, c, c.view(1, 8, 192), c.view(1, 8, 192), 1, 2, 8, 8, 96, (8 * 192, 192), (8 * 192, 192))


def test_empty_batch_returns_without_a_launch():
    import ctypes
    from speechclip_amd import _lib, ops
    L = _lib.lib()
    # null operands: a launch (or a look at them) would be an error
    rc = L.sc_attention_hd_bwd(None, None, None, None, None, None, 0, 2, 8, 8, 96, 0, 192, 0, 192, 0, 192, None, 0, 192, None, None, 0, 192,
                               ctypes.c_float(1.0), ctypes.c_float(0.0), 0, None, None)
    assert rc == 0
    rc = L.sc_attention_hd_bwd(None, None, None, None, None, None, 3, 2, 0, 0, 96, 0, 192, 0, 192, 0, 192, None, 0, 192, None, None, 0, 192,
                               ctypes.c_float(1.0), ctypes.c_float(0.0), 0, None, None)
    assert rc == 0
    assert L.sc_attention_hd_bwd_workspace_bytes(0, 2, 8) == 0
    out = ops.attention_hd_qkv_bwd(torch.zeros(0, 3 * 192, dtype=BF).cuda(), torch.zeros(0, 192, dtype=BF).cuda(), torch.zeros(0, 192, dtype=BF).cuda(), 0, 8, 2)
    assert out.shape == (0, 3 * 192)


def test_no_image_sized_temporary():
    """B = 2, H = 8, T = 500, head_dim 96: the call's peak memory above its inputs and its output stays below ONE bf16 [B*H, T, T] image; it is the
    statistics workspace the library asks for."""
    from speechclip_amd import _lib, ops
    nB, nH, nT, hd = 2, 8, 500, 96
    qkv, dO = _full_inputs(hd, 11, nB, nH, nT)
    qkv, dO = qkv.cuda(), dO.cuda()
    att = ops.attention_hd_qkv(qkv, nB, nT, nH)
    ops.attention_hd_qkv_bwd(qkv, att, dO, nB, nT, nH)           # warm: library load, kernel code objects
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.attention_hd_qkv_bwd(qkv, att, dO, nB, nT, nH)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before - out.numel() * 2
    image = nB * nH * nT * nT * 2
    ws = _lib.lib().sc_attention_hd_bwd_workspace_bytes(nB, nH, nT)
    print("peak above inputs and output:", extra, "bytes; workspace:", ws, "; one image:", image)
    assert ws == 2 * 4 * nB * nH * nT
    assert extra < image

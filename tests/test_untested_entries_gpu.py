"""Entry points of include/speechclip_hip.h that no other test reaches by name or through their `ops` wrapper -- sc_conv0_wgrad, sc_posconv_finish_train,
sc_posconv_pack, sc_attn_softmax_bwd_dropout, sc_split_hilo_bf16, sc_add_rows_f32 -- each against a plain fp64 (or exact) torch statement of the same
operation, and the argument forms of sc_attention_hd_fwd that no test passed: Tq != Tk with Tq > 1, bf16 output at Tq = 1, fp32 output at Tq > 128, a wide
output row stride into a sentinel-filled buffer, klens NULL / 0 / > Tk / < 0, a scale other than head_dim^-0.5, dropout at head_dim 64, and head_dim 64 against
the independent sc_attention_fwd kernel.

Tolerances are derived, not fitted: a bf16 store is half a bf16 ulp (2^-8 relative), an fp32 sum of n terms is within n 2^-24 sum|terms|; the attention
bound 2e-2 is the one tests/test_attention_hd_gpu.py and tests/test_kernels_gpu.py already hold the two kernels to against fp64."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HALF_ULP_BF16 = 2.0 ** -8 * 1.001          # round-to-nearest bf16 store, with room for the fp32 arithmetic in front of it


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


# ---------------------------------------------------------------------------------------------------------------- front-end gradient kernels
@pytest.mark.parametrize("B,L,C", [(2, 4000, 512), (3, 1235, 64), (1, 330, 128)])
def test_conv0_wgrad_vs_autograd_fp64(B, L, C):
    """dw[c, j] = sum_t du[t, c] wav[5 t + j], dbias[c] = sum_t du[t, c] over the T0 frames (T0 = 799 / 246 / 65: not multiples of the kernel's 4-frame step),
    against autograd of F.conv1d in fp64 on the same bf16 du.  Rows T0 .. P of du hold large values that must not be read.  Bound: the kernel adds T0 / 4 fp32
    products per wave and then four partial sums: |err| <= (T0 / 4 + 4) 2^-24 sum_t |du wav|."""
    from speechclip_amd import ops
    g = _g(L + C)
    T0 = (L - 10) // 5 + 1
    P = (T0 + 63) // 64 * 64
    assert T0 % 4 != 0 and P > T0
    wav = torch.randn(B, L, generator=g) * 0.3 + 0.1
    du = torch.randn(B, P, C, generator=g).to(BF)
    du[:, T0:] = 1e4
    dw, db, _ = ops.conv0_wgrad(wav.cuda(), du.cuda().view(B * P, C), C, T0, P)
    w = torch.zeros(C, 1, 10, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    gout = du[:, :T0].double().transpose(1, 2)
    F.conv1d(wav.double()[:, None], w, bias, stride=5).backward(gout)
    mag_w = F.conv1d(wav.double().abs()[:, None], torch.zeros(C, 1, 10, dtype=torch.float64, requires_grad=True), stride=5)
    wa = torch.zeros(C, 1, 10, dtype=torch.float64, requires_grad=True)
    F.conv1d(wav.double().abs()[:, None], wa, stride=5).backward(gout.abs())
    tol = (T0 / 4 + 4) * 2.0 ** -24
    assert mag_w.shape[-1] == T0
    err_w = (dw.double().cpu() - w.grad[:, 0]).abs()
    err_b = (db.double().cpu() - bias.grad).abs()
    assert (err_w <= tol * wa.grad[:, 0] + 1e-30).all(), (err_w.max().item(), (err_w / wa.grad[:, 0]).max().item(), tol)
    assert (err_b <= tol * gout.abs().sum((0, 2)) + 1e-30).all(), err_b.max().item()
    assert dw.abs().max().item() < 1e3                                                # the 1e4 rows past T0 were not read


@pytest.mark.parametrize("D,G,Kw,Tp,valid", [(768, 16, 128, 70, [69, 23]), (128, 4, 16, 33, [33, 1]), (1024, 16, 128, 65, [0, 64])])
def test_posconv_finish_train_both_outputs(D, G, Kw, Tp, valid):
    """u = bf16(conv + bias) regrouped from [B, G, Tp, D/G] to [B*Tp, D]; s = bf16(mask(x) + gelu(u)) with the erf GELU taken AT the bf16-rounded u (the backward
    differentiates it there); rows >= valid[b]: the same formulas with x read as zero (so s = gelu(u), u unchanged).  Each output is one bf16 store of an fp32 value."""
    from speechclip_amd import ops
    g = _g(D + Tp)
    B, cg = len(valid), D // G
    x = torch.randn(B, Tp, D, generator=g).to(BF)
    for b, v in enumerate(valid):
        x[b, v:] = 100.0                                                                # must be masked
    conv = (torch.randn(B, G, Tp, cg, generator=g) * 1.5).to(BF)
    bias = torch.randn(D, generator=g) * 0.3
    u, s = ops.posconv_finish_train(x.cuda().view(B * Tp, D), _i32(valid), conv.cuda(), bias.cuda(), B, Tp, D, G)
    u, s = u.cpu().view(B, Tp, D), s.cpu().view(B, Tp, D)
    u_ref = conv.double().permute(0, 2, 1, 3).reshape(B, Tp, D) + bias.double()
    assert ((u.double() - u_ref).abs() <= HALF_ULP_BF16 * u_ref.abs() + 1e-30).all()
    xm = x.double().clone()
    for b, v in enumerate(valid):
        xm[b, v:] = 0
    s_ref = xm + F.gelu(u.double())
    # + 1e-6 (1 + |u|): the kernel's erf is the A&S 7.1.26 form, |abs err| <= 1.5e-7, times |u| / 2, plus the fp32 exp / rcp in it
    assert ((s.double() - s_ref).abs() <= HALF_ULP_BF16 * s_ref.abs() + 1e-6 * (1 + u.double().abs())).all(), (s.double() - s_ref).abs().max().item()
    for b, v in enumerate(valid):
        assert (s[b, v:].double() - F.gelu(u[b, v:].double())).abs().max().item() < 0.02 if v < Tp else True      # rows >= valid: no trace of the 100.0 input


@pytest.mark.parametrize("D,G,Kw,Tp,valid", [(80, 4, 16, 30, [30, 7, 0]), (768, 16, 128, 37, [36, 1]), (96, 8, 6, 5, [5, 2])])
def test_posconv_pack_is_an_exact_copy_with_zero_fill(D, G, Kw, Tp, valid):
    """xg[b][g][Kw/2 + t][c] = t < valid[b] ? x[b][t][g*cg + c] : 0, rows [0, Kw/2) and [Kw/2 + Tp, Tp + Kw) zero: bitwise against an index-built tensor
    (D/G = 20 / 48 / 12: also widths the windowed kernel does not take, for which this layout feeds the batched GEMM)."""
    from speechclip_amd import ops
    g = _g(D + Tp)
    B, cg = len(valid), D // G
    x = torch.randn(B, Tp, D, generator=g).to(BF)
    xg = ops.posconv_pack(x.cuda().view(B * Tp, D), _i32(valid), B, Tp, D, G, Kw)
    got = xg[: B * G * (Tp + Kw) * cg].cpu().view(B, G, Tp + Kw, cg)
    want = torch.zeros(B, G, Tp + Kw, cg, dtype=BF)
    for b, v in enumerate(valid):
        want[b, :, Kw // 2: Kw // 2 + v] = x[b, :v].view(v, G, cg).permute(1, 0, 2)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("B,L,Lp,Tp,H,h,klens", [(2, 45, 64, 48, 3, 1, [45, 17]), (3, 130, 192, 130, 2, 0, [130, 1, 64]), (1, 64, 64, 70, 1, 0, [63])])
def test_attn_softmax_bwd_dropout_vs_fp64(B, L, Lp, Tp, H, h, klens):
    """P = m softmax(scale S) over keys < klens[z] and dS = scale P_undropped (m dP - dO_i . O_i), m = keep / (1 - p) from the forward's mask (row id (b*H + h)*L + i,
    one 16-bit half of a hash per key: tests/test_dropout_gpu.py restates it on the host); rows i >= L and keys >= klens[z] of the [Lp, Lp] images are zeros.
    fp32 arithmetic on O(1) values (|err| ~ 1e-6) followed by one bf16 store."""
    from speechclip_amd import ops
    from test_dropout_gpu import _keep_attn
    p, seed, scale = 0.1, 20240, 0.125
    g = _g(L + H)
    S = torch.randn(B, Lp, Lp, generator=g) * 6
    dP = torch.randn(B, Lp, Lp, generator=g)
    dO = (torch.randn(B * Tp, H * 64, generator=g) * 0.3).to(BF)
    O = (torch.randn(B * Tp, H * 64, generator=g) * 0.3).to(BF)
    dOc, Oc = dO.cuda(), O.cuda()
    P_k, dS_k = ops.attn_softmax_bwd(S.cuda(), dP.cuda(), dOc[:, h * 64:], H * 64, Oc[:, h * 64:], H * 64, Tp, _i32(klens), L, scale, drop=(p, seed, H, h))
    P_k, dS_k = P_k.cpu().double(), dS_k.cpu().double()
    m = _keep_attn(seed, B, H, L, p)[:, h].double() / (1 - p)                              # [B, L, L]
    P_ref, dS_ref = torch.zeros(B, Lp, Lp, dtype=torch.float64), torch.zeros(B, Lp, Lp, dtype=torch.float64)
    for b, kl in enumerate(klens):
        prob = torch.softmax(S[b, :L, :kl].double() * scale, -1)
        dd = (dO[b * Tp: b * Tp + L, h * 64: (h + 1) * 64].double() * O[b * Tp: b * Tp + L, h * 64: (h + 1) * 64].double()).sum(-1, keepdim=True)
        P_ref[b, :L, :kl] = prob * m[b, :, :kl]
        dS_ref[b, :L, :kl] = scale * prob * (m[b, :, :kl] * dP[b, :L, :kl].double() - dd)
    assert ((P_k - P_ref).abs() <= HALF_ULP_BF16 * P_ref.abs() + 2e-6).all(), (P_k - P_ref).abs().max().item()
    assert ((dS_k - dS_ref).abs() <= HALF_ULP_BF16 * dS_ref.abs() + 1e-5).all(), (dS_k - dS_ref).abs().max().item()
    assert (P_k == 0).float().mean().item() > 0.05 and P_ref.abs().max().item() > 0.1          # the mask is really applied
    plain, _ = ops.attn_softmax_bwd(S.cuda(), dP.cuda(), dOc[:, h * 64:], H * 64, Oc[:, h * 64:], H * 64, Tp, _i32(klens), L, scale)
    assert not torch.equal(plain.cpu().double(), P_k)


@pytest.mark.parametrize("M,K,ld,nblk", [(7, 512, 512, 2), (33, 68, 100, 3), (1, 4, 4, 2)])
def test_split_hilo_bf16(M, K, ld, nblk):
    """out [M, nblk K] = (hi | lo [| hi]): hi == bf16(a) and lo == bf16(a - hi) EXACTLY (round to nearest even, a - hi is exact in fp32), so
    |a - (hi + lo)| <= 2^-8 |a - hi| <= 2^-16 |a|; row stride of `a` larger than K."""
    from speechclip_amd import ops
    g = _g(M + K)
    a = (torch.randn(M, ld, generator=g) * torch.logspace(-6, 6, ld)[None]).cuda()[:, :K]
    out = ops.split_hilo(a, nblk).cpu()
    a = a.cpu()
    hi, lo = out[:, :K], out[:, K: 2 * K]
    assert torch.equal(hi, a.to(BF)) and torch.equal(lo, (a - hi.float()).to(BF))
    if nblk == 3:
        assert torch.equal(out[:, 2 * K:], hi)
    assert ((a.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * a.double().abs()).all()


@pytest.mark.parametrize("rows,cols,b_rows", [(9, 768, 9), (13, 100, 1), (12, 7, 4)])
def test_add_rows_f32_exact(rows, cols, b_rows):
    """out = alpha a + b[r % b_rows] as ONE fma: exact against torch for alpha = 1 and 0.5 (the product is exact, one rounding each), and the correctly rounded
    fp64 value for alpha = 0.3 (fp32(alpha) a is exact in fp64; the fp64 sum is rounded again, so allow the last fp32 bit)."""
    from speechclip_amd import ops
    g = _g(rows + cols)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(b_rows, cols, generator=g)
    bb = b[torch.arange(rows) % b_rows]
    for alpha in (1.0, 0.5):
        assert torch.equal(ops.add_rows(a.cuda(), b.cuda(), alpha).cpu(), alpha * a + bb)
    got = ops.add_rows(a.cuda(), b.cuda(), 0.3).cpu()
    want = float(torch.tensor(0.3, dtype=torch.float32)) * a.double() + bb.double()
    assert ((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all()


# ---------------------------------------------------------------------------------------------------------------- sc_attention_hd_fwd: the ABI forms
def _hd_call(q, k, v, out, klens, B, H, Tq, Tk, hd, q_st, kv_st, o_st, scale, drop_p=0.0, seed=0, out_f32=False):
    from speechclip_amd import _lib
    L = _lib.lib()
    rc = L.sc_attention_hd_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 0 if klens is None else klens.data_ptr(), B, H, Tq, Tk, hd,
                               q_st[0], q_st[1], kv_st[0], kv_st[1], o_st[0], o_st[1], scale, drop_p, seed, _lib.ATTN_HD_OUT_F32 if out_f32 else 0,
                               torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "sc_attention_hd_fwd")
    torch.cuda.synchronize()


def _hd_ref(q, k, v, klens, scale, mask=None):
    """q [B, Tq, H, hd], k / v [B, Tk, H, hd] -> fp64 [B, Tq, H*hd]; klens clamped to [0, Tk]; a sequence without keys gives zeros."""
    B, Tq, H, hd = q.shape
    Tk = k.shape[1]
    out = torch.zeros(B, Tq, H * hd, dtype=torch.float64)
    for b in range(B):
        kl = Tk if klens is None else max(0, min(Tk, int(klens[b])))
        if kl == 0:
            continue
        s = torch.einsum("qhd,khd->hqk", q[b].double(), k[b, :kl].double()) * scale
        p = torch.softmax(s, -1)
        if mask is not None:
            p = p * mask[b, :, :, :kl].double()
        out[b] = torch.einsum("hqk,khd->qhd", p, v[b, :kl].double()).reshape(Tq, H * hd)
    return out


def _hd_both_dtypes(q, k, v, klens, scale, drop_p=0.0, seed=0, pad_cols=0, guard_rows=0):
    """Runs the bf16 and the fp32 output forms on separate q / k|v tensors into sentinel-filled buffers [B, Tq + guard_rows, H*hd + pad_cols]; returns both outputs
    (sentinel columns / rows checked untouched here)."""
    B, Tq, H, hd = q.shape
    Tk = k.shape[1]
    D = H * hd
    qc = q.reshape(B, Tq, D).cuda().contiguous()
    kv = torch.cat([k.reshape(B, Tk, D), v.reshape(B, Tk, D)], -1).cuda().contiguous()
    kl = None if klens is None else _i32(klens)
    res = []
    for f32 in (False, True):
        buf = torch.full((B, Tq + guard_rows, D + pad_cols), 7.0, dtype=torch.float32 if f32 else BF, device="cuda")
        _hd_call(qc, kv, kv[:, :, D:], buf, kl, B, H, Tq, Tk, hd, (Tq * D, D), (Tk * 2 * D, 2 * D), ((Tq + guard_rows) * (D + pad_cols), D + pad_cols), scale,
                 drop_p, seed, f32)
        buf = buf.cpu()
        assert (buf[:, :, D:] == 7.0).all() and (buf[:, Tq:] == 7.0).all(), "wrote outside its [Tq, H*hd] block"
        res.append(buf[:, :Tq, :D])
    o16, o32 = res
    assert torch.equal(o16, o32.to(BF)), "bf16 output != fp32 output rounded to bf16"
    return o16, o32


def _rand_qkv(B, Tq, Tk, H, hd, seed):
    g = _g(seed)
    return (torch.randn(B, Tq, H, hd, generator=g).to(BF), torch.randn(B, Tk, H, hd, generator=g).to(BF), torch.randn(B, Tk, H, hd, generator=g).to(BF))


@pytest.mark.parametrize("hd", [64, 96, 128])
@pytest.mark.parametrize("Tq,Tk,klens", [(45, 300, [300, 77, 64]), (1, 301, [301, 1, 65]), (150, 150, [150, 149, 3]), (131, 70, [70, 33, 1])])
def test_attention_hd_tq_tk_forms_both_output_types(hd, Tq, Tk, klens):
    """Tq != Tk with Tq > 1 and not a multiple of 32 (45 queries on 300 keys; 131 on 70), bf16 output at Tq = 1, fp32 output at Tq > 128; the output row stride is
    wider than H*hd and the buffer has guard rows: nothing but the [Tq, H*hd] block is written; bf16 output == fp32 output rounded, bitwise."""
    B, H = 3, 2
    q, k, v = _rand_qkv(B, Tq, Tk, H, hd, Tq + Tk + hd)
    o16, o32 = _hd_both_dtypes(q, k, v, klens, hd ** -0.5, pad_cols=24, guard_rows=2)
    want = _hd_ref(q, k, v, klens, hd ** -0.5)
    assert (o32.double() - want).abs().max().item() < 2e-2 and (o16.double() - want).abs().max().item() < 2e-2


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_hd_klens_null_zero_clamped_and_scale(hd):
    """klens = NULL (all Tk keys); klens[b] = 0 and < 0 (no key: all-zero output rows), > Tk (clamped to Tk); a scale other than head_dim^-0.5."""
    B, H, Tq, Tk = 4, 2, 37, 100
    q, k, v = _rand_qkv(B, Tq, Tk, H, hd, hd)
    for scale in (hd ** -0.5, 0.07):
        o16, o32 = _hd_both_dtypes(q, k, v, None, scale)
        assert (o32.double() - _hd_ref(q, k, v, None, scale)).abs().max().item() < 2e-2
        klens = [0, Tk + 5, -3, 17]
        o16, o32 = _hd_both_dtypes(q, k, v, klens, scale)
        assert (o32.double() - _hd_ref(q, k, v, klens, scale)).abs().max().item() < 2e-2
        assert (o32[0] == 0).all() and (o32[2] == 0).all() and (o16[0] == 0).all() and (o16[2] == 0).all()
        full16, full32 = _hd_both_dtypes(q, k, v, [Tk] * B, scale)
        assert torch.equal(o32[1], full32[1])
    sharp = _hd_ref(q, k, v, None, hd ** -0.5)
    assert (sharp - _hd_ref(q, k, v, None, 0.07)).abs().max().item() > 5e-2          # the two scales are told apart at this bound


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,H,klens", [(2, 131, 3, [131, 70]), (3, 64, 12, [64, 1, 33])])
def test_attention_hd_head_dim_64_vs_fp64_and_vs_sc_attention_fwd(drop_p, B, T, H, klens):
    """head_dim 64 (with and without dropout, mask restated on the host) against fp64, and against sc_attention_fwd / sc_attention_fwd_dropout on the same q|k|v:
    two independent kernels that the header says share one dropout mask; each meets 2e-2 against fp64, so must their difference."""
    from speechclip_amd import ops
    from test_dropout_gpu import _keep_attn
    seed, D = 777, H * 64
    qkv = torch.randn(B * T, 3 * D, generator=_g(T + H)).to(BF)
    out = ops.attention_hd_qkv(qkv.cuda(), B, T, H, _i32(klens), drop_p=drop_p, seed=seed).float().cpu().view(B, T, D)
    x = qkv.view(B, T, 3, H, 64)
    mask = _keep_attn(seed, B, H, T, drop_p) / (1 - drop_p) if drop_p > 0 else None
    want = _hd_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], klens, 0.125, mask)
    assert (out.double() - want).abs().max().item() < 2e-2
    if drop_p > 0:
        assert (out.double() - _hd_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], klens, 0.125)).abs().max().item() > 5e-2
        twin = ops.attention_dropout(qkv.cuda(), B, T, H, _i32(klens), drop_p, seed)
    else:
        twin = ops.attention(qkv.cuda(), B, T, H, _i32(klens))
    twin = twin.float().cpu().view(B, T, D)
    for b, kl in enumerate(klens):            # sc_attention_fwd leaves query rows >= klens[b] to its caller (padded frames): compare the rows both define
        assert (out[b, :kl] - twin[b, :kl]).abs().max().item() < 2e-2

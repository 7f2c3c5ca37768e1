"""GPU: every row kernel of csrc/rowops.hip and the pooling head of csrc/attention.hip against the plain fp64 statements of tests/row_kernels_ref.py, element by
element, under bounds DERIVED there from the arithmetic (no element is excluded; tools/row_kernel_bounds.py is the CPU self-check of statements, bounds and mutants).
Every output lands in a sentinel-filled buffer and everything outside the written region must still hold the sentinel.  Each test prints, per case, the worst
err / bound and where it occurred (-s).

Which case reaches which code:
    sc_layernorm              layernorm768_kernel<false>      ln768                       layernorm512_kernel<false / true>   ln512 / ln512_gelu
                              layernorm1024f_kernel<false / true>  ln1024f / ln1024f_half  layernorm768f_kernel                ln768f
                              layernorm_kernel<bf16,bf16> gen_bf_bf-*, <bf16,f32> gen_bf_f32-*, <f32,bf16> gen_f32_bf-*, <f32,f32> gen_f32_f32-*, <f32,half> gen_f32_half-*
                              the fall-backs from a fast shape: gen_bf_bf-768-ld_in5x, gen_bf_bf-768-x_off4 (8- but not 16-byte aligned input), gen_bf_f32-512-out_f32,
                              gen_bf_bf-768-noaffine / -gelu / -ld_out, gen_f32_bf-1024-gelu, gen_f32_bf-768-ld_out; the 2- / 4-rows-per-wave and 8- / 16-rows-per-block tails:
                              rows 1 .. 33 of every fast case; partly filled 256-column chunks: D = 4 .. 1020
    sc_dropout_add_layernorm_bf16   layernorm768_kernel<true>      dropln768-p0.0 / -p0.1
    sc_weighted_sum_fwd       weighted_sum_kernel<false / true>    mix-*-bf16-* / mix-*-f32-*, normalize on (-norm) and off
    sc_l2norm_fwd             l2norm_kernel<false / true>          l2-*-bf16 / l2-*-f32 (l2-D260-*-slice: ld_in > D), clamp on a zero row
    sc_hidden_normalize       hidden_rownorm_kernel<bf16 / f32, MODE 1>   hn-*-method1;   <., MODE 0>, hidden_group_inv_mean_kernel, <., MODE 2>   hn-*-method2
    sc_wave_layernorm         wave_layernorm_kernel: the 16-byte path wave-ld8 / -ld4100 / -ld32772, the scalar path wave-ld5001
    sc_splitk_reduce_f32      splitk_reduce_kernel: splitk-*
    sc_cls_pool_fwd[_split]   cls_pool_kernel<DCH, SPLIT>: DCH 1 pool-NQ8-R8-D128-* and pool-NQ1-R1-D4-*, DCH 2 pool-NQ2-R8-D260-* (ld_x > D), DCH 3 pool-NQ1-R8-D768-*,
                              DCH 4 pool-NQ1-R4-D1024-*; SPLIT false [plain], true [split2] and [split3] of every case
    sc_cls_attention_fwd      cls_attn_kernel: one pass over hd clsattn-*-hd96 / -hd16 / -hd4, the hd > 256 loop clsattn-NQ2-H4-hd260-*, the hd > 512 loops
                              clsattn-NQ8-H1-hd768-* and clsattn-NQ1-H1-hd1024-*; the LDS layout at the headline length: every *-T499 case"""
import pytest
import torch

import row_kernels_ref as R

pytestmark = pytest.mark.gpu
F64, F32, BF, H16 = R.F64, R.F32, R.BF, R.H16
GUARD = R.GUARD


def _dev(t, dt):
    return t.to(F32).to(dt).cuda()


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


Guarded, _judge = R.Guarded, R.judge


def _strided_input(x64, dt, ld, off=0, col0=0):
    """x in columns col0 .. col0 + D of a [rows, ld] buffer whose other columns hold PAST_VALUE, the buffer starting `off` elements into its allocation"""
    rows, D = x64.shape
    flat = torch.full((off + rows * ld,), R.PAST_VALUE, dtype=dt, device="cuda")
    win = flat[off:off + rows * ld].view(rows, ld)
    win[:, col0:col0 + D] = _dev(x64, dt)
    return win[:, col0:col0 + D]


# ================================================================================================ sc_layernorm
def _run_ln(c, rows, x64, gamma, beta, inplace=False):
    from speechclip_amd import ops
    x = _strided_input(x64, c.in_dt, c.ld_in, c.x_off)
    g, b = (gamma.to(F32).cuda(), beta.to(F32).cuda()) if c.affine else (None, None)
    if inplace:
        ops.layernorm(x, g, b, R.LN_EPS, out=x, gelu=c.gelu)
        return x.cpu().to(F64)
    go = Guarded(rows, c.ld_out, c.out_dt, c.D)
    ops.layernorm(x, g, b, R.LN_EPS, out=go.out(), gelu=c.gelu)
    return go.check(c.id)


@pytest.mark.parametrize("c", R.ln_cases(), ids=lambda c: c.id)
def test_layernorm_every_dispatch_path(c):
    assert R.ln_dispatch(c) == c.path
    for rows in c.rows:
        x64, gamma, beta = R.ln_inputs(c, rows)
        got = _run_ln(c, rows, x64, gamma, beta)
        ref, _ = R.ln_ref(x64, gamma, beta, c.gelu)
        _judge(f"{c.id} rows={rows}", got, ref, R.ln_bound(x64, gamma, beta, c.gelu, c.out_dt, poly2=c.path == "ln512_gelu"))
        if c.out_dt != F32 and not c.gelu and rows >= 32:
            so = R.ln_scale_offset(got, x64, gamma, beta, c.out_dt)
            print(f"{c.id + ' rows=' + str(rows):60s} slope diff / allowance {so['slope_diff'] / so['slope_allow']:8.4f}   worst row offset / allowance "
                  f"{so['offset_ratio']:8.4f} (row {so['offset_row']})")
            assert so["slope_diff"] <= so["slope_allow"] and so["offset_ratio"] <= 1.0, (c.id, so)


@pytest.mark.parametrize("cid", ["ln512_gelu", "ln768", "gen_bf_bf-260-aff", "gen_f32_f32-772-aff"])
def test_layernorm_in_place_is_bit_identical(cid):
    c = {k.id: k for k in R.ln_cases()}[cid]
    assert c.in_dt == c.out_dt and c.ld_in == c.ld_out
    for rows in (1, 9, 33):
        x64, gamma, beta = R.ln_inputs(c, rows)
        assert torch.equal(_run_ln(c, rows, x64, gamma, beta, inplace=True), _run_ln(c, rows, x64, gamma, beta)), (cid, rows)


def test_layernorm_rejects_an_out_it_cannot_address():
    from speechclip_amd import ops
    x = torch.zeros(4, 256, device="cuda", dtype=BF)
    g = torch.ones(256, device="cuda")
    with pytest.raises(AssertionError):
        ops.layernorm(x, g, g, out=torch.empty(4, 512, device="cuda", dtype=BF)[:, ::2])          # last dim not contiguous
    with pytest.raises(AssertionError):
        ops.layernorm(x, g, g, out=torch.empty(5, 256, device="cuda", dtype=BF))                  # another row count


# ================================================================================================ sc_dropout_add_layernorm_bf16
@pytest.mark.parametrize("c", R.dln_cases(), ids=lambda c: c.id)
def test_dropout_add_layernorm_768(c):
    from speechclip_amd import ops
    for rows in c.rows:
        x64, res64, gamma, beta = R.dln_inputs(c, rows)
        go = Guarded(rows, 768, BF)
        ops.dropout_add_layernorm(_dev(x64, BF), _dev(res64, BF), gamma.to(F32).cuda(), beta.to(F32).cuda(), c.p, R.DLN_SEED, R.LN_EPS, out=go.out())
        v, dv = R.dln_sum(x64, res64, c.p, R.DLN_SEED)
        ref, _ = R.ln_ref(v, gamma, beta, False)
        _judge(f"{c.id} rows={rows}", go.check(c.id), ref, R.ln_bound(v, gamma, beta, False, BF, dx=dv))


# ================================================================================================ sc_weighted_sum_fwd
@pytest.mark.parametrize("c", R.ws_cases(), ids=lambda c: c.id)
def test_weighted_sum(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    for rows in c.rows:
        h64, w64 = R.ws_inputs(c, rows)
        h, w = _dev(h64, F32 if c.f32 else BF), w64.to(F32).cuda()
        go = Guarded(rows, c.D, BF)
        check(lib().sc_weighted_sum_fwd(ptr(h), rows * c.D, ptr(w), ptr(go.out()), c.n, rows, c.D, (1 if c.normalize else 0) | (2 if c.f32 else 0), R.LN_EPS, stream()), c.id)
        ref, pre = R.ws_ref(h64, w64, c.normalize)
        _judge(f"{c.id} rows={rows}", go.check(c.id), ref, pre + R.store_bound(ref, BF))


# ================================================================================================ sc_l2norm_fwd
@pytest.mark.parametrize("c", R.l2_cases(), ids=lambda c: c.id)
def test_l2norm(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    x64 = R.l2_inputs(c)
    dt = F32 if c.f32 else BF
    x = _strided_input(x64, dt, c.ld_in, col0=4 if c.ld_in > c.D else 0)
    go = Guarded(c.rows, c.D, F32)
    check(lib().sc_l2norm_fwd(ptr(x), x.stride(0), ptr(go.out()), c.rows, c.D, int(c.f32), stream()), c.id)
    ref = R.l2_ref(x64)
    _judge(c.id, go.check(c.id), ref, R.l2_bound(x64, ref))
    # clamp: the same rows within the same bound (no norm is near 1e-8), and an all-zero row gives exact zeros
    x64z = x64.clone()
    x64z[c.rows // 2] = 0
    xz = _strided_input(x64z, dt, c.ld_in, col0=4 if c.ld_in > c.D else 0)
    gz = Guarded(c.rows, c.D, F32)
    check(lib().sc_l2norm_fwd(ptr(xz), xz.stride(0), ptr(gz.out()), c.rows, c.D, int(c.f32) | 2, stream()), c.id)
    refz = R.l2_ref(x64z, 1e-8)
    got = gz.check(c.id)
    assert bool((got[c.rows // 2] == 0).all())
    _judge(c.id + " clamp", got, refz, R.l2_bound(x64z, refz))


# ================================================================================================ sc_hidden_normalize
@pytest.mark.parametrize("c", R.hn_cases(), ids=lambda c: c.id)
def test_hidden_normalize(c):
    """fp64 statement (R.hn_ref): method1 row / (||row|| + 1e-8); method2 row / mean_{t < T} ||x[layer, utterance, t]|| for ALL Tp rows of the pair"""
    from speechclip_amd import ops
    x64 = R.hn_inputs(c)
    dt = F32 if c.f32 else BF
    n = x64.numel()
    go = Guarded(1, n, dt)
    go.out().copy_(_dev(x64.reshape(1, n), dt))
    hidden = go.out().view(R.HN_N, R.HN_B, R.HN_TP, c.D)
    ops.hidden_normalize_(hidden, R.HN_T, c.method)
    nrm = x64.norm(dim=-1, keepdim=True)                                                     # the statement, written out: [n, B, Tp, 1] frame norms
    ref = x64 / (nrm + 1e-8) if c.method == "method1" else x64 / nrm[:, :, :R.HN_T].mean(2, keepdim=True)
    assert torch.equal(ref, R.hn_ref(x64, R.HN_T, c.method))                                # (the one tools/row_kernel_bounds.py checks against the oracle)
    _judge(c.id, go.check(c.id), ref, R.hn_bound(x64, ref, R.HN_T, c.method, c.f32))


# ================================================================================================ sc_wave_layernorm
@pytest.mark.parametrize("ld", R.WV_LDS)
def test_wave_layernorm(ld):
    from speechclip_amd._lib import lib, check, ptr, stream
    x64, lens = R.wv_inputs(ld)
    assert max(lens) <= ld
    B = len(lens)
    x = x64.to(F32).cuda()
    go = Guarded(B, ld, F32)
    check(lib().sc_wave_layernorm(ptr(x), ptr(go.out()), ptr(_i32(lens)), B, ld, R.LN_EPS, stream()), "sc_wave_layernorm")
    ref, bound, _ = R.wv_ref(x64, lens)
    got = go.check(f"wave-ld{ld}")
    for b, n in enumerate(lens):
        assert bool((got[b, n:] == 0).all()), (ld, b, n)
    _judge(f"wave-ld{ld} lens={lens}", got, ref, bound)


# ================================================================================================ sc_splitk_reduce_f32
@pytest.mark.parametrize("c", R.sk_cases(), ids=lambda c: c.id)
def test_splitk_reduce(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    part, bias, res, ldr = R.sk_inputs(c)
    dp, db, dr = part.to(F32).cuda(), (bias.to(F32).cuda() if bias is not None else None), (res.to(F32).cuda() if res is not None else None)
    go = Guarded(c.M, c.N, F32)
    check(lib().sc_splitk_reduce_f32(ptr(dp), c.S, c.M, c.N, ptr(db), ptr(dr), ldr, ptr(go.out()), 1 if c.gelu else 0, stream()), c.id)
    got = go.check(c.id)
    rmn = R.sk_res_view(res, c)
    ref, bound = R.sk_ref(part, bias, rmn, c.gelu)
    _judge(c.id, got, ref, bound)
    if not c.gelu:
        assert torch.equal(got.to(F32), R.sk_exact_f32(part, bias, rmn)), (c.id, "not the fixed-order fp32 sum")


# ================================================================================================ pooling head
@pytest.mark.parametrize("c", R.pool_cases(), ids=lambda c: c.id)
def test_cls_pool_plain_and_split(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    x64, cls64, s64, cs64 = R.pool_inputs(c)
    B = len(c.lens)
    x = _strided_input(x64.reshape(B * c.T, c.D), BF, c.ld_x, col0=4 if c.ld_x > c.D else 0)
    cls, s, cs, lens = _dev(cls64, BF), s64.to(F32).cuda().reshape(B * c.T, c.R).contiguous(), cs64.to(F32).cuda(), _i32(c.lens)
    ref, pre = R.pool_ref(c, x64, cls64, s64, cs64)
    go = Guarded(B * c.R, c.D, BF)
    check(lib().sc_cls_pool_fwd(ptr(x), x.stride(0), ptr(cls), ptr(s), ptr(cs), ptr(lens), ptr(go.out()), B, c.T, c.NQ, c.R, c.D, stream()), c.id)
    _judge(c.id + " [plain]", go.check(c.id), ref, R.pool_bound(ref, pre, False))
    for nblk in (2, 3):
        gs = Guarded(B * c.R, nblk * c.D, BF)
        check(lib().sc_cls_pool_fwd_split(ptr(x), x.stride(0), ptr(cls), ptr(s), ptr(cs), ptr(lens), ptr(gs.out()), B, c.T, c.NQ, c.R, c.D, nblk, stream()), c.id)
        blocks = gs.check(c.id).view(B, c.R, nblk, c.D)
        _judge(f"{c.id} [split{nblk}]", blocks[:, :, 0] + blocks[:, :, 1], ref, R.pool_bound(ref, pre, True))
        if nblk == 3:
            assert torch.equal(blocks[:, :, 2], blocks[:, :, 0]), (c.id, "block 3 is not block 1")


@pytest.mark.parametrize("c", R.attn_cases(), ids=lambda c: c.id)
def test_cls_attention(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    cq64, kv64 = R.attn_inputs(c)
    B, D = len(c.lens), c.H * c.hd
    cq, kv = _dev(cq64, BF), _dev(kv64.reshape(B * c.T, 2 * D), BF)
    go = Guarded(B * c.NQ, D, BF)
    check(lib().sc_cls_attention_fwd(ptr(cq), ptr(kv), 2 * D, ptr(_i32(c.lens)), ptr(go.out()), B, c.T, c.NQ, c.H, c.hd, c.hd ** -0.5, stream()), c.id)
    ref, pre = R.attn_ref(c, cq64, kv64)
    _judge(c.id, go.check(c.id), ref, pre + R.store_bound(ref, BF))

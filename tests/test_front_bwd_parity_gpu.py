"""GPU: the front-end BACKWARD kernels of csrc/train_front.hip through their padded and packed entries, and the host chains of speechclip_amd/train_front.py built on them,
against the plain fp64 statements of tests/front_bwd_ref.py: bit for bit where the inputs make every fp32 sum exact, element by element under bounds DERIVED there everywhere
else (no element is excluded; tools/front_bwd_bounds.py is the CPU self-check of statements, emulation, cap, bounds and mutants).  Operands sit between NaN (waves: PAST_VALUE
behind the last sample a frame may read; dy / du rows the layout does not hold: NaN), outputs in sentinel-filled guarded windows, and everything outside the written region
must still hold the sentinel.  Each test prints, per case, the worst err / bound and where it occurred, or the bitwise verdict (-s).  The first-generation tests of these
kernels (cosine / norm ratio against autograd, packed equals padded) stay where they are.

Which case reaches which code:
    sc_conv0_bwd            conv0_bwd_kernel<false>   c0b-C64-T1 / -T2 / -T3 (waves without a frame; T1: var = 0), -T4 / -T5 / -T7 (one or two frames per wave), -T64, -T1217,
                            -T4801; c0b-C128-*: blockIdx.x = 1; P > T0 with NaN alignment rows (all but -T4, -T64, -T4801); ld > L with PAST_VALUE behind the last sample;
                            utterances speech / dc / zero_tail / silent; c0b-long-C64-T31999: one block column, judged by the same bound plus the signed-error statistic
    sc_conv0_bwd_packed     conv0_bwd_kernel<true>    c0b-pk-geo (the tiny model's allotment 19 / 17 / 11 / 2 rows), c0b-pk-trap (19 / 9 / 11 / 2: hundreds of frames without
                            a gradient that still see samples), c0b-pk-full (row_scale rows_b = 1280 >= T0), c0b-pk-B1-C128, c0b-pk-C128-T7-scale4 (4 / 7 / 4 frames with a gradient)
    ops.conv0_bwd           the batch sums = sc_colsum's fixed-order sum of the partials, every c0b case
    sc_conv0_wgrad[_packed] conv0_wgrad_kernel<.>     c0w-*: the same T0 and packed edges with exact-integer operands, bit for bit, slot 11 zero
    sc_posconv_finish_train / sc_posconv_dgrad_finish / sc_reverse_rows_bf16 and their *_packed entries
                            <4, false> rows-D16-G4 (cg 4), rows-D24-G2 (cg 12); <8, false> rows-D64 / -D192 (cg 48) / -D768 / -D1024 -uniform; <8, true> rows-*-packed-B1 .. -B9
                            (every depth of the row_off search; one-row utterances first, inside and last; valid 0, 1, rows_b, above rows_b); no row count fills its last block
    sc_posconv_pack_gapped  posconv_pack_gapped_kernel    the packed rows-* cases: (x, valid, G, lead 2, gap 4, slab_rows + 5), (ds, rows, G = 1, lead 0), and gap = 0
    the argument rules      test_row_kernels_decline_what_they_do_not_cover: packed with D/G % 8 != 0, in-place reverse, slab_rows too small -> -1, nothing written
    adjoint chain           sc_reverse_rows[_packed]_bf16 -> sc_posconv_conv[_packed] on train_front._pos_operands' adjoint operand -> sc_posconv_dgrad_finish[_packed]:
                            adj-cg32 / 48 / 64 x Kw 2 / 3 / 16 x rows 1, Kw / 2, 70, 582 (three frame chunks) uniform (the pack + GEMM route where Kw D/G % 64 != 0); packed
                            where the windowed kernel takes the window (Kw D/G % 64 == 0), refused otherwise: test_packed_posconv_refuses_a_window_...
    posconv_wgrad           sc_posconv_pack -> sc_transpose_bf16 (rows_padded = Tq) -> sc_gemm_bf16_batched over S chunks -> sc_colsum: pw-*-uniform-B1 / 2 / 3 / 4 / 16 (S 1 / 2 / 1 / 4 /
                            16) x Tp 5 / 64 / 70 (Tq 64 / 64 / 128)
    posconv_wgrad_packed    sc_posconv_pack_gapped twice -> the same chain: pw-*-packed-B3-Rg511 .. -Rg2048 (S 1 / 1 / 1 / 2 / 2 / 4), -B1-Rg1024, a one-row utterance first,
                            du != 0 on rows [valid_b, rows_b); pw-real-*: the two real-valued cases
    conv_layer_backward     train_hubert.wgrad over the strided view + sc_gemm_bf16 per tap, tap s.. in place through residual == out: cl-k3s2-* (one overlapping tap, the last
                            output's tap 2 in slack row 0), cl-k2s2-* (none); rows_out 5 / 64 / 65; cl-real-*: the per-tap rounding model"""
import pytest
import torch

import front_bwd_ref as FB
import layer_kernels_ref as L
import row_kernels_ref as R

pytestmark = pytest.mark.gpu
F64, F32, BF = R.F64, R.F32, R.BF
Guarded, _judge = R.Guarded, R.judge
PAD = 64
NAN = float("nan")


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _op(t64, dt, fill=NAN):
    """an operand of the kernel's type between two runs of PAD NaN elements (16-byte aligned)"""
    n = t64.numel()
    buf = torch.full((2 * PAD + n,), fill, dtype=dt, device="cuda")
    buf[PAD:PAD + n] = t64.reshape(-1).to(F32).to(dt).cuda()
    return buf[PAD:PAD + n].view(t64.shape)


def _bitwise(what, got, want):
    got = got.reshape(want.shape)
    bad = got != want
    n = int(bad.sum())
    print(f"{what:60s} bitwise {'equal' if n == 0 else f'{n} of {want.numel()} elements differ'}")
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError((what, "differs at", i, "got", float(got[i]), "want", float(want[i]), "elements wrong", n))


def _wave(x64, ld):
    buf = torch.full((x64.shape[0], ld), R.PAST_VALUE, dtype=F32, device="cuda")
    buf[:, :x64.shape[1]] = x64.to(F32).cuda()
    return buf


def _grad_rows(c, g64):
    """g [B, T0, C] -> the bf16 device buffer of the layout (+ 8 slack rows): utterance b's frames t < tlim_b at its first row on, NaN everywhere else"""
    n, first = FB.c0b_dy_rows(c)
    buf = torch.full((n + 8, c.C), NAN, dtype=BF, device="cuda")
    for b, (r0, tl) in enumerate(zip(first, FB.c0b_tlim(c))):
        buf[r0:r0 + tl] = g64[b, :tl].to(F32).to(BF).cuda()
    return buf, n


def _off_dev(c):
    return _i32(FB.row_off(c.rows))


# ================================================================================================ 1. sc_conv0_bwd[_packed], ops.conv0_bwd
@pytest.mark.parametrize("c", FB.c0b_cases(), ids=lambda c: c.id)
def test_conv0_bwd(c):
    from speechclip_amd import ops
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = FB.c0b_inputs(c)
    B, ld = len(c.kinds), FB.conv0_L(c.T0) + c.pad
    wav = _wave(inp["x"], ld)
    w, gm, bt = _op(inp["w"], F32), _op(inp["gamma"], F32), _op(inp["beta"], F32)
    dy, n_rows = _grad_rows(c, inp["dy"])
    go = Guarded(B, c.C * 12, F32)
    if c.rows is None:
        check(lib().sc_conv0_bwd(ptr(wav), ld, ptr(w), ptr(gm), ptr(bt), ptr(dy), ptr(go.out()), B, c.C, c.T0, c.P, FB.EPS, stream()), c.id)
    else:
        check(lib().sc_conv0_bwd_packed(ptr(wav), ld, ptr(w), ptr(gm), ptr(bt), ptr(dy), ptr(go.out()), B, c.C, c.T0, ptr(_off_dev(c)), c.scale, FB.EPS, stream()), c.id)
    got = go.check(c.id).view(B, c.C, 12)
    ref, bound = FB.c0b_ref(c, inp)
    if c.cap:
        assert not FB.c0b_cap(ref, bound)[1], (c.id, FB.c0b_cap(ref, bound))
    _judge(f"{c.id} dw", got[..., :10], ref[..., :10], bound[..., :10])
    _judge(f"{c.id} dgamma", got[..., 10], ref[..., 10], bound[..., 10])
    _judge(f"{c.id} dbeta", got[..., 11], ref[..., 11], bound[..., 11])
    if not c.cap and c.T0 > 2:      # the long case: the signed-error statistic of the GEMM parity
        m, lim = FB.signed_stat(got, ref, bound)
        print(f"{c.id:60s} mean signed err/bound {m:+.5f} (limit {lim:.5f})")
        assert abs(m) <= lim, (c.id, m, lim)
    # the wrapper: the same partials, and batch sums in sc_colsum's fixed order
    P = c.P if c.rows is None else n_rows
    dw, dg, db, part = ops.conv0_bwd(wav, w, gm, bt, dy, c.T0, P, FB.EPS, None if c.rows is None else _off_dev(c), None if c.rows is None else c.scale)
    part = part.cpu()
    _bitwise(f"{c.id} ops.conv0_bwd partials", part.to(F64), got)
    tot = FB.c0b_batch_sum(part).to(F64)
    _bitwise(f"{c.id} ops.conv0_bwd batch sums", torch.cat([dw.cpu(), dg.cpu()[:, None], db.cpu()[:, None]], 1).to(F64), tot)


# ================================================================================================ 2. sc_conv0_wgrad[_packed], exact
@pytest.mark.parametrize("c", FB.c0w_cases(), ids=lambda c: "c0w-" + c.id)
def test_conv0_wgrad_exact(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    x64, du64, cond = FB.c0w_inputs(c)
    assert cond["worst"] < 2 ** 24
    B, ld = len(c.kinds), FB.conv0_L(c.T0) + c.pad
    wav = _wave(x64, ld)
    du, _ = _grad_rows(c, du64)
    go = Guarded(B, c.C * 12, F32)
    if c.rows is None:
        check(lib().sc_conv0_wgrad(ptr(wav), ld, ptr(du), ptr(go.out()), B, c.C, c.T0, c.P, stream()), c.id)
    else:
        check(lib().sc_conv0_wgrad_packed(ptr(wav), ld, ptr(du), ptr(go.out()), B, c.C, c.T0, ptr(_off_dev(c)), c.scale, stream()), c.id)
    _bitwise("c0w-" + c.id, go.check(c.id).view(B, c.C, 12), FB.c0w_ref(c, x64, du64))


# ================================================================================================ 3. the row kernels
def _row_operands(c, inp):
    return dict(x=_op(inp["x"], BF), ds=_op(inp["ds"], BF), slab=_op(inp["slab"], BF), bias=_op(inp["bias"], F32), valid=_i32(c.valid), off=_off_dev(c))


@pytest.mark.parametrize("c", FB.row_cases(), ids=lambda c: c.id)
def test_row_kernels_against_their_statements(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = FB.row_inputs(c)
    d = _row_operands(c, inp)
    B, total, Tp = len(c.rows), sum(c.rows), c.rows[0]
    # ---- finish_train
    gu, gs = Guarded(total, c.D, BF), Guarded(total, c.D, BF)
    if c.packed:
        check(lib().sc_posconv_finish_train_packed(ptr(d["x"]), ptr(d["valid"]), ptr(d["off"]), ptr(d["slab"]), ptr(d["bias"]), ptr(gu.out()), ptr(gs.out()), B, total, c.D, c.G,
                                                   stream()), c.id)
    else:
        check(lib().sc_posconv_finish_train(ptr(d["x"]), ptr(d["valid"]), ptr(d["slab"]), ptr(d["bias"]), ptr(gu.out()), ptr(gs.out()), B, Tp, c.D, c.G, stream()), c.id)
    u, s, bound = FB.finish_train_ref(c, inp)
    _bitwise(f"{c.id} finish_train u", gu.check(c.id), u)
    got_s = gs.check(c.id)
    _judge(f"{c.id} finish_train s", got_s, s, bound)
    if c.D >= 64:
        r, row, allow = L.slope_check(got_s, s, bound - R.BF_STORE * s.abs())
        print(f"{c.id:60s} finish_train s slope diff / allowance {r:8.4f} (row {row}, smallest allowance {allow:.2e})")
        assert r <= 1.0, (c.id, r, row)
    # ---- dgrad_finish
    gd = Guarded(total, c.D, BF)
    if c.packed:
        check(lib().sc_posconv_dgrad_finish_packed(ptr(d["slab"]), ptr(d["ds"]), ptr(d["valid"]), ptr(d["off"]), ptr(gd.out()), B, total, c.D, c.G, stream()), c.id)
    else:
        check(lib().sc_posconv_dgrad_finish(ptr(d["slab"]), ptr(d["ds"]), ptr(d["valid"]), ptr(gd.out()), B, Tp, c.D, c.G, stream()), c.id)
    _bitwise(f"{c.id} dgrad_finish", gd.check(c.id), FB.dgrad_finish_ref(c, inp))
    # ---- reverse
    gr = Guarded(total, c.D, BF)
    if c.packed:
        check(lib().sc_reverse_rows_packed_bf16(ptr(d["x"]), ptr(d["off"]), ptr(gr.out()), B, total, c.D, stream()), c.id)
    else:
        check(lib().sc_reverse_rows_bf16(ptr(d["x"]), ptr(gr.out()), B, Tp, c.D, stream()), c.id)
    _bitwise(f"{c.id} reverse_rows", gr.check(c.id), FB.reverse_ref(c, inp["x"]))
    if not c.packed:
        return
    # ---- pack_gapped: the window slab, the gradient's numbering, and no gap at all
    rows_d = _i32(c.rows)
    for what, src, lim, lim_d, G, gap, lead, extra in (("window", "x", c.valid, d["valid"], c.G, 4, 2, 5), ("gradient", "ds", c.rows, rows_d, 1, 4, 0, 0), ("gap0", "x", c.valid, d["valid"], c.G, 0, 0, 0)):
        n = lead + total + B * gap + extra
        gp = Guarded(G * n, c.D // G, BF)
        check(lib().sc_posconv_pack_gapped(ptr(d[src]), ptr(lim_d), ptr(d["off"]), ptr(gp.out()), B, total, c.D, G, gap, lead, n, stream()), c.id)
        _bitwise(f"{c.id} pack_gapped {what}", gp.check(c.id).view(G, n, c.D // G), FB.pack_gapped_ref(inp[src], lim, c.rows, G, gap, lead, n))


def test_row_kernels_decline_what_they_do_not_cover():
    """the argument rules: -1 and nothing written"""
    from speechclip_amd._lib import lib, ptr, stream
    c = next(k for k in FB.row_cases() if k.id.startswith("rows-D24-G2-uniform"))            # D/G = 12: the uniform entries take it, the packed ones must not
    inp = FB.row_inputs(c)
    d = _row_operands(c, inp)
    B, total = len(c.rows), sum(c.rows)
    g1, g2 = Guarded(total, c.D, BF), Guarded(total, c.D, BF)

    def untouched(*gs):
        return all(bool((g.buf.cpu().to(F64) == g.sent).all()) for g in gs)
    rc = lib().sc_posconv_finish_train_packed(ptr(d["x"]), ptr(d["valid"]), ptr(d["off"]), ptr(d["slab"]), ptr(d["bias"]), ptr(g1.out()), ptr(g2.out()), B, total, c.D, c.G, stream())
    assert rc == -1 and untouched(g1, g2), ("finish_train_packed, D/G = 12", rc)
    rc = lib().sc_posconv_dgrad_finish_packed(ptr(d["slab"]), ptr(d["ds"]), ptr(d["valid"]), ptr(d["off"]), ptr(g1.out()), B, total, c.D, c.G, stream())
    assert rc == -1 and untouched(g1), ("dgrad_finish_packed, D/G = 12", rc)
    rc = lib().sc_posconv_pack_gapped(ptr(d["x"]), ptr(d["valid"]), ptr(d["off"]), ptr(g1.out()), B, total, c.D, c.G, 0, 0, total, stream())
    assert rc == -1 and untouched(g1), ("pack_gapped, D/G = 12", rc)
    x20 = _op(torch.ones(total, 20, dtype=F64), BF)
    g20 = Guarded(total, 20, BF)
    rc = lib().sc_reverse_rows_packed_bf16(ptr(x20), ptr(d["off"]), ptr(g20.out()), B, total, 20, stream())
    assert rc == -1 and untouched(g20), ("reverse_rows_packed, D = 20", rc)
    # in-place reverse, either entry
    keep = d["x"].clone()
    rc = lib().sc_reverse_rows_bf16(ptr(d["x"]), ptr(d["x"]), B, c.rows[0], c.D, stream())
    assert rc == -1 and torch.equal(d["x"], keep), ("reverse in place", rc)
    c8 = next(k for k in FB.row_cases() if k.id == "rows-D64-G2-packed-B3")
    inp8 = FB.row_inputs(c8)
    d8 = _row_operands(c8, inp8)
    keep = d8["x"].clone()
    rc = lib().sc_reverse_rows_packed_bf16(ptr(d8["x"]), ptr(d8["off"]), ptr(d8["x"]), 3, sum(c8.rows), c8.D, stream())
    assert rc == -1 and torch.equal(d8["x"], keep), ("packed reverse in place", rc)
    # slab_rows one short of lead + total + B * gap
    t8 = sum(c8.rows)
    need = 2 + t8 + 3 * 4
    gp = Guarded(c8.G * need, c8.D // c8.G, BF)
    rc = lib().sc_posconv_pack_gapped(ptr(d8["x"]), ptr(d8["valid"]), ptr(d8["off"]), ptr(gp.out()), 3, t8, c8.D, c8.G, 4, 2, need - 1, stream())
    assert rc == -1 and untouched(gp), ("pack_gapped, slab_rows too small", rc)
    torch.cuda.synchronize()


# ================================================================================================ 4. the positional conv's adjoint chain
@pytest.mark.parametrize("c", FB.adj_cases(), ids=lambda c: c.id)
def test_posconv_adjoint_chain_exact(c):
    from speechclip_amd import ops, train_front as TF
    inp = FB.adj_inputs(c)
    want, worst = FB.adj_ref(c, inp)
    assert worst < 2 ** 24
    D, B, total = c.G * c.cg, len(c.rows), sum(c.rows)
    du, ds = _op(inp["du"], BF), _op(inp["ds"], BF)
    _, wg_adj = TF._pos_operands(inp["wfold"].to(F32).cuda().contiguous(), c.G, c.Kw)
    if c.packed:
        lay = TF.Layout(B, 1, total, max(c.rows), _off_dev(c), 0, 0)
    else:
        lay = TF.Layout(B, B, c.rows[0], c.rows[0], None, 0, 0)
    rows_b = _i32(c.rows)
    convT = TF._posconv(lay, ops.reverse_rows_bf16(du, B, lay.rows, D, lay.off), rows_b, wg_adj, D, c.G, c.Kw)
    dx = ops.posconv_dgrad_finish(convT, ds, _i32(c.valid), B, lay.rows, D, c.G, lay.off)
    _bitwise(c.id, dx.cpu().to(F64), want)


@pytest.mark.parametrize("cg,Kw", FB.ADJ_PACKED_DECLINED)
def test_packed_posconv_refuses_a_window_the_windowed_kernel_does_not_take(cg, Kw):
    """Kw D/G % 64 != 0: sc_posconv_conv_packed returns 1 with nothing written, and the wrapper raises instead of falling back"""
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError, lib, ptr, stream
    D, rows = 2 * cg, (3, 1)
    x = _op(torch.ones(sum(rows), D, dtype=F64), BF)
    wg = _op(torch.ones(2, cg, Kw * cg, dtype=F64), BF)
    go = Guarded(sum(rows), D, BF)
    rc = lib().sc_posconv_conv_packed(ptr(x), ptr(_i32(rows)), ptr(_i32(FB.row_off(rows))), ptr(wg), ptr(go.out()), 2, max(rows), D, 2, Kw, stream())
    assert rc == 1 and bool((go.buf.cpu().to(F64) == go.sent).all()), (cg, Kw, rc)
    with pytest.raises(SpeechClipHipError, match="multiple of 64"):
        ops.posconv_conv_packed(x, _i32(rows), _i32(FB.row_off(rows)), wg, 2, max(rows), sum(rows), D, 2, Kw)


# ================================================================================================ 5. posconv_wgrad / posconv_wgrad_packed
@pytest.mark.parametrize("c", FB.pw_cases(), ids=lambda c: c.id)
def test_posconv_wgrad(c):
    from speechclip_amd import train_front as TF
    inp = FB.pw_inputs(c)
    D, B, total = c.G * c.cg, len(c.rows), sum(c.rows)
    du, x, valid = _op(inp["du"], BF), _op(inp["x"], BF), _i32(c.valid)
    if c.packed:
        dW = TF.posconv_wgrad_packed(du, x, valid, _i32(c.rows), _off_dev(c), B, total, D, c.G, c.Kw)
    else:
        dW = TF.posconv_wgrad(du, x, valid, B, c.rows[0], D, c.G, c.Kw)
    assert dW.dtype == F32 and tuple(dW.shape) == (D, c.cg, c.Kw)
    sp = FB.pw_split(c)
    what = f"{c.id} S {sp['S']} K rows {sp['M']}"
    want = FB.pw_ref(c, inp)
    if c.real:
        _judge(what, dW.cpu().to(F64), want, FB.pw_bound(c, inp))
    else:
        assert float(FB.pw_ref(c, inp, absolute=True).max()) < 2 ** 24
        _bitwise(what, dW.cpu().to(F64), want)


# ================================================================================================ 6. conv_layer_backward
@pytest.mark.parametrize("c", FB.cl_cases(), ids=lambda c: c.id)
def test_conv_layer_backward(c):
    from speechclip_amd import train_front as TF
    inp = FB.cl_inputs(c)
    xin, du = _op(inp["xin"], BF), _op(inp["du"], BF)
    w = inp["w"].to(F32).cuda().contiguous()
    dW, dX = TF.conv_layer_backward(xin, w, du, c.B, c.rows_out, c.dim, c.k, c.s, c.C)
    assert tuple(dW.shape) == (c.dim, c.C, c.k) and tuple(dX.shape) == tuple(inp["xin"].shape)
    dW, dX = dW.cpu().to(F64), dX.cpu().to(F64)
    if c.real:
        rX, bX, rW, bW, _ = FB.cl_real_bound(c, inp)
        _judge(f"{c.id} dX (whole buffer)", dX, rX, bX)
        _judge(f"{c.id} dW", dW, rW, bW)
        return
    ref = FB.cl_ref(c, inp)
    assert ref["worst"] <= 256, ref["worst"]
    _bitwise(f"{c.id} dX (whole buffer, slack rows included)", dX, ref["dX"])
    _bitwise(f"{c.id} dW", dW, ref["dW"])

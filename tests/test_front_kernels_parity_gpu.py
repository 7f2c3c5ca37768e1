"""GPU: the front-end forward kernels of csrc/frontend.hip and csrc/posconv.hip through their padded entries, against the plain fp64 statements of
tests/front_kernels_ref.py: bit for bit where the inputs make every product and fp32 sum exact, element by element under bounds DERIVED there everywhere else (no element
is excluded; tools/front_kernel_bounds.py is the CPU self-check of statements, bounds and mutants).  Every output lands in a sentinel-filled buffer and everything outside
the written region must still hold the sentinel.  Each test prints, per case, the worst err / bound and where it occurred, or the bitwise verdict (-s).  No environment
switch is set: every path is chosen by shape alone.

Which case reaches which code:
    sc_conv0_gn_coef      conv0_stats_kernel + conv0_coef_kernel    gn-T1 .. gn-T17 (one partly filled split), gn-T4097 (the thread's stride loop runs twice), gn-T31999 (10 s:
                          the longest fp32 partial sum); gn-T17-C264 (the channel loop runs twice); -ld: ld > L, odd pitch; utterance 3 zero tail, utterance 4 silent (var = 0)
    sc_conv0_fwd          conv0_fwd_kernel (VALU)          mode 0 c0-valu-m0-*, mode 1 c0-valu-m1-* and c0x-valu-* (bitwise); C 8 (one live lane), 72 (a half-dead wave), 512, 64 with P % 64 != 0
                          conv0_mfma_kernel<512>           mode 0 c0-mfma-m0-*, mode 1 c0-mfma-m1-* and c0x-mfma-* (bitwise: -xlo the x_lo . w_hi slots, -wlo the x_hi . w_lo slots,
                          with and without a bias), mode 2 c0-mfma-m2-*; 1 / 2 / 3 / 7 / 8 channel chunks (the acc ping-pong, the prefetch guard): C 64 / 128 / 192 / 448 / 512; a partly
                          dead group -T49-P64, a whole dead block of groups -T64-P128, a second frame block with nfr = 64 -T570-P576; c0-mfma-m0-C64-T31999-P32000: 63 frame blocks
    sc_posconv_conv       posconv_mfma_kernel<2, 4> pcx-cg32-*-Tp70 / -Tp582, <2, 8> pcx-cg32-*-Tp500 / -Tp812, <3, 4> pcx-cg48-*-Tp70 / -Tp582 (waves 0-1 issue two DMAs, 2-3 one),
                          <3, 8> pcx-cg48-*-Tp500 / -Tp812 (waves 6-7 issue none), <4, 4> pcx-cg64-*-Tp70 / -Tp582, <4, 8> pcx-cg64-*-Tp500 / -Tp812; ring corners nk = 1 -cg32-Kw2 and
                          -cg64-Kw1, nk = 2 -cg32-Kw4, nk = 3 -cg48-Kw4 and -cg64-Kw3, nk = 4 -cg64-Kw4, long -Kw16 and the real -Kw128-G16; t_start > 0: -Tp582 (three chunks), -Tp812 (two);
                          valid 0, 1, Tp, above Tp, and either side of the chunk boundary; the return code 1: test_posconv_conv_declines_what_it_does_not_cover
    sc_posconv_finish     posconv_finish_kernel<false / true, 64> finish-D192-G3-* / finish-D1024-G16-*, <., 48> finish-D192-G4-* / finish-D768-G16-*, <., 0> finish-D80-G4-* (cg 20),
                          finish-D192-G6-* / finish-D1024-G32-* (cg 32), finish-D1020-G51-* (cg 20); -bf16 / -f32 the first argument; -ln: gamma given; 21 rows (not a multiple of 4)
    ops.posconv_conv      the pack + GEMM route bit for bit: pcx-pack-D64 (as it is), pcx-pack-D80 (D/G 20 -> 24, K 144 -> 192), pcx-pack-D272 (D/G 68 -> 72, K 432 -> 448)
    ops.posconv           the windowed route posconv-768-16-128-Tp70 / posconv-1024-16-128-Tp70; sc_posconv_pack + the batched GEMM posconv-64-4-16-Tp30 / posconv-272-4-6-Tp33
    sc_posconv_pack       posconv_pack_kernel   test_posconv_pack_is_an_exact_copy (cg 4, 20, 68)
    sc_vit_patchify       vit_patchify_kernel   test_vit_patchify_is_bitwise (p 32 / 14 with Kpad > K / 16)
    sc_vit_embed          vit_embed_kernel      embed-D4 .. embed-D1024, ntok 5 / 10 (15 / 30 rows)
    sc_image_normalize_u8 image_normalize_kernel    test_image_normalize_every_byte_value
    sc_crop_pad           crop_pad_kernel       test_crop_pad_is_an_exact_copy"""
import pytest
import torch

import front_kernels_ref as K
import row_kernels_ref as R

pytestmark = pytest.mark.gpu
F64, F32, BF = R.F64, R.F32, R.BF
Guarded, _judge = R.Guarded, R.judge


def _dev(t, dt):
    return t.to(F32).to(dt).cuda()


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _bitwise(what, got, want):
    got = got.reshape(want.shape)
    bad = got != want
    n = int(bad.sum())
    print(f"{what:60s} bitwise {'equal' if n == 0 else f'{n} of {want.numel()} elements differ'}")
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError((what, "differs from bf16(exact) at", i, "got", float(got[i]), "want", float(want[i]), "elements wrong", n))


def _wave(x64, ld):
    """x [B, L] in a [B, ld] fp32 buffer whose other columns hold PAST_VALUE"""
    buf = torch.full((x64.shape[0], ld), R.PAST_VALUE, dtype=F32, device="cuda")
    buf[:, :x64.shape[1]] = _dev(x64, F32)
    return buf


# ================================================================================================ sc_conv0_gn_coef
@pytest.mark.parametrize("c", K.gn_cases(), ids=lambda c: c.id)
def test_conv0_gn_coef(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    x64, w64, gamma, beta, offs = K.gn_inputs(c)
    B, L = x64.shape
    wav = _wave(x64, L + c.pad)
    ws = torch.empty(lib().sc_conv0_stats_workspace_bytes(B), device="cuda", dtype=torch.uint8)
    go = Guarded(B, 2 * c.C, F32)
    w, g, b = _dev(w64, F32), _dev(gamma, F32), _dev(beta, F32)
    check(lib().sc_conv0_gn_coef(ptr(wav), L + c.pad, ptr(w), ptr(g), ptr(b), ptr(ws), ptr(go.out()), B, c.C, c.T0, K.EPS, stream()), c.id)
    got = go.check(c.id).view(B, c.C, 2)
    ref = K.gn_ref(x64, w64, gamma, beta, c.T0)
    assert float(ref["rel"].max()) < K.GN_REL_CAP
    _judge(f"{c.id} scale (offsets {offs[1]:g} / {offs[2]:g} sd)", got[..., 0], ref["scale"], ref["b_scale"])
    _judge(f"{c.id} shift", got[..., 1], ref["shift"], ref["b_shift"])


# ================================================================================================ sc_conv0_fwd
def _run_conv0(C, T0, P, mode, x64, ld, L, w64, bias=None, coef=None):
    """-> fp64 [B, P, C]; the 8 slack rows behind the output are part of the guard"""
    from speechclip_amd._lib import lib, check, ptr, stream
    B = x64.shape[0]
    wav, w = _wave(x64, ld), _dev(w64, F32)
    go = Guarded(B * P + 8, C, BF)
    wfrag = torch.empty(lib().sc_conv0_wfrag_workspace_bytes(B), device="cuda", dtype=torch.uint8)
    check(lib().sc_conv0_fwd(ptr(wav), ld, L, ptr(w), ptr(bias), ptr(coef), ptr(go.out()), B, C, T0, P, mode, ptr(wfrag), stream()), "sc_conv0_fwd")
    full = go.check("sc_conv0_fwd")
    assert bool((full[B * P:] == go.sent).all()), "the 8 slack rows were written"
    return full[:B * P].view(B, P, C)


@pytest.mark.parametrize("c", K.c0_cases(), ids=lambda c: c.id)
def test_conv0_fwd(c):
    x64, w64, p = K.c0_inputs(c)
    L = x64.shape[1]
    if c.mode == 0:
        bias, coef = None, torch.stack([p["scale"], p["shift"]], -1).to(F32).cuda().contiguous()
    else:
        bias = _dev(p["bias"], F32) if p["bias"] is not None else None
        coef = torch.cat([p["gamma"], p["beta"], torch.tensor([K.EPS], dtype=F64)]).to(F32).cuda() if c.mode == 2 else None
    got = _run_conv0(c.C, c.T0, c.P, c.mode, x64, L + c.pad, L, w64, bias, coef)
    ref, bound = K.c0_ref(c, x64, w64, p)
    _judge(c.id, got, ref, bound)


@pytest.mark.parametrize("c", K.c0x_cases(), ids=lambda c: c.id)
def test_conv0_fwd_exact(c):
    x64, w64, bias, cond = K.c0x_inputs(c)
    assert cond["worst"] < 2 ** 24
    L = x64.shape[1]
    got = _run_conv0(c.C, c.T0, c.P, 1, x64, L, L, w64, _dev(bias, F32) if bias is not None else None)
    _bitwise(c.id, got, K.c0x_ref(c, x64, w64, bias))


def test_conv0_silent_utterance_end_to_end():
    """ops.conv0 (statistics and forward together): var = 0, scale = gamma / sqrt(eps), the output is gelu(beta) in every live frame"""
    from speechclip_amd import ops
    c = next(k for k in K.c0_cases() if k.id == "c0-mfma-m0-C128-T49-P64")
    x64, w64, p = K.c0_inputs(c)
    x64 = x64[:, :K.conv0_L(c.T0)].clone()
    out = ops.conv0(_dev(x64, F32), _dev(w64, F32), c.T0, c.P, gn_gamma=_dev(R.rnd(torch.ones(c.C, dtype=F64) * 1.25, F32), F32), gn_beta=_dev(p["beta"], F32), eps=K.EPS)
    got = out[:3 * c.P].view(3, c.P, c.C)[2].cpu().to(F64)
    ref = K._pad_frames(R.gelu64(p["beta"]).expand(1, c.T0, c.C), c.P)[0]
    live = (torch.arange(c.P) < c.T0).view(-1, 1)
    _judge("conv0 silent utterance = gelu(beta)", got, ref, (R.GELU_POLY2_ABS + R.GELU_POLY2_REL * ref.abs() + R.GELU_LIP * (K.SPLIT + 3 * R.U) * p["beta"].abs()) * live)


# ================================================================================================ sc_posconv_conv
def _run_posconv_conv(B, Tp, D, G, Kw, x64, valid, wg64):
    from speechclip_amd._lib import lib, ptr, stream
    cg = D // G
    go = Guarded(B * G * Tp, cg, BF)
    x, v, wg = _dev(x64, BF), _i32(valid), _dev(wg64, BF)
    rc = lib().sc_posconv_conv(ptr(x), ptr(v), ptr(wg), ptr(go.out()), B, Tp, D, G, Kw, stream())
    return rc, go


@pytest.mark.parametrize("c", K.pcx_cases(), ids=lambda c: c.id)
def test_posconv_conv_exact(c):
    D = c.G * c.cg
    x64, wg64 = K.pcx_inputs(c)
    want, mag = K.pc_conv64(x64, c.valid, wg64, c.B, c.Tp, D, c.G, c.Kw)
    assert float(mag.max()) < 2 ** 24
    rc, go = _run_posconv_conv(c.B, c.Tp, D, c.G, c.Kw, x64, c.valid, wg64)
    assert rc == 0, (c.id, rc)
    path = K.pc_path(c)
    _bitwise(f"{c.id} <{path['NJ']}, {path['NW']}> nk {path['nk']} chunks {path['chunks']}", go.check(c.id).view(c.B, c.G, c.Tp, c.cg), K.bits(want))


@pytest.mark.parametrize("c", K.pcx_pack_cases(), ids=lambda c: c.id)
def test_posconv_conv_pack_route_exact(c):
    """ops.posconv_conv where the windowed kernel declines: sc_posconv_pack + the batched GEMM, the group widened to a multiple of 8 channels and the window to a multiple of
    64 with zeros (D/G = 20, 68; Kw D/G = 144, 432) -- the same integers, the same bits"""
    from speechclip_amd import ops
    D = c.G * c.cg
    x64, wg64 = K.pcx_inputs(c)
    want, mag = K.pc_conv64(x64, c.valid, wg64, c.B, c.Tp, D, c.G, c.Kw)
    assert float(mag.max()) < 2 ** 24
    got = ops.posconv_conv(_dev(x64, BF), _i32(c.valid), _dev(wg64, BF), c.B, c.Tp, D, c.G, c.Kw)
    _bitwise(c.id, got.cpu().to(F64).view(c.B, c.G, c.Tp, c.cg), K.bits(want))


@pytest.mark.parametrize("D,G,Kw", K.PC_FALLBACK)
def test_posconv_conv_declines_what_it_does_not_cover(D, G, Kw):
    x64 = torch.ones(2 * 9, D, dtype=F64)
    rc, go = _run_posconv_conv(2, 9, D, G, Kw, x64, (9, 4), torch.ones(G, D // G, Kw * (D // G), dtype=F64))
    assert rc == 1, (D, G, Kw, rc)
    assert bool((go.buf.cpu().to(F64) == go.sent).all()), "wrote although it returned 1"


# ================================================================================================ sc_posconv_pack, sc_posconv_finish, ops.posconv
def test_posconv_pack_is_an_exact_copy():
    from speechclip_amd._lib import lib, check, ptr, stream
    for D, G, Kw, Tp, valid in K.PACK_CASES:
        x64 = R.rnd(torch.randn(2 * Tp, D, generator=R.gen("pack", D), dtype=F64), BF)
        go = Guarded(2 * G * (Tp + Kw), D // G, BF)
        x, v = _dev(x64, BF), _i32(valid)
        check(lib().sc_posconv_pack(ptr(x), ptr(v), ptr(go.out()), 2, Tp, D, G, Kw, stream()), "sc_posconv_pack")
        _bitwise(f"pack D{D} G{G} Kw{Kw} Tp{Tp}", go.check("pack").view(2, G, Tp + Kw, D // G), K.pack_ref(x64, valid, 2, Tp, D, G, Kw))


@pytest.mark.parametrize("c", K.pf_cases(), ids=lambda c: c.id)
def test_posconv_finish(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    B, Tp = K.PF_B, K.PF_TP
    dt = F32 if c.f32 else BF
    x64, cv64, bias, gamma, beta = K.pf_inputs(c.id, B, Tp, c.D, c.G, c.affine)
    g, b = (_dev(gamma, F32), _dev(beta, F32)) if c.affine else (None, None)
    go = Guarded(B * Tp, c.D, dt)
    x, v, cv, bi = _dev(x64, BF), _i32(K.PF_VALID), _dev(cv64, BF), _dev(bias, F32)
    check(lib().sc_posconv_finish(ptr(x), ptr(v), ptr(cv), ptr(bi), ptr(g), ptr(b), ptr(go.out()), B, Tp, c.D, c.G,
                                  int(c.f32), K.EPS, stream()), c.id)
    ref, bound = K.pf_ref(x64, K.PF_VALID, cv64, bias, gamma, beta, B, Tp, c.D, c.G, dt)
    _judge(c.id, go.check(c.id), ref, bound)


@pytest.mark.parametrize("c", K.E2E, ids=lambda c: c.id)
def test_posconv_end_to_end(c):
    from speechclip_amd import ops
    from speechclip_amd._lib import lib, ptr, stream
    x64, wg64, bias, gamma, beta = K.e2e_inputs(c)
    x, wg, valid = _dev(x64, BF), _dev(wg64, BF), _i32(c.valid)
    probe = torch.empty(2 * c.Tp * c.D, device="cuda", dtype=BF)
    assert lib().sc_posconv_conv(ptr(x), ptr(valid), ptr(wg), ptr(probe), 2, c.Tp, c.D, c.G, c.Kw, stream()) == (0 if c.route == "window" else 1)
    go = Guarded(2 * c.Tp, c.D, BF)
    ops.posconv(x, valid, wg, _dev(bias, F32), _dev(gamma, F32), _dev(beta, F32), 2, c.Tp, c.D, c.G, c.Kw, out=go.out(), eps=K.EPS)
    ref, bound = K.e2e_ref(c, x64, wg64, bias, gamma, beta)
    _judge(c.id, go.check(c.id), ref, bound)


# ================================================================================================ ViT stem
def test_vit_patchify_is_bitwise():
    from speechclip_amd._lib import lib, check, ptr, stream
    for p, Rr, Kpad in K.PT_CASES:
        img64 = K.pt_inputs(p, Rr)
        rows = 2 * (Rr // p) ** 2
        go = Guarded(rows, Kpad, BF)
        img = _dev(img64, F32)
        check(lib().sc_vit_patchify(ptr(img), ptr(go.out()), 2, Rr, p, Kpad, stream()), "sc_vit_patchify")
        _bitwise(f"patchify p{p} R{Rr} Kpad{Kpad}", go.check("patchify"), K.pt_ref(img64, p, Kpad))


@pytest.mark.parametrize("ntok", K.VE_NTOK)
@pytest.mark.parametrize("D", K.VE_D)
def test_vit_embed(D, ntok):
    from speechclip_amd._lib import lib, check, ptr, stream
    patch, cls, pos, gamma, beta = K.ve_inputs(D, ntok)
    go = Guarded(K.VE_B * ntok, D, F32)
    dev = [_dev(patch, BF)] + [_dev(t, F32) for t in (cls, pos, gamma, beta)]
    check(lib().sc_vit_embed(*[ptr(t) for t in dev], ptr(go.out()), K.VE_B, ntok, D, K.EPS, stream()), "sc_vit_embed")
    got = go.check("embed")
    ref, bound = K.ve_ref(patch, cls, pos, gamma, beta, ntok)
    rows = torch.arange(K.VE_B * ntok) % ntok == 0
    _judge(f"embed-D{D}-ntok{ntok} class rows", got[rows], ref[rows], bound[rows])
    _judge(f"embed-D{D}-ntok{ntok} patch rows", got[~rows], ref[~rows], bound[~rows])


# ================================================================================================ image normalize, crop + pad
@pytest.mark.parametrize("which", (0, 1), ids=("clip", "other"))
def test_image_normalize_every_byte_value(which):
    from speechclip_amd._lib import lib, check, ptr, stream
    mean, std = K.IN_STATS[which]
    u8 = K.in_inputs()
    u8d = u8.cuda()
    B, H, W = K.IN_HW
    go = Guarded(B * 3, H * W, F32)
    m, s = torch.tensor(mean, dtype=F32), torch.tensor(std, dtype=F32)            # host pointers
    check(lib().sc_image_normalize_u8(ptr(u8d), ptr(go.out()), B, H, W, m.data_ptr(), s.data_ptr(), stream()), "sc_image_normalize_u8")
    ref, bound = K.in_ref(u8, mean, std)
    _judge(f"normalize-{which}", go.check("normalize").view(B, 3, H, W), ref, bound)


def test_crop_pad_is_an_exact_copy():
    from speechclip_amd._lib import lib, check, ptr, stream
    c = K.CROP
    B = len(c["starts"])
    wav64 = R.rnd(torch.randn(B, c["ld"], generator=R.gen("crop"), dtype=F64), F32)
    go = Guarded(B, c["Lout"], F32)
    wav, starts, lens = _dev(wav64, F32), _i32(c["starts"]), _i32(c["lens"])
    check(lib().sc_crop_pad(ptr(wav), c["ld"], ptr(starts), ptr(lens), ptr(go.out()), B, c["Lout"], stream()), "sc_crop_pad")
    got, want = go.check("crop"), K.crop_ref(wav64, c["starts"], c["lens"], c["Lout"])
    assert torch.equal(got, want), ("sc_crop_pad", int((got != want).sum()), "elements differ")
    print(f"{'crop_pad':60s} bitwise equal")

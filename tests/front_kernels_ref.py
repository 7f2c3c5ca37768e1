"""Plain fp64 statements, case lists, deterministic inputs and DERIVED bounds of the front-end forward kernels (csrc/frontend.hip: conv0 statistics / coefficients /
VALU / matrix-core kernels, positional-conv pack and finish, ViT patchify and embed, image normalize, crop + pad; csrc/posconv.hip: the windowed positional conv)
for tests/test_front_kernels_parity_gpu.py and tools/front_kernel_bounds.py.  A helper module, not a test; no kernel runs here.

Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE before the reference sees it; the rules of the bounds (U, TR, BF_STORE,
n 2^-24 sum|terms| for an fp32 sum of n terms, the GELU constants, GELU_LIP) are those at the top of tests/row_kernels_ref.py and are imported, not restated.

Two kinds of statement:
  * EXACT-INTEGER cases.  Inputs are chosen so that every product and every fp32 partial sum is exact in any order (the condition -- every term a multiple of one
    power of two q, sum|terms| / q < 2^24 -- is returned by the input functions and asserted on the CPU); the only rounding left is the final RNE store, so the output
    must equal exact.to(float32).to(bfloat16) bit for bit.  conv0: samples a + b 2^-8 make x = x_hi + x_lo exact with x_lo != 0 (kind "xlo", integer weights: the
    x_lo . w_hi slots) or weights a + b 2^-8 with bf16-exact samples (kind "wlo": the x_hi . w_lo slots); the dropped x_lo . w_lo term is exactly zero in both.
  * BOUNDED cases, every element judged:
    conv0 coefficients: the kernel sums the 10 + 55 sample statistics in fp32 inside a thread and a wave (n = frames one wave sees, gn_wave_n) and in fp64 from there
        on, so  |d mean| <= (n + 1) U mean_t sum_j |w_j x_tj|,  |d E y^2| <= (n + 1) U mean_t (sum_j |w_j x_tj|)^2,  d var = d E y^2 + 2 |mean| d mean + d mean^2 and the
        relative error of scale is half of d var / (var + eps): the partial sums amplified by (mean^2 + var) / var.  A case whose bound on scale exceeds GN_REL_CAP
        proves nothing: gn_inputs halves the utterance's offset until it holds.
    conv0 forward, matrix cores: bf16 hi + lo splits of x, of fl32(w * scale) and of the shift leave 2^-16 each (two RNE roundings of 2^-8), the dropped lo . lo
        term is <= 2^-16 |x w|, fl32(w * scale) U, and the 32 k-slots are budgeted as an ordinary fp32 sum (33 U sum|terms|); then the packed-half GELU constant
        (modes 0, 2) or one bf16 store (mode 1).  Mode 2 adds the fp32 SINGLE-PASS mean / variance over the C channels ((C + 4) U E y^2 on the variance, the
        input's own error through 2 mean(|d| dx)), rsqrtf (TR), and the roundings of y * a + b with b = -mean * a; all through ln_bound(..., dx=).
    conv0 forward, VALU: an fp32 FMA chain of 10 (11 U sum|terms|), scale and shift (2 U), gelu_erf2 (GELU_ERF_FIT, v_exp / v_rcp) and one bf16 store.
    positional conv end to end: the conv slab is an fp32 sum of K = Kw cg products (K U sum|terms|) stored as bf16.  The reference rounds the slab to bf16 too;
        bf16(c + e) and bf16(c) each lie within half an ulp of their arguments, so d slab = 2 BF_STORE |c| + 1.01 K U sum|terms|.
    finish: u = slab + bias (U), gelu_poly2 (its constant, GELU_LIP d u), the residual add (U), then the two-pass LayerNorm of ln_bound(..., dx=) or the store alone.
    ViT embed: one add (U) in front of ln_bound(..., dx=); fp32 out.  Image normalize: v / 255 (TR), - mean (U), * fl32(1 / std) (2 U).

Mutants (tools/front_kernel_bounds.py shows that each leaves its bound or fails its bitwise comparison) are branches of the same reference functions.
NOT separable under an honest bound, hence judged where they are: in modes 0 and 2 the packed-half GELU constant (3.2e-3 + 2^-7 |want|) hides x_lo . w_hi dropped and
w_lo dropped (2^-8 relative on a value of order 1); both fail the bitwise mode 1 cases, which run the same MFMA slots."""
import collections

import torch
import torch.nn.functional as F

import row_kernels_ref as R
from row_kernels_ref import (F64, F32, BF, U, TR, BF_STORE, GELU_LIP, GELU_ERF_FIT, GELU_POLY2_ABS, GELU_POLY2_REL, PAST_VALUE,      # noqa: F401
                             gen, rnd, store_bound, gelu64, ln_ref, ln_bound, fsum, Guarded, judge)

EPS = float(torch.tensor(1e-5, dtype=F32))      # the fp32 value the kernels receive
CK, CS = 10, 5
SPLIT = 2.0 ** -16 * 1.01                       # what a bf16 hi + lo pair leaves of an fp32 value
GN_REL_CAP = 1e-2
LOUD = 96.0                                     # rows >= valid of an exact-integer positional-conv input


def bits(t64):
    """fp64 -> the bf16 the kernel must store (through fp32: exact for every value here), back in fp64"""
    return t64.to(F32).to(BF).to(F64)


def randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def frames(x, T0):
    """x [B, >= 5 (T0 - 1) + 10] -> [B, T0, 10]"""
    return x[:, :CS * (T0 - 1) + CK].unfold(1, CK, CS)


def conv0_L(T0):
    return CS * (T0 - 1) + CK


# ================================================================================================ conv0 GroupNorm coefficients
GNCase = collections.namedtuple("GNCase", "id T0 C pad")
GN_KINDS = ("off0", "off2.5", "off10", "zero_tail", "silent")
GN_STD = 0.1


def gn_cases():
    return [GNCase(f"gn-T{T0}-C{C}{'-ld' if pad else ''}", T0, C, pad) for T0, C, pad in ((1, 16, 0), (15, 16, 3), (16, 16, 0), (17, 264, 7), (4097, 16, 0), (31999, 16, 5))]


def gn_wave_n(T0):
    """frames whose statistics ONE wave adds in fp32: 16 splits per utterance, 256 threads striding a split"""
    per = -(-T0 // 16)
    return min(per, 64 * -(-per // 256))


def gn_ref(x, w, gamma, beta, T0, eps=EPS, mutant=None):
    """fp64: y = conv(x); scale = gamma / sqrt(var_t y + eps), shift = beta - mean_t y * scale (biased variance over the T0 frames).  -> dict of [B, C] tensors"""
    fr = frames(x, T0)
    y = torch.einsum("btj,cj->bct", fr, w)
    nb = torch.full((x.shape[0], 1), float(T0), dtype=F64)
    if mutant == "unpadded_len":
        live = (fr != 0).any(-1)
        last = torch.where(live.any(-1), T0 - live.flip(1).to(torch.int8).argmax(-1), torch.ones(x.shape[0], dtype=torch.long))
        nb = last.to(F64).view(-1, 1)
    mean = y.sum(-1) / nb
    var = ((y * y).sum(-1) / nb - mean * mean).clamp_min(0) if mutant == "unpadded_len" else ((y - mean.unsqueeze(-1)) ** 2).sum(-1) / T0
    if mutant == "var_T0m1" and T0 > 1:
        var = var * T0 / (T0 - 1)
    rstd = 1 / (var.sqrt() + eps) if mutant == "eps_outside" else 1 / (var + eps).sqrt()
    scale = gamma * rstd
    shift = beta - mean * scale
    if mutant == "next_channel":
        scale, shift = torch.roll(scale, -1, 1), torch.roll(shift, -1, 1)
    aw = torch.einsum("btj,cj->bct", fr.abs(), w.abs())
    n = gn_wave_n(T0) + 1
    dmean = n * U * aw.sum(-1) / T0
    dvar = n * U * (aw * aw).sum(-1) / T0 + 2 * mean.abs() * dmean + dmean ** 2
    r0 = 0.5 * dvar / (var + eps)
    rel = r0 * (1 + 3 * r0) + 3 * U                               # 1 / sqrt(1 - 2 r0) - 1 <= r0 (1 + 3 r0) below the cap; the casts to fp32
    b_scale = scale.abs() * rel
    b_shift = U * shift.abs() + scale.abs() * dmean + mean.abs() * b_scale + dmean * b_scale + U * (beta.abs() + (mean * scale).abs())
    return dict(scale=scale, shift=shift, b_scale=b_scale, b_shift=b_shift, rel=rel, mean=mean, var=var)


def gn_inputs(c):
    """x [5, L] (GN_KINDS: offsets of 0 / 2.5 / 10 standard deviations, a zero second half, silence), w [C, 10], gamma, beta [C]; fp32 values.
    -> (x, w, gamma, beta, the offsets in standard deviations after the cap's halvings)"""
    g = gen("gn", c.id)
    L = conv0_L(c.T0)
    w = rnd(0.3 * torch.randn(c.C, CK, generator=g, dtype=F64), F32)
    gamma = rnd(1 + 0.3 * torch.randn(c.C, generator=g, dtype=F64), F32)
    beta = rnd(0.3 * torch.randn(c.C, generator=g, dtype=F64), F32)
    base = GN_STD * torch.randn(5, L, generator=g, dtype=F64)
    offs = [0.0, 2.5, 10.0, 0.0, 0.0]
    for _ in range(12):
        x = base + GN_STD * torch.tensor(offs, dtype=F64).view(5, 1)
        x[3, L // 2:] = 0
        x[4] = 0
        x = rnd(x, F32)
        worst = gn_ref(x, w, gamma, beta, c.T0)["rel"].amax(-1)
        if float(worst.max()) < GN_REL_CAP:
            return x, w, gamma, beta, offs
        offs = [o / 2 if float(worst[b]) >= GN_REL_CAP else o for b, o in enumerate(offs)]
    raise AssertionError((c.id, "no offset keeps the bound on scale below the cap", worst))


def gn_emulate(x, w, gamma, beta, T0, order, eps=EPS):
    """fp32 statistics per block of gn_wave_n frames in `order`, fp64 across the blocks and in the coefficients, the result cast to fp32"""
    fr = frames(x, T0).to(F32)
    iu = torch.triu_indices(CK, CK)
    terms = torch.cat([fr, fr[..., iu[0]] * fr[..., iu[1]]], -1).transpose(1, 2)            # [B, 65, T0]
    n = gn_wave_n(T0)
    terms = F.pad(terms, (0, (-T0) % n)).reshape(x.shape[0], terms.shape[1], -1, n)
    st = fsum(terms.contiguous(), order).to(F64).sum(-1)                                      # [B, 65]
    s, Rm = st[:, :CK], torch.zeros(x.shape[0], CK, CK, dtype=F64)
    Rm[:, iu[0], iu[1]] = st[:, CK:]
    Rm = Rm + Rm.triu(1).transpose(1, 2)
    mean = torch.einsum("cj,bj->bc", w, s) / T0
    var = (torch.einsum("cj,bjk,ck->bc", w, Rm, w) / T0 - mean * mean).clamp_min(0)
    scale = gamma / (var + eps).sqrt()
    return scale.to(F32).to(F64), (beta - mean * scale).to(F32).to(F64)


# ================================================================================================ conv0 forward, bounded
C0Case = collections.namedtuple("C0Case", "id form mode C T0 P extra pad bias")          # extra: samples past the last frame; pad: ld - L
C0_MFMA_C, C0_MFMA_TP = (64, 128, 192, 448, 512), ((49, 64), (64, 128), (570, 576))
C0_VALU = ((8, 49, 64), (72, 100, 128), (512, 70, 70), (64, 97, 100))
C0_B = 3


def c0_form(C, P):
    return "mfma" if C % 64 == 0 and P % 64 == 0 else "valu"


def c0_cases():
    out, k = [], 0
    for mode in (0, 1, 2):
        for C in C0_MFMA_C:
            for T0, P in C0_MFMA_TP:
                out.append(C0Case(f"c0-mfma-m{mode}-C{C}-T{T0}-P{P}", "mfma", mode, C, T0, P, 23 if k % 2 else 0, 3 if k % 3 == 1 else 0, k % 4 != 3))
                k += 1
    for mode in (0, 1):
        for C, T0, P in C0_VALU:
            out.append(C0Case(f"c0-valu-m{mode}-C{C}-T{T0}-P{P}", "valu", mode, C, T0, P, 23 if k % 2 else 0, 3 if k % 3 == 1 else 0, k % 4 != 3))
            k += 1
    out.append(C0Case("c0-mfma-m0-C64-T31999-P32000", "mfma", 0, 64, 31999, 32000, 0, 0, True))
    assert all(c0_form(c.C, c.P) == c.form for c in out)
    return out


def c0_inputs(c):
    """x [3, L + extra] (samples at and past 5 (T0 - 1) + 10: PAST_VALUE; mode 0: utterance 2 silent), w [C, 10], and per mode
    0: (scale, shift) [3, C] = the fp32-rounded fp64 coefficients   1: bias [C] | None   2: bias, gamma, beta [C]"""
    g = gen("c0", c.id)
    L = conv0_L(c.T0)
    x = GN_STD * (torch.randn(C0_B, L + c.extra, generator=g, dtype=F64) + torch.tensor([0.0, 1.0, 0.0], dtype=F64).view(3, 1))
    if c.mode == 0:
        x[2] = 0
    x[:, L:] = PAST_VALUE
    x = rnd(x, F32)
    w = rnd(0.3 * torch.randn(c.C, CK, generator=g, dtype=F64), F32)
    gamma = rnd(1 + 0.3 * torch.randn(c.C, generator=g, dtype=F64), F32)
    beta = rnd(0.3 * torch.randn(c.C, generator=g, dtype=F64), F32)
    bias = rnd(0.05 * torch.randn(c.C, generator=g, dtype=F64), F32) if c.bias else None
    if c.mode == 0:
        gn = gn_ref(x, w, gamma, beta, c.T0)
        return x, w, dict(scale=rnd(gn["scale"], F32), shift=rnd(gn["shift"], F32), beta=beta)
    return x, w, dict(bias=bias, gamma=gamma, beta=beta)


def _pad_frames(t, P):
    return F.pad(t, (0, 0, 0, P - t.shape[1]))


def c0_ref(c, x, w, p, eps=EPS, mutant=None):
    """-> (ref [3, P, C], bound [3, P, C]); frames [T0, P) are exactly zero"""
    T0 = c.T0 + 1 if mutant == "frame_T0_live" and c.P > c.T0 else c.T0
    xx = F.pad(x[:, :conv0_L(c.T0) + c.extra], (0, CS)) if T0 > c.T0 else x               # (what lies past L reads as zero)
    fr = frames(xx, T0)
    y = torch.einsum("btj,cj->btc", fr, w)
    S = torch.einsum("btj,cj->btc", fr.abs(), w.abs())
    if c.mode == 0:
        scale, shift = p["scale"].unsqueeze(1), p["shift"].unsqueeze(1)
        if mutant == "next_channel":
            scale, shift = torch.roll(scale, -1, 2), torch.roll(shift, -1, 2)
    else:
        scale = torch.ones(1, 1, c.C, dtype=F64)
        shift = (p["bias"] if p["bias"] is not None else torch.zeros(c.C, dtype=F64)).view(1, 1, -1)
    if mutant == "shift_dropped":
        shift = torch.zeros_like(shift)
    ys, Su = y * scale, S * scale.abs()
    u = ys + shift
    if c.form == "mfma":
        pre = (3 * SPLIT + (U if c.mode == 0 else 0)) * Su + SPLIT * shift.abs() + 33 * U * 1.01 * (Su + shift.abs())
    else:
        pre = 11 * U * Su + 2 * U * (ys.abs() + u.abs())
    if c.mode == 1:
        ref, bound = u, BF_STORE * u.abs() + pre
    elif c.mode == 0:
        ref = gelu64(u)
        if c.form == "mfma":
            bound = GELU_POLY2_ABS + GELU_POLY2_REL * ref.abs() + GELU_LIP * pre
        else:
            bound = BF_STORE * ref.abs() + GELU_LIP * pre + GELU_ERF_FIT + (2 * TR + 8 * U) * ref.abs()
    else:
        gamma, beta, C = p["gamma"], p["beta"], c.C
        if mutant == "ln_512":
            mean = u.sum(-1, keepdim=True) / 512
            var = ((u * u).sum(-1, keepdim=True) / 512 - mean * mean).clamp_min(0)
            ref = gelu64((u - mean) / (var + eps).sqrt() * gamma + beta)
        else:
            ref, _ = ln_ref(u, gamma, beta, True, eps)
        mean = u.mean(-1, keepdim=True)
        d = u - mean
        var = (d * d).mean(-1, keepdim=True)
        rstd = 1 / (var + eps).sqrt()
        dmean = U * u.abs().sum(-1, keepdim=True) + pre.mean(-1, keepdim=True)
        dvar = (C + 4) * U * (mean * mean + var) + 2 * mean.abs() * dmean + 2 * (d.abs() * pre).mean(-1, keepdim=True)
        e_sp = (0.5 * dvar / (var + eps) + TR) * 1.01
        extra = (d * rstd * gamma).abs() * e_sp + 3 * U * (u.abs() + mean.abs()) * rstd * gamma.abs()
        bound = ln_bound(u, gamma, beta, True, BF, poly2=True, eps=eps, dx=pre) + GELU_LIP * extra
    return _pad_frames(ref, c.P), _pad_frames(bound, c.P)[:, :c.P] * (torch.arange(c.P).view(1, -1, 1) < c.T0)


def _split_bf(t32):
    hi = t32.to(BF)
    return hi.to(F32), (t32 - hi.to(F32)).to(BF).to(F32)


def c0_emulate(c, x, w, p, order, drop=None, eps=EPS):
    """The arithmetic of a correct kernel in torch fp32 / bf16: the 32 MFMA slots (matrix cores) or the FMA chain (VALU) summed in `order`, the exact erf GELU in fp32
    (the forms' own errors are constants of the bound), the bf16 store.  drop: "x_lo" / "w_lo" leaves those ten slots out (the mutants).  -> fp64 [3, P, C]"""
    fr = frames(x, c.T0).to(F32)                                                                # [B, T0, 10]
    w32 = w.to(F32)
    if c.mode == 0:
        scale, shift = p["scale"].to(F32), p["shift"].to(F32)                                   # [B, C]
    else:
        scale = torch.ones(x.shape[0], c.C, dtype=F32)
        shift = (p["bias"].to(F32) if p["bias"] is not None else torch.zeros(c.C, dtype=F32)).expand(x.shape[0], c.C)
    if c.form == "mfma":
        wh, wl = _split_bf(w32.unsqueeze(0) * scale.unsqueeze(-1))                               # [B, C, 10]
        xh, xl = _split_bf(fr)
        sh, sl = _split_bf(shift)
        if drop == "x_lo":
            xl = torch.zeros_like(xl)
        if drop == "w_lo":
            wl = torch.zeros_like(wl)
        terms = torch.cat([xh.unsqueeze(2) * wh.unsqueeze(1), xl.unsqueeze(2) * wh.unsqueeze(1), xh.unsqueeze(2) * wl.unsqueeze(1),
                           sh.view(-1, 1, c.C, 1).expand(-1, c.T0, -1, -1), sl.view(-1, 1, c.C, 1).expand(-1, c.T0, -1, -1)], -1)
        a = fsum(terms.contiguous(), order)
    else:
        a = fsum((fr.unsqueeze(2) * w32.view(1, 1, c.C, CK)).contiguous(), order) * scale.unsqueeze(1) + shift.unsqueeze(1)
    if c.mode == 2:
        s1, s2 = fsum(a.contiguous(), order), fsum((a * a).contiguous(), order)
        mean = s1 / c.C
        ln_a = torch.rsqrt((s2 / c.C - mean * mean).clamp_min(0) + torch.tensor(eps, dtype=F32))
        a = (a * ln_a.unsqueeze(-1) + (-mean * ln_a).unsqueeze(-1)) * p["gamma"].to(F32) + p["beta"].to(F32)
    if c.mode != 1:
        a = F.gelu(a)
    return _pad_frames(a.to(BF).to(F64), c.P)


# ================================================================================================ conv0 forward, exact (mode 1)
C0XCase = collections.namedtuple("C0XCase", "id form kind C T0 P bias")
C0X_SHAPES = (("mfma", 128, 49, 64), ("mfma", 64, 570, 576), ("valu", 72, 49, 70), ("valu", 64, 97, 100))


def c0x_cases():
    return [C0XCase(f"c0x-{form}-{kind}-C{C}-T{T0}-P{P}{'-bias' if bias else ''}", form, kind, C, T0, P, bias)
            for form, C, T0, P in C0X_SHAPES for kind in ("xlo", "wlo") for bias in (True, False)]


def _ab(g, *shape):
    return randint(g, -3, 3, *shape) + randint(g, -127, 127, *shape) / 256


def c0x_inputs(c):
    """-> x [2, L], w [C, 10], bias [C] | None, and the condition dict(quantum, worst sum|terms| / quantum)"""
    g = gen("c0x", c.id)
    L = conv0_L(c.T0)
    if c.kind == "xlo":
        x, w = _ab(g, 2, L), randint(g, -4, 4, c.C, CK)
    else:
        x, w = randint(g, -8, 8, 2, L) / 4, _ab(g, c.C, CK)
    bias = _ab(g, c.C) if c.bias else None
    q = 2.0 ** -10
    mag = torch.einsum("btj,cj->btc", frames(x, c.T0).abs(), w.abs()) + (bias.abs() if c.bias else 0)
    return x, w, bias, dict(quantum=q, worst=float(mag.max()) / q)


def c0x_ref(c, x, w, bias):
    y = torch.einsum("btj,cj->btc", frames(x, c.T0), w) + (bias if bias is not None else 0)
    return _pad_frames(bits(y), c.P)


# ================================================================================================ positional conv
PCCase = collections.namedtuple("PCCase", "id B G cg Kw Tp valid")
PC_TP = {70: ((0, 70), (1, 99)), 500: ((500, 1), (0, 700)), 582: ((255, 256), (257, 582), (0, 1)), 812: ((511, 512), (513, 900), (255, 257))}
PC_SMALL = ((32, 2), (32, 4), (48, 4), (64, 4), (64, 1), (64, 3))
PC_LONG = ((32, 16), (48, 16), (64, 16))            # the ring runs 8 / 12 / 16 stages across every chunk of the multi-chunk lengths
PC_REAL = ((48, 128), (64, 128))
PC_FALLBACK = ((64, 4, 4), (272, 4, 16), (100, 5, 4))            # (D, G, Kw): cg = 16, cg = 68, D % 8 != 0 -> return code 1, nothing written


PC_PACK_EXACT = ((64, 4, 16, 30, (30, 11)), (80, 4, 6, 9, (9, 4)), (272, 4, 6, 33, (0, 33)))            # (D, G, Kw, Tp, valid): the pack + GEMM route as it is, with D/G widened (20 -> 24, 68 -> 72), with K widened


def pcx_pack_cases():
    return [PCCase(f"pcx-pack-D{D}-G{G}-Kw{Kw}-Tp{Tp}", 2, G, D // G, Kw, Tp, v) for D, G, Kw, Tp, v in PC_PACK_EXACT]


def pc_nw(Tp):
    waste8, waste4 = -(-Tp // 512) * 512 - Tp, -(-Tp // 256) * 256 - Tp
    return 8 if waste8 <= waste4 + Tp // 8 else 4


def pc_path(c):
    """-> dict(NJ, NW, nk, chunks) of the windowed kernel this case reaches"""
    nw = pc_nw(c.Tp)
    return dict(NJ=c.cg // 16, NW=nw, nk=c.Kw * c.cg // 64, chunks=-(-c.Tp // (64 * nw)))


def pcx_cases():
    out = []
    for cg, Kw in PC_SMALL:
        for Tp, valids in PC_TP.items():
            out += [PCCase(f"pcx-cg{cg}-Kw{Kw}-Tp{Tp}-v{v[0]}_{v[1]}", 2, 4, cg, Kw, Tp, v) for v in valids]
    for cg, Kw in PC_LONG:
        out += [PCCase(f"pcx-cg{cg}-Kw{Kw}-Tp{Tp}-v{v[0]}_{v[1]}", 2, 4, cg, Kw, Tp, v) for Tp, v in ((582, (257, 582)), (812, (513, 900)))]
    out += [PCCase(f"pcx-cg{cg}-Kw{Kw}-Tp70-G16", 2, 16, cg, Kw, 70, (70, 33)) for cg, Kw in PC_REAL]
    return out


def pc_conv64(x, valid, wg, B, Tp, D, G, Kw, mutant=None, chunk=None):
    """fp64 conv1d(mask(x), w, padding = Kw // 2, groups = G)[..., :Tp] as [B, G, Tp, cg] with w[g cg + n, c, tap] = wg[g, n, tap cg + c]; rows >= min(valid, Tp)
    read as zero.  -> (out, sum|terms|).  chunk: the block's frame count, for the mutant that forgets the previous chunk's rows."""
    cg = D // G
    v = [max(0, min(Tp, int(n) + (1 if mutant == "valid_plus1" else -1 if mutant == "valid_minus1" else 0))) for n in valid]
    xm = x.view(B, Tp, D).clone()
    for b in range(B):
        xm[b, v[b]:] = 0
    w = wg.view(G, cg, Kw, cg)
    if mutant == "product_dropped":
        w = w.clone()
        w[:, :, Kw // 2, cg // 2] = 0
    lead = Kw // 2 + (1 if mutant == "tap_shift" else 0)

    def conv(xs):
        xg = xs.view(B, Tp, G, cg).permute(0, 2, 1, 3)
        if mutant == "neighbour_group":
            xg = torch.roll(xg, -1, 1)
        win = F.pad(xg, (0, 0, lead, Kw)).unfold(2, Kw, 1)[:, :, :Tp]                            # [B, G, Tp, cg, Kw]
        return torch.einsum("bgtck,gnkc->bgtn", win, w), torch.einsum("bgtck,gnkc->bgtn", win.abs(), w.abs())
    out, mag = conv(xm)
    if mutant == "chunk_no_halo":
        for ts in range(chunk, Tp, chunk):
            xs = xm.clone()
            xs[:, :ts] = 0
            out[:, :, ts:ts + chunk] = conv(xs)[0][:, :, ts:ts + chunk]
    return out, mag


def pcx_inputs(c):
    """small integers in bf16; rows >= valid[b] of x hold LOUD + (0 .. 7).  -> x [B Tp, D], wg [G, cg, Kw cg]"""
    g = gen("pcx", c.id)
    D = c.G * c.cg
    x = randint(g, -3, 3, c.B, c.Tp, D)
    for b, n in enumerate(c.valid):
        if n < c.Tp:
            x[b, n:] = LOUD + randint(g, 0, 7, c.Tp - n, D)
    return x.view(c.B * c.Tp, D), randint(g, -2, 2, c.G, c.cg, c.Kw * c.cg)


# ------------------------------------------------------------------------------------------------ finish, and the whole operation
PFCase = collections.namedtuple("PFCase", "id D G affine f32")
PF_SHAPES = ((80, 4), (192, 4), (192, 3), (192, 6), (768, 16), (1020, 51), (1024, 16), (1024, 32))            # cg 20, 48, 64, 32, 48, 20, 64, 32
PF_B, PF_TP, PF_VALID = 3, 7, (0, 4, 7)
E2ECase = collections.namedtuple("E2ECase", "id D G Kw Tp route valid")
E2E = (E2ECase("posconv-768-16-128-Tp70", 768, 16, 128, 70, "window", (70, 33)), E2ECase("posconv-1024-16-128-Tp70", 1024, 16, 128, 70, "window", (70, 33)),
       E2ECase("posconv-64-4-16-Tp30", 64, 4, 16, 30, "pack", (30, 11)), E2ECase("posconv-272-4-6-Tp33", 272, 4, 6, 33, "pack", (0, 33)))


def pf_cases():
    return [PFCase(f"finish-D{D}-G{G}{'-ln' if a else ''}-{'f32' if f else 'bf16'}", D, G, a, f) for D, G in PF_SHAPES for a in (False, True) for f in (False, True)]


def pf_kernel(c):
    cg = c.D // c.G
    return (c.f32, cg if cg in (64, 48) else 0)


def pf_inputs(key, B, Tp, D, G, affine, conv=True):
    """x [B Tp, D] bf16 values (rows >= valid are NOT zero: the kernel must mask them), conv [B, G, Tp, cg] bf16 values, bias, gamma, beta fp32 values"""
    g = gen("pf", key)
    x = rnd(torch.randn(B * Tp, D, generator=g, dtype=F64) + 0.5, BF)
    cv = rnd(1.5 * torch.randn(B, G, Tp, D // G, generator=g, dtype=F64), BF) if conv else None
    bias = rnd(0.3 * torch.randn(D, generator=g, dtype=F64), F32)
    gamma = rnd(1 + 0.3 * torch.randn(D, generator=g, dtype=F64), F32) if affine else None
    beta = rnd(0.3 * torch.randn(D, generator=g, dtype=F64), F32) if affine else None
    return x, cv, bias, gamma, beta


def pf_ref(x, valid, conv, bias, gamma, beta, B, Tp, D, G, out_dt, eps=EPS, dconv=None, mutant=None):
    """out[b, t] = [LN](mask(x)[b, t] + gelu(conv[b, g, t, c] + bias)), EVERY row (rows >= valid: [LN](gelu(conv + bias))).  -> (ref, bound) [B Tp, D]"""
    cv = conv.permute(0, 2, 1, 3).reshape(B * Tp, D)
    u = cv + bias
    du = U * u.abs() + (dconv.permute(0, 2, 1, 3).reshape(B * Tp, D) if dconv is not None else 0)
    a = gelu64(cv) + bias if mutant == "bias_after_gelu" else gelu64(u)
    da = GELU_POLY2_ABS + GELU_POLY2_REL * a.abs() + GELU_LIP * du
    live = (torch.arange(Tp).view(1, Tp) < torch.tensor([min(int(n), Tp) for n in valid]).view(B, 1)).reshape(B * Tp, 1)
    v = (x if mutant == "residual_unmasked" else x * live) + a
    dv = da + U * v.abs()
    if gamma is None:
        return v, store_bound(v, out_dt) + dv
    return ln_ref(v, gamma, beta, False, eps)[0], ln_bound(v, gamma, beta, False, out_dt, eps=eps, dx=dv)


def pf_emulate(x, valid, conv, bias, gamma, beta, B, Tp, D, G, out_dt, order, eps=EPS):
    cv = conv.permute(0, 2, 1, 3).reshape(B * Tp, D).to(F32)
    live = (torch.arange(Tp).view(1, Tp) < torch.tensor([min(int(n), Tp) for n in valid]).view(B, 1)).reshape(B * Tp, 1)
    v = x.to(F32) * live + F.gelu(cv + bias.to(F32))
    if gamma is None:
        return v.to(out_dt).to(F64)
    return R.ln_emulate(v, gamma, beta, False, out_dt, order, eps)


def e2e_inputs(c):
    g = gen("e2e", c.id)
    cg = c.D // c.G
    x, _, bias, gamma, beta = pf_inputs(("e2e", c.id), 2, c.Tp, c.D, c.G, True, conv=False)
    wg = rnd(torch.randn(c.G, cg, c.Kw * cg, generator=g, dtype=F64) * (c.Kw * cg) ** -0.5, BF)
    return x, wg, bias, gamma, beta


def e2e_ref(c, x, wg, bias, gamma, beta, out_dt=BF, mutant=None):
    K = c.Kw * (c.D // c.G)
    conv, mag = pc_conv64(x, c.valid, wg, 2, c.Tp, c.D, c.G, c.Kw, mutant if mutant not in ("bias_after_gelu", "residual_unmasked") else None,
                          chunk=64 * pc_nw(c.Tp))
    return pf_ref(x, c.valid, bits(conv), bias, gamma, beta, 2, c.Tp, c.D, c.G, out_dt, dconv=2 * BF_STORE * conv.abs() + 1.01 * K * U * mag,
                  mutant=mutant if mutant in ("bias_after_gelu", "residual_unmasked") else None)


# ------------------------------------------------------------------------------------------------ pack
def pack_ref(x, valid, B, Tp, D, G, Kw):
    """xg[b][g][Kw / 2 + t][c] = t < valid[b] ? x[b][t][g cg + c] : 0; Kw / 2 zero rows in front, Kw - Kw / 2 behind"""
    cg = D // G
    xm = x.view(B, Tp, D).clone()
    for b, n in enumerate(valid):
        xm[b, max(0, min(Tp, int(n))):] = 0
    return F.pad(xm.view(B, Tp, G, cg).permute(0, 2, 1, 3), (0, 0, Kw // 2, Kw - Kw // 2)).contiguous()


PACK_CASES = ((16, 4, 4, 9, (9, 3)), (80, 4, 6, 21, (0, 40)), (272, 4, 5, 17, (17, 1)))            # (D, G, Kw, Tp, valid): cg = 4, 20, 68


# ================================================================================================ ViT stem
PT_CASES = ((32, 64, 3072), (14, 42, 640), (16, 48, 768))            # (p, R, Kpad)
VE_D, VE_NTOK, VE_B = (4, 260, 768, 1020, 1024), (5, 10), 3


def pt_inputs(p, R):
    """img [2, 3, R, R]: a distinct value per (b, c, y, x) (multiples of 2^-9 below 2^7: fp32-exact, most not bf16-exact)"""
    n = 2 * 3 * R * R
    return ((torch.arange(n, dtype=F64) * 7919 % 65521) / 512 - 60).view(2, 3, R, R)


def pt_ref(img, p, Kpad, mutant=None):
    B, _, Rr, _ = img.shape
    g = Rr // p
    t = img.view(B, 3, g, p, g, p)                                                                # b c gy py gx px
    t = t.permute(0, 4, 2, 1, 3, 5) if mutant == "gyx_swapped" else t.permute(0, 2, 4, 1, 3, 5)
    return F.pad(bits(t.reshape(B * g * g, 3 * p * p)), (0, Kpad - 3 * p * p))


def ve_inputs(D, ntok):
    """patch [B (ntok - 1), D] bf16 values; cls [D], pos [ntok, D], gamma, beta fp32 values.  pos row 1 carries an offset of 40 (|mean| >> std), pos row 0 one of -3"""
    g = gen("ve", D, ntok)
    patch = rnd(torch.randn(VE_B * (ntok - 1), D, generator=g, dtype=F64), BF)
    pos = 0.3 * torch.randn(ntok, D, generator=g, dtype=F64)
    pos[1] += 40.0
    pos[0] -= 3.0
    cls = rnd(torch.randn(D, generator=g, dtype=F64), F32)
    gamma = rnd(1 + 0.3 * torch.randn(D, generator=g, dtype=F64), F32)
    beta = rnd(0.3 * torch.randn(D, generator=g, dtype=F64), F32)
    return patch, cls, rnd(pos, F32), gamma, beta


def ve_sum(patch, cls, pos, ntok, mutant=None):
    D = cls.shape[0]
    v = torch.cat([cls.view(1, 1, D).expand(VE_B, 1, D), patch.view(VE_B, ntok - 1, D)], 1) + pos
    if mutant == "cls_pos1":
        v[:, 0] = cls + pos[1]
    return v.reshape(VE_B * ntok, D)


def ve_ref(patch, cls, pos, gamma, beta, ntok, eps=EPS, mutant=None):
    v = ve_sum(patch, cls, pos, ntok, mutant)
    return ln_ref(v, gamma, beta, False, eps)[0], ln_bound(v, gamma, beta, False, F32, eps=eps, dx=U * v.abs())


def ve_emulate(patch, cls, pos, gamma, beta, ntok, order, eps=EPS):
    return R.ln_emulate(ve_sum(patch, cls, pos, ntok).to(F32), gamma, beta, False, F32, order, eps)


# ================================================================================================ image normalize, crop + pad
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IN_STATS = ((CLIP_MEAN, CLIP_STD), ((0.5, 0.25, 0.0), (0.5, 2.0, 0.125)))
IN_HW = (2, 17, 23)            # B, H, W: 391 pixels an image, every byte value in every channel


def in_inputs():
    B, H, W = IN_HW
    n = B * H * W
    return torch.stack([(torch.arange(n) * (2 * ch + 3) + 50 * ch) % 256 for ch in range(3)], -1).to(torch.uint8).view(B, H, W, 3)


def in_ref(u8, mean, std):
    m, s = rnd(torch.tensor(mean, dtype=F64), F32).view(1, 3, 1, 1), rnd(torch.tensor(std, dtype=F64), F32).view(1, 3, 1, 1)
    pix = u8.permute(0, 3, 1, 2).to(F64) / 255
    ref = (pix - m) / s
    return ref, (TR * pix + U * (pix - m).abs()) / s + 3 * U * ref.abs()


def in_emulate(u8, mean, std):
    m, s = torch.tensor(mean, dtype=F32).view(1, 3, 1, 1), torch.tensor(std, dtype=F32).view(1, 3, 1, 1)
    return ((u8.permute(0, 3, 1, 2).to(F32) / 255.0 - m) * (1.0 / s)).to(F64)


CROP = dict(ld=1000, Lout=300, starts=(0, 700, 123, 999, 5), lens=(300, 300, 0, 1, 250))            # utterance 1 ends at the row's last sample; Lout % 256 != 0; ld > Lout


def crop_ref(wav, starts, lens, Lout):
    out = torch.zeros(wav.shape[0], Lout, dtype=F64)
    for b, (s, n) in enumerate(zip(starts, lens)):
        out[b, :n] = wav[b, s:s + n]
    return out

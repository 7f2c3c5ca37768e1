"""Plain fp64 statements, case lists, deterministic inputs and DERIVED per-element bounds of the front-end BACKWARD kernels (csrc/train_front.hip: sc_conv0_bwd,
sc_conv0_wgrad, sc_posconv_finish_train, sc_posconv_dgrad_finish, sc_reverse_rows_bf16, their *_packed entries, sc_posconv_pack_gapped) and of the host chains of
speechclip_amd/train_front.py built on them (the positional conv's adjoint chain, posconv_wgrad / posconv_wgrad_packed, conv_layer_backward), for
tests/test_front_bwd_parity_gpu.py and tools/front_bwd_bounds.py.  A helper module, not a test; no kernel runs here.  The constants, the generator, the rounding helper, the
guarded window and the judge are those of tests/row_kernels_ref.py; slope_check, the GELU-backward budget (gb_pre) and the split-K weight gradient's bound are those of
tests/layer_kernels_ref.py; the rounding model of a GEMM with a residual is gemm_ref.rounding_points.  Imported, not restated.

Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE before the reference sees it.

1. conv layer 0 backward (GroupNorm extractor), per-utterance partials [B, C, 12] = (dw[0..9], dgamma, dbeta).  The statement is the kernel's CONTRACT in fp64 (c0b_ref), not
   autograd of fp32 modules: u = conv(wav), mean and biased variance over all T0 frames, dz = dy gelu'(gamma uhat + beta) on the frames that carry a gradient and 0 elsewhere,
   m1 = sum(dz gamma) / T0 and m2 = sum(dz gamma uhat) / T0 (T0, not the number of frames with a gradient), du = rstd (dz gamma - m1 - uhat m2) on ALL T0 frames,
   dw_j = sum_t du x[5 t + j], dgamma = sum dz uhat, dbeta = sum dz.  tools/front_bwd_bounds.py shows that it IS fp64 autograd of conv1d -> group_norm -> gelu.
   The bound, term by term (U, TR: row_kernels_ref):
     conv         an FMA chain of 10: d u_t = 10 U S_t, S_t = sum_j |w_j x_tj|
     mean, var    fp64 sums of the fp32 conv values: only the conv's rounding reaches them.  d mean = mean_t(d u_t) and the cast U |mean|;
                  d var = 2 mean_t(|u_t - mean| d u_t) + mean_t(d u_t^2) (the cross term with d mean vanishes: sum(u - mean) = 0), the fp64 one-sweep difference
                  2 (T0 + 2) 2^-53 (mean^2 + var), the cast and the + eps 2 U (var + eps); rsqrtf TR:  e_rstd = d var / (2 (var + eps)) + TR + U
     uhat         rstd (d u_t + d mean + U |mean| + U |u_t - mean|) + |uhat| (e_rstd + U)
     z            |gamma| d uhat + U (|z| + |gamma uhat|)    (the FMA rounds once; both terms allow the unfused form too)
     dz           layer_kernels_ref.gb_pre(z, dy) -- fast_erf's 1.5e-7, __expf's |z^2 / 2| 2^-23, the absolute U |1 + erf|, the product -- and |dy| GP_LIP d z with
                  GP_LIP = 0.8 >= max |gelu''| = 2 phi(0) = 0.798
     every sum    n U sum|terms| with n = ceil(T0 / 4) + 3 (a wave's chain of ceil(T0 / 4) frames, then the tree over the four waves), on top of the terms' own errors
     m1, m2       the sums' errors / T0 and TR for the division
     du           rstd (d(dz gamma) + d m1 + d(uhat m2) + 2 U (|dz gamma| + |m1| + |uhat m2|)) + |du| (e_rstd + U)
     dw           n U sum_t |du x| + sum_t d du_t |x_tj|: the errors of m1 / m2 reach it through rstd sum|x| and rstd sum|uhat x|
   and 1 % on the whole for the second-order products.  dy is bf16 on input and exact.
   THE CAP (a condition on the reference alone, c0b_cap): in a real-valued case the median over elements of bound / |ref| is at most 0.05 for each of dw, dgamma, dbeta and no
   more than 1 % of elements have bound > |ref|.  The DC utterance's offset (DC_START standard deviations of its noise) is halved until it holds (c0b_inputs), never the cap: the
   honest bound on dw grows with the SQUARE of the offset (du sums to zero against the DC part of x analytically, its errors do not), so the offset that survives shrinks with T0;
   channels with mean^2 / var >= 100 are asserted on the cases with 4 <= T0 <= 64, where it stays at 5 or 10.  Outside the cap by construction: T0 <= 2, where
   du -- the residual of projecting dz gamma on span{1, uhat} -- is identically zero (two frames span the plane; one frame: var = 0, uhat = 0, dgamma = 0 too) so that the
   statement's dw is rounding noise of its own and no RELATIVE cap can hold; these cases are judged by the same bound, which is absolute, and keep the full DC offset -- the
   fp32 one-sweep variance (E[u^2] - E[u]^2) is rejected there, where mean^2 / var is largest.  The long case (T0 = 31999) is outside
   the cap as the issue states and carries the signed-error statistic instead.
2. sc_conv0_wgrad: the exact-integer arm.  Samples a + b 2^-8, integer du: every term is a multiple of 2^-8 and sum|terms| / 2^-8 < 2^24, so the partials are exact in any order.
3. row kernels against statements: u = bf16_rne(fp32(conv) + bias) bit for bit (an IEEE fp32 add on the host), s within BF_STORE |s| + the precise GELU's budget of
   tail_kernels_ref.sk_ref evaluated AT THE ROUNDED u; dgrad_finish bf16_rne(fp32 add) bit for bit and exactly zero from valid_b on; reverse / pack_gapped: equality.
4. the positional conv's adjoint chain, integers: dx = mask(bf16(bf16(sum_{tap, out} du[t - tap + Kw / 2, out] w[out, in, tap]) + ds)).
5. posconv_wgrad[_packed], integers: dW[out, in, tap] = sum_{b, t < rows_b} du[b, t, out] mask(x)[b, t + tap - Kw / 2, in], bit for bit; two real cases under (M + S + 1) U sum|du x|.
   The chain is ALSO stated literally (pw_chain: the gapped slabs, then the product over gapped rows) for the mutants of the host's geometry.  Note on "gap Kw - 1": a
   window starting at a du row of utterance b reaches Kw - 1 - Kw / 2 rows past its end and Kw / 2 rows before its start, so Kw - 1 zero rows in BOTH slabs would still separate
   neighbours; the mutant is the window slab numbered with gap Kw - 1 while the gradient keeps Kw (the two calls take the gap separately).
6. conv_layer_backward, integers in [-1, 1]: dX over the whole buffer (the 8 slack rows included) = the adjoint of the strided view, every tap GEMM and every in-place sum an
   integer of magnitude <= 256 (bf16-exact; asserted on the reference); dW = du^T view.  Real cases: K U_ACC sum|terms| per tap GEMM, one bf16 store per tap, and per overlapping
   tap the once / twice model of gemm_ref.rounding_points on the stored value of the tap below."""
import collections
import math

import torch
import torch.nn.functional as F

import front_kernels_ref as K
import gemm_ref as Gm
import layer_kernels_ref as L
import row_kernels_ref as R
from row_kernels_ref import F64, F32, BF, U, TR, BF_STORE, GELU_PRECISE, PAST_VALUE, gen, rnd, gelu64   # noqa: F401

EPS = K.EPS
CK, CS = K.CK, K.CS
GP_LIP = 0.8
LOUD = K.LOUD
bits, randint, frames, conv0_L = K.bits, K.randint, K.frames, K.conv0_L


# ================================================================================================ 1. sc_conv0_bwd / sc_conv0_bwd_packed
C0BCase = collections.namedtuple("C0BCase", "id C T0 kinds P pad rows scale cap")          # rows None: uniform rows b * P + t; else packed transformer rows, scale = row_scale
KINDS4 = ("speech", "dc", "zero_tail", "silent")
GEO_ROWS, TRAP_ROWS = (19, 17, 11, 2), (19, 9, 11, 2)            # module.hubert.packed_geometry of the tiny model for 6091 / 5200 / 3040 / 330 samples (asserted on the CPU); the hand-made trap
CAP_MEDIAN, CAP_FRACTION = 0.05, 0.01
DC_START = 80.0                                                  # offset of the DC utterance in standard deviations of its noise, before the cap's halvings


def c0b_cases():
    C_, out = C0BCase, []
    for T0 in (1, 2, 3, 4, 5, 7, 64):
        out.append(C_(f"c0b-C64-T{T0}", 64, T0, KINDS4, T0 if T0 in (4, 64) else T0 + 3, 7, None, 0, T0 > 2))
    out.append(C_("c0b-C128-T5", 128, 5, KINDS4[:2], 8, 3, None, 0, True))
    out.append(C_("c0b-C128-T64", 128, 64, KINDS4, 67, 0, None, 0, True))
    out.append(C_("c0b-C64-T1217", 64, 1217, KINDS4, 1280, 5, None, 0, True))
    out.append(C_("c0b-C64-T4801", 64, 4801, KINDS4[:2], 4801, 0, None, 0, True))
    out.append(C_("c0b-pk-geo-T1217", 64, 1217, KINDS4, 0, 5, GEO_ROWS, 64, True))
    out.append(C_("c0b-pk-trap-T1217", 64, 1217, KINDS4, 0, 0, TRAP_ROWS, 64, True))
    out.append(C_("c0b-pk-full-T1217", 64, 1217, KINDS4[:2], 0, 3, (20, 3), 64, True))          # utterance 0: row_scale rows_b = 1280 >= T0
    out.append(C_("c0b-pk-B1-C128-T1217", 128, 1217, KINDS4[:1], 0, 0, (19,), 64, True))
    out.append(C_("c0b-pk-C128-T7-scale4", 128, 7, KINDS4[:3], 0, 2, (1, 2, 1), 4, True))       # frames with a gradient 4 / 7 / 4
    out.append(C_("c0b-long-C64-T31999", 64, 31999, KINDS4[:1], 32000, 0, None, 0, False))
    return out


def c0b_tlim(c):
    """frames of each utterance that carry a gradient"""
    return [c.T0] * len(c.kinds) if c.rows is None else [min(c.T0, c.scale * r) for r in c.rows]


def c0b_dy_rows(c):
    """-> (rows of the dy buffer without its 8 slack rows, first row of each utterance)"""
    B = len(c.kinds)
    if c.rows is None:
        return B * c.P, [b * c.P for b in range(B)]
    off = [0]
    for r in c.rows:
        off.append(off[-1] + r)
    return c.scale * off[-1], [c.scale * o for o in off[:-1]]


def _wave_kind(kind, base, off_sd):
    x = 0.3 * base
    if kind == "speech":
        return x + 0.05
    if kind == "dc":
        return x + 0.3 * off_sd
    if kind == "zero_tail":
        x = x + 0.05
        x[x.numel() // 2:] = 0
        return x
    return torch.zeros_like(x)


def c0b_inputs(c, check_cap=True):
    """x [B, L] (0.3 N(0, 1) + offset per kind), w [C, 10], gamma, beta [C] fp32 values; dy [B, T0, C] bf16 values (frames >= c0b_tlim are not part of the operation: the
    device buffer holds NaN there).  The DC utterance's offset starts at DC_START standard deviations and is halved until the cap holds on that utterance."""
    g = gen("c0b", c.id)
    B, L = len(c.kinds), conv0_L(c.T0)
    w = rnd(0.3 * torch.randn(c.C, CK, generator=g, dtype=F64), F32)
    gamma = rnd(1 + 0.2 * torch.randn(c.C, generator=g, dtype=F64), F32)
    beta = rnd(0.1 * torch.randn(c.C, generator=g, dtype=F64), F32)
    base = torch.randn(B, L, generator=g, dtype=F64)
    dy = rnd(torch.randn(B, c.T0, c.C, generator=g, dtype=F64), BF)
    dc = DC_START
    for _ in range(8):
        x = rnd(torch.stack([_wave_kind(k, base[b].clone(), dc) for b, k in enumerate(c.kinds)]), F32)
        inp = dict(x=x, w=w, gamma=gamma, beta=beta, dy=dy, dc=dc)
        if not (check_cap and c.cap and "dc" in c.kinds):
            return inp
        b = c.kinds.index("dc")
        ref, bound = c0b_ref(c, inp)
        if not c0b_cap(ref[b:b + 1], bound[b:b + 1])[1]:
            return inp
        dc /= 2
    raise AssertionError((c.id, "no DC offset keeps the bound inside the cap"))


def c0b_cap(ref, bound):
    """-> ({output: (median bound / |ref|, fraction of elements with bound > |ref|)}, [what violates the cap]); 0 / 0 counts as 0"""
    out, bad = {}, []
    for name, sl in (("dw", slice(0, 10)), ("dgamma", slice(10, 11)), ("dbeta", slice(11, 12))):
        r, b = ref[..., sl].abs().reshape(-1), bound[..., sl].reshape(-1)
        ratio = torch.where(b > 0, b / r.clamp_min(1e-300), torch.zeros_like(b))
        med, frac = float(ratio.median()), float((b > r).double().mean())
        out[name] = (med, frac)
        if not (med <= CAP_MEDIAN and frac <= CAP_FRACTION):
            bad.append((name, med, frac))
    return out, bad


def gelu_grad64(z, mutant=None):
    return L._gb_f(z, "tanh_form" if mutant == "tanh_gelu" else None)


def c0b_ref(c, inp, mutant=None):
    """-> (part [B, C, 12], bound [B, C, 12]) in fp64; the module header derives the bound term by term"""
    x, w, gamma, beta, dy = inp["x"], inp["w"], inp["gamma"], inp["beta"], inp["dy"]
    T0, B = c.T0, x.shape[0]
    fr = frames(x, T0)                                                         # [B, T0, 10]
    u = torch.einsum("btj,cj->bct", fr, w)
    S = torch.einsum("btj,cj->bct", fr.abs(), w.abs())
    mean = u.mean(-1, keepdim=True)
    d = u - mean
    var = (d * d).mean(-1, keepdim=True)
    if mutant == "var_T0m1" and T0 > 1:
        var = var * T0 / (T0 - 1)
    if mutant == "one_sweep_f32":
        var = _one_sweep_f32_var(u)
    rstd = 1 / (var + EPS).sqrt()
    uh = d * rstd
    gm, bt = gamma.view(1, -1, 1), beta.view(1, -1, 1)
    z = gm * uh + bt
    tl = torch.tensor(c0b_tlim(c)).view(B, 1, 1)
    live = (torch.arange(T0).view(1, 1, T0) < tl).to(F64)
    dyt = dy.transpose(1, 2) * live                                            # [B, C, T0], zero where there is no gradient
    dz = dyt * gelu_grad64(z, mutant)
    dg, db = (dz * uh).sum(-1), dz.sum(-1)
    A = dz * gm
    div = tl.to(F64).view(B, 1) if mutant == "m_over_grad_frames" else float(T0)
    m1, m2 = (A.sum(-1) / div).unsqueeze(-1), ((A * uh).sum(-1) / div).unsqueeze(-1)
    if mutant == "m1_dropped":
        m1 = torch.zeros_like(m1)
    Cc = uh * m2
    sub = m1 + Cc
    if mutant == "mean_terms_skipped":
        sub = sub * live
    du = rstd * (A - sub)
    dw = torch.einsum("bct,btj->bcj", du, fr)
    part = torch.cat([dw, dg.unsqueeze(-1), db.unsqueeze(-1)], -1)
    if mutant is not None:
        return part, None
    n = -(-T0 // 4) + 3
    eu = 10 * U * S
    dmean = eu.mean(-1, keepdim=True)
    dvar = 2 * (d.abs() * eu).mean(-1, keepdim=True) + (eu * eu).mean(-1, keepdim=True) + 2 * (T0 + 2) * 2.0 ** -53 * (mean * mean + var) + 2 * U * (var + EPS)
    e_rstd = 0.5 * dvar / (var + EPS) + TR + U
    euh = rstd * (eu + dmean + U * mean.abs() + U * d.abs()) + uh.abs() * (e_rstd + U)
    ez = gm.abs() * euh + U * (z.abs() + (gm * uh).abs())
    edz = (L.gb_pre(None, dict(u=z, dh=dyt)) + dyt.abs() * GP_LIP * ez) * live

    def mag(t):
        return t.abs().sum(-1)
    b_db = n * U * mag(dz) + edz.sum(-1)
    b_dg = n * U * mag(dz * uh) + (edz * uh.abs() + dz.abs() * euh).sum(-1)
    eA = gm.abs() * edz + U * A.abs()
    em1 = ((n * U * mag(A) + eA.sum(-1)) / T0).unsqueeze(-1) + TR * m1.abs()
    em2 = ((n * U * mag(A * uh) + (eA * uh.abs() + A.abs() * euh).sum(-1)) / T0).unsqueeze(-1) + TR * m2.abs()
    eC = euh * m2.abs() + uh.abs() * em2 + U * Cc.abs()
    edu = rstd * (eA + em1 + eC + 2 * U * (A.abs() + m1.abs() + Cc.abs())) + du.abs() * (e_rstd + U)
    b_dw = n * U * torch.einsum("bct,btj->bcj", du.abs(), fr.abs()) + torch.einsum("bct,btj->bcj", edu, fr.abs())
    return part, 1.01 * torch.cat([b_dw, b_dg.unsqueeze(-1), b_db.unsqueeze(-1)], -1)


def wave_sum(terms, rev=False):
    """fp32 sum over the last dim as the kernels form it: wave k adds the frames k, k + 4, ... in turn (rev: last to first), then (p0 + p1) + (p2 + p3)"""
    assert terms.dtype == F32
    T = terms.shape[-1]
    t = F.pad(terms, (0, (-T) % 4)).reshape(*terms.shape[:-1], -1, 4)
    acc = torch.zeros(*terms.shape[:-1], 4, dtype=F32)
    steps = range(t.shape[-2] - 1, -1, -1) if rev else range(t.shape[-2])
    for i in steps:
        acc = acc + t[..., i, :]
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def _conv32(fr32, w32):
    a = torch.zeros(fr32.shape[0], w32.shape[0], fr32.shape[1], dtype=F32)
    for j in range(CK):
        a = a + w32[:, j].view(1, -1, 1) * fr32[:, :, j].unsqueeze(1)
    return a


def _one_sweep_f32_var(u):
    """the mutant: E[u^2] - E[u]^2 with both sums and the difference in fp32 (the kernel's split over the waves)"""
    u32 = u.to(F32)
    T0 = u.shape[-1]
    m = wave_sum(u32) / T0
    return ((wave_sum(u32 * u32) / T0 - m * m).clamp_min(0)).to(F64).unsqueeze(-1)


def c0b_emulate(c, inp, order):
    """The arithmetic of a correct kernel in torch fp32 (the transcendentals of gelu' in fp64 rounded once: fast_erf's own error is a constant of the bound), statistics in
    fp64 over the fp32 conv values, every sum in the kernel's split; order "wave4" first frame to last, "wave4rev" last to first.  -> part fp64 [B, C, 12]"""
    rev = order == "wave4rev"
    x, w, gamma, beta, dy = (inp[k].to(F32) for k in ("x", "w", "gamma", "beta", "dy"))
    T0, B = c.T0, x.shape[0]
    fr = frames(x, T0)
    a = _conv32(fr, w)
    a64 = a.to(F64)
    mean_d = a64.sum(-1, keepdim=True) / T0
    var32 = ((a64 * a64).sum(-1, keepdim=True) / T0 - mean_d * mean_d).to(F32)
    rstd = torch.rsqrt(var32 + torch.tensor(EPS, dtype=F32))
    uh = (a - mean_d.to(F32)) * rstd
    gm, bt = gamma.view(1, -1, 1), beta.view(1, -1, 1)
    z = gm * uh + bt
    z64 = z.to(F64)
    gp = (torch.tensor(0.5, dtype=F32) * (1 + torch.erf(z64 / 2 ** 0.5).to(F32))) + z * torch.tensor(0.3989422804014327, dtype=F32) * torch.exp(-0.5 * z64 * z64).to(F32)
    live = (torch.arange(T0).view(1, 1, T0) < torch.tensor(c0b_tlim(c)).view(B, 1, 1)).to(F32)
    dz = dy.transpose(1, 2) * live * gp
    dzh = dz * gm
    s = wave_sum(torch.stack([dzh, dzh * uh, dz * uh, dz]), rev)
    m1, m2 = (s[0] / T0).unsqueeze(-1), (s[1] / T0).unsqueeze(-1)
    du = rstd * (dzh - m1 - uh * m2)
    dw = wave_sum((du.unsqueeze(-2) * fr.permute(0, 2, 1).unsqueeze(1)).contiguous(), rev)          # [B, C, 10, T0] -> [B, C, 10]
    return torch.cat([dw, s[2].unsqueeze(-1), s[3].unsqueeze(-1)], -1).to(F64)


def c0b_batch_sum(part32):
    """ops.conv0_bwd's batch sums in the order of sc_colsum on B <= 4 rows: four row-interleaved partials of one row each, then (p0 + p1) + (p2 + p3)"""
    B = part32.shape[0]
    assert B <= 4 and part32.dtype == F32
    p = [part32[b] if b < B else torch.zeros_like(part32[0]) for b in range(4)]
    return (p[0] + p[1]) + (p[2] + p[3])


def signed_stat(got, ref, bound):
    """the signed-error statistic of the GEMM parity: mean of r = (got - ref) / bound over the elements with a bound, against 6 / sqrt(n)"""
    ok = bound > 0
    r = ((got - ref)[ok] / bound[ok])
    return float(r.mean()), 6 / math.sqrt(max(1, int(ok.sum())))


# ================================================================================================ 2. sc_conv0_wgrad[_packed], exact integers
def c0w_cases():
    return [c for c in c0b_cases() if c.T0 <= 4801]


def c0w_inputs(c):
    """x [B, L] = a + b 2^-8 (|a| <= 3, |b| <= 127), du [B, T0, C] integers in [-3, 3] -> (x, du, dict(quantum, worst sum|terms| / quantum))"""
    g = gen("c0w", c.id)
    B = len(c.kinds)
    x = randint(g, -3, 3, B, conv0_L(c.T0)) + randint(g, -127, 127, B, conv0_L(c.T0)) / 256
    du = randint(g, -3, 3, B, c.T0, c.C)
    q = 2.0 ** -8
    return x, du, dict(quantum=q, worst=float(torch.einsum("btc,btj->bcj", du.abs(), frames(x, c.T0).abs()).max()) / q)


def c0w_ref(c, x, du):
    """part [B, C, 12]: dw_j = sum_{t < tlim} du x[5 t + j], slot 10 = sum du, slot 11 = 0"""
    B = x.shape[0]
    live = (torch.arange(c.T0).view(1, c.T0, 1) < torch.tensor(c0b_tlim(c)).view(B, 1, 1)).to(F64)
    dul = du * live
    return torch.cat([torch.einsum("btc,btj->bcj", dul, frames(x, c.T0)), dul.sum(1).unsqueeze(-1), torch.zeros(B, c.C, 1, dtype=F64)], -1)


# ================================================================================================ 3. the row kernels
RowCase = collections.namedtuple("RowCase", "id D G rows valid packed")
ROW_SHAPES = ((16, 4), (24, 2), (64, 2), (192, 4), (768, 16), (1024, 16))
ROW_B = (1, 2, 3, 5, 8, 9)
ROW_B_UNIFORM = (1, 2, 8, 5, 3, 9)                   # per shape: no total of rows D / V may be a multiple of 256 (asserted on the CPU)
ROW_PATTERN = (1, 3, 4, 1, 5, 2, 6, 2, 1)            # a one-row utterance first, in the middle and (B = 9) last


def _valids(rows):
    return tuple((r, 0, 1, r + 2, max(r - 1, 0))[b % 5] for b, r in enumerate(rows))


def row_vec(D, G):
    return 8 if (D // G) % 8 == 0 else 4


def row_cases():
    out = []
    for i, (D, G) in enumerate(ROW_SHAPES):
        B = ROW_B_UNIFORM[i]
        rows = (5,) * B
        out.append(RowCase(f"rows-D{D}-G{G}-uniform-B{B}-Tp5-V{row_vec(D, G)}", D, G, rows, _valids(rows)[::-1], False))
    rows = (7,) * 3
    out.append(RowCase("rows-D64-G2-uniform-B3-Tp7-V8", 64, 2, rows, (7, 0, 9), False))
    for B in ROW_B:
        rows = ROW_PATTERN[:B]
        out.append(RowCase(f"rows-D64-G2-packed-B{B}", 64, 2, rows, _valids(rows), True))
    for (D, G), B in (((192, 4), 8), ((768, 16), 5), ((1024, 16), 9)):
        rows = ROW_PATTERN[:B]
        out.append(RowCase(f"rows-D{D}-G{G}-packed-B{B}", D, G, rows, _valids(rows), True))
    return out


def row_off(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


def row_inputs(c):
    """x, ds [total, D] bf16 values (rows >= valid of x: LOUD + (0 .. 7), they must be masked), slab [total * D] bf16 values (utterance b = [G][rows_b][cg] at element
    row_off[b] D), bias [D] fp32 values"""
    g = gen("rows", c.id)
    total, off = sum(c.rows), row_off(c.rows)
    x = rnd(torch.randn(total, c.D, generator=g, dtype=F64) + 0.5, BF)
    for b, v in enumerate(c.valid):
        lo = off[b] + min(v, c.rows[b])
        x[lo:off[b + 1]] = LOUD + randint(g, 0, 7, off[b + 1] - lo, c.D)
    ds = rnd(torch.randn(total, c.D, generator=g, dtype=F64), BF)
    slab = rnd(1.5 * torch.randn(total * c.D, generator=g, dtype=F64), BF)
    bias = rnd(0.3 * torch.randn(c.D, generator=g, dtype=F64), F32)
    return dict(x=x, ds=ds, slab=slab, bias=bias)


def slab_rows(c, slab, flip=False, mutant=None):
    """the slabs regrouped to rows: out[row_off[b] + t, g cg + ci] = slab_b[g][t][ci] (flip: slab_b[g][rows_b - 1 - t][ci])"""
    cg, off = c.D // c.G, row_off(c.rows)
    out = []
    for b, r in enumerate(c.rows):
        s = slab[off[b] * c.D:off[b + 1] * c.D].view(c.G, r, cg)
        if flip and mutant != "slab_row_t":
            s = s.flip(1)
        out.append(s.permute(1, 0, 2).reshape(r, c.D))
    return torch.cat(out, 0)


def live_rows(c, mutant=None):
    off = row_off(c.rows)
    m = torch.zeros(sum(c.rows), 1, dtype=torch.bool)
    for b, v in enumerate(c.valid):
        m[off[b]:off[b] + min(v + (1 if mutant == "mask_t_le_valid" else 0), c.rows[b])] = True
    return m


def finish_train_ref(c, inp, mutant=None):
    """-> (u bits, s ref, s bound): u = bf16_rne(fp32(conv) + bias) by an IEEE fp32 add; s = mask(x) + gelu(u rounded)"""
    u = (slab_rows(c, inp["slab"]).to(F32) + inp["bias"].to(F32)).to(BF).to(F64)
    a = gelu64(u)
    s = inp["x"] * live_rows(c, mutant) + a
    bound = BF_STORE * s.abs() + GELU_PRECISE * (1 + u.abs()) + 0.5 * u.abs() * (2 * TR + 6 * U) + 2 * U * a.abs() + U * s.abs()
    return u, s, bound


def dgrad_finish_ref(c, inp, mutant=None):
    """bf16_rne(fp32(convT[rows_b - 1 - t]) + fp32(ds)) below valid_b, exactly zero from there on"""
    v = (slab_rows(c, inp["slab"], flip=True, mutant=mutant).to(F32) + inp["ds"].to(F32)).to(BF).to(F64)
    return v * live_rows(c, mutant)


def reverse_ref(c, x, mutant=None):
    off = row_off(c.rows)
    if mutant == "reverse_rows_b_minus_t":            # out[r0 + rows_b - t] = in[r0 + t]: one row late; what falls behind the buffer is lost, row r0 of utterance 0 is never written
        out = torch.full_like(x, R.SENT16)
        for b, r in enumerate(c.rows):
            for t in range(r):
                if off[b] + r - t < x.shape[0]:
                    out[off[b] + r - t] = x[off[b] + t]
        return out
    return torch.cat([x[off[b]:off[b + 1]].flip(0) for b in range(len(c.rows))], 0)


def pack_gapped_ref(x, lim, rows, G, gap, lead, n_rows):
    """out [G, n_rows, cg]: row lead + row_off[b] + b gap + t of group g = columns of group g of x[row_off[b] + t] for t < min(lim[b], rows_b); zero everywhere else"""
    D = x.shape[1]
    cg, off = D // G, row_off(rows)
    out = torch.zeros(G, n_rows, cg, dtype=F64)
    for b, r in enumerate(rows):
        n = max(0, min(int(lim[b]), r))
        p0 = lead + off[b] + b * gap
        out[:, p0:p0 + n] = x[off[b]:off[b] + n].view(n, G, cg).permute(1, 0, 2)
    return out


ROW_ARG_RULES = ("packed_cg_not_8", "reverse_in_place", "slab_rows_too_small")


# ================================================================================================ 4. the positional conv's adjoint chain, exact
AdjCase = collections.namedtuple("AdjCase", "id cg Kw G rows valid packed")
ADJ_CG, ADJ_KW, ADJ_CHUNKED = (32, 48, 64), (2, 3, 16), 582            # 582 rows: three frame chunks of the windowed kernel (front_kernels_ref.pc_path)


def adj_cases():
    out = []
    for cg in ADJ_CG:
        for Kw in ADJ_KW:
            for Tp in sorted({1, max(1, Kw // 2), 70, ADJ_CHUNKED}):
                out.append(AdjCase(f"adj-cg{cg}-Kw{Kw}-uniform-Tp{Tp}", cg, Kw, 2, (Tp, Tp), (Tp, max(0, Tp - 3)), False))
            if adj_windowed(cg, Kw):
                rows = (70, 1, ADJ_CHUNKED, max(1, Kw // 2), 5)
                out.append(AdjCase(f"adj-cg{cg}-Kw{Kw}-packed", cg, Kw, 2, rows, (69, 1, ADJ_CHUNKED, 0, 7), True))
    return out


def adj_windowed(cg, Kw):
    """sc_posconv_conv's own rule (posconv.hip): the windowed kernel takes a group width of 32 / 48 / 64 whose window Kw D/G is a multiple of 64.  Padded batches fall back to
    the pack + GEMM route where it declines (the uniform cases run either); packed batches have no other route and ops.posconv_conv_packed raises."""
    return cg in (32, 48, 64) and (Kw * cg) % 64 == 0


ADJ_PACKED_DECLINED = tuple((cg, Kw) for cg in ADJ_CG for Kw in ADJ_KW if not adj_windowed(cg, Kw))            # (32, 3), (48, 2), (48, 3)


def adj_inputs(c):
    """du [total, D] integers in [-3, 3] on EVERY row (rows >= valid carry a gradient too), ds [total, D] integers in [-8, 8] with LOUD + (0 .. 7) on rows >= valid (the mask
    must remove them), wfold f32 [D, cg, Kw] integers in [-2, 2]"""
    g = gen("adj", c.id)
    D, total, off = c.G * c.cg, sum(c.rows), row_off(c.rows)
    du = randint(g, -3, 3, total, D)
    ds = randint(g, -8, 8, total, D)
    for b, v in enumerate(c.valid):
        lo = off[b] + min(v, c.rows[b])
        ds[lo:off[b + 1]] = LOUD + randint(g, 0, 7, off[b + 1] - lo, D)
    return dict(du=du, ds=ds, wfold=randint(g, -2, 2, D, c.cg, c.Kw))


def convT64(du_b, wfold, G, Kw):
    """fp64 transposed conv of ONE utterance: out[t, g cg + in] = sum_{tap, out} du_b[t - tap + Kw / 2, g cg + out] wfold[g cg + out, in, tap], rows outside [0, rows_b) zero
    -> (out, sum|terms|)"""
    r, D = du_b.shape
    cg, h = D // G, Kw // 2
    pad = F.pad(du_b.view(r, G, cg), (0, 0, 0, 0, Kw - 1 - h, h))                       # padded row p = t' + Kw - 1 - h; the window at t: rows t .. t + Kw - 1, element k <-> tap Kw - 1 - k
    win = pad.unfold(0, Kw, 1)                                                          # [r, G, cg(out), Kw]
    wf = wfold.view(G, cg, cg, Kw).flip(-1)                                             # [g, out, in, k]
    return (torch.einsum("tgok,goik->tgi", win, wf).reshape(r, D), torch.einsum("tgok,goik->tgi", win.abs(), wf.abs()).reshape(r, D))


def adj_ref(c, inp, mutant=None):
    """-> (dx bits [total, D], worst sum|terms|): the slab rounded to bf16 once, bf16 again after adding ds, zero from valid_b on"""
    off, outs, worst = row_off(c.rows), [], 0.0
    for b, r in enumerate(c.rows):
        t, mag = convT64(inp["du"][off[b]:off[b + 1]], inp["wfold"], c.G, c.Kw)
        worst = max(worst, float(mag.max()))
        if mutant == "slab_row_t":
            t = t.flip(0)
        v = bits(bits(t) + inp["ds"][off[b]:off[b + 1]])
        v[min(c.valid[b] + (1 if mutant == "mask_t_le_valid" else 0), r):] = 0
        outs.append(v)
    return torch.cat(outs, 0), worst


# ================================================================================================ 5. posconv_wgrad / posconv_wgrad_packed
PWCase = collections.namedtuple("PWCase", "id cg Kw G rows valid packed real")
PW_SHAPES = ((8, 4), (32, 16))            # (D / G, Kw), G = 2


def pw_split(c):
    """the host's decisions restated -> dict(S, Tq | Ktot, chunk, Rg)"""
    B = len(c.rows)
    if not c.packed:
        Tq = -(-c.rows[0] // 64) * 64
        S = max(s for s in (16, 8, 4, 2, 1) if B % s == 0)
        return dict(S=S, Tq=Tq, M=B * Tq, chunk=B * Tq // S, Rg=0)
    Rg = sum(c.rows) + B * c.Kw
    S = max(s for s in (16, 8, 4, 2, 1) if s == 1 or Rg >= 512 * s)
    Ktot = -(-Rg // (64 * S)) * 64 * S
    return dict(S=S, Tq=Ktot, M=Ktot, chunk=Ktot // S, Rg=Rg)


def _pw_valid(rows):
    return tuple((max(r - 2, 0), r, 0, r + 3, 1)[b % 5] for b, r in enumerate(rows))


def pw_cases():
    out = []
    for cg, Kw in PW_SHAPES:
        for B in (1, 2, 3, 4, 16):
            for Tp in (5, 64, 70):
                rows = (Tp,) * B
                valid = (Tp - 2,) if B == 1 else _pw_valid(rows)
                out.append(PWCase(f"pw-cg{cg}-Kw{Kw}-uniform-B{B}-Tp{Tp}", cg, Kw, 2, rows, valid, False, False))
        for Rg in (511, 512, 1023, 1024, 2047, 2048):
            total = Rg - 3 * Kw
            rows = (1, total - 41, 40)
            out.append(PWCase(f"pw-cg{cg}-Kw{Kw}-packed-B3-Rg{Rg}", cg, Kw, 2, rows, (1, total - 50, 40), True, False))
        out.append(PWCase(f"pw-cg{cg}-Kw{Kw}-packed-B1-Rg1024", cg, Kw, 2, (1024 - Kw,), (1000 - Kw,), True, False))
    out.append(PWCase("pw-real-cg32-Kw16-uniform-B4-Tp70", 32, 16, 2, (70,) * 4, (70, 33, 0, 69), False, True))
    out.append(PWCase("pw-real-cg32-Kw16-packed-B3-Rg1100", 32, 16, 2, (1, 1100 - 48 - 41, 40), (1, 900, 40), True, True))
    return out


def pw_inputs(c):
    """x [total, D] (rows >= valid: LOUD + (0 .. 7), masked by the chain), du [total, D] non-zero on EVERY row; integers in [-3, 3], or bf16 values in a real case"""
    g = gen("pw", c.id)
    D, total, off = c.G * c.cg, sum(c.rows), row_off(c.rows)
    if c.real:
        x = rnd(0.5 * torch.randn(total, D, generator=g, dtype=F64) + 0.1, BF)
        du = rnd(0.3 * torch.randn(total, D, generator=g, dtype=F64), BF)
    else:
        x, du = randint(g, -3, 3, total, D), randint(g, -3, 3, total, D)
    for b, v in enumerate(c.valid):
        lo = off[b] + min(v, c.rows[b])
        x[lo:off[b + 1]] = LOUD + randint(g, 0, 7, off[b + 1] - lo, D)
    return dict(x=x, du=du)


def pw_ref(c, inp, absolute=False):
    """dW [D, cg, Kw] = sum_{b, t < rows_b} du[b, t, out] mask(x)[b, t + tap - Kw / 2, in]   (absolute: the magnitude reference)"""
    D, h, off = c.G * c.cg, c.Kw // 2, row_off(c.rows)
    out = torch.zeros(c.G, c.cg, c.cg, c.Kw, dtype=F64)
    for b, r in enumerate(c.rows):
        xm = inp["x"][off[b]:off[b + 1]].clone()
        xm[min(c.valid[b], r):] = 0
        du = inp["du"][off[b]:off[b + 1]]
        if absolute:
            xm, du = xm.abs(), du.abs()
        win = F.pad(xm.view(r, c.G, c.cg), (0, 0, 0, 0, h, c.Kw)).unfold(0, c.Kw, 1)[:r]            # [r, G, cg(in), Kw]: win[t, :, :, k] = xm[t + k - h]
        out += torch.einsum("tgo,tgik->goik", du.view(r, c.G, c.cg), win)
    return out.reshape(D, c.cg, c.Kw)


def pw_chain(c, inp, mutant=None):
    """The host chain stated literally in fp64, for the mutants of its geometry.  Packed: the window slab (lead Kw / 2, gap Kw) and the gradient (no lead, gap Kw) in gapped rows,
    dW[out, in, tap] = sum_p dug[p, out] xg[p + tap, in] over the S chunks.  Uniform: K index b Tq + t, the Tq - Tp padding rows zero.  -> dW, or None where the mutant cannot differ"""
    D, h, off, B = c.G * c.cg, c.Kw // 2, row_off(c.rows), len(c.rows)
    sp = pw_split(c)
    S, M, chunk = sp["S"], sp["M"], sp["chunk"]
    if c.packed:
        gap_x = c.Kw - 1 if mutant == "gap_Kw_minus_1" else c.Kw
        lead = h - 1 if mutant == "lead_minus_1" else h
        xg = pack_gapped_ref(inp["x"], c.valid, c.rows, c.G, gap_x, lead, M + c.Kw)                    # [G, M + Kw, cg]
        dug = pack_gapped_ref(inp["du"], c.rows, c.rows, 1, c.Kw, 0, M)[0]                              # [M, D]
    else:
        Tp, Tq = c.rows[0], sp["Tq"]
        if mutant in ("gap_Kw_minus_1", "lead_minus_1"):
            return None
        dug = torch.zeros(M, D, dtype=F64)
        wins = torch.zeros(M, c.G, c.cg, c.Kw, dtype=F64)            # K row b Tq + t holds the Kw window rows of utterance b's OWN slab (Kw / 2 zero rows in front, Kw behind)
        for b in range(B):
            n = max(0, min(c.valid[b], Tp))
            xb = torch.zeros(Tp, c.G, c.cg, dtype=F64)
            xb[:n] = inp["x"][off[b]:off[b] + n].view(n, c.G, c.cg)
            dug[b * Tq:b * Tq + Tp] = inp["du"][off[b]:off[b + 1]]
            wins[b * Tq:b * Tq + Tp] = F.pad(xb, (0, 0, 0, 0, h, c.Kw)).unfold(0, c.Kw, 1)[:Tp]
        if mutant == "tq_padding_not_zero":
            if Tq == Tp:
                return None
            for b in range(B):
                wins[b * Tq + Tp:(b + 1) * Tq] = R.SENT16
                dug[b * Tq + Tp:(b + 1) * Tq] = R.SENT16
    if c.packed:
        if mutant == "tq_padding_not_zero":
            return None
        wins = xg.permute(1, 0, 2).unfold(0, c.Kw, 1)[:M]                                               # [M, G, cg, Kw]
    if mutant == "last_chunk_dropped":
        if S == 1:
            return None
        dug = dug.clone()
        dug[(S - 1) * chunk:] = 0
    return torch.einsum("pgo,pgik->goik", dug.view(M, c.G, c.cg), wins).reshape(D, c.cg, c.Kw)


def pw_bound(c, inp):
    """layer_kernels_ref.wg_bound's rule: an M-term fp32 accumulation in S parts joined by an (S + 1)-term column sum: (M + S + 1) U sum|du x|"""
    sp = pw_split(c)
    return (sp["M"] + sp["S"] + 1) * U * pw_ref(c, inp, absolute=True)


# ================================================================================================ 6. conv_layer_backward
CLCase = collections.namedtuple("CLCase", "id k s C dim B rows_out real")


def cl_cases():
    out = []
    for k, s in ((3, 2), (2, 2)):
        for i, rows_out in enumerate((5, 64, 65)):
            C, dim = ((64, 128), (128, 64), (128, 128))[i]
            out.append(CLCase(f"cl-k{k}s{s}-C{C}-dim{dim}-rows{rows_out}", k, s, C, dim, 2, rows_out, False))
        out.append(CLCase(f"cl-real-k{k}s{s}-C64-dim128-rows65", k, s, 64, 128, 2, 65, True))
    return out


def cl_inputs(c):
    """xin [B rows_in + 8, C] (the 8 slack rows hold values too: the strided view reads the first of them when k > s), w f32 [dim, C, k], du [B rows_out, dim];
    integers in [-1, 1], or bf16 values in a real case"""
    g = gen("cl", c.id)
    Mi, rows_in = c.B * c.rows_out, c.rows_out * c.s
    if c.real:
        xin = rnd(0.5 * torch.randn(c.B * rows_in + 8, c.C, generator=g, dtype=F64), BF)
        w = rnd(c.dim ** -0.5 * torch.randn(c.dim, c.C, c.k, generator=g, dtype=F64), BF)
        du = rnd(0.3 * torch.randn(Mi, c.dim, generator=g, dtype=F64), BF)
    else:
        xin, w, du = randint(g, -1, 1, c.B * rows_in + 8, c.C), randint(g, -1, 1, c.dim, c.C, c.k), randint(g, -1, 1, Mi, c.dim)
    return dict(xin=xin, w=w, du=du)


def cl_view(c, xin):
    """the strided view over the whole buffer: row m = xin rows s m .. s m + k - 1 -> [Mi, k, C]"""
    Mi = c.B * c.rows_out
    return torch.stack([xin[j:j + c.s * Mi:c.s][:Mi] for j in range(c.k)], 1)


def cl_ref(c, inp, mutant=None):
    """-> dict(dW [dim, C, k], dX [B rows_in + 8, C] exact, taps: the per-tap GEMM results [k][Mi, C], mag likewise, worst |intermediate|)"""
    Mi = c.B * c.rows_out
    xin, w, du = inp["xin"], inp["w"], inp["du"]
    dW = torch.einsum("md,mkc->dck", du, cl_view(c, xin))
    dX = torch.zeros_like(xin)
    taps, mags, worst = [], [], 0.0
    for j in range(c.k):
        y = du @ w[:, :, j]
        taps.append(y)
        mags.append(du.abs() @ w[:, :, j].abs())
        tgt = dX[j:j + c.s * Mi:c.s]
        if mutant == "slack_tap_dropped" and j >= c.s:
            y = y.clone()
            y[Mi - 1] = 0
        if mutant == "tap_overwrites" and j >= c.s:
            tgt[:Mi] = y
        else:
            tgt[:Mi] += y
        worst = max(worst, float(y.abs().max()), float(dX.abs().max()))
    return dict(dW=dW, dX=dX, taps=taps, mags=mags, worst=worst)


def cl_gemm_case(c, j):
    """the GemmCase of tap j's product (M = Mi, N = C, K = dim; a residual from tap s on) with its dispatch path"""
    g = Gm._c(f"{c.id}-tap{j}", "?", 0, "real", c.B * c.rows_out, c.C, c.dim, ldc=c.s * c.C, res=j >= c.s, bias=False, out=16)
    return g._replace(path=Gm.dispatch(g)["path"])


def cl_real_bound(c, inp):
    """-> (dX ref, dX bound, dW ref, dW bound, the store part of dX's bound).  Tap j < s: K U_ACC sum|terms| and one bf16 store.  Tap j >= s adds in place to the STORED value r of tap j - s (error e_r):
    once:  e_r + K U_ACC sum|terms| + U |y + r| + BF_STORE |y + r|;   twice: BF_STORE |y| on top (gemm_ref.rounding_points)"""
    Mi = c.B * c.rows_out
    ref = cl_ref(c, inp)
    dX, bound, store = ref["dX"], torch.zeros_like(ref["dX"]), torch.zeros_like(ref["dX"])
    run = torch.zeros_like(dX)
    for j in range(c.k):
        y, mag = ref["taps"][j], ref["mags"][j]
        rows = slice(j, j + c.s * Mi, c.s)
        acc = c.dim * Gm.U_ACC * mag
        if j < c.s:
            run[rows] = y
            bound[rows] = acc + BF_STORE * y.abs()
            store[rows] = BF_STORE * y.abs()
        else:
            tot = run[rows][:Mi] + y
            twice = Gm.rounding_points(cl_gemm_case(c, j)) == "twice"
            st = BF_STORE * tot.abs() + (BF_STORE * y.abs() if twice else 0)
            bound[rows] = bound[rows][:Mi] + acc + U * tot.abs() + st
            store[rows] = store[rows][:Mi] + st
            run[rows] = tot
    S = L.wg_split(Mi, c.dim, c.k * c.C)[0]
    bW = (Mi + S + 1) * U * torch.einsum("md,mkc->dck", inp["du"].abs(), cl_view(c, inp["xin"]).abs())
    return dX, bound, ref["dW"], bW, store


MUTANTS = {"c0b": ("var_T0m1", "m_over_grad_frames", "mean_terms_skipped", "m1_dropped", "tanh_gelu", "one_sweep_f32"),
           "rows": ("mask_t_le_valid", "reverse_rows_b_minus_t", "slab_row_t"), "adj": ("mask_t_le_valid", "slab_row_t"),
           "pw": ("gap_Kw_minus_1", "lead_minus_1", "last_chunk_dropped", "tq_padding_not_zero"), "cl": ("tap_overwrites", "slack_tap_dropped")}

"""Plain fp64 statements, case lists, deterministic inputs and DERIVED per-element bounds of the bf16 kernels of the layer-training path (csrc/train_hubert.hip
apart from its attention kernels: sc_layernorm_bwd_bf16, sc_gelu_bwd_bf16, sc_colsum_bf16, sc_axpy_bf16, sc_cls_pool_dz, sc_transpose_bf16) and of the host-side
split-K weight gradient built on them (train_hubert.wgrad), for tests/test_layer_kernels_parity_gpu.py and tools/layer_kernel_bounds.py.  A helper module, not a test;
no kernel runs here.  The constants, the generator, the rounding helper, the judge, Bd and Group are those of tests/row_kernels_ref.py and tests/tail_kernels_ref.py
and are imported, not restated.

Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE (bf16 operands, fp32 parameters and scalars) before the reference sees
it; every reference is torch fp64 of exactly the stated operation; every bound function returns, per output, a tensor of the output's shape.

The rules of the bounds are those of row_kernels_ref.py's header: an n-term fp32 sum n U sum|terms| against the MAGNITUDE reference; every other fp32 operation U;
hardware rcp / rsq / exp and the `/` lowered to them TR each; __expf(a): |a| 2^-23 on top; one bf16 store BF_STORE |ref|.  fast_erf carries the project's own figure
GELU_PRECISE (1.5e-7 absolute, common.h); its fp32 EVALUATION (one rcp, one exp, six FMAs on the complement poly(t) exp(-a^2) = erfc|a|) is budgeted
erfc|a| (2 TR + 6 U + 3 a^2 U) as tail_kernels_ref.sk_ref budgets it -- a budget, not a documented figure.
One absolute FLOOR is added: an output whose value lies below the smallest normal fp32 number (2^-126) may be flushed to zero by the kernel or the compiler (a
subnormal product, __expf of an argument below -87, the reciprocal of a number above 2^126), so every bound of the GELU backward carries + 2^-126.

Case ids name the dispatch path they reach (ln_bwd/vec/rpb32/D768/rows4097, colsum16/rpb128/st2loop+tail/...), so the table the GPU test prints shows both sides of
every threshold by name.  Groups (tail_kernels_ref.Group): inputs(c) -> dict of fp64 tensors; ref(c, inp, mutant) -> dict output -> fp64 tensor (None: the mutant
cannot differ on this case); bound(c, inp) -> dict output -> Bd(bound, store, limit); emulate(c, inp, order) -> the outputs from a torch fp32 emulation."""
import collections
import math

import torch

from row_kernels_ref import (BF, BF_STORE, F32, F64, GELU_PRECISE, LN_EPS, ORDERS, PAST_VALUE, ROW_MEANS, ROW_STDS, SENT16, SENT32, TR, U, fsum, gen, rnd,  # noqa: F401
                             store_bound, worst)
from tail_kernels_ref import Bd, Group, f32v, fma32, loguniform, signs, t32

FLOOR = 2.0 ** -126


def bfr(t):
    """fp32 tensor -> the bf16 the kernel stores (round to nearest even), fp64 back"""
    return t.to(BF).to(F64)


# ================================================================================================ sc_layernorm_bwd_bf16
LNBCase = collections.namedtuple("LNBCase", "id kern rpb D rows")
LNB_D_SCALAR, LNB_D_VEC = (64, 192, 960), (256, 768, 1024)
LNB_ROWS_SMALL, LNB_ROWS_LARGE = (1, 3, 4, 5), (4095, 4096, 4097, 4096 + 33)
LNB_D_LARGE = (64, 960, 256, 768)                       # the large row counts run at two values of D per kernel
LNB_MUTANTS = ("s2_missing", "s1_missing", "gamma_missing_in_dx", "dgamma_from_g_dy", "eps_outside", "mean_Dm64", "last_chunk_partial_dropped",
               "wave3_rows_dropped", "var_Dm1")


def lnb_partials(rows):
    """sc_layernorm_bwd_bf16_partials restated: a block owns 32 consecutive rows from 4096 rows on, 4 below -> (partial rows, rows per block)"""
    rpb = 32 if rows >= 4096 else 4
    return -(-rows // rpb), rpb


def lnb_kernel(D):
    return "vec" if D % 256 == 0 else "scalar"


def lnb_cases():
    out = []
    for D in LNB_D_SCALAR + LNB_D_VEC:
        for rows in LNB_ROWS_SMALL + (LNB_ROWS_LARGE if D in LNB_D_LARGE else ()):
            rpb = lnb_partials(rows)[1]
            out.append(LNBCase(f"ln_bwd/{lnb_kernel(D)}/rpb{rpb}/D{D}/rows{rows}", lnb_kernel(D), rpb, D, rows))
    return out


def lnb_inputs(c):
    """x bf16: row r has mean ROW_MEANS[r % 4] and std ROW_STDS[(r // 4 + r) % 3] (small: 2^-5 |mean|, or 1e-2 at mean 0: rstd near 1 / sqrt(eps)); dy bf16 randn;
    gamma fp32 0.3 + randn (mixed signs) with ONE element exactly zero"""
    g_ = gen("lnb", c.D, c.rows)
    x = torch.randn(c.rows, c.D, generator=g_, dtype=F64)
    r = torch.arange(c.rows)
    m = torch.tensor(ROW_MEANS, dtype=F64)[r % 4]
    k = (r // 4 + r) % 3
    s = torch.where(k == 0, torch.where(m != 0, 2.0 ** -5 * m.abs(), torch.full_like(m, 1e-2)), torch.where(k == 1, torch.ones_like(m), torch.full_like(m, 30.0)))
    x = x * s.view(-1, 1) + m.view(-1, 1)
    dy = torch.randn(c.rows, c.D, generator=g_, dtype=F64)
    gamma = 0.3 + torch.randn(c.D, generator=g_, dtype=F64)
    gamma[c.D // 3] = 0.0
    return dict(x=rnd(x, BF), dy=rnd(dy, BF), gamma=rnd(gamma, F32))


def _lnb_parts(c, inp, mutant=None, eps=LN_EPS):
    x, dy, gamma = inp["x"], inp["dy"], inp["gamma"]
    rows, D = x.shape
    if mutant == "mean_Dm64":
        if D == 64:
            return None
        mean = x[:, :D - 64].mean(-1, keepdim=True)
    else:
        mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / ((D - 1) if mutant == "var_Dm1" else D)
    rstd = 1 / (var.sqrt() + eps) if mutant == "eps_outside" else 1 / (var + eps).sqrt()
    xh = d * rstd
    gv = dy * gamma
    s1, s2 = gv.mean(-1, keepdim=True), (gv * xh).mean(-1, keepdim=True)
    return dict(mean=mean, d=d, var=var, rstd=rstd, xh=xh, gv=gv, s1=s1, s2=s2)


def _chunk_sums(t, rpb):
    """[rows, D] -> [chunks, D]: the sums over blocks of rpb consecutive rows"""
    rows, D = t.shape
    n = -(-rows // rpb)
    return torch.nn.functional.pad(t, (0, 0, 0, n * rpb - rows)).view(n, rpb, D).sum(1)


def lnb_ref(c, inp, mutant=None):
    """dx = rstd (g dy - mean(g dy) - xh mean(g dy xh)), xh = (x - mean) rstd, biased variance, eps inside the root; part[k] = (sum dy xh, sum dy) over the rows of
    chunk k; dgamma / dbeta = the column sums of the partial rows"""
    q = _lnb_parts(c, inp, mutant)
    if q is None:
        return None
    dy, rows = inp["dy"], c.rows
    nparts, rpb = lnb_partials(rows)
    gv = dy if mutant == "gamma_missing_in_dx" else q["gv"]
    s1 = 0 * q["s1"] if mutant == "s1_missing" else gv.mean(-1, keepdim=True) if mutant == "gamma_missing_in_dx" else q["s1"]
    s2 = 0 * q["s2"] if mutant == "s2_missing" else (gv * q["xh"]).mean(-1, keepdim=True) if mutant == "gamma_missing_in_dx" else q["s2"]
    dx = q["rstd"] * (gv - s1 - q["xh"] * s2)
    tg = (q["gv"] if mutant == "dgamma_from_g_dy" else dy) * q["xh"]
    tb = dy.clone()
    if mutant == "wave3_rows_dropped":
        keep = ((torch.arange(rows) % rpb) % 4 != 3).to(F64).view(-1, 1)
        if bool(keep.all()):
            return None
        tg, tb = tg * keep, tb * keep
    part = torch.stack([_chunk_sums(tg, rpb), _chunk_sums(tb, rpb)], 1)          # [nparts, 2, D]
    if mutant == "last_chunk_partial_dropped":
        part[-1] = 0
    return dict(dx=dx, part=part, dgamma=part[:, 0].sum(0), dbeta=part[:, 1].sum(0))


def lnb_pre(c, inp, eps=LN_EPS):
    """the fp32 error of dx before its store, and of the terms of the partials -> dict(dx, e_xh)
    mean = sum(x) / D: |d mean| <= U sum|x| + TR |mean| (the D-term sum, divided by D; the division TR).  rstd = rsq(sum(d^2) / D + eps): relative
    e_rstd = ((D + 4) U + TR + d mean^2 / (var + eps)) / 2 + TR.  xh = (x - mean) rstd: e_xh = rstd (|d mean| + U |d|) + |xh| (e_rstd + U): the mean's error is
    MULTIPLIED by rstd, which reaches 1 / sqrt(eps) on the near-constant rows.  gv = g dy: U |gv|.  s1 = sum(gv) / D: ((D + 1) U + TR) sum|gv| / D.
    s2 = sum(gv xh) / D: (sum|gv| e_xh + ((D + 2) U + TR) sum|gv xh|) / D.  t = gv - s1 - xh s2: the three terms' errors, |s2| e_xh + |xh| e_s2 for the product,
    3 U (|gv| + |s1| + |xh s2|) for the product and the two differences.  dx = rstd t: rstd e_t + |dx| (e_rstd + U): stated against rstd (|gv| + |s1| + |xh s2|)."""
    q = _lnb_parts(c, inp)
    x = inp["x"]
    D = c.D
    dmean = U * x.abs().sum(-1, keepdim=True) + TR * q["mean"].abs()
    e_rstd = 0.5 * ((D + 4) * U + TR + dmean ** 2 / (q["var"] + eps)) + TR
    xh, gv, s1, s2, rstd = q["xh"], q["gv"], q["s1"], q["s2"], q["rstd"]
    e_xh = rstd * (dmean + U * q["d"].abs()) + xh.abs() * (e_rstd + U)
    e_s1 = ((D + 1) * U + TR) * gv.abs().sum(-1, keepdim=True) / D
    e_s2 = ((gv.abs() * e_xh).sum(-1, keepdim=True) + ((D + 2) * U + TR) * (gv * xh).abs().sum(-1, keepdim=True)) / D
    e_t = U * gv.abs() + e_s1 + s2.abs() * e_xh + xh.abs() * e_s2 + 3 * U * (gv.abs() + s1.abs() + (xh * s2).abs())
    dx = rstd * (gv - s1 - xh * s2)
    return dict(dx=rstd * e_t + dx.abs() * (e_rstd + U), e_xh=e_xh, xh=xh)


def lnb_bound(c, inp):
    """dx: lnb_pre + one bf16 store.  part[k][0]: every term dy xh carries |dy| (e_xh + U |xh|), the chunk's n_k-term sum (per wave, then the four waves) n_k U
    sum|dy xh|; part[k][1]: n_k U sum|dy|.  dgamma / dbeta: the partials' errors summed + the (nparts + 1)-term fp32 column sum of them."""
    ref, pre = lnb_ref(c, inp), lnb_pre(c, inp)
    dy = inp["dy"]
    nparts, rpb = lnb_partials(c.rows)
    nk = _chunk_sums(torch.ones(c.rows, 1, dtype=F64), rpb)                                          # rows in each chunk
    e_g = _chunk_sums(dy.abs() * (pre["e_xh"] + U * pre["xh"].abs()), rpb) + nk * U * _chunk_sums((dy * pre["xh"]).abs(), rpb)
    e_b = nk * U * _chunk_sums(dy.abs(), rpb)
    e_part = torch.stack([e_g, e_b], 1)
    e_dg = e_g.sum(0) + (nparts + 1) * U * ref["part"][:, 0].abs().sum(0)
    e_db = e_b.sum(0) + (nparts + 1) * U * ref["part"][:, 1].abs().sum(0)
    st = BF_STORE * ref["dx"].abs()
    f32st = lambda e, r: Bd(e, torch.minimum(U * r.abs(), e), 0.5)      # noqa: E731
    return dict(dx=Bd(pre["dx"] + st, st, 0.5), part=f32st(e_part, ref["part"]), dgamma=f32st(e_dg, ref["dgamma"]), dbeta=f32st(e_db, ref["dbeta"]))


def lnb_emulate(c, inp, order, eps=LN_EPS):
    x, dy, gamma = (inp[k].to(F32) for k in ("x", "dy", "gamma"))
    rows, D = x.shape
    nparts, rpb = lnb_partials(rows)
    mean = (fsum(x, order) / D).unsqueeze(-1)
    d = x - mean
    rstd = torch.rsqrt(fsum(d * d, order) / D + t32(eps)).unsqueeze(-1)
    xh = d * rstd
    gv = dy * gamma
    s1, s2 = (fsum(gv, order) / D).unsqueeze(-1), (fsum(gv * xh, order) / D).unsqueeze(-1)
    dx = rstd * (gv - s1 - xh * s2)
    tg, tb = dy * xh, dy
    part = torch.zeros(nparts, 2, D, dtype=F32)
    for k in range(nparts):
        for j, t in enumerate((tg, tb)):
            seg = t[k * rpb:(k + 1) * rpb]
            if order == "seq":
                part[k, j] = fsum(seg.t().contiguous(), "seq")
            else:       # the kernel's own shape: wave w sums rows w, w + 4, ...; then (w0 + w1) + (w2 + w3)
                w = [fsum(seg[i::4].t().contiguous(), "seq") if seg[i::4].shape[0] else torch.zeros(D, dtype=F32) for i in range(4)]
                part[k, j] = (w[0] + w[1]) + (w[2] + w[3])
    sums = fsum(part.view(nparts, 2 * D).t().contiguous(), order)
    return dict(dx=bfr(dx), part=part.to(F64), dgamma=sums[:D].to(F64), dbeta=sums[D:].to(F64))


def slope_check(got, ref, pre):
    """The sub-ulp check of a bf16 output: per row of `ref` (the last dim; a 1-d tensor is one row) the slope sum(got ref) / sum(ref ref) against the same slope of the
    fp64 reference ROUNDED to bf16 (which removes the rounding's own bias).  Allowance, derived as in row_kernels_ref.ln_scale_offset: an fp32 error e_i before the
    store reaches the slope as e_i itself plus the roundings it flips -- a fraction 2 e_i / ulp_i of the elements move by one ulp_i, i.e. by 2 e_i again:
    3 sum(pre |ref|) / sum(ref^2); the flips scatter with variance sum(2 pre_i ulp_i ref_i^2), ulp_i <= 2^-7 |ref_i|: four standard deviations of it.
    -> (worst slope difference / allowance over the rows, that row, the smallest allowance of any row)"""
    if ref.dim() == 1:
        got, ref, pre = got.view(1, -1), ref.view(1, -1), pre.view(1, -1)
    got = got.reshape(ref.shape)
    zz = (ref * ref).sum(-1)
    ok = zz > 0
    rr = bfr(ref.to(F32))
    diff = (((got - rr) * ref).sum(-1) / zz.clamp_min(1e-300)).abs()
    allow = (3 * (pre * ref.abs()).sum(-1) + 4 * (2 * pre * 2.0 ** -7 * ref.abs() ** 3).sum(-1).sqrt()) / zz.clamp_min(1e-300)
    ratio = torch.where(ok, diff / allow.clamp_min(1e-300), torch.zeros_like(diff))
    r = int(ratio.argmax())
    return float(ratio[r]), r, float(allow[ok].min()) if bool(ok.any()) else 0.0


# ================================================================================================ sc_gelu_bwd_bf16
GBCase = collections.namedtuple("GBCase", "id kind n")          # kind: allbits | tail | slope
GB_TAIL_N = (0, 2, 6, 8, 10, 8 * 256 + 2, 8 * 256 + 4, 8 * 256 + 6)
GB_MUTANTS = ("tanh_form", "cdf_alone", "fit_derivative", "last_pair_dropped", "dh_u_swapped")
GB_FIT = (1.59491694, 0.0741006897, -7.17464634e-4)             # the forward's sigmoid-of-quintic fit (common.h): x sigmoid(a x + b x^3 + c x^5), x clamped to +-8


def gb_path(n):
    """which code of gelu_bwd_bf16_kernel a length reaches: lanes of 8 elements (16 bytes), the last lane pair by pair when n % 8 != 0"""
    return ("vec8" if n >= 8 else "") + ("+" if n >= 8 and n % 8 else "") + (f"tail{n % 8}" if n % 8 else "") or "empty"


def gb_cases():
    out = [GBCase("gelu_bwd/allbits/n65280/vec8", "allbits", 65280)]
    out += [GBCase(f"gelu_bwd/tail/n{n}/{gb_path(n)}", "tail", n) for n in GB_TAIL_N]
    out.append(GBCase("gelu_bwd/slope/n4096/vec8", "slope", 4096))
    return out


def gb_all_finite_bits():
    """every bf16 bit pattern that is neither NaN nor infinity: 65280 of them, as fp64"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xff) != 0xff]
    return bits.to(torch.int16).view(BF).to(F64)


def gb_inputs(c):
    """allbits: u = every finite bf16 value (in a fixed shuffle), dh mixed signs with sizes log-uniform over [1e-3, 1e2]; tail: u randn 2; slope: u uniform in [-4, 4]"""
    g_ = gen("gelubwd", c.kind, c.n)
    if c.kind == "allbits":
        u = gb_all_finite_bits()
        u = u[torch.randperm(u.numel(), generator=g_)]
    elif c.kind == "slope":
        u = 8 * torch.rand(c.n, generator=g_, dtype=F64) - 4
    else:
        u = 2 * torch.randn(c.n, generator=g_, dtype=F64)
    dh = loguniform(g_, c.n, 1e-3, 1e2) * signs(g_, c.n)
    return dict(u=rnd(u, BF), dh=rnd(dh, BF))


def _gb_f(u, mutant=None):
    """gelu'(u) = Phi(u) + u phi(u) in fp64 (Phi through erfc: no cancellation in the negative tail)"""
    if mutant == "tanh_form":
        uu = u.clone().requires_grad_(True)
        return torch.autograd.grad(torch.nn.functional.gelu(uu, approximate="tanh").sum(), uu)[0]
    if mutant == "fit_derivative":
        uu = u.clone().requires_grad_(True)
        xc = uu.clamp(-8, 8)
        y = uu * torch.sigmoid(GB_FIT[0] * xc + GB_FIT[1] * xc ** 3 + GB_FIT[2] * xc ** 5)
        return torch.autograd.grad(y.sum(), uu)[0]
    cdf = 0.5 * torch.erfc(-u / 2 ** 0.5)
    if mutant == "cdf_alone":
        return cdf
    return cdf + u * (2 * math.pi) ** -0.5 * torch.exp(-0.5 * u * u)


def gb_ref(c, inp, mutant=None):
    u, dh = inp["u"], inp["dh"]
    if c.n == 0:
        return None if mutant else dict(du=torch.zeros(0, dtype=F64))
    if mutant == "dh_u_swapped":
        u, dh = dh, u
    if mutant == "last_pair_dropped":
        if c.n % 8 == 0:
            return None
        out = dh * _gb_f(u)
        out[-2:] = SENT16                                       # what the guarded output holds where nothing was written
        return dict(du=out)
    return dict(du=dh * _gb_f(u, mutant))


def gb_pre(c, inp):
    """a = u / sqrt 2 rounds once and its constant once: erf moves by (2 / sqrt pi) e^(-a^2) 2 U |a|.  fast_erf: GELU_PRECISE absolute, its fp32 evaluation
    erfc|a| (2 TR + 6 U + 3 a^2 U) (the module header's budget: rcp, exp of a rounded -a^2 with __expf's |a^2| 2^-23, six FMAs) and U |erf| for the 1 - p.
    E = 1 + erf: U |E| -- absolute in |erf|, because E cancels for u < -3.  Phi = E / 2: exact.  u phi(u) = u c __expf(-u^2 / 2): the argument rounds once
    (U |arg| on the result), __expf TR + |arg| 2^-23, the constant and two products 3 U.  f = Phi + u phi: U (|Phi| + |u phi|).  du = dh f: U |du|."""
    u, dh = inp["u"], inp["dh"]
    a = u / 2 ** 0.5
    erf, erfc = torch.erf(a), torch.erfc(a.abs())
    e_erf = 2 / math.pi ** 0.5 * torch.exp(-a * a) * 2 * U * a.abs() + GELU_PRECISE + erfc * (2 * TR + 6 * U + 3 * a * a * U) + U * erf.abs()
    cdf = 0.5 * torch.erfc(-a)
    arg = 0.5 * u * u
    upd = u * (2 * math.pi) ** -0.5 * torch.exp(-arg)
    e_f = 0.5 * (e_erf + U * (1 + erf).abs()) + upd.abs() * (TR + arg * (2.0 ** -23 + U) + 3 * U) + U * (cdf + upd.abs())
    ref = dh * (cdf + upd)
    return dh.abs() * e_f + U * ref.abs() + FLOOR


def gb_bound(c, inp):
    ref = gb_ref(c, inp)["du"]
    if c.n == 0:
        return dict(du=Bd(ref, ref, 0.5))
    st = BF_STORE * ref.abs()
    return dict(du=Bd(gb_pre(c, inp) + st, st, 0.5))


def gb_emulate(c, inp, order):
    """"seq": torch's fp32 erf / exp; "pair64": the transcendentals exact (fp64, rounded once), everything around them fp32 -- fast_erf's own error is a constant
    of the bound"""
    u, dh = inp["u"].to(F32), inp["dh"].to(F32)
    fn = (lambda f, t: f(t)) if order == "seq" else (lambda f, t: f(t.to(F64)).to(F32))
    cdf = t32(0.5) * (t32(1.0) + fn(torch.erf, u * t32(0.70710678118654752)))
    f = cdf + u * t32(0.3989422804014327) * fn(torch.exp, t32(-0.5) * u * u)
    return dict(du=bfr(dh * f))


# ================================================================================================ sc_colsum_bf16
CBCase = collections.namedtuple("CBCase", "id rows cols ld acc")
CB_ROWS_SMALL = (1, 3, 4, 5, 63, 64, 65, 64 * 8, 64 * 8 + 1, 64 * 9 + 7)
CB_ROWS_LARGE = (65535, 65536, 65536 + 129)
CB_COLS, CB_COLS_WIDE, CB_ROWS_WIDE, CB_GAP = (1, 7, 256, 257), 2304, (1, 5, 65), 24
CB_MUTANTS = ("rows_mod4_tail_dropped", "last_partial_dropped", "stage2_tail_dropped", "accumulate_ignored", "accumulate_always", "ld_as_cols")


def cb_chunks(rows):
    """sc_colsum_bf16's chunk rule restated: 128 rows per block from 65536 rows on, 64 below -> (partial rows, rows per block)"""
    rpb = 128 if rows >= 65536 else 64
    return -(-rows // rpb), rpb


def cb_workspace_bytes(rows, cols):
    return cb_chunks(rows)[0] * cols * 4


def cb_path(rows):
    n, rpb = cb_chunks(rows)
    st2 = "st2loop" if n >= 8 and n % 8 == 0 else "st2loop+tail" if n >= 8 else "st2tail"
    return f"rpb{rpb}/{st2}"


def cb_cases():
    out = []

    def add(rows, cols, wide, acc):
        ld = cols + CB_GAP if wide else cols
        out.append(CBCase(f"colsum16/{cb_path(rows)}/{rows}x{cols}/ld{'+24' if wide else '=cols'}/{'acc' if acc else 'set'}", rows, cols, ld, acc))
    for rows in CB_ROWS_SMALL:
        for cols in CB_COLS:
            for wide in (False, True):
                for acc in (0, 1):
                    add(rows, cols, wide, acc)
    for i, rows in enumerate(CB_ROWS_WIDE):
        for j in range(2):
            add(rows, CB_COLS_WIDE, (i + j) % 2 == 1, j)
    # the large row counts: every one at 7 and 257 columns, both leading dimensions and both values of accumulate at each
    for i, rows in enumerate(CB_ROWS_LARGE):
        for k, cols in enumerate((7, 257)):
            for j in range(2):
                add(rows, cols, (i + j + k) % 2 == 1, 1 - j)
    return out


def cb_inputs(c):
    """x bf16 [rows, ld]: randn + a per-column offset in {0.5, 1.0} (a dropped row shows in every column); the gap columns hold PAST_VALUE; out0 fp32 non-zero"""
    g_ = gen("colsum16", c.rows, c.cols, c.ld)
    x = torch.randn(c.rows, c.ld, generator=g_, dtype=F64) + 0.5 * (1 + torch.arange(c.ld) % 2).to(F64)
    x[:, c.cols:] = PAST_VALUE
    return dict(x=rnd(x, BF), out0=rnd(3.0 + torch.rand(c.cols, generator=g_, dtype=F64), F32))


def cb_ref(c, inp, mutant=None):
    x, out0 = inp["x"], inp["out0"]
    nparts, rpb = cb_chunks(c.rows)
    if mutant == "ld_as_cols":
        if c.ld == c.cols or c.rows == 1:
            return None
        xs = x.reshape(-1)[:c.rows * c.cols].view(c.rows, c.cols)
    else:
        xs = x[:, :c.cols]
    n = c.rows
    if mutant == "rows_mod4_tail_dropped":
        if c.rows % 4 == 0:
            return None
        n = c.rows - c.rows % 4
    if mutant == "last_partial_dropped":
        n = (nparts - 1) * rpb
    if mutant == "stage2_tail_dropped":
        if nparts % 8 == 0:
            return None
        n = (nparts - nparts % 8) * rpb
    s = xs[:n].sum(0)
    acc = 0 if mutant == "accumulate_ignored" else 1 if mutant == "accumulate_always" else c.acc
    if mutant in ("accumulate_ignored", "accumulate_always") and acc == c.acc:
        return None
    return dict(out=s + out0 if acc else s)


def cb_bound(c, inp):
    """a sum of rows (+ 1 with accumulate) terms in the kernel's fixed order -- four interleaved partials per chunk, eight over the chunks, their trees:
    (rows + 1) U (sum|x| + |out0|)"""
    mag = inp["x"][:, :c.cols].abs().sum(0) + (inp["out0"].abs() if c.acc else 0.0)
    ref = cb_ref(c, inp)["out"]
    b = (c.rows + 1) * U * mag
    return dict(out=Bd(b, torch.minimum(U * ref.abs(), b), 0.5))


def _seq_rows(t):
    """fp32 [n, cols] -> the left-to-right sum over the rows"""
    s = torch.zeros(t.shape[1], dtype=F32)
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


def cb_emulate(c, inp, order):
    x = inp["x"][:, :c.cols].to(F32)
    if order == "seq":
        s = _seq_rows(x)
    else:               # the kernel's own shape
        nparts, rpb = cb_chunks(c.rows)
        pad = torch.nn.functional.pad(x, (0, 0, 0, nparts * rpb - c.rows)).view(nparts, rpb // 4, 4, c.cols)      # adding a zero is exact
        lanes = torch.zeros(nparts, 4, c.cols, dtype=F32)
        full = (min(c.rows, nparts * rpb) - (nparts - 1) * rpb) // 4                                                # groups of four in the last chunk
        for i in range(rpb // 4):
            lanes = lanes + pad[:, i]
        if c.rows % 4:      # the last chunk's tail rows all go to lane 0, after its groups of four
            last = x[(nparts - 1) * rpb:]
            l4 = torch.zeros(4, c.cols, dtype=F32)
            for i in range(full):
                l4 = l4 + last[4 * i:4 * i + 4]
            for i in range(4 * full, last.shape[0]):
                l4[0] = l4[0] + last[i]
            lanes[-1] = l4
        part = (lanes[:, 0] + lanes[:, 1]) + (lanes[:, 2] + lanes[:, 3])
        a = torch.zeros(8, c.cols, dtype=F32)
        p = 0
        while p + 8 <= nparts:
            a = a + part[p:p + 8]
            p += 8
        for i in range(p, nparts):
            a[0] = a[0] + part[i]
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))
    if c.acc:
        s = inp["out0"].to(F32) + s
    return dict(out=s.to(F64))


# ================================================================================================ sc_axpy_bf16
AXCase = collections.namedtuple("AXCase", "id n alpha")
AX_N, AX_ALPHA = (2, 510, 512, 514, 4096 + 2), (1.0, 0.37, -2.5, 0.0)
AX_CANCEL = 0.37                                                 # every fourth y is bf16(-0.37 x): y + 0.37 x cancels there and the bound is the product's U alone
AX_MUTANTS = ("alpha_bf16", "overwritten", "last_pair_dropped")


def ax_cases():
    return [AXCase(f"axpy/n{n}/{(n // 2 + 255) // 256}blk/alpha{a:g}", n, a) for n in AX_N for a in AX_ALPHA]


def ax_inputs(c):
    g_ = gen("axpy", c.n)
    x = rnd(torch.randn(c.n, generator=g_, dtype=F64) * loguniform(g_, c.n, 1e-2, 1e2), BF)
    y = torch.randn(c.n, generator=g_, dtype=F64) * loguniform(g_, c.n, 1e-2, 1e2)
    y[::4] = -AX_CANCEL * x[::4]
    return dict(x=x, y=rnd(y, BF))


def ax_ref(c, inp, mutant=None):
    """y + alpha x with alpha the fp32 value the kernel receives"""
    x, y = inp["x"], inp["y"]
    alpha = f32v(c.alpha)
    if mutant == "alpha_bf16":
        alpha = float(torch.tensor(c.alpha, dtype=F32).to(BF))
        if alpha == f32v(c.alpha):
            return None
    out = (0.0 if mutant == "overwritten" else y) + alpha * x
    if mutant == "last_pair_dropped":
        out = out.clone()
        out[-2:] = y[-2:]
    return dict(y=out)


def ax_bound(c, inp):
    """the product U |alpha x|, the sum U |y'| (an FMA: the second alone), the bf16 store -- which rounds the fp32 VALUE, so where y + alpha x cancels it carries
    the fp32 error too: (1 + BF_STORE) on it (every operation is IEEE and each U is attained: the emulation is held to the whole bound)"""
    ref = ax_ref(c, inp)["y"]
    st = BF_STORE * ref.abs()
    return dict(y=Bd((U * (f32v(c.alpha) * inp["x"]).abs() + U * ref.abs()) * (1 + BF_STORE) + st, st, 1.0))


def ax_emulate(c, inp, order):
    return dict(y=bfr(fma32(t32(c.alpha), inp["x"].to(F32), inp["y"].to(F32), order == "pair64")))


# ================================================================================================ sc_cls_pool_dz
PZCase = collections.namedtuple("PZCase", "id B T NQ R D lens ld_dz")
PZ_SHAPES = ((3, 5, 1, 8, 768), (2, 9, 2, 4, 80), (1, 1, 1, 1, 64), (2, 7, 1, 8, 260))
PZ_LENS = {(3, 5): ((0, 5, 2),), (2, 9): ((9, 4), (0, 5)), (1, 1): ((1,), (0,)), (2, 7): ((7, 3), (0, 7))}
PZ_MUTANTS = ("nq_offset_missing", "ds_term_missing", "pp_term_missing", "masked_rows_not_zeroed", "r_to_Rm1")


def pz_cases():
    out = []
    for (B, T, NQ, R, D) in PZ_SHAPES:
        for lens in PZ_LENS[(B, T)]:
            for wide in (False, True):
                out.append(PZCase(f"cls_pool_dz/B{B}-T{T}-NQ{NQ}-R{R}-D{D}/lens{'-'.join(map(str, lens))}/ld{'+8' if wide else '=D'}", B, T, NQ, R, D, lens,
                                  D + 8 if wide else D))
    return out


def pz_inputs(c):
    """pp, ds fp32 [B, R, NQ + T]: the first NQ columns of every row (the CLS keys, which no frame's gradient reads) hold PAST_VALUE; dzbar [B, R, D], u [R, D]"""
    g_ = gen("poolz", c.B, c.T, c.NQ, c.R, c.D)
    rn = lambda *s: torch.randn(*s, generator=g_, dtype=F64)      # noqa: E731
    pp, ds = rn(c.B, c.R, c.NQ + c.T).abs() / c.T, rn(c.B, c.R, c.NQ + c.T)
    pp[:, :, :c.NQ] = PAST_VALUE
    ds[:, :, :c.NQ] = PAST_VALUE
    return dict(pp=rnd(pp, F32), ds=rnd(ds, F32), dzbar=rnd(rn(c.B, c.R, c.D), F32), u=rnd(rn(c.R, c.D), F32))


def _pz_terms(c, inp, mutant=None):
    off = 0 if mutant == "nq_offset_missing" else c.NQ
    R = c.R - 1 if mutant == "r_to_Rm1" else c.R
    pp, ds = inp["pp"][:, :R, off:off + c.T], inp["ds"][:, :R, off:off + c.T]                      # [B, R, T]
    a = torch.einsum("brt,brd->btrd", pp, inp["dzbar"][:, :R])
    b = torch.einsum("brt,rd->btrd", ds, inp["u"][:R])
    if mutant == "ds_term_missing":
        b = 0 * b
    if mutant == "pp_term_missing":
        a = 0 * a
    mask = (torch.arange(c.T).view(1, -1) < torch.tensor(c.lens).view(-1, 1)).to(F64).view(c.B, c.T, 1, 1)
    if mutant == "masked_rows_not_zeroed":
        if min(c.lens) == c.T:
            return None
        mask = torch.ones_like(mask)
    return a * mask, b * mask


def pz_ref(c, inp, mutant=None):
    """dz[b, t, :] = sum_r pp[b, r, NQ + t] dzbar[b, r, :] + ds[b, r, NQ + t] u[r, :] for t < lens[b], else exactly 0"""
    q = _pz_terms(c, inp, mutant)
    if q is None:
        return None
    return dict(dz=(q[0] + q[1]).sum(2).view(c.B * c.T, c.D))


def pz_bound(c, inp):
    """a 2 R-term fp32 sum of products: (2 R + 1) U sum|terms|, and one bf16 store; a masked row's bound is 0: it must be exact"""
    a, b = _pz_terms(c, inp)
    mag = (a.abs() + b.abs()).sum(2).view(c.B * c.T, c.D)
    ref = pz_ref(c, inp)["dz"]
    st = BF_STORE * ref.abs()
    return dict(dz=Bd((2 * c.R + 1) * U * mag + st, st, 0.5))


def pz_emulate(c, inp, order):
    pp, ds, dzb, u = (inp[k].to(F32) for k in ("pp", "ds", "dzbar", "u"))
    acc = torch.zeros(c.B, c.T, c.D, dtype=F32)
    for r in (range(c.R) if order == "seq" else reversed(range(c.R))):
        p, s = pp[:, r, c.NQ:].unsqueeze(-1), ds[:, r, c.NQ:].unsqueeze(-1)
        if order == "seq":
            acc = acc + (p * dzb[:, r].unsqueeze(1) + s * u[r])
        else:
            acc = fma32(s, u[r].expand(c.B, c.T, c.D), fma32(p, dzb[:, r].unsqueeze(1).expand(c.B, c.T, c.D), acc, True), True)
    mask = (torch.arange(c.T).view(1, -1) < torch.tensor(c.lens).view(-1, 1)).view(c.B, c.T, 1)
    return dict(dz=bfr(torch.where(mask, acc, torch.zeros_like(acc))).view(c.B * c.T, c.D))


# ================================================================================================ train_hubert.wgrad (real-valued cases)
WGCase = collections.namedtuple("WGCase", "id M N K exact")
WG_M = (48, 4095, 4096, 4097, 6144 + 5)
WG_BINDING = (8192 + 5, 16640, 64)                      # 130 tiles: 512 // 130 = 3 binds below M // 2048 = 4
WG_S32 = (65536, 64, 64)
WG_MUTANTS = ("last_row_dropped", "last_split_dropped", "padding_not_zero")


def wg_split(M, N, K):
    """wgrad's split rule restated from its description -> (S, chunk, Mp, tile).  The product is cut into tiles of 256 x 256 when both N and K reach 256, of
    128 x 128 otherwise.  The number of K-splits S is the smallest of: 32; 512 divided by the number of tiles (rounded down); and one split per 2048 rows of M --
    but no splitting at all below 4096 rows; S is never below 1.  Every split covers `chunk` rows, a multiple of 64, and the S chunks cover Mp >= M rows."""
    tile = 256 if (N >= 256 and K >= 256) else 128
    tiles = -(-N // tile) * (-(-K // tile))
    by_rows = M // 2048 if M >= 4096 else 1
    S = 32
    if 512 // tiles < S:
        S = 512 // tiles
    if by_rows < S:
        S = by_rows
    if S < 1:
        S = 1
    chunk = 64
    while chunk * S < M:
        chunk += 64
    return S, chunk, chunk * S, tile


def wg_clause(M, N, K):
    """the clause of the split rule that decides S: 'floor1' | 'cap32' | 'tiles' | 'rows' | 'below4096'"""
    S, _, _, tile = wg_split(M, N, K)
    tiles = -(-N // tile) * (-(-K // tile))
    if M < 4096:
        return "below4096" if 512 // tiles >= 1 else "floor1"
    if 512 // tiles < 1:
        return "floor1"
    c = {"cap32": 32, "tiles": 512 // tiles, "rows": M // 2048}
    return min(c, key=lambda k: (c[k], ("rows", "tiles", "cap32").index(k)))


def wg_id(M, N, K, kind):
    S, chunk, Mp, tile = wg_split(M, N, K)
    return f"wgrad/{kind}/tile{tile}/{wg_clause(M, N, K)}/S{S}/M{M}-N{N}-K{K}/Mp{Mp}"


def wg_exact_shapes():
    return [(M, n, n) for n in (128, 256) for M in WG_M] + [WG_S32, WG_BINDING]


def wg_cases():
    """the real-valued cases: one per path (one split and several, on either tile size)"""
    return [WGCase(wg_id(M, N, K, "real"), M, N, K, False) for (M, N, K) in ((48, 128, 128), (6144 + 5, 128, 128), (300, 256, 256), (6144 + 5, 256, 256))]


def wg_int_inputs(M, N, K):
    """integers in [-3, 3] (exact in bf16); every partial and total stays below 9 M <= 2^20 < 2^24: an fp32 accumulation in ANY order is exact"""
    g_ = gen("wgrad-int", M, N, K)
    return torch.randint(-3, 4, (M, N), generator=g_, dtype=torch.int8), torch.randint(-3, 4, (M, K), generator=g_, dtype=torch.int8)


def wg_inputs(c):
    g_ = gen("wgrad", c.M, c.N, c.K)
    return dict(dy=rnd(0.3 * torch.randn(c.M, c.N, generator=g_, dtype=F64), BF), x=rnd(0.5 * torch.randn(c.M, c.K, generator=g_, dtype=F64) + 0.1, BF))


def wg_ref(c, inp, mutant=None):
    """dW [N, K] = dy^T x"""
    dy, x = inp["dy"], inp["x"]
    S, chunk, Mp, _ = wg_split(c.M, c.N, c.K)
    if mutant == "last_row_dropped":
        dy = dy[:-1]
        x = x[:-1]
    if mutant == "last_split_dropped":
        if S == 1:
            return None
        dy, x = dy[:(S - 1) * chunk], x[:(S - 1) * chunk]
    out = dy.t() @ x
    if mutant == "padding_not_zero":
        if Mp == c.M:
            return None
        out = out + (Mp - c.M) * SENT16 * SENT16
    return dict(dW=out)


def wg_bound(c, inp):
    """an M-term sum of products of bf16 numbers (each exact in fp32) accumulated in fp32, in S parts that an (S + 1)-term column sum joins:
    (M + S + 1) U sum_m |dy x|; the fp32 store is the sum's own last rounding"""
    S = wg_split(c.M, c.N, c.K)[0]
    mag = inp["dy"].abs().t() @ inp["x"].abs()
    ref = wg_ref(c, inp)["dW"]
    b = (c.M + S + 1) * U * mag
    return dict(dW=Bd(b, torch.minimum(U * ref.abs(), b), 0.5))


def wg_emulate(c, inp, order):
    """"seq": the exact product rounded once per block of 64 rows and accumulated in fp32; "pair64": per split chunk, then the chunks in turn"""
    dy, x = inp["dy"], inp["x"]
    S, chunk, _, _ = wg_split(c.M, c.N, c.K)
    step = 64 if order == "seq" else chunk
    acc = torch.zeros(c.N, c.K, dtype=F32)
    for m in range(0, c.M, step):
        acc = acc + (dy[m:m + step].t() @ x[m:m + step]).to(F32)
    return dict(dW=acc.to(F64))


# ================================================================================================ sc_transpose_bf16 (bit for bit: a case list and a statement)
TRCase = collections.namedtuple("TRCase", "id R C Rp batch ld_in stride_in ld_out stride_out in_off out_off")
TR_RC = (1, 63, 64, 65, 130)


def tr_vec(c):
    """the dispatcher restated: the 8-byte form needs cols, rows_padded, both leading dimensions and both strides multiples of 4 and both bases 8-byte aligned
    (an allocation is; in_off / out_off count bf16 elements from one)"""
    return all(v % 4 == 0 for v in (c.C, c.Rp, c.ld_in, c.ld_out, c.stride_in, c.stride_out, c.in_off, c.out_off))


def _tr(tag, R, C, Rp, batch, ld_in=None, stride_in=None, ld_out=None, stride_out=None, in_off=0, out_off=0):
    ld_in = C if ld_in is None else ld_in
    stride_in = (R * ld_in if ld_in >= C else (R - 1) * ld_in + C) if stride_in is None else stride_in
    ld_out = Rp if ld_out is None else ld_out
    stride_out = C * ld_out if stride_out is None else stride_out
    c = TRCase("", R, C, Rp, batch, ld_in, stride_in, ld_out, stride_out, in_off, out_off)
    return c._replace(id=f"transpose/{'vec' if tr_vec(c) else 'scalar'}/{tag}/R{R}-C{C}-Rp{Rp}-b{batch}")


def tr_pads(R):
    """rows_padded: R itself, the next multiple of 64, and a multiple of 4 that is not a multiple of 64"""
    p4 = -(-R // 4) * 4
    return (R, -(-R // 64) * 64, p4 if p4 % 64 else p4 + 4)


def tr_grid_cases():
    return [_tr("grid", R, C, Rp, b) for R in TR_RC for C in TR_RC for Rp in dict.fromkeys(tr_pads(R)) for b in (1, 3)]      # (R = 64 is its own next multiple)


def tr_vector_cases():
    """the vector form, then each of its conditions failing ALONE; the overlapping-row view on both forms; ld_out > rows_padded and the side-by-side placement"""
    R, C, Rp, b = 130, 64, 132, 3
    base = dict(ld_in=72, stride_in=R * 72 + 8, ld_out=136, stride_out=C * 136 + 4)
    out = [_tr("all-aligned", R, C, Rp, b, **base),
           _tr("cols%4", R, C - 1, Rp, b, **base),
           _tr("rows_padded%4", R, C, Rp - 1, b, **base),
           _tr("ld_in%4", R, C, Rp, b, **dict(base, ld_in=73)),
           _tr("ld_out%4", R, C, Rp, b, **dict(base, ld_out=137, stride_out=C * 137 + 4)),
           _tr("stride_in%4", R, C, Rp, b, **dict(base, stride_in=R * 72 + 10)),
           _tr("stride_out%4", R, C, Rp, b, **dict(base, stride_out=C * 136 + 6)),
           _tr("in-base+4B", R, C, Rp, b, in_off=2, **base),
           _tr("out-base+4B", R, C, Rp, b, out_off=2, **base),
           _tr("overlap-ld_in8", 70, 64, 128, 1, ld_in=8),
           _tr("overlap-ld_in6", 70, 64, 128, 1, ld_in=6),
           _tr("side-by-side", R, C, Rp, b, ld_in=72, stride_in=R * 72, ld_out=b * Rp + 8, stride_out=Rp),
           _tr("side-by-side", 65, 63, 65, b, ld_out=b * 65 + 3, stride_out=65)]
    assert [tr_vec(c) for c in out] == [True] + [False] * 8 + [True, False, True, False]
    return out


def tr_input(c):
    """the flat bf16 input as int16 bit patterns (every element distinct where the size allows), in_off elements into its allocation"""
    n = c.in_off + (c.batch - 1) * c.stride_in + (c.R - 1) * c.ld_in + c.C
    g_ = gen("transpose", c.id)
    return (torch.randperm(max(n, 1), generator=g_) % 0x7f00 + 1).to(torch.int16)[:n]


def tr_ref(c, flat):
    """out[z, col, r] = in[z stride_in + r ld_in + col] for r < R, 0 for R <= r < rows_padded -> int16 [batch, C, Rp]"""
    out = torch.zeros(c.batch, c.C, c.Rp, dtype=torch.int16)
    r, col = torch.arange(c.R).view(-1, 1), torch.arange(c.C).view(1, -1)
    for z in range(c.batch):
        out[z, :, :c.R] = flat[c.in_off + z * c.stride_in + r * c.ld_in + col].t()
    return out


GROUPS = collections.OrderedDict((g.name, g) for g in (
    Group("ln_bwd", lnb_cases, lnb_inputs, lnb_ref, lnb_bound, lnb_emulate, LNB_MUTANTS),
    Group("gelu_bwd", gb_cases, gb_inputs, gb_ref, gb_bound, gb_emulate, GB_MUTANTS),
    Group("colsum16", cb_cases, cb_inputs, cb_ref, cb_bound, cb_emulate, CB_MUTANTS),
    Group("axpy", ax_cases, ax_inputs, ax_ref, ax_bound, ax_emulate, AX_MUTANTS),
    Group("cls_pool_dz", pz_cases, pz_inputs, pz_ref, pz_bound, pz_emulate, PZ_MUTANTS),
    Group("wgrad", wg_cases, wg_inputs, wg_ref, wg_bound, wg_emulate, WG_MUTANTS),
))

"""Plain fp64 statements, case lists, deterministic inputs and DERIVED per-element bounds of the row kernels (csrc/rowops.hip) and of the pooling head
(csrc/attention.hip: cls_attn_kernel, cls_pool_kernel) for tests/test_row_kernels_parity_gpu.py and tools/row_kernel_bounds.py.  A helper module, not a
test; no kernel runs here.

Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE before the reference sees it; every reference is torch
fp64 of exactly the stated operation; every bound function returns a tensor of the output's shape and every element is judged against it.

The rules of the bounds (tests/test_untested_entries_gpu.py states the first three):
    one bf16 store                       <= 2^-8 * 1.001 |ref|          (BF_STORE)
    one IEEE-half store                  <= 2^-11 * 1.001 |ref| + 2^-25 (the second term: half's subnormal spacing below 2^-14)
    an fp32 sum of n terms               within n * 2^-24 * sum|terms|
    every other fp32 operation           2^-24 relative                 (U)
    v_rcp_f32 / v_rsq_f32 / v_exp_f32 / v_sqrt_f32, and the `/` and sqrtf the compiler lowers to them: 2^-22 relative each (TR).  The ISA document is
    not available to this suite, so this is the BUDGETED figure (one ulp of the 1-ulp instructions, with a factor 4), not a documented one.
    exp(a) is formed as exp2(a * log2 e): the subtraction of the maximum and the product each round the ARGUMENT, so the result carries |a| 2^-23 on top.
Terms are carried where the arithmetic amplifies them: the error of a LayerNorm's fp32 mean is multiplied by rstd |gamma| (rows with |mean| >> std are in
the case lists), the error of a score by the probability it produces, and a softmax-weighted sum is judged against sum_k p_k |x_kd| (the MAGNITUDE
reference), not against |ref|.
GELU forms, with the project's own constants: gelu_erf (the sigmoid-of-quintic fit, common.h) 3.0e-5; the packed-half gelu_poly2 3.2e-3 + |want| 2^-7,
which already holds the bf16 store (tests/test_gemm8p_gpu.py); gelu_erf_precise 1.5e-7 (1 + |u|).  |gelu'| <= 1.13 carries the argument's error through."""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from test_dropout_gpu import _keep   # noqa: F401  (the counter-based mask, restated once in the suite)

F64, F32, BF, H16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24
TR = 2.0 ** -22
BF_STORE = 2.0 ** -8 * 1.001
H16_STORE = 2.0 ** -11 * 1.001
GELU_LIP = 1.13
GELU_ERF_FIT, GELU_POLY2_ABS, GELU_POLY2_REL, GELU_PRECISE = 3.0e-5, 3.2e-3, 2.0 ** -7, 1.5e-7
LN_EPS = 1e-5
SENT16, SENT32 = -77.0, -7777.0            # sentinels of the output buffers (exact in bf16 / half / fp32)
PAST_SCORE, PAST_VALUE = 30.0, 1.0e4       # what the first key past `len` carries: reading one key too many is as loud as dropping one


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def rnd(t, dt):
    """the value the kernel reads: rounded to its input type, back in fp64"""
    return t.to(F32).to(dt).to(F64)


def store_bound(ref, dt):
    a = ref.abs()
    if dt == BF:
        return BF_STORE * a
    if dt == H16:
        return H16_STORE * a + 2.0 ** -25
    return U * a


def gelu64(y):
    return 0.5 * y * (1 + torch.erf(y / 2 ** 0.5))


def worst(err, bound):
    """(worst err / bound, flat index); an element whose bound is 0 must be exact"""
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.reshape(-1).argmax()) if ratio.numel() else 0
    return (float(ratio.reshape(-1)[i]) if ratio.numel() else 0.0), i


# ================================================================================================ what every GPU parity test shares
GUARD = 64


class Guarded:
    """a [rows, ld] window inside a sentinel-filled flat buffer; columns < width of every row are the region a kernel may write"""

    def __init__(self, rows, ld, dt, width=None):
        self.rows, self.ld, self.width = rows, ld, ld if width is None else width
        self.sent = SENT32 if dt == F32 else SENT16
        self.buf = torch.full((2 * GUARD + rows * ld,), self.sent, dtype=dt, device="cuda")
        self.win = self.buf[GUARD:GUARD + rows * ld].view(rows, ld)

    def out(self):
        return self.win[:, :self.width]

    def check(self, what):
        flat = self.buf.cpu().to(F64)
        written = torch.zeros(flat.numel(), dtype=torch.bool)
        w = written[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)
        w[:, :self.width] = True
        assert bool((flat[~written] == self.sent).all()), (what, "wrote outside its output region")
        return flat[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width].clone()


def judge(what, got, ref, bound, shape=None):
    got = got.reshape(ref.shape)
    err = (got - ref).abs()
    r, i = worst(err, bound)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.numel() else ()
    print(f"{what:60s} worst err/bound {r:8.4f} at {idx}")
    assert torch.isfinite(got).all(), what
    assert r <= 1.0, (what, "err / bound", r, "at", idx, "got", float(got[idx]), "ref", float(ref[idx]), "bound", float(bound[idx]))
    return r


# ================================================================================================ LayerNorm
LNCase = collections.namedtuple("LNCase", "id path D in_dt out_dt affine gelu ld_in ld_out x_off rows")
LN_ROWS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)
LN_GENERIC_D = (4, 8, 252, 256, 260, 508, 516, 772, 1020, 1024)
ROW_MEANS = (0.0, 3.0, -3.0, 50.0)
ROW_STDS = ("small", 1.0, 30.0)            # small: 2^-5 |mean|, or 1e-2 when the mean is 0
LN_PATHS = ("ln768", "ln512", "ln512_gelu", "ln1024f", "ln1024f_half", "ln768f", "gen_bf_bf", "gen_bf_f32", "gen_f32_bf", "gen_f32_f32", "gen_f32_half")


def ln_cases():
    C, out = LNCase, []
    out += [C("ln768", "ln768", 768, BF, BF, True, False, 768, 768, 0, LN_ROWS), C("ln512", "ln512", 512, BF, BF, True, False, 512, 512, 0, LN_ROWS),
            C("ln512_gelu", "ln512_gelu", 512, BF, BF, True, True, 512, 512, 0, LN_ROWS), C("ln1024f", "ln1024f", 1024, F32, BF, True, False, 1024, 1024, 0, LN_ROWS),
            C("ln1024f_half", "ln1024f_half", 1024, F32, H16, True, False, 1024, 1024, 0, LN_ROWS), C("ln768f", "ln768f", 768, F32, BF, True, False, 768, 768, 0, LN_ROWS)]
    # the fall-backs from a fast shape to the generic kernel
    out += [C("gen_bf_bf-768-ld_in5x", "gen_bf_bf", 768, BF, BF, True, False, 5 * 768, 768, 0, LN_ROWS),
            C("gen_bf_bf-768-x_off4", "gen_bf_bf", 768, BF, BF, True, False, 768, 768, 4, LN_ROWS),
            C("gen_bf_f32-512-out_f32", "gen_bf_f32", 512, BF, F32, True, False, 512, 512, 0, LN_ROWS),
            C("gen_bf_bf-768-noaffine", "gen_bf_bf", 768, BF, BF, False, False, 768, 768, 0, LN_ROWS),
            C("gen_bf_bf-768-gelu", "gen_bf_bf", 768, BF, BF, True, True, 768, 768, 0, LN_ROWS),
            C("gen_bf_bf-768-ld_out", "gen_bf_bf", 768, BF, BF, True, False, 768, 772, 0, LN_ROWS),
            C("gen_f32_bf-1024-gelu", "gen_f32_bf", 1024, F32, BF, True, True, 1024, 1024, 0, LN_ROWS),
            C("gen_f32_bf-768-ld_out", "gen_f32_bf", 768, F32, BF, True, False, 768, 776, 0, LN_ROWS)]
    # the five generic instantiations over the partly filled chunks; the options rotate so that every one meets every instantiation
    inst = (("gen_bf_bf", BF, BF), ("gen_bf_f32", BF, F32), ("gen_f32_bf", F32, BF), ("gen_f32_f32", F32, F32), ("gen_f32_half", F32, H16))
    for pi, (path, i_dt, o_dt) in enumerate(inst):
        for di, D in enumerate(LN_GENERIC_D):
            k = pi + di
            affine, gelu = k % 3 != 0, k % 4 == 1
            ld_in = D + 8 if k % 2 else D
            ld_out = D + 4 if k % 5 in (1, 3) else D
            rows = LN_ROWS if D in (260, 1020) else (1, 3, 9, 33)
            out.append(C(f"{path}-{D}{'-aff' if affine else ''}{'-gelu' if gelu else ''}{'-ldi' if ld_in > D else ''}{'-ldo' if ld_out > D else ''}",
                         path, D, i_dt, o_dt, affine, gelu, ld_in, ld_out, 0, rows))
    return out


def ln_dispatch(c):
    """sc_layernorm's dispatcher restated on a case's arguments (pointers: 16-byte aligned buffers, the input advanced by x_off elements) -> the path's name"""
    esz = 4 if c.in_dt == F32 else 2
    x_al16 = (c.x_off * esz) % 16 == 0
    in32, out32, out16h = c.in_dt == F32, c.out_dt == F32, c.out_dt == H16
    tight = c.ld_in == c.D and c.ld_out == c.D and c.affine
    if c.D == 768 and not (in32 or out32 or out16h or c.gelu) and tight and x_al16:
        return "ln768"
    if c.D == 512 and not (in32 or out32 or out16h) and tight and x_al16:
        return "ln512_gelu" if c.gelu else "ln512"
    if c.D == 1024 and in32 and not out32 and not c.gelu and tight and x_al16:
        return "ln1024f_half" if out16h else "ln1024f"
    if c.D == 768 and in32 and not out32 and not out16h and not c.gelu and tight and x_al16:
        return "ln768f"
    return "gen_" + ("f32" if in32 else "bf") + "_" + ("f32" if out32 else "half" if out16h else "bf")


def ln_inputs(c, rows):
    """x fp64 [rows, D] (values of the input type), gamma / beta fp64 [D] (fp32 values) or None.  Row r: mean ROW_MEANS[r % 4], std ROW_STDS[(r // 4 + r) % 3]
    (all 12 pairs within 12 rows, neighbours always differ); with an affine the LAST row of a block of >= 7 rows is constant (0.25: its fp32 mean is exact)."""
    g = gen("ln", c.id, rows)
    x = torch.randn(rows, c.D, generator=g, dtype=F64)
    for r in range(rows):
        m = ROW_MEANS[r % 4]
        s = ROW_STDS[(r // 4 + r) % 3]
        s = (2.0 ** -5 * abs(m) if m else 1e-2) if s == "small" else s
        x[r] = x[r] * s + m
    if c.affine and rows >= 7:
        x[rows - 1] = 0.25
    gamma = rnd(1 + 0.3 * torch.randn(c.D, generator=g, dtype=F64), F32) if c.affine else None
    beta = rnd(0.3 * torch.randn(c.D, generator=g, dtype=F64), F32) if c.affine else None
    return rnd(x, c.in_dt), gamma, beta


def ln_ref(x, gamma, beta, gelu, eps=LN_EPS, mutant=None):
    """fp64 [gelu]((x - mean) rstd gamma + beta), biased variance, eps inside the root.  -> (out, z) with z = (x - mean) rstd."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if mutant == "mean_Dm4":
        mean = x[..., :D - 4].mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / ((D - 1) if mutant == "var_Dm1" else D)
    rstd = 1 / (var.sqrt() + eps) if mutant == "eps_outside" else 1 / (var + eps).sqrt()
    if mutant == "neighbour_stats" and x.shape[0] > 1:
        mean, rstd = torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0)
        d = x - mean
    z = d * rstd
    g = torch.ones(D, dtype=F64) if gamma is None else gamma
    b = torch.zeros(D, dtype=F64) if beta is None else beta
    if mutant == "affine_shift4":
        g, b = torch.roll(g, 4), torch.roll(b, 4)
    if mutant == "gelu_first" and gelu:
        return gelu64(z) * g + b, z
    y = z * g + b
    return (gelu64(y) if gelu else y), z


def ln_pre_store_error(x, gamma, eps=LN_EPS, dx=None, final_add=True):
    """|error| of the fp32 (x - mean) rstd gamma + beta before any activation or store, per element, and the pieces the scale check needs.
    mean:  sum of D terms, then one division (or a product with the rounded 1 / D): |d mean| <= U (sum|x| + 2 |mean|)
    d_i = x_i - mean: |d mean| + U |d_i|
    var:   each d_i^2 carries 3 U (d's own rounding twice, the product), the sum D U, the division 2 U, the + eps U; the mean's error adds d mean^2 (the cross
           term vanishes: sum d = 0); rsqrt TR and half the relative error of its argument
    y:     |gamma| rstd (|d mean| + U |d|) + |z gamma| (e_rstd + 2 U) + U |y| for the last add
    dx: an elementwise error of the INPUT itself (the fused residual + dropout sum), carried into x_i and into the mean."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1 / (var + eps).sqrt()
    dmean = U * (x.abs().sum(-1, keepdim=True) + 2 * mean.abs())
    dxi = 0.0
    if dx is not None:
        dmean = dmean + dx.mean(-1, keepdim=True)
        dxi = dx
    e_rstd = 0.5 * ((D + 6) * U + dmean ** 2 / (var + eps)) + TR
    g = torch.ones(D, dtype=F64) if gamma is None else gamma.abs()
    z = d * rstd
    err = g * rstd * (dmean + dxi + U * d.abs()) + (z * g).abs() * (e_rstd + 2 * U)
    return err, dict(e_rstd=e_rstd, offset=rstd * dmean, z=z)


def ln_bound(x, gamma, beta, gelu, out_dt, poly2=False, eps=LN_EPS, dx=None):
    ref, _ = ln_ref(x, gamma, beta, gelu, eps)
    pre, _ = ln_pre_store_error(x, gamma, eps, dx)
    y, _ = ln_ref(x, gamma, beta, False, eps)
    pre = pre + U * y.abs()
    if not gelu:
        return store_bound(ref, out_dt) + pre
    if poly2:                                                   # the packed-half form: its constant holds the half input and the bf16 store
        return GELU_POLY2_ABS + GELU_POLY2_REL * ref.abs() + GELU_LIP * pre
    return store_bound(ref, out_dt) + GELU_LIP * pre + GELU_ERF_FIT + (2 * TR + 8 * U) * ref.abs()


def ln_emulate(x, gamma, beta, gelu, out_dt, order, eps=LN_EPS):
    """fp32 two-pass emulation (GELU: the exact erf form in fp32 -- the forms' own errors are constants of the bound), stored to out_dt; fp64 back."""
    x = x.to(F32)
    D = x.shape[-1]
    mean = (fsum(x, order) / D).unsqueeze(-1)
    d = x - mean
    rstd = torch.rsqrt(fsum(d * d, order) / D + torch.tensor(eps, dtype=F32)).unsqueeze(-1)
    y = d * rstd
    if gamma is not None:
        y = y * gamma.to(F32) + beta.to(F32)
    if gelu:
        y = F.gelu(y)
    return y.to(out_dt).to(F64)


def fsum(t, order):
    """fp32 sum over the last dim in a stated order: "seq" (left to right) or "pair64" (a binary tree inside every chunk of 64, the chunks left to right)"""
    assert t.dtype == F32
    if order == "seq":
        s = torch.zeros(t.shape[:-1], dtype=F32)
        for i in range(t.shape[-1]):
            s = s + t[..., i]
        return s
    n = t.shape[-1]
    pad = (-n) % 64
    t = F.pad(t, (0, pad)).reshape(*t.shape[:-1], (n + pad) // 64, 64)
    w = 64
    while w > 1:
        w //= 2
        t = t[..., :w] + t[..., w:2 * w]
    return fsum(t[..., 0], "seq")


ORDERS = ("seq", "pair64")


def ln_scale_offset(got, x, gamma, beta, out_dt, eps=LN_EPS):
    """The sub-ulp check of a 16-bit LayerNorm output WITHOUT GELU.  With u = (got - beta) / gamma and z = (x - mean) rstd in fp64:
        slope  = sum(u z) / sum(z z) over every element        offset_r = mean_i(u - z) of every row r
    both compared with the same statistics of the fp64 reference rounded to the output type (which removes the rounding's own bias).
    Allowances, derived: an error of the fp32 mean is a constant within a row and z sums to zero within a row, so it does not reach the slope except through
    the roundings it flips -- roundings flipped by an error e_i are a fraction 2 e_i / ulp_i of the elements and move the result by one ulp_i, i.e. by 2 e_i
    again.  So  slope: 3 (e_rstd + 3 U, averaged over the rows with the weight sum z^2 of each)  [own error + flips]  + sqrt(mean(offset) 2^-7 / N)  [the scatter of the flips an offset causes; their mean IS
    the offset and is orthogonal to z];   offset_r: the mean's error rstd_r |d mean_r| + 3 (e_rstd + 3 U) mean|z| + 4 sqrt(2 offset_r 2^-7 / D) [flip scatter].
    The slope allowance must stay below a quarter of 1 / (2 D), the shift of a variance taken over D - 1.
    -> dict(slope_diff, slope_allow, offset_ratio (worst over rows), offset_row)"""
    D = x.shape[-1]
    g = torch.ones(D, dtype=F64) if gamma is None else gamma
    b = torch.zeros(D, dtype=F64) if beta is None else beta
    ref, z = ln_ref(x, gamma, beta, False, eps)
    _, parts = ln_pre_store_error(x, gamma, eps)
    rr = ref.to(F32).to(out_dt).to(F64)
    zz = (z * z).sum()

    def stats(o):
        u = (o - b) / g
        return float((u * z).sum() / zz), (u - z).mean(-1)
    s_got, o_got = stats(got)
    s_ref, o_ref = stats(rr)
    e_row = parts["e_rstd"].reshape(-1) + 3 * U
    e = float((e_row * (z * z).sum(-1)).sum() / zz)               # a row's relative error reaches the slope with the weight of its sum z^2
    off = parts["offset"].reshape(-1)
    slope_allow = 3 * e + float(off.mean() * 2.0 ** -7 / z.numel()) ** 0.5
    assert slope_allow <= 0.25 / (2 * D), (slope_allow, D)
    off_allow = off + 3 * e_row * z.abs().mean(-1) + 4 * (2 * off * 2.0 ** -7 / D).sqrt()
    ratio = (o_got - o_ref).abs() / off_allow
    r = int(ratio.argmax())
    return dict(slope_diff=abs(s_got - s_ref), slope_allow=slope_allow, offset_ratio=float(ratio[r]), offset_row=r)


# ================================================================================================ residual + dropout + LayerNorm (D = 768)
DLN_ROWS, DLN_P, DLN_SEED = (1, 2, 7, 9, 33), (0.0, 0.1), 0x5EED1234
DLNCase = collections.namedtuple("DLNCase", "id p rows")


def dln_cases():
    return [DLNCase(f"dropln768-p{p}", p, DLN_ROWS) for p in DLN_P]


def dln_inputs(c, rows):
    base = LNCase("dln" + c.id, "ln768", 768, BF, BF, True, False, 768, 768, 0, (rows,))
    res, gamma, beta = ln_inputs(base, rows)
    x = rnd(torch.randn(rows, 768, generator=gen("dlnx", c.id, rows), dtype=F64) * res.std(-1, keepdim=True).clamp_min(0.1), BF)
    return x, res, gamma, beta


def dln_sum(x, res, p, seed, mutant=None):
    """fp64 res + keep x / (1 - p); element index row * 768 + column.  -> (sum, its fp32 error: the product, the rounded 1 / (1 - p), the add)"""
    rows = x.shape[0]
    if p > 0:
        idx = np.arange(rows * 768)
        if mutant == "mask_no_row":
            idx = idx % 768
        keep = _keep(seed, idx, p).view(rows, 768).to(F64)
    else:
        keep = torch.ones(rows, 768, dtype=F64)
    ks = 1.0 if mutant == "no_keep_scale" else 1 / (1 - p)
    t = keep * x * ks
    v = res + t
    return v, 3 * U * t.abs() + U * v.abs()


# ================================================================================================ layer mix
WSCase = collections.namedtuple("WSCase", "id n D f32 normalize wkind rows")
WS_ROWS = (1, 5, 50)
WS_N, WS_D = (1, 2, 13, 25, 64), (4, 260, 768, 1024)
WS_KINDS = ("random", "equal", "spread30", "one_dead")


def ws_cases():
    out, k = [], 0
    for n in WS_N:
        for D in WS_D:
            for f32 in (False, True):
                normalize = bool((k // 2 + k) % 2)
                if normalize and D == 4 and n == 1:
                    normalize = False
                kind = WS_KINDS[(k // 3) % 4] if n > 1 else "random"
                out.append(WSCase(f"mix-n{n}-D{D}-{'f32' if f32 else 'bf16'}{'-norm' if normalize else ''}-{kind}", n, D, f32, normalize, kind, WS_ROWS))
                k += 1
    return out


def ws_inputs(c, rows):
    """hidden fp64 [n, rows, D] (layer i scaled by i + 1 and, so that normalize has a mean to remove, offset by (i % 3 - 1) * 2), w fp64 [n] (fp32 values)"""
    g = gen("ws", c.id, rows)
    h = torch.randn(c.n, rows, c.D, generator=g, dtype=F64)
    for i in range(c.n):
        h[i] = h[i] * (i + 1) + (i % 3 - 1) * 2.0
    w = torch.randn(c.n, generator=g, dtype=F64)
    if c.wkind == "equal":
        w[:] = 0.25
    elif c.wkind == "spread30":
        w = w * 30
    elif c.wkind == "one_dead":
        w[c.n // 2] = -1e4
    return rnd(h, F32 if c.f32 else BF), rnd(w, F32)


def softmax_parts(a, n_sum):
    """fp64 softmax over the last dim of scores a with the relative error of every fp32 probability exp(a - max) / sum:
    exp: TR + |a - max| 2^-23; the sum: n_sum U and the probability-weighted mean of the exp errors; the reciprocal TR and the product U."""
    am = a - a.amax(-1, keepdim=True)
    p = torch.softmax(a, -1)
    e_exp = TR + am.abs() * 2.0 ** -23
    e_exp = torch.where(p > 0, e_exp, torch.zeros_like(e_exp))
    return p, e_exp + (p * e_exp).sum(-1, keepdim=True) + n_sum * U + TR + U


def ws_ref(h, w, normalize, eps=LN_EPS, mutant=None):
    """-> (ref [rows, D], bound-before-store [rows, D])"""
    n, rows, D = h.shape
    if mutant == "softmax_nm1" and n > 1:
        p = torch.cat([torch.softmax(w[:n - 1], 0), torch.zeros(1, dtype=F64)])
        e_p = torch.zeros(n, dtype=F64)
    else:
        p, e_p = softmax_parts(w, n)
    if mutant == "stride_short" and rows > 1:
        flat = h.reshape(-1)
        h = torch.stack([flat[i * (rows - 1) * D: i * (rows - 1) * D + rows * D].view(rows, D) for i in range(n)])
    if normalize:
        t, _ = ln_ref(h, None, None, False, eps, "mean_Dm4" if mutant == "norm_Dm4" else None)
        dt, _ = ln_pre_store_error(h, None, eps)
    else:
        t, dt = h, torch.zeros_like(h)
    if mutant == "last_dropped":
        p = p.clone()
        p[n - 1] = 0
    pw = p.view(n, 1, 1)
    ref = (pw * t).sum(0)
    mag = (pw * t.abs()).sum(0)
    pre = (pw * t.abs() * (e_p.view(n, 1, 1) + U)).sum(0) + n * U * mag + (pw * dt).sum(0)
    return ref, pre


def ws_emulate(h, w, normalize, order, eps=LN_EPS):
    n, rows, D = h.shape
    w = w.to(F32)
    e = torch.exp(w - w.max())
    p = e / fsum(e, "seq")
    acc = torch.zeros(rows, D, dtype=F32)
    for i in (range(n) if order == "seq" else reversed(range(n))):
        t = h[i].to(F32)
        if normalize:
            mean = (fsum(t, order) / D).unsqueeze(-1)
            d = t - mean
            t = d * torch.rsqrt(fsum(d * d, order) / D + torch.tensor(eps, dtype=F32)).unsqueeze(-1)
        acc = acc + p[i] * t
    return acc.to(BF).to(F64)


# ================================================================================================ L2 normalise
L2Case = collections.namedtuple("L2Case", "id D f32 ld_in rows")


def l2_cases():
    return [L2Case(f"l2-D{D}-{'f32' if f32 else 'bf16'}{'-slice' if D == 260 else ''}", D, f32, D + 12 if D == 260 else D, 9) for D in (4, 260, 512, 1024) for f32 in (False, True)]


def l2_inputs(c):
    x = torch.randn(c.rows, c.D, generator=gen("l2", c.id), dtype=F64) * torch.logspace(-3, 2, c.rows, dtype=F64).view(-1, 1)
    return rnd(x, F32 if c.f32 else BF)


def l2_ref(x, floor=0.0):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(floor)


def l2_bound(x, ref):
    """sum of D squares: D U for the sum and U for each product; the root halves that and costs TR, the reciprocal TR, the final product U (+ U to spare)"""
    D = x.shape[-1]
    return (0.5 * (D + 1) * U + 2 * TR + 2 * U) * ref.abs()


def l2_emulate(x, order):
    x = x.to(F32)
    return (x * (1.0 / torch.sqrt(fsum(x * x, order))).unsqueeze(-1)).to(F64)


# ================================================================================================ hidden-state normalisation (method1 / method2)
HNCase = collections.namedtuple("HNCase", "id D f32 method")
HN_N, HN_B, HN_TP, HN_T = 2, 2, 9, 7
HN_NORMS = ((1.0, 30.0), (3e-4, 5.0))            # [layer][utterance]: the frame norm scale


def hn_cases():
    return [HNCase(f"hn-D{D}-{'f32' if f32 else 'bf16'}-{m}", D, f32, m) for D in (64, 260, 1024) for f32 in (False, True) for m in ("method1", "method2")]


def hn_inputs(c):
    """[n, B, Tp, D]: frame t of (layer i, utterance b) has norm about HN_NORMS[i][b] (1 + t / 4); rows T .. Tp-1 are three times larger still."""
    x = torch.randn(HN_N, HN_B, HN_TP, c.D, generator=gen("hn", c.id), dtype=F64) / c.D ** 0.5
    for i in range(HN_N):
        for b in range(HN_B):
            for t in range(HN_TP):
                x[i, b, t] *= HN_NORMS[i][b] * (1 + t / 4) * (3.0 if t >= HN_T else 1.0)
    return rnd(x, F32 if c.f32 else BF)


def hn_ref(x, T, method, mutant=None):
    """method1: every frame x / (||x|| + 1e-8).  method2: every frame of (layer, utterance) divided by the mean over the FIRST T frames of ||x||."""
    nrm = x.norm(dim=-1, keepdim=True)
    if method == "method1":
        return x / ((nrm * nrm + 1e-8).sqrt() if mutant == "eps_inside" else nrm + 1e-8)
    Tm = x.shape[2] if mutant == "Tp_for_T" else T
    m = nrm[:, :, :Tm].mean(2, keepdim=True)
    if mutant == "per_layer":
        m = m.mean(1, keepdim=True)
    if mutant == "mean_sq":
        m = (nrm[:, :, :Tm] ** 2).mean(2, keepdim=True).sqrt()
    return x / m


def hn_bound(x, ref, T, method, f32):
    """norm: (D + 1) U / 2 + TR; method1: + U (the 1e-8) + TR (reciprocal) + U (product); method2: + T U (sum of T norms) + TR (T / s) + U; then the store"""
    D = x.shape[-1]
    e = 0.5 * (D + 1) * U + 2 * TR + 2 * U + (T * U if method == "method2" else 0.0)
    return e * ref.abs() + store_bound(ref, F32 if f32 else BF)


def hn_emulate(x, T, method, f32, order):
    x = x.to(F32)
    nrm = torch.sqrt(fsum(x * x, order))
    if method == "method1":
        y = x * (1.0 / (nrm + torch.tensor(1e-8, dtype=F32))).unsqueeze(-1)
    else:
        y = x * (torch.tensor(float(T), dtype=F32) / fsum(nrm[:, :, :T], "seq")).view(x.shape[0], x.shape[1], 1, 1)
    return y.to(F32 if f32 else BF).to(F64)


# ================================================================================================ waveform LayerNorm
WV_LDS = (8, 4100, 5001, 32772)
WV_SEG = 8


def wv_lens(ld):
    """len = ld, 1, 0, len % 4 in {1, 2, 3}, and a length inside the first, a middle and the last of the 8 segments; never above ld"""
    per = ((ld + WV_SEG - 1) // WV_SEG + 3) & ~3
    want = [ld, 1, 0, per // 2 | 1, 3 * per + 2, min(7 * per + 3, ld - 1), 5, 6, 7]
    out = []
    for n in want:
        n = max(0, min(int(n), ld))
        if n not in out:
            out.append(n)
    assert {n % 4 for n in out} >= {1, 2, 3} and max(out) <= ld
    return out


def wv_inputs(ld):
    """[B, ld] fp32 values: speech-like 0.1 randn + 0.02; utterance 3 has a DC offset of 5.0 and std 0.01 (the cancellation case); every sample at or past its
    utterance's length is PAST_VALUE (the kernel must neither read it into the statistics nor leave it in the output)."""
    lens = wv_lens(ld)
    x = torch.randn(len(lens), ld, generator=gen("wv", ld), dtype=F64) * 0.1 + 0.02
    if len(lens) > 3:
        x[3] = 5.0 + 0.01 * torch.randn(ld, generator=gen("wvdc", ld), dtype=F64)
    for b, n in enumerate(lens):
        x[b, n:] = PAST_VALUE
    return rnd(x, F32), lens


def wv_ref(x, lens, eps=LN_EPS, mutant=None):
    """-> (ref, bound, the bound's single-rounding part).  The kernel's sums are fp64 (2^-53 (E x^2 / var) on the variance); mean and variance are then cast to fp32 (U each), + eps (U), rsqrt (TR):
    |err| <= rstd U (|mean| + |d|) + |z| (e_var / 2 + TR + U) + U |z|."""
    ref, bound, store = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for b, n in enumerate(lens):
        m = max(0, min(x.shape[1], n + (1 if mutant == "len_plus1" else -1 if mutant == "len_minus1" else 0)))
        if m == 0:
            continue
        v = x[b, :m]
        mean = v.mean()
        if mutant == "single_pass_f32":
            var = ((v.to(F32) * v.to(F32)).to(F64).mean().to(F32) - (mean.to(F32) * mean.to(F32))).to(F64).clamp_min(0)
        else:
            var = ((v - mean) ** 2).sum() / ((m - 1) if mutant == "unbiased" and m > 1 else m)
        rstd = 1 / (var + eps).sqrt()
        z = (v - mean) * rstd
        ref[b, :m] = z
        e_var = 2 * U + 2.0 ** -52 * (v * v).mean() / (var + eps)
        store[b, :m] = rstd * U * mean.abs() + U * z.abs()                  # single roundings that are attained: the mean's cast and the output's
        bound[b, :m] = store[b, :m] + rstd * U * (v - mean).abs() + z.abs() * (0.5 * e_var + TR + U)
    return ref, bound, store


def wv_emulate(x, lens, order, eps=LN_EPS):
    out = torch.zeros_like(x)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        v = x[b, :n]
        s, q = (v.sum(), (v * v).sum()) if order == "seq" else (v.flip(0).sum(), (v * v).flip(0).sum())
        mean = s / n
        var = (q / n - mean * mean).clamp_min(0)
        rstd = torch.rsqrt(var.to(F32) + torch.tensor(eps, dtype=F32))
        out[b, :n] = ((v.to(F32) - mean.to(F32)) * rstd).to(F64)
    return out


# ================================================================================================ split-K finish
SKCase = collections.namedtuple("SKCase", "id S M N bias gelu res")            # res: None / "ldN" / "ldwide" / "ld0"


def sk_cases():
    out, k = [], 0
    for S in (1, 2, 7):
        for (M, N) in ((3, 260), (40, 512)):
            for gelu in (False, True):
                for res in (None, "ldN", "ldwide", "ld0"):
                    bias = (k // 4 + k) % 2 == 0
                    out.append(SKCase(f"splitk-S{S}-{M}x{N}{'-bias' if bias else ''}{'-gelu' if gelu else ''}-res{res}", S, M, N, bias, gelu, res))
                    k += 1
    return out


def sk_inputs(c):
    """partials fp64 [S, M, N], bias [N] | None, residual buffer [M or 1, ldr] | None (all fp32 values), ldr"""
    g = gen("sk", c.id)
    part = rnd(torch.randn(c.S, c.M, c.N, generator=g, dtype=F64) * 1.5, F32)
    bias = rnd(torch.randn(c.N, generator=g, dtype=F64), F32) if c.bias else None
    ldr = {None: 0, "ldN": c.N, "ldwide": c.N + 8, "ld0": 0}[c.res]
    res = None
    if c.res is not None:
        res = rnd(torch.randn(1 if c.res == "ld0" else c.M, max(ldr, c.N), generator=g, dtype=F64) * 2, F32)
    return part, bias, res, ldr


def sk_res_view(res, c, mutant=None):
    """the [M, N] residual the kernel adds: row m at res_flat[m * ldr + n]"""
    if res is None:
        return None
    ldr = 0 if c.res == "ld0" else res.shape[1]
    if mutant == "ldr_ignored":
        ldr = c.N
    flat = res.reshape(-1)
    rows = []
    for m in range(c.M):
        seg = flat[m * ldr: m * ldr + c.N]
        rows.append(torch.cat([seg, torch.zeros(c.N - seg.numel(), dtype=flat.dtype)]))      # (the mutant may run off the end of a broadcast row: zeros)
    return torch.stack(rows)


def sk_exact_f32(part, bias, res_mn):
    """act none: the kernel's own fixed-order fp32 adds (IEEE: bit-exact on any machine)"""
    acc = part[0].to(F32).clone()
    for s in range(1, part.shape[0]):
        acc = acc + part[s].to(F32)
    if bias is not None:
        acc = acc + bias.to(F32)
    if res_mn is not None:
        acc = acc + res_mn.to(F32)
    return acc


def sk_ref(part, bias, res_mn, gelu, mutant=None):
    """-> (ref, bound): u = sum_s part + bias with (S + 1) U sum|terms| in front of the GELU; gelu_erf_precise 1.5e-7 (1 + |u|) plus its fp32 evaluation
    (v_rcp, v_exp and six FMAs on erf, |.| <= 1: |u| / 2 (2 TR + 6 U)); the residual add U |out|."""
    u = part.sum(0)
    mag = part.abs().sum(0)
    b = bias if bias is not None else torch.zeros(part.shape[-1], dtype=F64)
    r = res_mn if res_mn is not None else torch.zeros_like(u)
    if mutant == "bias_res_swapped":
        b, r = r, b
    u = u + b
    du = (part.shape[0] + 1) * U * (mag + b.abs())
    if gelu:
        a = gelu64(u)
        da = GELU_LIP * du + GELU_PRECISE * (1 + u.abs()) + 0.5 * u.abs() * (2 * TR + 6 * U) + 2 * U * a.abs()
    else:
        a, da = u, du
    out = a + r
    return out, da + U * out.abs()


# ================================================================================================ pooling head
POOL_LENS70 = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 69, 70)
POOL_BATCHES = {"T70": (70, POOL_LENS70), "T499": (499, (499, 498))}
POOL_SHAPES = ((1, 8, 768), (8, 8, 128), (2, 8, 260), (1, 4, 1024), (1, 1, 4))            # (NQ, R, D): DCH 3, 1, 2, 4, 1
POOL_WIDE = (2, 8, 260)                                                                   # this one reads x_rows as a column slice (ld_x = D + 8)
ATTN_SHAPES = ((1, 8, 96), (8, 1, 768), (1, 1, 1024), (2, 4, 260), (1, 4, 16), (1, 2, 4))  # (NQ, H, hd): one pass / hd > 512 / hd > 512 / hd > 256 / small
PoolCase = collections.namedtuple("PoolCase", "id NQ R D batch T lens ld_x")
AttnCase = collections.namedtuple("AttnCase", "id NQ H hd batch T lens")


def pool_cases():
    return [PoolCase(f"pool-NQ{NQ}-R{R}-D{D}-{bn}", NQ, R, D, bn, T, lens, D + 8 if (NQ, R, D) == POOL_WIDE else D)
            for (NQ, R, D) in POOL_SHAPES for bn, (T, lens) in POOL_BATCHES.items()]


def attn_cases():
    return [AttnCase(f"clsattn-NQ{NQ}-H{H}-hd{hd}-{bn}", NQ, H, hd, bn, T, lens) for (NQ, H, hd) in ATTN_SHAPES for bn, (T, lens) in POOL_BATCHES.items()]


def pool_inputs(c):
    """x [B, T, D] and cls [NQ, D] (bf16 values), scores [B, T, R] and cls_scores [NQ, R] (fp32 values, std 3).  In utterance b the LAST valid key holds the
    maximum of row r = b % R (by 2), the first key past len has score PAST_SCORE above every other and frame values PAST_VALUE."""
    g = gen("pool", c.id)
    B = len(c.lens)
    x = torch.randn(B, c.T, c.D, generator=g, dtype=F64)
    cls = torch.randn(c.NQ, c.D, generator=g, dtype=F64)
    s = 3 * torch.randn(B, c.T, c.R, generator=g, dtype=F64)
    cs = 3 * torch.randn(c.NQ, c.R, generator=g, dtype=F64)
    for b, n in enumerate(c.lens):
        if n > 0:
            r = b % c.R
            s[b, n - 1, r] = max(float(s[b, :n, r].max()), float(cs[:, r].max())) + 2.0
        if n < c.T:
            s[b, n] = float(max(s[b].max(), cs.max())) + PAST_SCORE
            x[b, n] = PAST_VALUE
    return rnd(x, BF), rnd(cls, BF), rnd(s, F32), rnd(cs, F32)


def weighted_sum_ref(p, e_p, vals, n_sum):
    """sum_k p_k vals_k over dim -2 of vals [..., K, D] with p [..., K]: -> (ref, magnitude, fp32 error: every product U + e_p, the sum n_sum U)"""
    pw = p.unsqueeze(-1)
    ref, mag = (pw * vals).sum(-2), (pw * vals.abs()).sum(-2)
    return ref, mag, (pw * vals.abs() * (e_p.unsqueeze(-1) + U)).sum(-2) + n_sum * U * mag


def pool_ref(c, x, cls, s, cs, mutant=None):
    """fp64 xbar [B, R, D] = sum over [CLS keys ; frames < len] of softmax(scores)_k z_k, and its fp32 error before the store."""
    B = len(c.lens)
    ref, pre = torch.zeros(B, c.R, c.D, dtype=F64), torch.zeros(B, c.R, c.D, dtype=F64)
    for b, n in enumerate(c.lens):
        if mutant == "keys_plus1":
            n = min(c.T, n + 1)
        elif mutant == "keys_minus1":
            n = max(0, n - 1)
        csb = cs.t() if mutant == "cls_scores_transposed" and c.NQ == c.R else cs
        if mutant == "cls_scores_transposed" and c.NQ != c.R:
            csb = cs.reshape(-1)[: c.NQ * c.R].view(c.R, c.NQ).t()                       # read as [R, NQ]
        z = torch.cat([cls, x[b, :n]], 0)
        a = torch.cat([csb, s[b, :n]], 0)
        if mutant == "no_cls":
            z, a = z[c.NQ:], a[c.NQ:]
            if n == 0:
                continue
        p, e_p = softmax_parts(a.t(), a.shape[0])                                         # [R, K]
        if mutant == "wave_tail_dropped":                                                 # the last group of four keys of the wave that owns the last key
            K = a.shape[0]
            own = [k for k in range(K) if k % 4 == (K - 1) % 4]
            p = p.clone()
            p[:, own[-4:]] = 0
        ref[b], _, pre[b] = weighted_sum_ref(p, e_p, z.unsqueeze(0).expand(c.R, -1, -1), a.shape[0])
    return ref, pre


def pool_bound(ref, pre, split):
    """split: hi + lo keeps the fp32 sum to 2^-16 (lo is the bf16 of the exact remainder s - hi, itself <= 2^-8 |s|)"""
    return pre + (2.0 ** -16 * 1.002 * ref.abs() if split else BF_STORE * ref.abs())


def pool_emulate(c, x, cls, s, cs, order):
    """fp32: softmax as the kernel forms it, the keys summed in `order` ("seq", or "pair64": four interleaved partial sums as the four waves, then their sum)"""
    B = len(c.lens)
    out = torch.zeros(B, c.R, c.D, dtype=F32)
    for b, n in enumerate(c.lens):
        z = torch.cat([cls, x[b, :n]], 0).to(F32)
        a = torch.cat([cs, s[b, :n]], 0).to(F32).t()
        e = torch.exp(a - a.amax(-1, keepdim=True))
        p = e * (1.0 / fsum(e, order)).unsqueeze(-1)
        terms = p.unsqueeze(-1) * z.unsqueeze(0)                                          # [R, K, D]
        if order == "seq":
            out[b] = fsum(terms.transpose(1, 2).contiguous(), "seq")
        else:
            parts = [fsum(terms[:, w::4].transpose(1, 2).contiguous(), "seq") if terms[:, w::4].shape[1] else torch.zeros(c.R, c.D, dtype=F32) for w in range(4)]
            out[b] = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    return out


def attn_inputs(c):
    """cls_qkv [NQ, 3 D] and kv [B, T, 2 D] (bf16 values).  q has std 3 so that the scores have std about 3; in utterance b the last valid key is aligned with query 0
    of head b % H to score 2 above that row's maximum; the first key past len scores PAST_SCORE above it in every head of query 0 and its values are PAST_VALUE."""
    g = gen("clsattn", c.id)
    B, D, hd = len(c.lens), c.H * c.hd, c.hd
    cq = torch.randn(c.NQ, 3 * D, generator=g, dtype=F64)
    cq[:, :D] *= 3
    kv = torch.randn(B, c.T, 2 * D, generator=g, dtype=F64)
    cq = rnd(cq, BF)
    q0 = cq[0, :D].view(c.H, hd)
    unit = q0 / ((q0 * q0).sum(-1, keepdim=True) * hd ** -0.5)                            # key u with q0 . u / sqrt(hd) = 1 per head
    for b, n in enumerate(c.lens):
        kvb = rnd(kv[b], BF)
        sc = torch.einsum("hd,khd->hk", q0, torch.cat([cq[:, D:2 * D], kvb[:n, :D]], 0).view(-1, c.H, hd)) * hd ** -0.5
        if n > 0:
            h = b % c.H
            kv[b, n - 1, h * hd:(h + 1) * hd] = unit[h] * (float(sc[h].max()) + 2.0)
        if n < c.T:
            kv[b, n, :D] = (unit * (sc.max(-1, keepdim=True).values + PAST_SCORE)).reshape(-1)
            kv[b, n, D:] = PAST_VALUE
    return cq, rnd(kv, BF)


def attn_ref(c, cq, kv, mutant=None):
    """fp64 out [B, NQ, D]: per head softmax(q . k / sqrt(hd)) v over [CLS keys ; frames < len].  The score's fp32 error: q scale (2 U: the product, then its use),
    a dot product of hd terms (hd U sum|q k| scale); it reaches a probability as (d s_k + sum_j p_j d s_j)."""
    B, D, hd, H, NQ = len(c.lens), c.H * c.hd, c.hd, c.H, c.NQ
    ref, pre = torch.zeros(B, NQ, D, dtype=F64), torch.zeros(B, NQ, D, dtype=F64)
    q = cq[:, :D].view(NQ, H, hd)
    for b, n in enumerate(c.lens):
        if mutant == "keys_plus1":
            n = min(c.T, n + 1)
        elif mutant == "keys_minus1":
            n = max(0, n - 1)
        k = torch.cat([cq[:, D:2 * D], kv[b, :n, :D]], 0).view(-1, H, hd)
        v = torch.cat([cq[:, 2 * D:], kv[b, :n, D:]], 0).view(-1, H, hd)
        if mutant == "no_cls":
            k, v = k[NQ:], v[NQ:]
            if n == 0:
                continue
        K = k.shape[0]
        a = torch.einsum("qhd,khd->hqk", q, k) * hd ** -0.5
        ds = (hd + 3) * U * torch.einsum("qhd,khd->hqk", q.abs(), k.abs()) * hd ** -0.5
        p, e_p = softmax_parts(a, K)
        e_p = e_p + 1.01 * (ds + (p * ds).sum(-1, keepdim=True))
        if mutant == "wave_tail_dropped":
            p = p.clone()
            p[..., [kk for kk in range(K) if kk % 4 == (K - 1) % 4][-4:]] = 0
        vh = v.permute(1, 0, 2).unsqueeze(1).expand(H, NQ, K, hd)                         # [H, NQ, K, hd]
        r, _, e = weighted_sum_ref(p, e_p, vh, K)
        ref[b], pre[b] = r.permute(1, 0, 2).reshape(NQ, D), e.permute(1, 0, 2).reshape(NQ, D)
    return ref, pre


def attn_emulate(c, cq, kv, order):
    B, D, hd, H, NQ = len(c.lens), c.H * c.hd, c.hd, c.H, c.NQ
    out = torch.zeros(B, NQ, D, dtype=F32)
    q = (cq[:, :D].to(F32) * torch.tensor(hd ** -0.5, dtype=F32)).view(NQ, H, hd)
    for b, n in enumerate(c.lens):
        k = torch.cat([cq[:, D:2 * D], kv[b, :n, :D]], 0).to(F32).view(-1, H, hd)
        v = torch.cat([cq[:, 2 * D:], kv[b, :n, D:]], 0).to(F32).view(-1, H, hd)
        a = fsum(q.permute(1, 0, 2).unsqueeze(2) * k.permute(1, 0, 2).unsqueeze(1), order)        # [H, NQ, K]
        e = torch.exp(a - a.amax(-1, keepdim=True))
        p = e * (1.0 / fsum(e, order)).unsqueeze(-1)
        terms = p.unsqueeze(-1) * v.permute(1, 0, 2).unsqueeze(1)                                   # [H, NQ, K, hd]
        o = fsum(terms.transpose(2, 3).contiguous(), order)
        out[b] = o.permute(1, 0, 2).reshape(NQ, D)
    return out.to(BF).to(F64)

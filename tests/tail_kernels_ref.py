"""Plain fp64 statements, case lists, deterministic inputs and DERIVED per-element bounds of the fp32 kernels of the trainable tail (csrc/train.hip below
the pooling kernels, csrc/infonce.hip, csrc/sgemm.hip, csrc/train_cascaded.hip) for tests/test_tail_kernels_parity_gpu.py and tools/tail_kernel_bounds.py.  A helper module, not
a test; no kernel runs here.  The constants, the generator, the rounding helper and the judge are those of tests/row_kernels_ref.py and are imported, not restated.

Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE (fp32, hyper-parameters included) before the reference sees it; every
reference is torch fp64 of exactly the stated operation; every bound function returns, per output, a tensor of the output's shape.

The rules of the bounds are those of row_kernels_ref.py's header (n-term fp32 sum: n U sum|terms| against the MAGNITUDE reference; every other fp32 operation U;
hardware rcp / rsq / exp / sqrt and the `/` lowered to them TR each; __expf(a): |a| 2^-23 on top; one bf16 store BF_STORE).  One BUDGET is added here: the
library functions erff, expf, logf and powf have no figure in this project and are budgeted TR relative each -- a budget, not a documented figure.

Every group is a Group(cases, inputs, ref, bound, emulate, mutants):
    inputs(c)            -> dict of fp64 tensors holding fp32 (or bf16) values
    ref(c, inp, mutant)  -> dict output name -> fp64 tensor; with a mutant name, the statement of that WRONG kernel, or None where the mutant cannot differ on this case
    bound(c, inp)        -> dict output name -> Bd(bound, store, limit): `store` is the part of the bound that one attained rounding of the output itself takes
                            (U |ref| of an fp32 store, BF_STORE |ref| of a bf16 one), `limit` what the CPU emulation is held to on (bound - store): 0.5, or 1.0 for
                            an output made of IEEE operations alone (products, sums of two, FMAs: the emulation IS the kernel's arithmetic and each U is attained)
    emulate(c, inp, o)   -> the same outputs from a torch fp32 emulation of the kernel's arithmetic; o in ("seq", "pair64") is the summation order, and for
                            arithmetic without sums "seq" rounds after every operation while "pair64" fuses every a * b + c into one rounding (what the compiler
                            may contract)"""
import collections
import math

import torch

from row_kernels_ref import (BF, BF_STORE, F32, F64, LN_EPS, ORDERS, PAST_VALUE, ROW_MEANS, ROW_STDS, SENT16, SENT32, TR, U, fsum, gen, rnd, softmax_parts,  # noqa: F401
                             store_bound, worst)

Bd = collections.namedtuple("Bd", "bound store limit")
Group = collections.namedtuple("Group", "name cases inputs ref bound emulate mutants")


def f32v(v):
    """a Python float rounded to fp32 (what a `float` kernel argument holds)"""
    return float(torch.tensor(v, dtype=F32))


def loguniform(g, n, lo, hi):
    return 10 ** (math.log10(lo) + (math.log10(hi) - math.log10(lo)) * torch.rand(n, generator=g, dtype=F64))


def signs(g, n):
    return torch.where(torch.rand(n, generator=g, dtype=F64) < 0.5, -1.0, 1.0).to(F64)


def t32(v):
    return torch.tensor(v, dtype=F32)


def fma32(a, b, c, fused):
    """fp32 a * b + c: two roundings, or one (the product of two fp32 values is exact in fp64)"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32) if fused else a * b + c


# ================================================================================================ sc_adam_step
AdamCase = collections.namedtuple("AdamCase", "id n step wd clip")
ADAM_N, ADAM_STEPS, ADAM_WD = (1, 257, 100003), (1, 2, 10, 1000, 100000), (0.0, 1e-6, 1e-2)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_NORM, ADAM_COEF = 37.5, 0.0042              # the two floats sc_grad_norm leaves: the kernel must read the second
ADAM_MUTANTS = ("eps_inside_root", "eps_times_sqrt_bc2", "no_bc1", "decoupled_decay", "decay_after_m", "clip_ignored", "clip_reads_norm", "v_unclipped")


def adam_cases():
    return [AdamCase(f"adam-n{n}-t{t}-wd{wd:g}-{'clip' if clip else 'noclip'}", n, t, wd, clip)
            for n in ADAM_N for t in ADAM_STEPS for wd in ADAM_WD for clip in (False, True)]


def adam_inputs(c):
    """g: sizes log-uniform over [1e-10, 10]; p: sizes log-uniform over [1e-4, 10]; m, v: the state after step - 1 steps of the fp64 recursion on a warm-up
    gradient gw that is constant per element (closed form: m = gw (1 - b1^(t-1)), v = gw^2 (1 - b2^(t-1))), rounded to fp32; the step's own gradient is gw times a
    random sign and a factor in [0.5, 2] (clamped back into the range), so that m and g disagree in sign on half the elements."""
    g_ = gen("adam", c.id)
    n, t = c.n, c.step - 1
    b1, b2 = f32v(ADAM_B1), f32v(ADAM_B2)
    gw = loguniform(g_, n, 1e-10, 10.0) * signs(g_, n)
    m, v = rnd(gw * (1 - b1 ** t), F32), rnd(gw * gw * (1 - b2 ** t), F32)
    g = gw * signs(g_, n) * (0.5 + 1.5 * torch.rand(n, generator=g_, dtype=F64))
    g = g.sign() * g.abs().clamp(1e-10, 10.0)
    p = loguniform(g_, n, 1e-4, 10.0) * signs(g_, n)
    return dict(p=rnd(p, F32), g=rnd(g, F32), m=m, v=v)


def _adam_parts(c, inp, mutant=None):
    lr, b1, b2, eps, wd = (f32v(x) for x in (ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, c.wd))
    p, g, m, v = inp["p"], inp["g"], inp["m"], inp["v"]
    if mutant in ("clip_ignored", "clip_reads_norm", "v_unclipped") and not c.clip:
        return None
    if mutant in ("decoupled_decay", "decay_after_m") and c.wd == 0:
        return None
    if mutant == "no_bc1" and c.step >= 1000:
        return None
    coef = f32v(ADAM_COEF) if c.clip else 1.0
    cm = 1.0 if mutant == "clip_ignored" else f32v(ADAM_NORM) if mutant == "clip_reads_norm" else coef
    gc = g * cm
    gi = gc if mutant in ("decoupled_decay", "decay_after_m") else gc + wd * p
    gv = g + wd * p if mutant == "v_unclipped" else gc + wd * p if mutant == "decay_after_m" else gi
    m2 = b1 * m + (1 - b1) * gi
    v2 = b2 * v + (1 - b2) * gv * gv
    bc1, bc2 = 1 - b1 ** c.step, 1 - b2 ** c.step
    if mutant == "no_bc1":
        bc1 = 1.0
    if mutant == "eps_inside_root":
        denom = (v2 / bc2 + eps).sqrt()
    elif mutant == "eps_times_sqrt_bc2":
        denom = v2.sqrt() / bc2 ** 0.5 + eps * bc2 ** 0.5
    else:
        denom = v2.sqrt() / bc2 ** 0.5 + eps
    step = lr / bc1 * m2 / denom
    if mutant == "decoupled_decay":
        step = step + lr * wd * p
    return dict(gc=gc, gi=gi, m=m2, v=v2, denom=denom, step=step, bc1=bc1, bc2=bc2, lr=lr, b1=b1, b2=b2, wd=wd)


def adam_ref(c, inp, mutant=None):
    """torch.optim.Adam (L2 decay added to the gradient, eps outside the root, both bias corrections) in fp64 on the fp32-rounded hyper-parameters; the gradient
    is first multiplied by the clip coefficient.  -> m_new, v_new and the STEP p_old - p_new."""
    q = _adam_parts(c, inp, mutant)
    return None if q is None else dict(m=q["m"], v=q["v"], step=q["step"])


def adam_bound(c, inp):
    """gi = fma(wd, p, g coef): U |g coef| for the product, U |gi| for the FMA.  m' = b1 m + (1 - b1) gi: a rounding each for the two products and the sum (1 - b1
    is exact: Sterbenz).  v' likewise with gi^2 carrying gi's error twice.  The corrections 1 - powf(b, t): TR b^t / (1 - b^t) + U each (the powf budget, amplified
    by the cancellation), sqrtf(bc2) halves its own and adds TR.  denom = sqrt(v') / sqrt(bc2) + eps: half v's relative error, TR for the root, TR for the quotient,
    U for the sum.  step = (lr / bc1) (m' / denom): TR for each quotient, U for the product; the final p - step rounds once: U |p_new|, the store term."""
    q = _adam_parts(c, inp)
    p, g, m, v = inp["p"], inp["g"], inp["m"], inp["v"]
    b1, b2 = q["b1"], q["b2"]
    e_gi = (U * q["gc"].abs() if c.clip else 0.0) + (U * q["gi"].abs() if c.wd else 0.0)
    e_m = U * (b1 * m).abs() + (1 - b1) * (e_gi + U * q["gi"].abs()) + U * q["m"].abs()
    e_v = U * b2 * v + (1 - b2) * (2 * U * q["gi"] ** 2 + 2 * q["gi"].abs() * e_gi) + U * q["v"]
    e_bc1 = TR * b1 ** c.step / q["bc1"] + U
    e_bc2s = 0.5 * (TR * b2 ** c.step / q["bc2"] + U) + TR
    Q = q["v"].sqrt() / q["bc2"] ** 0.5
    e_den = Q * (0.5 * e_v / q["v"] + 2 * TR + e_bc2s) + U * q["denom"]
    e_s = q["lr"] / q["bc1"] / q["denom"] * e_m + q["step"].abs() * (e_den / q["denom"] + 2 * TR + e_bc1 + 2 * U)
    st = U * (p - q["step"]).abs()
    return dict(m=Bd(e_m, 0 * e_m, 1.0), v=Bd(e_v, 0 * e_v, 1.0), step=Bd(e_s + st, st, 0.5))


def adam_emulate(c, inp, order):
    fused = order == "pair64"
    p, g, m, v = (inp[k].to(F32) for k in "pgmv")
    lr, b1, b2, eps, wd = (t32(x) for x in (ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS, c.wd))
    gi = g * t32(ADAM_COEF) if c.clip else g
    if c.wd:
        gi = fma32(wd, p, gi, True)
    one = t32(1.0)
    mi = fma32(b1, m, (one - b1) * gi, fused)
    vi = fma32(b2, v, (one - b2) * gi * gi, fused)
    bc1, bc2 = one - torch.pow(b1, t32(float(c.step))), one - torch.pow(b2, t32(float(c.step)))
    pn = p - (lr / bc1) * (mi / (torch.sqrt(vi) / torch.sqrt(bc2) + eps))
    return dict(m=mi.to(F64), v=vi.to(F64), step=p.to(F64) - pn.to(F64))


# ================================================================================================ sc_grad_norm
GNCase = collections.namedtuple("GNCase", "id n max_norm small")
GN_N, GN_MAX = (1, 255, 256, 257, 262143, 262144, 262145, 1000003), (0.0, 4.0, 1e9)
GN_MUTANTS = ("last_partial_block_dropped", "stride_blocks_x255", "no_1e-6", "coef_unclamped")


def gn_blocks(n):
    """sc_grad_norm's block rule restated: one block of 256 per 256 elements plus one, capped at 1024 -> (blocks, 'single' | 'stride'); 'stride': the cap holds and
    the grid-stride loop is what covers the buffer (at n = 262144 exactly with one pass, above it with several)"""
    want = n // 256 + 1
    return min(want, 1024), ("stride" if want > 1024 else "single")


def gn_cases():
    out = [GNCase(f"gradnorm-n{n}-max{mx:g}", n, mx, False) for n in GN_N for mx in GN_MAX]
    # beyond the issue's list: with max_norm = 4 the clipping case has norm > 4, where the + 1e-6 of the coefficient is 2.5e-7 relative -- below the quotient's TR.  A
    # small clipped norm (one gradient of size 2e-4, inside the stated range, max_norm 1e-4) makes that term 5e-3 of the coefficient.
    out.append(GNCase("gradnorm-n1-small-max0.0001", 1, 1e-4, True))
    return out


def gn_inputs(c):
    """sizes log-uniform over [1e-10, 10], random signs; the last element has size 10 (what the last partial block holds is then loud)"""
    g_ = gen("gradnorm", c.n)
    g = loguniform(g_, c.n, 1e-10, 10.0) * signs(g_, c.n)
    g[-1] = 2e-4 if c.small else -10.0
    return dict(g=rnd(g, F32))


def gn_ref(c, inp, mutant=None):
    g, n = inp["g"], c.n
    w = torch.ones(n, dtype=F64)
    if mutant == "last_partial_block_dropped":
        w[n // 256 * 256:] = 0
    elif mutant == "stride_blocks_x255":
        blocks, path = gn_blocks(n)
        if path != "stride":
            return None
        j = torch.arange(n)
        w = torch.zeros(n, dtype=F64)
        for k in range(n // (blocks * 255) + 1):
            i = j - k * blocks * 255
            w += ((i >= 0) & (i < blocks * 256)).to(F64)
    norm = (w * g * g).sum().sqrt()
    mx = f32v(c.max_norm)
    if mx > 0:
        coef = mx / (norm + (0.0 if mutant == "no_1e-6" else f32v(1e-6)))
        if mutant != "coef_unclamped":
            coef = coef.clamp(max=1.0)
    else:
        coef = torch.ones((), dtype=F64)
    return dict(out=torch.stack([norm, coef]))


def gn_bound(c, inp):
    """the norm is the fp32 rounding of an fp64 sum and root: 2 U |norm| (U of it the store).  The coefficient: the norm's 2 U, U for the fp32 norm + 1e-6 and TR
    for the quotient, which is the stored value: (3 U + TR) coef in all.  A coefficient the clamp (or max_norm <= 0) sets to 1 is exact unless the quotient is within
    that error of 1."""
    r = gn_ref(c, inp)["out"]
    norm, coef = r[0], r[1]
    e_c = (3 * U + TR) * coef
    mx = f32v(c.max_norm)
    if mx <= 0 or float(mx / (norm + 1e-6)) * (1 - 3 * U - TR) > 1:
        e_c = torch.zeros((), dtype=F64)
    return dict(out=Bd(torch.stack([2 * U * norm, e_c]), torch.stack([U * norm, U * coef if float(e_c) > 0 else e_c]), 0.5))


def gn_emulate(c, inp, order):
    g = inp["g"]
    s = (g * g).sum() if order == "seq" else (g * g).flip(0).cumsum(0)[-1]
    norm = s.sqrt().to(F32)
    mx = t32(c.max_norm)
    coef = torch.minimum(t32(1.0), mx / (norm + t32(1e-6))) if float(mx) > 0 else t32(1.0)
    return dict(out=torch.stack([norm, coef]).to(F64))


# ================================================================================================ sc_colsum
CSCase = collections.namedtuple("CSCase", "id rows cols ld acc")
CS_SHAPES = ((1, 1, 1), (255, 65, 65), (256, 65, 72), (257, 64, 64), (1000, 130, 130), (256, 32704, 32704), (256, 32768, 32768))
CS_MUTANTS = ("last_row_dropped", "last_chunk_twice", "memset_skipped", "ld_as_cols")


def cs_chunks(rows, cols):
    """sc_colsum's chunk rule restated -> (row chunks, rows per chunk); chunks > 1 is the atomic path"""
    cb = (cols + 63) // 64
    chunks = 1
    if rows >= 256 and cb < 512:
        chunks = min((rows + 63) // 64, max(1, 1024 // cb))
    rpb = (rows + chunks - 1) // chunks
    return (rows + rpb - 1) // rpb, rpb


def cs_cases():
    return [CSCase(f"colsum-{r}x{c_}-ld{ld}-{'acc' if acc else 'set'}", r, c_, ld, acc) for (r, c_, ld) in CS_SHAPES for acc in (0, 1)]


def cs_inputs(c):
    """x [rows, ld]: randn with a per-column offset in {0, 0.5}; the columns past `cols` hold PAST_VALUE; out0 [cols] non-zero"""
    g_ = gen("colsum", c.id)
    x = torch.randn(c.rows, c.ld, generator=g_, dtype=F64) + 0.5 * (torch.arange(c.ld) % 2).to(F64)
    x[:, c.cols:] = PAST_VALUE
    return dict(x=rnd(x, F32), out0=rnd(3.0 + torch.rand(c.cols, generator=g_, dtype=F64), F32))


def cs_ref(c, inp, mutant=None):
    x, out0 = inp["x"], inp["out0"]
    chunks, rpb = cs_chunks(c.rows, c.cols)
    if mutant == "ld_as_cols":
        if c.ld == c.cols:
            return None
        xs = x.reshape(-1)[:c.rows * c.cols].view(c.rows, c.cols)
    else:
        xs = x[:, :c.cols]
    s = xs.sum(0)
    if mutant == "last_row_dropped":
        s = xs[:-1].sum(0)
    if mutant == "last_chunk_twice":
        if chunks == 1:
            return None
        s = s + xs[(chunks - 1) * rpb:].sum(0)
    if mutant == "memset_skipped":
        if chunks == 1 or c.acc:
            return None
        s = s + out0
    return dict(out=s + out0 if c.acc else s)


def cs_bound(c, inp):
    """a sum of rows (+ 1 with accumulate) terms in any order -- four interleaved partials, their tree, atomics between the chunks: (rows + 1) U (sum|x| + |out0|)"""
    mag = inp["x"][:, :c.cols].abs().sum(0) + (inp["out0"].abs() if c.acc else 0.0)
    ref = cs_ref(c, inp)["out"]
    b = (c.rows + 1) * U * mag
    return dict(out=Bd(b, torch.minimum(U * ref.abs(), b), 0.5))


def cs_emulate(c, inp, order):
    x = inp["x"][:, :c.cols].to(F32).t().contiguous()
    if order == "seq":
        s = fsum(x, "seq")
    else:       # the kernel's own shape: per chunk four row-interleaved partials and their tree, the chunks then added in turn
        chunks, rpb = cs_chunks(c.rows, c.cols)
        s = torch.zeros(c.cols, dtype=F32)
        for k in range(chunks):
            seg = x[:, k * rpb:(k + 1) * rpb]
            parts = [fsum(seg[:, w::4].contiguous(), "seq") if seg[:, w::4].shape[1] else torch.zeros(c.cols, dtype=F32) for w in range(4)]
            s = s + ((parts[0] + parts[1]) + (parts[2] + parts[3]))
    if c.acc:
        s = s + inp["out0"].to(F32)
    return dict(out=s.to(F64))


# ================================================================================================ sc_layernorm_bwd
LBCase = collections.namedtuple("LBCase", "id D acc params rows")
LB_D, LB_ROWS = (4, 252, 256, 260, 516, 768, 772, 1020, 1024), (1, 3, 4, 5, 33)
LB_MUTANTS = ("var_Dm1", "eps_outside", "sgx_dropped", "neighbour_stats", "dgamma_overwritten", "dbeta_from_dy_gamma")


def lb_cases():
    """every D with every row count; accumulate_dx and dgamma / dbeta given or NULL rotate so that every D meets both values of each"""
    out = []
    for i, D in enumerate(LB_D):
        for j in range(2):
            acc, params = bool((i + j) % 2), bool(j == 0)
            out.append(LBCase(f"lnbwd-D{D}-{'acc' if acc else 'set'}-{'params' if params else 'noparams'}", D, acc, params, LB_ROWS))
    return out


def lb_inputs(c, rows):
    """x: row r has mean ROW_MEANS[r % 4] and std ROW_STDS[(r // 4 + r) % 3] (small: 2^-5 |mean|, or 1e-2 at mean 0); dy randn; gamma 1 + 0.3 randn;
    dx0 (the gradient accumulate_dx adds onto), dgamma0 and dbeta0 (the buffers the kernel adds onto) non-zero"""
    g_ = gen("lnbwd", c.id, rows)
    x = torch.randn(rows, c.D, generator=g_, dtype=F64)
    for r in range(rows):
        m = ROW_MEANS[r % 4]
        s = ROW_STDS[(r // 4 + r) % 3]
        s = (2.0 ** -5 * abs(m) if m else 1e-2) if s == "small" else s
        x[r] = x[r] * s + m
    rn = lambda *sh: torch.randn(*sh, generator=g_, dtype=F64)      # noqa: E731
    return dict(x=rnd(x, F32), dy=rnd(rn(rows, c.D), F32), gamma=rnd(1 + 0.3 * rn(c.D), F32), dx0=rnd(rn(rows, c.D), F32), dg0=rnd(2 + rn(c.D), F32),
                db0=rnd(2 + rn(c.D), F32))


def _lb_parts(c, inp, mutant=None, eps=LN_EPS):
    x, dy, gamma = inp["x"], inp["dy"], inp["gamma"]
    rows, D = x.shape
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / ((D - 1) if mutant == "var_Dm1" else D)
    rstd = 1 / (var.sqrt() + eps) if mutant == "eps_outside" else 1 / (var + eps).sqrt()
    if mutant == "neighbour_stats":
        if rows < 2:
            return None
        mean, rstd = torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0)
        d = x - mean
    xh = d * rstd
    gv = dy * gamma
    sg, sgx = gv.mean(-1, keepdim=True), (gv * xh).mean(-1, keepdim=True)
    if mutant == "sgx_dropped":
        sgx = 0 * sgx
    core = rstd * (gv - sg - xh * sgx)
    return dict(mean=mean, d=d, var=var, rstd=rstd, xh=xh, gv=gv, sg=sg, sgx=sgx, core=core)


def lb_ref(c, inp, mutant=None):
    """dx = rstd (dy gamma - mean(dy gamma) - xh mean(dy gamma xh)) [+ dx0], xh = (x - mean) rstd, biased variance, eps inside the root;
    dgamma = dgamma0 + sum_r dy xh and dbeta = dbeta0 + sum_r dy: the kernel ADDS onto both buffers"""
    if mutant in ("dgamma_overwritten", "dbeta_from_dy_gamma") and not c.params:
        return None
    q = _lb_parts(c, inp, mutant)
    if q is None:
        return None
    out = dict(dx=q["core"] + (inp["dx0"] if c.acc else 0.0))
    if c.params:
        out["dgamma"] = (0.0 if mutant == "dgamma_overwritten" else inp["dg0"]) + (inp["dy"] * q["xh"]).sum(0)
        out["dbeta"] = inp["db0"] + ((inp["dy"] * inp["gamma"]) if mutant == "dbeta_from_dy_gamma" else inp["dy"]).sum(0)
    return out


def lb_bound(c, inp, eps=LN_EPS):
    """mean: |d mean| <= U (sum|x| + 2 |mean|).  rstd: relative e_rstd = ((D + 6) U + d mean^2 / (var + eps)) / 2 + TR (row_kernels_ref.ln_pre_store_error).
    xh = (x - mean) rstd: e_xh = rstd (|d mean| + U |d|) + |xh| (e_rstd + U) -- the mean's error is MULTIPLIED by rstd, and through gv xh by |gamma|.
    gv = dy gamma: U |gv|.  sg = sum(gv) / D: (D + 2) U sum|gv| / D.  sgx = sum(gv xh) / D: (sum|gv| e_xh + (D + 2) U sum|gv xh|) / D.
    t = gv - sg - xh sgx: the three terms' errors, |sgx| e_xh + |xh| e_sgx for the product, 3 U (|gv| + |sg| + |xh sgx|) for the product and the two differences.
    dx = rstd t: rstd e_t + |rstd t| (e_rstd + U) [+ U |dx| for the accumulate].
    dgamma: sum_r |dy| (e_xh + U |xh|) (the column kernel forms xh again from the stored statistics) + (rows + 2) U (sum|dy xh| + |dgamma0|).
    dbeta: (rows + 1) U (sum|dy| + |dbeta0|)."""
    q = _lb_parts(c, inp)
    x, dy = inp["x"], inp["dy"]
    rows, D = x.shape
    dmean = U * (x.abs().sum(-1, keepdim=True) + 2 * q["mean"].abs())
    e_rstd = 0.5 * ((D + 6) * U + dmean ** 2 / (q["var"] + eps)) + TR
    e_xh = q["rstd"] * (dmean + U * q["d"].abs()) + q["xh"].abs() * (e_rstd + U)
    gv, xh, sg, sgx = q["gv"], q["xh"], q["sg"], q["sgx"]
    e_gv = U * gv.abs()
    e_sg = (D + 2) * U * gv.abs().sum(-1, keepdim=True) / D
    e_sgx = ((gv.abs() * e_xh).sum(-1, keepdim=True) + (D + 2) * U * (gv * xh).abs().sum(-1, keepdim=True)) / D
    e_t = e_gv + e_sg + sgx.abs() * e_xh + xh.abs() * e_sgx + 3 * U * (gv.abs() + sg.abs() + (xh * sgx).abs())
    ref = lb_ref(c, inp)
    e_dx = q["rstd"] * e_t + q["core"].abs() * (e_rstd + U) + U * ref["dx"].abs()
    out = dict(dx=Bd(e_dx, U * ref["dx"].abs(), 0.5))
    if c.params:
        e_g = (dy.abs() * (e_xh + U * xh.abs())).sum(0) + (rows + 2) * U * ((dy * xh).abs().sum(0) + inp["dg0"].abs()) + U * ref["dgamma"].abs()
        e_b = (rows + 1) * U * (dy.abs().sum(0) + inp["db0"].abs()) + U * ref["dbeta"].abs()
        out["dgamma"] = Bd(e_g, U * ref["dgamma"].abs(), 0.5)
        out["dbeta"] = Bd(e_b, U * ref["dbeta"].abs(), 0.5)
    return out


def lb_emulate(c, inp, order, eps=LN_EPS):
    x, dy, gamma = (inp[k].to(F32) for k in ("x", "dy", "gamma"))
    rows, D = x.shape
    mean = (fsum(x, order) / D).unsqueeze(-1)
    d = x - mean
    rstd = torch.rsqrt(fsum(d * d, order) / D + t32(eps)).unsqueeze(-1)
    xh = d * rstd
    gv = dy * gamma
    sg, sgx = (fsum(gv, order) / D).unsqueeze(-1), (fsum(gv * xh, order) / D).unsqueeze(-1)
    dx = rstd * (gv - sg - xh * sgx)
    if c.acc:
        dx = dx + inp["dx0"].to(F32)
    out = dict(dx=dx.to(F64))
    if c.params:
        rows_order = range(rows) if order == "seq" else reversed(range(rows))
        g, b = torch.zeros(D, dtype=F32), torch.zeros(D, dtype=F32)
        for r in rows_order:
            g = g + dy[r] * (x[r] - mean[r]) * rstd[r]
            b = b + dy[r]
        out["dgamma"], out["dbeta"] = (inp["dg0"].to(F32) + g).to(F64), (inp["db0"].to(F32) + b).to(F64)
    return out


# ================================================================================================ sc_gelu_f32 / sc_quickgelu_f32
ActCase = collections.namedtuple("ActCase", "id kind n")          # kind: gelu_fwd gelu_bwd qgelu_fwd qgelu_fwd_bf16 qgelu_bwd
ACT_KINDS = ("gelu_fwd", "gelu_bwd", "qgelu_fwd", "qgelu_fwd_bf16", "qgelu_bwd")
ACT_N = (1, 255, 256, 257)
ACT_MUTANTS = ("tanh_form", "pdf_no_half", "const_1.7", "bf16_truncation")
QG = 1.702


def act_grid():
    """[-12, 12] in steps of 2^-6, +0 and -0, points dense around 0, and -- above 10.5, where fp32 sigmoid(1.702 x) is exactly 1 and QuickGELU returns x itself --
    inputs that lie exactly half way between two bf16 numbers (the ties of the bf16 store)"""
    z = torch.arange(-12 * 64, 12 * 64 + 1, dtype=F64) / 64
    small = torch.tensor([2.0 ** -k for k in range(7, 30, 3)], dtype=F64)
    ties = torch.tensor([10.5 + 1 / 32, 10.5 + 3 / 32, 11 + 1 / 32, 11.5 + 3 / 32, 11.75 + 1 / 32], dtype=F64)
    return torch.cat([z, torch.tensor([0.0, -0.0], dtype=F64), small, -small, ties])


def act_cases():
    full = act_grid().numel()
    return [ActCase(f"{k}-n{n}", k, n) for k in ACT_KINDS for n in ACT_N + (full,)]


def act_inputs(c):
    """the grid in a fixed shuffle, its first n points; dh (the backward's incoming gradient) randn"""
    z = act_grid()
    g_ = gen("act")
    z = torch.cat([torch.tensor([0.75], dtype=F64), z[torch.randperm(z.numel(), generator=g_)]])[:c.n]      # (n = 1: a point where no output vanishes)
    return dict(z=rnd(z, F32), dh=rnd(torch.randn(z.numel(), generator=gen("act-dh"), dtype=F64)[:c.n] + 0.1, F32))


def _act_f(c, z, mutant=None):
    """the fp64 function the kernel applies (forward value, or the derivative the backward multiplies by)"""
    gelu = c.kind.startswith("gelu")
    if mutant in ("tanh_form", "pdf_no_half") and not gelu or mutant == "const_1.7" and gelu:
        return None
    if mutant == "pdf_no_half" and c.kind != "gelu_bwd" or mutant == "bf16_truncation" and c.kind != "qgelu_fwd_bf16":
        return None
    if gelu:
        if mutant == "tanh_form":
            zz = z.clone().requires_grad_(True)
            y = torch.nn.functional.gelu(zz, approximate="tanh")
            if c.kind == "gelu_fwd":
                return y.detach()
            return torch.autograd.grad(y.sum(), zz)[0]
        cdf = 0.5 * (1 + torch.erf(z / 2 ** 0.5))
        if c.kind == "gelu_fwd":
            return z * cdf
        pdf = (2 * math.pi) ** -0.5 * torch.exp(-(1.0 if mutant == "pdf_no_half" else 0.5) * z * z)
        return cdf + z * pdf
    k = 1.7 if mutant == "const_1.7" else QG
    s = torch.sigmoid(k * z)
    return s * (1 + k * z * (1 - s)) if c.kind == "qgelu_bwd" else z * s


def act_ref(c, inp, mutant=None):
    f = _act_f(c, inp["z"], mutant)
    if f is None:
        return None
    if c.kind.endswith("bwd"):
        return dict(out=inp["dh"] * f)
    if mutant == "bf16_truncation":
        f = (f.to(F32).view(torch.int32) & -65536).view(F32).to(F64)
    return dict(out=f)


def act_bound(c, inp):
    """GELU: a = z / sqrt 2 rounds once (and the constant once): erf moves by (2 / sqrt pi) e^(-a^2) 2 U |a|; erff itself TR |erf| (the budget); 1 + erf: U.
    The error of E = 1 + erf is ABSOLUTE in |erf|, because E cancels for z < -3: forward |z| e_E / 2 + 2 U |y|.  Backward: cdf = E / 2; pdf = c expf(-z^2 / 2):
    the argument rounds twice (2 U |arg| on the result), expf TR, the constant and the product 2 U; f = cdf + z pdf: e_cdf + |z| e_pdf + 2 U (|cdf| + |z pdf|)
    -- absolute in the magnitudes |cdf| + |z pdf|; the product with dh: U.
    QuickGELU: a = -1.702 z rounds twice (constant, product); __expf(a): TR + |a| 2^-23; s = 1 / (1 + E): e_s = s (e_E / (1 + E) + U + TR); forward |z| e_s + U |y|
    (+ the bf16 store); backward f = s (1 + t), t = 1.702 z (1 - s): e_t = |1.702 z| (e_s + U (1 - s)) + 3 U |t|, e_f = |1 + t| e_s + s (e_t + U |1 + t|) + U |f|."""
    z, dh = inp["z"], inp["dh"]
    ref = act_ref(c, inp)["out"]
    if c.kind.startswith("gelu"):
        a = z / 2 ** 0.5
        erf = torch.erf(a)
        e_E = TR * erf.abs() + 2 / math.pi ** 0.5 * torch.exp(-a * a) * 2 * U * a.abs() + U * (1 + erf).abs()
        if c.kind == "gelu_fwd":
            return dict(out=Bd(0.5 * z.abs() * e_E + 2 * U * ref.abs() + U * ref.abs(), U * ref.abs(), 0.5))
        cdf = 0.5 * (1 + erf)
        pdf = (2 * math.pi) ** -0.5 * torch.exp(-0.5 * z * z)
        e_pdf = pdf * (TR + 2 * U * 0.5 * z * z + 2 * U)
        e_f = 0.5 * e_E + z.abs() * e_pdf + 2 * U * (cdf.abs() + (z * pdf).abs())
        return dict(out=Bd(dh.abs() * e_f + U * ref.abs(), U * ref.abs(), 0.5))
    a = QG * z
    E = torch.exp(-a)
    s = torch.sigmoid(a)
    e_s = s * (E / (1 + E) * (TR + a.abs() * 2.0 ** -23 + 2 * U * a.abs()) + U + TR)
    if c.kind != "qgelu_bwd":
        st = store_bound(ref, BF if c.kind == "qgelu_fwd_bf16" else F32)
        return dict(out=Bd(z.abs() * e_s + U * ref.abs() + st, st, 0.5))
    t = a * (1 - s)
    f = s * (1 + t)
    e_t = a.abs() * (e_s + U * (1 - s)) + 3 * U * t.abs()
    e_f = (1 + t).abs() * e_s + s * (e_t + U * (1 + t).abs()) + U * f.abs()
    return dict(out=Bd(dh.abs() * e_f + U * ref.abs(), U * ref.abs(), 0.5))


def act_emulate(c, inp, order):
    """"seq": torch's fp32 erf / exp; "pair64": the transcendental exact (fp64, rounded once), everything around it fp32"""
    z, dh = inp["z"].to(F32), inp["dh"].to(F32)
    fn = (lambda f, t: f(t)) if order == "seq" else (lambda f, t: f(t.to(F64)).to(F32))
    if c.kind.startswith("gelu"):
        erf = fn(torch.erf, z * t32(0.70710678118654752))
        if c.kind == "gelu_fwd":
            return dict(out=(t32(0.5) * z * (t32(1.0) + erf)).to(F64))
        cdf = t32(0.5) * (t32(1.0) + erf)
        pdf = t32(0.3989422804014327) * fn(torch.exp, t32(-0.5) * z * z)
        return dict(out=(dh * (cdf + z * pdf)).to(F64))
    s = t32(1.0) / (t32(1.0) + fn(torch.exp, t32(-QG) * z))
    if c.kind == "qgelu_bwd":
        return dict(out=(dh * (s * (t32(1.0) + t32(QG) * z * (t32(1.0) - s)))).to(F64))
    y = z * s
    return dict(out=(y.to(BF) if c.kind == "qgelu_fwd_bf16" else y).to(F64))


# ================================================================================================ the small row kernels
SM_D, SM_ROWS = (4, 60, 64, 68, 512), (1, 5)
SmallCase = collections.namedtuple("SmallCase", "id kind rows D opt")


def _row_scales(rows):
    return torch.logspace(-2, 2, rows, dtype=F64).view(-1, 1) if rows > 1 else torch.ones(1, 1, dtype=F64)


# ---- sc_l2norm_bwd
def l2b_cases():
    return [SmallCase(f"l2bwd-{r}x{D}", "l2bwd", r, D, None) for D in SM_D for r in SM_ROWS]


def l2b_inputs(c):
    g_ = gen("l2bwd", c.id)
    return dict(x=rnd(torch.randn(c.rows, c.D, generator=g_, dtype=F64) * _row_scales(c.rows), F32), dy=rnd(torch.randn(c.rows, c.D, generator=g_, dtype=F64), F32))


def _l2b_parts(inp):
    x, dy = inp["x"], inp["dy"]
    ss, dot = (x * x).sum(-1, keepdim=True), (x * dy).sum(-1, keepdim=True)
    inv = ss ** -0.5
    return ss, dot, inv, x * dot * inv * inv


def l2b_ref(c, inp, mutant=None):
    """y = x / |x|: dx = (dy - y (y . dy)) / |x|"""
    ss, dot, inv, proj = _l2b_parts(inp)
    return dict(dx=inv * (inp["dy"] - (0.0 if mutant == "projection_dropped" else proj)))


def l2b_bound(c, inp):
    """ss: (D + 1) U relative, inv = rsqrt(ss): e_inv = (D + 1) U / 2 + TR; dot: (D + 1) U sum|x dy|; proj = x dot inv inv: |x| inv^2 e_dot + |proj| (2 e_inv + 3 U);
    dx = inv (dy - proj): inv (e_proj + U |dy - proj|) + |dx| (e_inv + U)"""
    x, dy = inp["x"], inp["dy"]
    D = c.D
    ss, dot, inv, proj = _l2b_parts(inp)
    e_inv = 0.5 * (D + 1) * U + TR
    e_dot = (D + 1) * U * (x * dy).abs().sum(-1, keepdim=True)
    e_proj = x.abs() * inv * inv * e_dot + proj.abs() * (2 * e_inv + 3 * U)
    ref = inv * (dy - proj)
    return dict(dx=Bd(inv * (e_proj + U * (dy - proj).abs()) + ref.abs() * (e_inv + U), U * ref.abs(), 0.5))


def l2b_emulate(c, inp, order):
    x, dy = inp["x"].to(F32), inp["dy"].to(F32)
    inv = torch.rsqrt(fsum(x * x, order)).unsqueeze(-1)
    dot = fsum(x * dy, order).unsqueeze(-1)
    return dict(dx=(inv * (dy - x * dot * inv * inv)).to(F64))


# ---- sc_add_rows_f32
ADD_ALPHA = 0.7


def add_cases():
    return [SmallCase(f"addrows-{r}x{D}-{'bcast' if bc else 'rows'}", "addrows", r, D, bc) for D in SM_D for r in SM_ROWS for bc in (False, True)]


def add_inputs(c):
    g_ = gen("addrows", c.id)
    return dict(a=rnd(torch.randn(c.rows, c.D, generator=g_, dtype=F64) * _row_scales(c.rows), F32), b=rnd(1 + torch.randn(1 if c.opt else c.rows, c.D, generator=g_, dtype=F64), F32))


def add_ref(c, inp, mutant=None):
    """out[r, c] = alpha a[r, c] + b[r % b_rows, c]"""
    b = inp["b"]
    if mutant == "broadcast_mod_rows":
        if not c.opt or c.rows == 1:
            return None
        b = torch.cat([b, torch.zeros(c.rows - 1, c.D, dtype=F64)])          # row r of a one-row b: past its end (zeros here)
    return dict(out=f32v(ADD_ALPHA) * inp["a"] + b)


def add_bound(c, inp):
    """one FMA: U |out|; a compiler that splits it adds U |alpha a|"""
    ref = add_ref(c, inp)["out"]
    return dict(out=Bd(U * (f32v(ADD_ALPHA) * inp["a"]).abs() + U * ref.abs(), 0 * ref, 1.0))


def add_emulate(c, inp, order):
    return dict(out=fma32(t32(ADD_ALPHA), inp["a"].to(F32), inp["b"].to(F32).expand(c.rows, c.D), order == "pair64").to(F64))


# ---- sc_mix_softmax_bwd
MIX_N, MIX_B = (1, 13, 25, 64), (1, 256)


def mix_cases():
    return [SmallCase(f"mixbwd-n{n}-B{B}", "mixbwd", B, n, None) for n in MIX_N for B in MIX_B]


def mix_inputs(c):
    """w spread over 20 (the extremes are pinned), dalpha_b [B, n] randn + 0.2, dw non-zero on entry"""
    g_ = gen("mixbwd", c.id)
    n, B = c.D, c.rows
    w = 20 * torch.rand(n, generator=g_, dtype=F64) - 10
    if n > 1:
        w[0], w[n - 1] = -10.0, 10.0
        w[n // 2] = 9.5
    return dict(w=rnd(w, F32), da=rnd(torch.randn(B, n, generator=g_, dtype=F64) + 0.2, F32), dw0=rnd(1 + torch.rand(n, generator=g_, dtype=F64), F32))


def mix_ref(c, inp, mutant=None):
    """alpha = softmax(w); dw += alpha (dalpha - sum alpha dalpha), dalpha = column sums of dalpha_b"""
    n = c.D
    da = inp["da"].sum(0)
    if mutant == "softmax_nm1":
        if n == 1:
            return None
        al = torch.cat([torch.softmax(inp["w"][:n - 1], 0), torch.zeros(1, dtype=F64)])
    else:
        al = torch.softmax(inp["w"], 0)
    return dict(dw=inp["dw0"] + al * (da - (al * da).sum()))


def mix_bound(c, inp):
    """dalpha: (B + 1) U sum_b|.|; alpha = expf(w - max) / sum: the argument a = w - max rounds once (2 U |a| carried, as in act_bound), the library expf TR (the
    budget), the n-term sum n U and the probability-weighted mean of the exp errors, the quotient TR and U; cbar = sum alpha dalpha: sum alpha (|dalpha| e_alpha
    + e_dalpha) + (n + 1) U sum alpha |dalpha|; alpha (dalpha - cbar): alpha (e_dalpha + e_cbar + U |diff|) + alpha |diff| (e_alpha + U); the add onto dw: U |dw|"""
    n, B = c.D, c.rows
    da, e_da = inp["da"].sum(0), (B + 1) * U * inp["da"].abs().sum(0)
    w = inp["w"]
    al = torch.softmax(w, 0)
    e_exp = TR + 2 * U * (w - w.max()).abs()
    e_al = e_exp + (al * e_exp).sum() + n * U + TR + U
    cbar = (al * da).sum()
    e_c = (al * (da.abs() * e_al + e_da)).sum() + (n + 1) * U * (al * da.abs()).sum()
    diff = da - cbar
    ref = inp["dw0"] + al * diff
    e = al * (e_da + e_c + U * diff.abs()) + al * diff.abs() * (e_al + U) + U * ref.abs()
    return dict(dw=Bd(e, U * ref.abs(), 0.5))


def mix_emulate(c, inp, order):
    w, da_b = inp["w"].to(F32), inp["da"].to(F32)
    da = fsum(da_b.t().contiguous(), order)
    e = torch.exp(w - w.max())
    al = e / fsum(e, order)
    cbar = fsum(al * da, order)
    return dict(dw=(inp["dw0"].to(F32) + al * (da - cbar)).to(F64))


# ---- sc_cosine_bwd_finish
COS_EPS = 1e-8


def cos_cases():
    return [SmallCase(f"cosfin-{r}x{E}", "cosfin", r, E, None) for E in SM_D for r in SM_ROWS]


def cos_inputs(c):
    """a [R, E] with row scales over 1e-2 .. 1e2; the LAST row has |a| < eps (elements of size 1e-10: the clamp decides); G randn, rowdot randn"""
    g_ = gen("cosfin", c.id)
    a = torch.randn(c.rows, c.D, generator=g_, dtype=F64) * _row_scales(c.rows)
    a[-1] = 1e-10 * torch.randn(c.D, generator=g_, dtype=F64)
    return dict(a=rnd(a, F32), G=rnd(torch.randn(c.rows, c.D, generator=g_, dtype=F64), F32), rd=rnd(0.5 + torch.randn(c.rows, 1, generator=g_, dtype=F64), F32))


def _cos_parts(inp):
    a = inp["a"]
    inv = 1 / a.norm(dim=-1, keepdim=True).clamp_min(f32v(COS_EPS))
    return inv, inp["rd"] * a * inv


def cos_ref(c, inp, mutant=None):
    """da = (G - rowdot a / |a|) / |a| with |a| clamped from below by eps"""
    inv, t = _cos_parts(inp)
    return dict(da=(inp["G"] - (0.0 if mutant == "projection_dropped" else t)) * inv)


def cos_bound(c, inp):
    """inv = 1 / max(sqrt(sum a^2), eps): e_inv = (E + 1) U / 2 + 2 TR; t = rowdot a inv: |t| (e_inv + 2 U); (G - t) inv: inv (e_t + U |G - t|) + |da| (e_inv + U)"""
    inv, t = _cos_parts(inp)
    e_inv = 0.5 * (c.D + 1) * U + 2 * TR
    ref = (inp["G"] - t) * inv
    return dict(da=Bd(inv * (t.abs() * (e_inv + 2 * U) + U * (inp["G"] - t).abs()) + ref.abs() * (e_inv + U), U * ref.abs(), 0.5))


def cos_emulate(c, inp, order):
    a, G, rd = (inp[k].to(F32) for k in ("a", "G", "rd"))
    inv = (t32(1.0) / torch.maximum(torch.sqrt(fsum(a * a, order)), t32(COS_EPS))).unsqueeze(-1)
    return dict(da=((G - rd * a * inv) * inv).to(F64))


# ---- sc_split_hilo_bf16
def hilo_cases():
    """nblk 2 and 3 at every shape; lda = K + 8 on every other case (both nblk meet it at every K)"""
    out, k = [], 0
    for K in SM_D:
        for r in SM_ROWS:
            for nb in (2, 3):
                lda = K + 8 if (k // 2 + k) % 2 else K
                out.append(SmallCase(f"hilo-{r}x{K}-nblk{nb}-lda{lda}", "hilo", r, K, (nb, lda)))
                k += 1
    return out


def hilo_inputs(c):
    g_ = gen("hilo", c.id)
    return dict(a=rnd(torch.randn(c.rows, c.D, generator=g_, dtype=F64) * 10 ** (6 * torch.rand(c.rows, c.D, generator=g_, dtype=F64) - 3), F32))


def hilo_ref(c, inp, mutant=None):
    """hi = bf16(a) (round to nearest even: judged BITWISE), and hi + lo = a: lo = bf16(a - hi) keeps 8 more bits, |hi + lo - a| <= 2^-16 1.001 |a|"""
    a = inp["a"]
    hi = a.to(F32).to(BF).to(F64)
    if mutant == "lo_truncated":
        lo = ((a - hi).to(F32).view(torch.int32) & -65536).view(F32).to(F64)
        return dict(hi=hi, sum=hi + lo)
    return dict(hi=hi, sum=a)


HILO_STATED = 2.0 ** -16 * 1.001          # the bound the product states (hi + lo keeps the gradient to ~16 bits); asserted as it stands


def hilo_bound(c, inp):
    """hi: exact.  hi + lo: for a in [2^e, 2^(e+1)) the remainder a - hi is at most 2^(e-8) and, a being fp32, a multiple of 2^(e-23): rounding it to bf16's 8 bits
    costs at most half a unit of 2^(e-16), so |hi + lo - a| <= 2^-17 |a| -- half the stated 2^-16, which a TRUNCATED lo (error below 2^(e-16)) would still meet.
    The tighter figure is the one judged; all of it is the one rounding of lo."""
    a = inp["a"]
    b = 2.0 ** -17 * 1.001 * a.abs()
    return dict(hi=Bd(0 * a, 0 * a, 1.0), sum=Bd(b, b, 0.5))


def hilo_emulate(c, inp, order):
    a = inp["a"].to(F32)
    hi = a.to(BF)
    return dict(hi=hi.to(F64), sum=hi.to(F64) + (a - hi.to(F32)).to(BF).to(F64))


# ================================================================================================ sc_sgemm / sc_sgemm_batched
GemmCase = collections.namedtuple("GemmCase", "id ta tb M N K batch layout ldc_pad alpha beta bias")     # layout: aligned | ldodd | off1
GEMM_MN, GEMM_K = (1, 5, 63, 64, 65, 130), (1, 15, 16, 17, 19, 2047, 2048, 2050)
GEMM_AB = ((1.0, 0.0, False), (0.5, 2.0, True), (1.0, 1.0, False))            # (alpha, beta, bias); beta = 0 runs over a NaN-filled C
GEMM_LAYOUTS = ("aligned", "ldodd", "off1")
GEMM_MUTANTS = ("last_k_dropped", "last_slice_dropped", "bias_per_slice", "beta_twice_split", "bias_n_plus1", "c_stride_ignored", "a_untransposed")


def gemm_split(M, N, K, batch):
    """sc_sgemm_batched's split-K rule restated -> (slices, k per slice); slices > 1 is the atomic path"""
    tiles = ((M + 63) // 64) * ((N + 63) // 64) * batch
    split = 1
    if tiles < 128 and K >= 2048:
        split = min(64, max(1, 512 // tiles))
        while split > 1 and K // split < 256:
            split -= 1
    kps = ((K + split - 1) // split + 15) // 16 * 16
    return (K + kps - 1) // kps, kps


def gemm_cases():
    """every (transa, transb) meets every K; M, N, the operand layout, ldc = N + 3, the (alpha, beta, bias) triple and the batch rotate underneath, and the tail of
    the list pins what the rotation could miss: every triple in both the split and the non-split path, batch 3 with K = 2050 and a per-batch bias"""
    out, k = [], 0

    def add(ta, tb, M, N, K, batch, layout, pad, abi):
        al, be, bias = GEMM_AB[abi]
        out.append(GemmCase(f"sgemm-{'t' if ta else 'n'}{'t' if tb else 'n'}-{M}x{N}x{K}-b{batch}-{layout}{'-ldc3' if pad else ''}-a{al:g}b{be:g}{'-bias' if bias else ''}",
                            ta, tb, M, N, K, batch, layout, pad, al, be, bias))
    for ti, (ta, tb) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        for ki, K in enumerate(GEMM_K):
            big = K >= 2047
            add(ta, tb, GEMM_MN[(k + ti) % 6], GEMM_MN[(2 * k + ki + 3) % 6], K, 3 if (k % 4 == 3 and not big) else 1, GEMM_LAYOUTS[k % 3], k % 2 == 1, (k // 2) % 3)
            k += 1
    for abi in range(3):
        add(False, True, 65, 5, 2048, 1, "aligned", abi == 1, abi)
        add(True, False, 5, 65, 19, 1, "ldodd", abi == 0, abi)
    add(True, False, 63, 130, 2050, 3, "aligned", True, 1)
    add(False, True, 130, 64, 2050, 3, "off1", False, 1)
    add(False, False, 64, 63, 2050, 3, "ldodd", False, 2)
    add(True, True, 5, 130, 17, 3, "off1", True, 1)
    return out


def gemm_ld(c, rows_len):
    """leading dimension of an operand whose rows hold rows_len elements: aligned / off1: the next multiple of 4 (+ 4 when already one, so that a gap exists);
    ldodd: the next value that is NOT a multiple of 4"""
    if c.layout == "ldodd":
        ld = rows_len + 1
        return ld + 1 if ld % 4 == 0 else ld
    return (rows_len // 4 + 1) * 4


def gemm_inputs(c):
    """A, B as STORED ([batch, rows, ld], the gap columns PAST_VALUE), bias [batch, N] (per-batch: strideBias = N), C0 [batch, M, N] (NaN when beta = 0)"""
    g_ = gen("sgemm", c.id)
    ar, ac = (c.K, c.M) if c.ta else (c.M, c.K)
    br, bc = (c.N, c.K) if c.tb else (c.K, c.N)
    lda, ldb = gemm_ld(c, ac), gemm_ld(c, bc)
    A = torch.full((c.batch, ar, lda), PAST_VALUE, dtype=F64)
    B = torch.full((c.batch, br, ldb), PAST_VALUE, dtype=F64)
    A[:, :, :ac] = torch.randn(c.batch, ar, ac, generator=g_, dtype=F64)
    B[:, :, :bc] = torch.randn(c.batch, br, bc, generator=g_, dtype=F64) + 0.25
    bias = 1 + torch.randn(c.batch, c.N, generator=g_, dtype=F64)
    C0 = 2 + torch.randn(c.batch, c.M, c.N, generator=g_, dtype=F64)
    if c.beta == 0:
        C0[:] = float("nan")
    return dict(A=rnd(A, F32), B=rnd(B, F32), bias=rnd(bias, F32), C0=rnd(C0, F32))


def _gemm_ops(c, inp, a_untransposed=False):
    ar, ac = (c.K, c.M) if c.ta else (c.M, c.K)
    bc = c.K if c.tb else c.N
    A, B = inp["A"], inp["B"][:, :, :bc]
    if a_untransposed:          # A read as [M, K] with the same leading dimension: element (m, k) at m lda + k of the stored buffer (zeros past its end)
        lda = A.shape[-1]
        flat = torch.cat([A.reshape(c.batch, -1), torch.zeros(c.batch, c.M * lda + c.K, dtype=F64)], 1)
        opA = torch.stack([flat[:, m * lda: m * lda + c.K] for m in range(c.M)], 1)
    else:
        opA = A[:, :, :ac].transpose(1, 2) if c.ta else A[:, :, :ac]
    opB = B.transpose(1, 2) if c.tb else B
    return opA, opB


def gemm_ref(c, inp, mutant=None):
    """C = alpha op(A) op(B) + beta C0 + bias[n] per batch; beta = 0 does not read C0"""
    split, kps = gemm_split(c.M, c.N, c.K, c.batch)
    if mutant in ("last_slice_dropped", "bias_per_slice", "beta_twice_split") and split == 1:
        return None
    if mutant in ("bias_per_slice", "bias_n_plus1") and not c.bias or mutant == "beta_twice_split" and c.beta in (0.0, 1.0):
        return None
    if mutant == "c_stride_ignored" and c.batch == 1 or mutant == "a_untransposed" and not c.ta:
        return None
    opA, opB = _gemm_ops(c, inp, mutant == "a_untransposed")
    if mutant == "last_k_dropped":
        opA, opB = opA[:, :, :c.K - 1], opB[:, :c.K - 1]
    if mutant == "last_slice_dropped":
        opA, opB = opA[:, :, :(split - 1) * kps], opB[:, :(split - 1) * kps]
    out = c.alpha * (opA @ opB)
    if c.beta != 0:
        out = out + (c.beta * c.beta if mutant == "beta_twice_split" else c.beta) * inp["C0"]
    if c.bias:
        b = inp["bias"]
        if mutant == "bias_n_plus1":
            b = torch.cat([b[:, 1:], torch.zeros(c.batch, 1, dtype=F64)], 1)
        out = out + (split if mutant == "bias_per_slice" else 1) * b.unsqueeze(1)
    if mutant == "c_stride_ignored":
        out = torch.cat([out[:1], inp["C0"][1:]])          # (batch 0 holds SOME batch's result; the others are never written)
    return dict(C=out)


def gemm_bound(c, inp):
    """(K + 2) U (|alpha| sum_k |a b| + |beta c| + |bias|), nothing added: K FMAs in any order (the k loop, the slices' atomics), the product with alpha, the two adds"""
    opA, opB = _gemm_ops(c, inp)
    mag = abs(c.alpha) * (opA.abs() @ opB.abs())
    if c.beta != 0:
        mag = mag + abs(c.beta) * inp["C0"].abs()
    if c.bias:
        mag = mag + inp["bias"].abs().unsqueeze(1)
    b = (c.K + 2) * U * mag                                  # (the last add IS the rounding of the stored value: nothing on top)
    return dict(C=Bd(b, torch.minimum(U * gemm_ref(c, inp)["C"].abs(), b), 0.5))


def gemm_emulate(c, inp, order):
    """fp32: the k products summed in `order` per slice, alpha, then the slices added onto beta C0 + bias ("seq": first to last, "pair64": last to first)"""
    opA, opB = _gemm_ops(c, inp)
    opA, opB = opA.to(F32), opB.to(F32)
    split, kps = gemm_split(c.M, c.N, c.K, c.batch)
    base = torch.zeros(c.batch, c.M, c.N, dtype=F32)
    if c.beta != 0:
        base = t32(c.beta) * inp["C0"].to(F32)
    if c.bias:
        base = base + inp["bias"].to(F32).unsqueeze(1)
    parts = []
    for s in range(split):
        a, b = opA[:, :, s * kps:(s + 1) * kps], opB[:, s * kps:(s + 1) * kps]
        parts.append(t32(c.alpha) * fsum(a.unsqueeze(2) * b.transpose(1, 2).unsqueeze(1), order))
    if split == 1:
        return dict(C=(parts[0] + base).to(F64))
    for p_ in (parts if order == "seq" else parts[::-1]):
        base = base + p_
    return dict(C=base.to(F64))


# ================================================================================================ sc_kw_bn_train_fwd / sc_kw_bn_bwd
KBCase = collections.namedtuple("KBCase", "id B K E running")
KB_SHAPES = ((2, 1, 5), (6, 8, 16), (256, 8, 64), (3, 3, 257))
KB_MOM, KB_EPS = 0.1, 1e-5
KB_MUTANTS = ("param_index_kE_e", "biased_running_var", "momentum_wrong_side", "no_1_over_B")


def kb_cases():
    return [KBCase(f"kwbn-B{B}-K{K}-E{E}-{'run' if run else 'norun'}", B, K, E, run) for (B, K, E) in KB_SHAPES for run in (True, False)]


def kb_inputs(c):
    """x [B, K E]: data column j has mean (0, 50)[j % 2] and std (1, small)[(j // 2) % 2], small = 2^-5 |mean| (1e-2 at mean 0): all four pairs in every case.
    The backward's saved statistics are the fp64 ones rounded to fp32 (its input type)."""
    g_ = gen("kwbn", c.id)
    C = c.K * c.E
    j = torch.arange(C)
    mean = torch.where(j % 2 == 1, 50.0, 0.0).to(F64)
    std = torch.where((j // 2) % 2 == 1, torch.where(mean > 0, 2.0 ** -5 * mean, torch.full_like(mean, 1e-2)), torch.ones_like(mean))
    rn = lambda *sh: torch.randn(*sh, generator=g_, dtype=F64)      # noqa: E731
    x = rnd(rn(c.B, C) * std + mean, F32)
    m = x.mean(0)
    rs = 1 / (((x - m) ** 2).mean(0) + f32v(KB_EPS)).sqrt()
    return dict(x=x, dy=rnd(rn(c.B, C), F32), gamma=rnd(1 + 0.3 * rn(C), F32), beta=rnd(0.2 * rn(C), F32), rm0=rnd(0.1 * rn(C) + 1, F32),
                rv0=rnd(1 + 0.1 * torch.rand(C, generator=g_, dtype=F64), F32), mean32=rnd(m, F32), rstd32=rnd(rs, F32))


def _kb_pidx(c, mutant=None):
    j = torch.arange(c.K * c.E)
    return j if mutant == "param_index_kE_e" else (j % c.E) * c.K + j // c.E


def kb_ref(c, inp, mutant=None):
    """nn.BatchNorm1d(E K) in train mode over the (B, E, K)-flattened keywords: the parameter of data column j = k E + e lives at e K + k.  Forward: y, the batch
    mean and rstd (biased variance, eps inside the root), running_mean / running_var (momentum on the NEW value, UNBIASED variance).  Backward, on the saved fp32
    statistics: dx = gamma rstd (dy - (sum dy + xh sum(dy xh)) / B), dgamma = sum dy xh, dbeta = sum dy (both WRITTEN at the parameter's index)."""
    if mutant == "param_index_kE_e" and (c.K == 1 or c.E == 1):
        return None
    if mutant in ("biased_running_var", "momentum_wrong_side") and not c.running:
        return None
    if mutant == "biased_running_var" and c.B == 1:
        return None
    x, dy, B = inp["x"], inp["dy"], c.B
    pidx = _kb_pidx(c, mutant)
    mom, eps = f32v(KB_MOM), f32v(KB_EPS)
    g, bt = inp["gamma"][pidx], inp["beta"][pidx]
    mean = x.mean(0)
    d = x - mean
    q = (d * d).sum(0)
    var = q / B
    rstd = 1 / (var + eps).sqrt()
    out = dict(y=d * rstd * g + bt, mean=mean, rstd=rstd)
    if c.running:
        uvar = var if (mutant == "biased_running_var" or B == 1) else q / (B - 1)
        w_old, w_new = (mom, 1 - mom) if mutant == "momentum_wrong_side" else (1 - mom, mom)
        rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
        rm[pidx] = w_old * inp["rm0"][pidx] + w_new * mean
        rv[pidx] = w_old * inp["rv0"][pidx] + w_new * uvar
        out["run_mean"], out["run_var"] = rm, rv
    xh = (x - inp["mean32"]) * inp["rstd32"]
    sg, sb = (dy * xh).sum(0), dy.sum(0)
    out["dx"] = g * inp["rstd32"] * (dy - (1.0 if mutant == "no_1_over_B" else 1.0 / B) * (sb + xh * sg))
    dg, db = torch.zeros_like(sg), torch.zeros_like(sb)
    dg[pidx], db[pidx] = sg, sb
    out["dgamma"], out["dbeta"] = dg, db
    return out


def kb_bound(c, inp):
    """Forward, as the LayerNorm with B in place of D: |d mean| <= U (sum|x| + 2 |mean|); e_rstd = ((B + 6) U + d mean^2 / (var + eps)) / 2 + TR;
    y: |gamma| rstd (|d mean| + U |d|) + |z gamma| (e_rstd + 2 U) + U |y|.  Running buffers: the new value's error times momentum and 3 U on each of the two products
    and the sum (1 - momentum rounds too); the unbiased variance carries (B + 6) U + TR relative and d mean^2 B / (B - 1).
    Backward: xh = (x - m) rs from fp32 inputs: U (|x| + |m|) rs for the difference (it cancels where |mean| >> std) and U |xh| for the product; sg = sum dy xh:
    sum|dy| e_xh + (B + 1) U sum|dy xh|; sb: (B + 1) U sum|dy|; inner = sb + xh sg: the two errors, |sg| e_xh and 2 U; t = dy - inner / B: the reciprocal TR, the
    product and the difference U each; dx = gamma rs t: two more products."""
    x, dy, B = inp["x"], inp["dy"], c.B
    r = kb_ref(c, inp)
    pidx = _kb_pidx(c)
    mom, eps = f32v(KB_MOM), f32v(KB_EPS)
    g = inp["gamma"][pidx]
    mean = r["mean"]
    d = x - mean
    var = (d * d).mean(0)
    dmean = U * (x.abs().sum(0) + 2 * mean.abs())
    e_rstd = 0.5 * ((B + 6) * U + dmean ** 2 / (var + eps)) + TR
    z = d * r["rstd"]
    fin = lambda t: U * t.abs()      # noqa: E731
    out = dict(y=Bd(g.abs() * r["rstd"] * (dmean + U * d.abs()) + (z * g).abs() * (e_rstd + 2 * U) + 2 * fin(r["y"]), fin(r["y"]), 0.5),
               mean=Bd(dmean + fin(mean), fin(mean), 0.5), rstd=Bd(r["rstd"] * e_rstd + fin(r["rstd"]), fin(r["rstd"]), 0.5))
    if c.running:
        uvar = var * B / (B - 1) if B > 1 else var
        e_rm = torch.zeros_like(inp["rm0"])
        e_rv = torch.zeros_like(inp["rv0"])
        e_rm[pidx] = mom * dmean + 3 * U * (((1 - mom) * inp["rm0"][pidx]).abs() + (mom * mean).abs())
        e_rv[pidx] = mom * (uvar * ((B + 6) * U + TR) + dmean ** 2 * (B / (B - 1) if B > 1 else 1)) + 3 * U * ((1 - mom) * inp["rv0"][pidx] + mom * uvar)
        out["run_mean"] = Bd(e_rm + fin(r["run_mean"]), fin(r["run_mean"]), 0.5)
        out["run_var"] = Bd(e_rv + fin(r["run_var"]), fin(r["run_var"]), 0.5)
    m32, rs32 = inp["mean32"], inp["rstd32"]
    xh = (x - m32) * rs32
    e_xh = U * (x.abs() + m32.abs()) * rs32 + U * xh.abs()
    sg, sb = (dy * xh).sum(0), dy.sum(0)
    e_sg = (dy.abs() * e_xh).sum(0) + (B + 1) * U * (dy * xh).abs().sum(0)
    e_sb = (B + 1) * U * dy.abs().sum(0)
    inner = sb + xh * sg
    e_in = e_sb + xh.abs() * e_sg + sg.abs() * e_xh + 2 * U * (sb.abs() + (xh * sg).abs())
    t = dy - inner / B
    e_t = (e_in + (TR + U) * inner.abs()) / B + U * t.abs()
    e_dx = (g * rs32).abs() * e_t + 2 * U * r["dx"].abs() + fin(r["dx"])
    e_dg, e_db = torch.zeros_like(sg), torch.zeros_like(sb)
    e_dg[pidx], e_db[pidx] = e_sg, e_sb
    out["dx"] = Bd(e_dx, fin(r["dx"]), 0.5)
    out["dgamma"] = Bd(e_dg + fin(r["dgamma"]), fin(r["dgamma"]), 0.5)
    out["dbeta"] = Bd(e_db + fin(r["dbeta"]), fin(r["dbeta"]), 0.5)
    return out


def kb_emulate(c, inp, order):
    x, dy = inp["x"].to(F32), inp["dy"].to(F32)
    B = c.B
    pidx = _kb_pidx(c)
    g, bt = inp["gamma"].to(F32)[pidx], inp["beta"].to(F32)[pidx]
    cs = lambda t: fsum(t.t().contiguous(), order)      # noqa: E731
    mean = cs(x) / B
    d = x - mean
    q = cs(d * d)
    var = q / B
    rstd = torch.rsqrt(var + t32(KB_EPS))
    out = dict(y=d * rstd * g + bt, mean=mean, rstd=rstd)
    if c.running:
        mom = t32(KB_MOM)
        rm, rv = inp["rm0"].to(F32).clone(), inp["rv0"].to(F32).clone()
        rm[pidx] = (t32(1.0) - mom) * rm[pidx] + mom * mean
        rv[pidx] = (t32(1.0) - mom) * rv[pidx] + mom * (q / (B - 1) if B > 1 else var)
        out["run_mean"], out["run_var"] = rm, rv
    m32, rs32 = inp["mean32"].to(F32), inp["rstd32"].to(F32)
    xh = (x - m32) * rs32
    sg, sb = cs(dy * xh), cs(dy)
    out["dx"] = g * rs32 * (dy - (t32(1.0) / t32(float(B))) * (sb + xh * sg))
    dg, db = torch.zeros_like(sg), torch.zeros_like(sb)
    dg[pidx], db[pidx] = sg, sb
    out["dgamma"], out["dbeta"] = dg, db
    return {k: v.to(F64) for k, v in out.items()}


# ================================================================================================ sc_vq_st_bwd
VQCase = collections.namedtuple("VQCase", "id R V temp nmask")
VQ_SHAPES, VQ_TEMPS, VQ_NMASK = ((1, 5), (7, 255), (7, 256), (7, 257), (3, 49408)), (0.1, 1.0), (0, 3, 8)
VQ_MUTANTS = ("masked_in_denominator", "no_inv_temp", "rowdot_over_dprob")


def vq_cases():
    return [VQCase(f"vqst-{R}x{V}-T{t:g}-mask{nm}", R, V, t, nm) for (R, V) in VQ_SHAPES for t in VQ_TEMPS for nm in VQ_NMASK]


def vq_mask_ids(c):
    """always id 0 and id V - 1; V = 5 repeats three ids (two sub-words stay live)"""
    ids = [0, c.V - 1, 2] * 3 if c.V < 16 else [0, c.V - 1, 2, 3, 7, c.V // 2, c.V - 2, 100]
    return ids[:c.nmask]


def vq_inputs(c):
    """cos: fp64 cosine similarities of unit vectors in 16 dimensions, rounded to fp32; dprob = randn + 4 cos (so that rowdot, a covariance of the two under p,
    stands clear of the rounding of its V-term sum)"""
    g_ = gen("vqst", c.id)
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)      # noqa: E731
    cos = rnd(nrm(torch.randn(c.R, 16, generator=g_, dtype=F64)) @ nrm(torch.randn(c.V, 16, generator=g_, dtype=F64)).t(), F32)
    return dict(cos=cos, g=rnd(torch.randn(c.R, c.V, generator=g_, dtype=F64) + 4 * cos, F32))


def _vq_parts(c, inp, mutant=None):
    cos, g = inp["cos"], inp["g"]
    live = torch.ones(c.V, dtype=torch.bool)
    live[vq_mask_ids(c)] = False
    it = 1 / f32v(c.temp)
    a = cos * it
    if mutant == "masked_in_denominator":
        p = torch.softmax(a, -1)
    else:
        p = torch.softmax(a.masked_fill(~live, float("-inf")), -1)
    dot = (p * g * live).sum(-1, keepdim=True) if mutant == "masked_in_denominator" else (p * g).sum(-1, keepdim=True)
    d = p * (g - dot) * (1.0 if mutant == "no_inv_temp" else it) * live
    return live, a, p, dot, d, it


def vq_ref(c, inp, mutant=None):
    """p = softmax(cos / temp) over the live sub-words; dcos = p (dprob - sum p dprob) / temp, 0 on the masked ones; rowdot = sum_v dcos cos"""
    if mutant == "masked_in_denominator" and c.nmask == 0 or mutant == "no_inv_temp" and c.temp == 1.0:
        return None
    live, a, p, dot, d, it = _vq_parts(c, inp, mutant)
    return dict(dcos=d, rowdot=(d * (inp["g"] if mutant == "rowdot_over_dprob" else inp["cos"])).sum(-1))


def vq_bound(c, inp):
    """a = (cos - max) / temp rounds three times (the difference, the host's 1 / temp, the product): 3 U |a| on top of __expf's TR + |a| 2^-23; p = e / den:
    softmax_parts with the V-term sum.  dot = sum(e dprob) / sum(e): sum p |dprob| e_p + V U sum p |dprob| + (TR + U) |dot|.  dcos = p (dprob - dot) / temp:
    p / temp (e_dot + U |dprob - dot|) + |dcos| (e_p + 3 U).  rowdot: sum|cos| e_dcos + (V + 1) U sum|dcos cos| -- against the magnitude sum|dcos cos|."""
    live, a, p, dot, d, it = _vq_parts(c, inp)
    g, cos = inp["g"], inp["cos"]
    am = a.masked_fill(~live, float("-inf"))
    _, e_p = softmax_parts(am, c.V)
    rel = 3 * U * (am - am.amax(-1, keepdim=True)).abs()
    rel = torch.where(live, rel, torch.zeros_like(rel))
    e_p = torch.where(live, e_p + rel + (p * rel).sum(-1, keepdim=True), torch.zeros_like(rel))
    pg = p * g.abs()
    e_dot = (pg * e_p).sum(-1, keepdim=True) + c.V * U * pg.sum(-1, keepdim=True) + (TR + U) * dot.abs()
    e_d = p * it * (e_dot + U * (g - dot).abs()) * live + d.abs() * (e_p + 3 * U) + U * d.abs()
    rowdot = (d * cos).sum(-1)
    e_r = (cos.abs() * e_d).sum(-1) + (c.V + 1) * U * (d * cos).abs().sum(-1) + U * rowdot.abs()
    return dict(dcos=Bd(e_d, U * d.abs(), 0.5), rowdot=Bd(e_r, U * rowdot.abs(), 0.5))


def vq_emulate(c, inp, order):
    cos, g = inp["cos"].to(F32), inp["g"].to(F32)
    live = torch.ones(c.V, dtype=torch.bool)
    live[vq_mask_ids(c)] = False
    it = t32(1.0) / t32(c.temp)
    mx = cos.masked_fill(~live, float("-inf")).amax(-1, keepdim=True)
    e = torch.where(live, torch.exp((cos - mx) * it), torch.zeros((), dtype=F32))
    den, num = fsum(e, order).unsqueeze(-1), fsum(e * g, order).unsqueeze(-1)
    d = torch.where(live, e / den * (g - num / den) * it, torch.zeros((), dtype=F32))
    return dict(dcos=d.to(F64), rowdot=fsum(d * cos, order).to(F64))


# ================================================================================================ sc_attn_small_bwd
ATCase = collections.namedtuple("ATCase", "id B L H causal scale")
AT_SHAPES, AT_SCALES = ((1, 1, 1), (2, 7, 2), (3, 10, 8), (2, 16, 12)), (0.7, 4.0)
AT_MUTANTS = ("mask_j_lt_i", "scale_once", "dk_from_dS_ij", "dv_from_P_ij")


def at_cases():
    return [ATCase(f"attnbwd-B{B}-L{L}-H{H}-{'causal' if ca else 'full'}-s{sc:g}", B, L, H, ca, sc) for (B, L, H) in AT_SHAPES for ca in (True, False) for sc in AT_SCALES]


def at_inputs(c):
    """qkv [B L, 3 W] bf16 values at the case's scale (4: peaked rows), dout fp32 [B L, W]; head dim 64"""
    g_ = gen("attnbwd", c.id)
    W = c.H * 64
    return dict(qkv=rnd(c.scale * torch.randn(c.B * c.L, 3 * W, generator=g_, dtype=F64), BF), dout=rnd(torch.randn(c.B * c.L, W, generator=g_, dtype=F64), F32))


def _at_heads(c, inp):
    W = c.H * 64
    q, k, v = (t.reshape(c.B, c.L, c.H, 64).transpose(1, 2) for t in inp["qkv"].split(W, dim=1))          # [B, H, L, 64]
    return q, k, v, inp["dout"].reshape(c.B, c.L, c.H, 64).transpose(1, 2)


def _at_pack(c, dq, dk, dv):
    return torch.cat([t.transpose(1, 2).reshape(c.B * c.L, c.H * 64) for t in (dq, dk, dv)], 1)


def at_autograd(c, inp):
    """the statement: fp64 autograd of softmax(q k^T / 8 [+ causal mask]) v on the bf16-rounded qkv"""
    x = inp["qkv"].clone().requires_grad_(True)
    q, k, v, do = _at_heads(c, dict(qkv=x, dout=inp["dout"]))
    s = q @ k.transpose(-1, -2) / 8.0
    if c.causal:
        s = s + torch.full((c.L, c.L), float("-inf"), dtype=F64).triu(1)
    ((torch.softmax(s, -1) @ v) * do).sum().backward()
    return x.grad


def _at_manual(c, inp, mutant=None):
    q, k, v, do = _at_heads(c, inp)
    scale = 0.125
    s = q @ k.transpose(-1, -2) * scale
    if c.causal:
        s = s + torch.full((c.L, c.L), float("-inf"), dtype=F64).triu(0 if mutant == "mask_j_lt_i" else 1)
    P = torch.softmax(s, -1)
    dP = do @ v.transpose(-1, -2)
    dot = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - dot) * (1.0 if mutant == "scale_once" else scale)
    dq = dS @ k
    dk = (dS if mutant == "dk_from_dS_ij" else dS.transpose(-1, -2)) @ q
    dv = (P if mutant == "dv_from_P_ij" else P.transpose(-1, -2)) @ do
    return dict(q=q, k=k, v=v, do=do, s=s, P=P, dP=dP, dot=dot, dS=dS, dq=dq, dk=dk, dv=dv)


def at_ref(c, inp, mutant=None):
    if mutant is None:
        return dict(dqkv=at_autograd(c, inp))
    if mutant == "mask_j_lt_i" and not c.causal or mutant in ("dk_from_dS_ij", "dv_from_P_ij") and c.L == 1:
        return None
    m = _at_manual(c, inp, mutant)
    return dict(dqkv=_at_pack(c, m["dq"], m["dk"], m["dv"]))


def at_bound(c, inp):
    """s_ij = (sum of 64 q k) / 8: 65 U sum|q k| / 8.  dP_ij = sum of 64 do v: 64 U sum|do v|.  P = softmax(s): softmax_parts over the L keys, plus the score's error
    MULTIPLIED by the probability it feeds (e_s_ij + sum_j P_ij e_s_ij), plus 2^-126 absolute (an fp32 exp below the normal range is flushed).
    dot = sum_j P dP: sum P (|dP| e_P + e_dP) + (L + 1) U sum P |dP|.  dS = P (dP - dot) / 8: P (e_dP + e_dot + U |dP - dot|) / 8 + |dS| (e_P + 2 U).
    dq_i = sum_j dS_ij k_j: sum e_dS |k| + (L + 1) U sum|dS k|; dk_i = sum_j dS_ji q_j likewise; dv_i = sum_j P_ji do_j: sum P e_P |do| + (L + 1) U sum P |do|."""
    m = _at_manual(c, inp)
    q, k, v, do, P, dP, dot, dS = (m[n] for n in ("q", "k", "v", "do", "P", "dP", "dot", "dS"))
    L = c.L
    T_ = lambda t: t.transpose(-1, -2)      # noqa: E731
    e_s = 65 * U * (q.abs() @ T_(k.abs())) * 0.125
    e_dP = 64 * U * (do.abs() @ T_(v.abs()))
    _, e_P = softmax_parts(m["s"], L)
    live = torch.isfinite(m["s"])
    e_s = torch.where(live, e_s, torch.zeros_like(e_s))
    e_Pa = P * (e_P + 1.01 * (e_s + (P * e_s).sum(-1, keepdim=True))) + 2.0 ** -126          # absolute
    e_dot = (e_Pa * dP.abs() + P * e_dP).sum(-1, keepdim=True) + (L + 1) * U * (P * dP.abs()).sum(-1, keepdim=True)
    e_dS = 0.125 * (P * (e_dP + e_dot + U * (dP - dot).abs()) + e_Pa * (dP - dot).abs()) + 2 * U * dS.abs()
    e_dq = e_dS @ k.abs() + (L + 1) * U * (dS.abs() @ k.abs())
    e_dk = T_(e_dS) @ q.abs() + (L + 1) * U * (T_(dS.abs()) @ q.abs())
    e_dv = T_(e_Pa) @ do.abs() + (L + 1) * U * (T_(P) @ do.abs())
    ref = at_autograd(c, inp)
    return dict(dqkv=Bd(_at_pack(c, e_dq, e_dk, e_dv) + U * ref.abs(), U * ref.abs(), 0.5))


def at_emulate(c, inp, order):
    q, k, v, do = (t.to(F32) for t in _at_heads(c, inp))
    L = c.L
    sc = t32(0.125)
    s = fsum(q.unsqueeze(3) * k.unsqueeze(2), order) * sc                    # [B, H, L, L]
    dP = fsum(do.unsqueeze(3) * v.unsqueeze(2), order)
    if c.causal:
        s = s + torch.full((L, L), float("-inf"), dtype=F32).triu(1)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    P = e / fsum(e, order).unsqueeze(-1)
    dot = fsum(P * dP, order).unsqueeze(-1)
    dS = P * (dP - dot) * sc
    mm = lambda a, b: fsum((a.unsqueeze(-1) * b.unsqueeze(-3)).transpose(-1, -2).contiguous(), order)      # noqa: E731  [.., i, j] x [.., j, d] -> [.., i, d]
    dq, dk, dv = mm(dS, k), mm(dS.transpose(-1, -2), q), mm(P.transpose(-1, -2), do)
    return dict(dqkv=_at_pack(c, dq, dk, dv).to(F64))


# ================================================================================================ sc_infonce_fwd + sc_infonce_bwd (+ the two sc_sgemm behind dfeat)
NCECase = collections.namedtuple("NCECase", "id Bg E inv_t ids margin dcl a2b b2a zero")      # ids: none | unique | dup | allsame
NCE_BG, NCE_E, NCE_INVT, NCE_KINDS, NCE_DIRS = (1, 2, 63, 64, 65, 130, 257), (4, 20, 64, 512), (1 / 0.07, 50.0), ("none", "unique", "dup", "allsame"), ((True, True), (True, False), (False, True))
NCE_MUTANTS = ("diag_excluded", "margin_denominator_only", "ids_32bit", "slab_dropped", "sums_swapped", "half_kept_single", "dinv_before_margin")


def nce_cases():
    """every (Bg, E) of the two lists, and Bg = 2048 at E = 64.  The temperature, the margin, the id kind, dcl and the direction pair are each a function of the Bg
    index j and the E index e chosen so that no two of them move together: for a fixed E the pair (inv_t, margin) takes all four values over j, every id kind meets
    both margins and (where a negative exists) both dcl, tests/test_tail_kernel_bounds_cpu.py asserts it.  dcl = 1 needs
    a negative in every row: it is switched off where the rotation would leave none (Bg = 1, two rows sharing an id, all ids equal); those cases are `zero`."""
    out, k = [], 0

    def add(Bg, E, it, kind, margin, dcl, dirs):
        lone = kind == "allsame" or Bg == 1 or (Bg == 2 and kind == "dup")          # no negative but the diagonal: loss and G are 0 up to the bound
        dcl = False if lone else True if Bg == 2 else dcl                              # (two rows: the one negative must not drown beside the diagonal)
        out.append(NCECase(f"infonce-Bg{Bg}-E{E}-it{it:.4g}-{kind}-m{margin:g}-{'dcl' if dcl else 'nodcl'}-{'a2b' if dirs[0] else ''}{'b2a' if dirs[1] else ''}",
                           Bg, E, it, kind, margin, dcl, dirs[0], dirs[1], lone))
    for j, Bg in enumerate(NCE_BG):
        for e, E in enumerate(NCE_E):
            add(Bg, E, NCE_INVT[(j + e) % 2], NCE_KINDS[(2 * e + j // 2 + e // 2) % 4], (0.0, 0.2)[(j // 2 + e) % 2], bool(j % 2), NCE_DIRS[k % 3])
            k += 1
    add(2048, 64, NCE_INVT[0], "dup", 0.2, True, NCE_DIRS[0])
    return out


def nce_ids(c):
    """unique ids ABOVE 2^32 whose low words collide in pairs (rows 2k and 2k + 1): a 32-bit comparison would call them equal.  dup: rows 0 / 1 share an id, and
    rows 63 / 64 / 65 -- across the border of the first 64-row tile -- share one."""
    if c.ids == "none":
        return None
    i = torch.arange(c.Bg, dtype=torch.int64)
    ids = (i // 2) + (1 + i % 2) * 2 ** 32
    if c.ids == "allsame":
        ids[:] = 7 + 2 ** 33
    if c.ids == "dup":
        if c.Bg > 1:
            ids[1] = ids[0]
        if c.Bg > 65:
            ids[64], ids[65] = ids[63], ids[63]
    return ids


def nce_inputs(c):
    """unit rows a_i, b_i = normalize(a_i + 0.3 noise), noise standard normal per element: cos(a_i, b_i) = 1 / sqrt(1 + 0.09 E) against negatives of size 1 / sqrt(E)
    -- the positives dominate, and the loss stays of order 1 (no row whose -l_ii + log sum cancels to nothing)"""
    g_ = gen("infonce", c.id)
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)      # noqa: E731
    a = nrm(torch.randn(c.Bg, c.E, generator=g_, dtype=F64))
    b = nrm(a + 0.3 * torch.randn(c.Bg, c.E, generator=g_, dtype=F64))
    out = dict(a=rnd(a, F32), b=rnd(b, F32))
    if c.ids != "none":
        out["ids"] = nce_ids(c)
    return out


def _nce_parts(c, inp, mutant=None):
    a, b, Bg = inp["a"], inp["b"], c.Bg
    it, mg = f32v(c.inv_t), f32v(c.margin)
    eye = torch.eye(Bg, dtype=torch.bool)
    sdot = a @ b.t()
    l0 = sdot * it
    lm = l0 - mg * eye if mg > 0 else l0
    ids = inp.get("ids")
    if ids is None:
        neg = ~eye
    else:
        idc = ids & 0xffffffff if mutant == "ids_32bit" else ids
        neg = idc[:, None] != idc[None, :]
    if not c.dcl and mutant != "diag_excluded":
        neg = neg | eye
    pos = (l0 if mutant == "margin_denominator_only" else lm).diagonal()
    e = torch.where(neg, lm.exp(), torch.zeros((), dtype=F64))
    rs, cs = e.sum(1), e.sum(0)
    if mutant == "slab_dropped":
        cut = (Bg - 1) // 64 * 64
        rs, cs = e[:, :cut].sum(1), e[:cut].sum(0)
    la, lb = (-pos + rs.log()).mean(), (-pos + cs.log()).mean()
    both = c.a2b and c.b2a
    half = 0.5 if (both or mutant == "half_kept_single") else 1.0
    loss = ((la if c.a2b else 0.0) + (lb if c.b2a else 0.0)) * half
    wa, wb = (half / Bg if c.a2b else 0.0), (half / Bg if c.b2a else 0.0)

    def G_of(ee):
        if mutant == "sums_swapped":
            return wa * ee / cs[:, None] + wb * ee / rs[None, :] - (wa + wb) * eye
        return wa * ee / rs[:, None] + wb * ee / cs[None, :] - (wa + wb) * eye
    G = G_of(e)
    dinv = ((G_of(torch.where(neg, l0.exp(), torch.zeros((), dtype=F64))) if mutant == "dinv_before_margin" else G) * sdot).sum()
    return dict(sdot=sdot, lm=lm, e=e, rs=rs, cs=cs, pos=pos, la=la, lb=lb, loss=loss, wa=wa, wb=wb, G=G, dinv=dinv, it=it, mg=mg, eye=eye)


def nce_ref(c, inp, mutant=None):
    """logits = a b^T inv_t (diagonal - margin); negatives: ids differ (no ids: off the diagonal), plus the diagonal unless dcl; NO maximum is subtracted, as in the
    reference code.  out3 = (loss, mean_i(-l_ii + log sum_j e), mean_j(-l_jj + log sum_i e)); G = d loss / d logits; dinv = sum G_ij (a_i . b_j);
    dfeat_a = inv_t G b, dfeat_b = inv_t G^T a"""
    if mutant == "diag_excluded" and c.dcl or mutant in ("margin_denominator_only", "dinv_before_margin") and c.margin == 0:
        return None
    if mutant == "ids_32bit" and c.ids in ("none", "allsame") or mutant == "slab_dropped" and c.Bg <= 64 or mutant == "half_kept_single" and c.a2b and c.b2a:
        return None
    if mutant == "diag_excluded" and (c.zero or c.Bg == 1 or (c.Bg == 2 and c.ids == "dup")):
        return None          # (no negative would be left: the wrong kernel's loss is log 0)
    q = _nce_parts(c, inp, mutant)
    return dict(out3=torch.stack([q["loss"] + 0 * q["la"], q["la"], q["lb"]]), G=q["G"], dinv=q["dinv"].reshape(1), dfeat_a=q["it"] * q["G"] @ inp["b"],
                dfeat_b=q["it"] * q["G"].t() @ inp["a"])


def nce_bound(c, inp):
    """sdot: (E + 1) U sum|a b|.  l = sdot inv_t - margin: inv_t e_sdot + 2 U |l| + U margin.  e = __expf(l): relative TR + |l| 2^-23 + e_l -- the logit's error is
    MULTIPLIED by the probability the exp feeds.  Row / column sums of Bg terms over the tiles' slabs: sum e rel + (Bg + 1) U sum; relative r = that / sum.
    -l_ii + logf(sum): e_l_ii + TR |log| (the logf budget) + r + 2 U (|l_ii| + |log|); the mean is taken in fp64 and rounds twice on the way out.
    G_ij = wa e / rs_i + wb e / cs_j - (wa + wb) [i = j]: each quotient rel + r + TR, the products and sums 2 U, the diagonal's difference 2 U (wa + wb), and 2^-126 absolute:
    an fp32 term below the normal range is flushed (E = 4 at inv_t = 50 has negatives at e^-50 of a row sum of e^+50).
    dinv = sum G sdot: sum(|sdot| e_G + |G| e_sdot) and the fp32 part of the sum -- 16 terms per thread, 6 wave steps, 3 adds per block, fp64 after -- 26 U sum|G sdot|
    (tighter than the n-term rule over Bg^2 terms; the magnitude sum|G sdot| is what it is judged against).
    dfeat: the sc_sgemm bound (Bg + 2) U inv_t sum|G b| on top of inv_t e_G |b|."""
    q = _nce_parts(c, inp)
    a, b, Bg, E = inp["a"], inp["b"], c.Bg, c.E
    it, mg, eye = q["it"], q["mg"], q["eye"]
    e, rs, cs, G, sdot, wa, wb = (q[k] for k in ("e", "rs", "cs", "G", "sdot", "wa", "wb"))
    e_sd = (E + 1) * U * (a.abs() @ b.abs().t())
    e_l = it * e_sd + 2 * U * q["lm"].abs() + U * mg * eye
    rel = TR + q["lm"].abs() * 2.0 ** -23 + e_l
    r_rs = ((e * rel).sum(1) + (Bg + 1) * U * rs) / rs
    r_cs = ((e * rel).sum(0) + (Bg + 1) * U * cs) / cs
    e_pos = e_l.diagonal()

    def e_mean(sm, r, val):
        return (e_pos + TR * sm.log().abs() + r + 2 * U * (q["pos"].abs() + sm.log().abs())).mean() + 2 * U * val.abs()
    e_la, e_lb = e_mean(rs, r_rs, q["la"]), e_mean(cs, r_cs, q["lb"])
    half = 0.5 if (c.a2b and c.b2a) else 1.0
    e_loss = ((e_la if c.a2b else 0.0) + (e_lb if c.b2a else 0.0)) * half + 2 * U * q["loss"].abs()
    out3 = torch.stack([e_loss + 0 * e_la, e_la, e_lb])
    ref3 = torch.stack([q["loss"] + 0 * q["la"], q["la"], q["lb"]])
    e_G = wa * e / rs[:, None] * (rel + r_rs[:, None] + TR + 2 * U) + wb * e / cs[None, :] * (rel + r_cs[None, :] + TR + 2 * U) + 2 * U * (wa + wb) * eye + 2 * U * G.abs() + 2.0 ** -126
    e_dinv = ((sdot.abs() * e_G + G.abs() * e_sd).sum() + 26 * U * (G * sdot).abs().sum() + U * q["dinv"].abs()).reshape(1)
    dfa, dfb = it * G @ b, it * G.t() @ a
    e_dfa = it * (e_G @ b.abs()) + (Bg + 2) * U * it * (G.abs() @ b.abs())
    e_dfb = it * (e_G.t() @ a.abs()) + (Bg + 2) * U * it * (G.abs().t() @ a.abs())
    st = lambda t: U * t.abs()      # noqa: E731
    return dict(out3=Bd(out3, st(ref3), 0.5), G=Bd(e_G, st(G), 0.5), dinv=Bd(e_dinv, st(q["dinv"]).reshape(1), 0.5), dfeat_a=Bd(e_dfa, torch.minimum(st(dfa), e_dfa), 0.5),
                dfeat_b=Bd(e_dfb, torch.minimum(st(dfb), e_dfb), 0.5))


def nce_emulate(c, inp, order):
    """fp32; the E-term dot products in torch's own order ("seq") or with the columns reversed ("pair64"), the Bg-term sums in `order`"""
    a, b = inp["a"].to(F32), inp["b"].to(F32)
    if order != "seq":
        a, b = a.flip(1).contiguous(), b.flip(1).contiguous()
    Bg = c.Bg
    eye = torch.eye(Bg, dtype=torch.bool)
    sdot = a @ b.t()
    l = sdot * t32(c.inv_t)
    if c.margin > 0:
        l = torch.where(eye, l - t32(c.margin), l)
    ids = inp.get("ids")
    neg = ~eye if ids is None else ids[:, None] != ids[None, :]
    if not c.dcl:
        neg = neg | eye
    e = torch.where(neg, torch.exp(l), torch.zeros((), dtype=F32))
    rs, cs = fsum(e, order), fsum(e.t().contiguous(), order)
    pos = l.diagonal()
    la, lb = (-pos + torch.log(rs)).to(F64).sum() / Bg, (-pos + torch.log(cs)).to(F64).sum() / Bg
    both = c.a2b and c.b2a
    loss = ((la if c.a2b else 0.0) + (lb if c.b2a else 0.0)) * (0.5 if both else 1.0)
    scale = t32(0.5 if both else 1.0) / t32(float(Bg))
    wa, wb = (scale if c.a2b else t32(0.0)), (scale if c.b2a else t32(0.0))
    G = wa * (e / rs[:, None]) + wb * (e / cs[None, :])
    G = torch.where(eye, G - (wa + wb), G)
    it = t32(c.inv_t)
    return dict(out3=torch.stack([loss + 0 * la, la, lb]).to(F32).to(F64), G=G.to(F64), dinv=(G * sdot).to(F64).sum().to(F32).to(F64).reshape(1),
                dfeat_a=(it * (G @ inp["b"].to(F32))).to(F64), dfeat_b=(it * (G.t() @ inp["a"].to(F32))).to(F64))


# ================================================================================================ the groups
GROUPS = collections.OrderedDict((g.name, g) for g in (
    Group("adam", adam_cases, adam_inputs, adam_ref, adam_bound, adam_emulate, ADAM_MUTANTS),
    Group("gradnorm", gn_cases, gn_inputs, gn_ref, gn_bound, gn_emulate, GN_MUTANTS),
    Group("colsum", cs_cases, cs_inputs, cs_ref, cs_bound, cs_emulate, CS_MUTANTS),
    Group("act", act_cases, act_inputs, act_ref, act_bound, act_emulate, ACT_MUTANTS),
    Group("l2bwd", l2b_cases, l2b_inputs, l2b_ref, l2b_bound, l2b_emulate, ("projection_dropped",)),
    Group("addrows", add_cases, add_inputs, add_ref, add_bound, add_emulate, ("broadcast_mod_rows",)),
    Group("mixbwd", mix_cases, mix_inputs, mix_ref, mix_bound, mix_emulate, ("softmax_nm1",)),
    Group("cosfin", cos_cases, cos_inputs, cos_ref, cos_bound, cos_emulate, ("projection_dropped",)),
    Group("hilo", hilo_cases, hilo_inputs, hilo_ref, hilo_bound, hilo_emulate, ("lo_truncated",)),
    Group("sgemm", gemm_cases, gemm_inputs, gemm_ref, gemm_bound, gemm_emulate, GEMM_MUTANTS),
    Group("kwbn", kb_cases, kb_inputs, kb_ref, kb_bound, kb_emulate, KB_MUTANTS),
    Group("vqst", vq_cases, vq_inputs, vq_ref, vq_bound, vq_emulate, VQ_MUTANTS),
    Group("attnbwd", at_cases, at_inputs, at_ref, at_bound, at_emulate, AT_MUTANTS),
    Group("infonce", nce_cases, nce_inputs, nce_ref, nce_bound, nce_emulate, NCE_MUTANTS),
))
# sc_layernorm_bwd: one case runs at every row count of LB_ROWS; the variants below are (case, rows) pairs under the same interface
LBVar = collections.namedtuple("LBVar", "id D acc params rows base")


def lbv_cases():
    return [LBVar(f"{c.id}-rows{r}", c.D, c.acc, c.params, r, c) for c in lb_cases() for r in c.rows]


GROUPS["lnbwd"] = Group("lnbwd", lbv_cases, lambda v: lb_inputs(v.base, v.rows), lb_ref, lb_bound, lb_emulate, LB_MUTANTS)

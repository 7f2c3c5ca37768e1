"""Plain fp64 statements, case lists, deterministic inputs and DERIVED per-element bounds of the quantizer-mode kernels (csrc/vq_modes.hip) for
tests/test_vq_modes_parity_gpu.py and tools/vq_mode_bounds.py.  A helper module, not a test; no kernel runs here.  The constants, the generator, the rounding
helper, the judge and the Group / Bd tuples are those of tests/row_kernels_ref.py and tests/tail_kernels_ref.py; the noise contract is that of tests/vq_modes_ref.py.

Every input is generated on the CPU from a fixed seed and ROUNDED TO FP32 before the reference sees it; every reference is torch fp64 of exactly the stated
operation; every bound function returns, per output, a tensor of the output's shape, and every element is judged.

The rules are row_kernels_ref.py's (n-term fp32 sum: n U sum|terms| against the MAGNITUDE reference; every other fp32 operation U; rcp / exp / `/`: TR each;
__expf(a): |a| 2^-23 on top) with tail_kernels_ref.py's BUDGET for the library logf (TR relative).  What this file adds:

  noise        g = -logf(e), e = -logf(u), u exact: a relative error TR of e is an ABSOLUTE error TR of g, and the outer logf adds TR |g|:  TR (1 + |g|).
  logit        s = x + g rounds once more: d_s = TR (1 + |g|) + U |s| (0 without noise).  The softmax is invariant under a common shift of a row, so the error of
               the row maximum cancels in every probability; what remains per column is d_s / T, which moves p_v by p_v (d_v + sum_w p_w d_w) -- 1 / T in the
               logit, p in the probability, and the sum over the row through sum p d.  row_den is NOT shift-invariant: it also carries the maximum's d_s / T.
  flush        an fp32 result below the smallest normal number 2^-126 may be flushed to zero (exp of a logit 88 below the maximum): FTZ absolute on every
               probability, and through it on dcos.
  (hi, lo)     bf16 keeps 8 significand bits: |x - hi| <= 2^-8 |x| at the bottom of a binade (2^-9 at its top, the half-ulp figure usually quoted), and the
               remainder, at most half an ulp of hi, rounds to lo within 2^-17 |x| (hilo_bound of tail_kernels_ref.py).  P E - (P_hi E_hi + P_lo E_hi + P_hi E_lo)
               = eps_P E + P eps_E + P_lo E_lo - eps_P eps_E with |eps| <= 2^-17 and |P_lo E_lo| <= 2^-16 |P E|:  HILO = 2^-15 * 1.001 of sum p |emb|.
  product      3 * ceil(V / 32) * 32 products accumulate in fp32 (the MFMA's own order is unknown: the n-term rule), the finish kernel adds nsplit - 1 more.

Exact statements (no bound): the fragment-ordered table, the one-hot / two-hot products on a table of 16-bit integers times powers of two, the arg-max with
planted ties, and the row with every column masked."""
import collections
import functools

import numpy as np
import torch

import vq_modes_ref as R
from row_kernels_ref import BF, F32, F64, ORDERS, TR, U, fsum, gen, rnd, softmax_parts, worst  # noqa: F401  (ORDERS, worst: for the tool and the test)
from tail_kernels_ref import Bd, Group, f32v, t32, vq_mask_ids

FTZ = 2.0 ** -126
HILO = 2.0 ** -15 * 1.001
SEED = 11
SE_BM, SE_BK = 128, 32
NOISE_FALLBACK = None          # None: the derived TR (1 + |g|) is what the GPU test asserts; a float: the figure the suite asserted before, used INSTEAD (and said so in the table)


# ================================================================================================ the host-side rules of sc_vq_soft_embed restated
def soft_ne(E):
    n = E // 64
    for c in (8, 6, 4, 3, 2, 1):
        if n % c == 0:
            return c
    return 1


def grid_y(E):
    return E // (64 * soft_ne(E))


def nsteps(V):
    return (V + SE_BK - 1) // SE_BK


def soft_nsplit(Rr, V, E, nsplit, cus=256):
    """the split count sc_vq_soft_embed launches (0 = auto: the device's compute units over the output tiles, at most 64), clamped to the steps"""
    if nsplit <= 0:
        tiles = ((Rr + SE_BM - 1) // SE_BM) * grid_y(E)
        nsplit = min(cus // max(tiles, 1), 64)
    return max(1, min(nsplit, nsteps(V)))


def split_of(v, V, ns):
    """the chunk (grid.z) that holds column v"""
    sps = (nsteps(V) + ns - 1) // ns
    return (v // SE_BK) // sps


def row_paths(Rr):
    """which parts of the 128-row tile a row count reaches: wave row 0 / 1 of a full or partly filled tile, a tile after the first"""
    out = set()
    rem = Rr % SE_BM
    if Rr >= SE_BM:
        out.add("full_tile")
    if 0 < rem <= 64:
        out.add("partial_wm0")
    if 64 < rem < SE_BM:
        out.add("partial_wm1")
    if Rr > SE_BM:
        out.add("second_tile")
    if Rr > 64:
        out.add("wm1")
    return out


# ================================================================================================ noise
@functools.lru_cache(maxsize=8)
def _gumbel_np(seed, Rr, V):
    return R.gumbel_matrix(seed, Rr, V)


def gumbel64(seed, Rr, V):
    """the float64 noise contract as a torch tensor (cached per (seed, R, V): the 49408-column matrices are shared by the cases that use them)"""
    return torch.from_numpy(_gumbel_np(seed, Rr, V)).clone()


def noise_err(g):
    return TR * (1 + g.abs())


NoiseCase = collections.namedtuple("NoiseCase", "id R V seed extreme")
NOISE_CASES = (NoiseCase("noise-5x333-seed77", 5, 333, 77, None), NoiseCase("noise-16x49408-seed12-low", 16, 49408, 12, (8981, "low")),
               NoiseCase("noise-16x49408-seed9-high", 16, 49408, 9, (486993, "high")))


def noise_cases():
    return list(NOISE_CASES)


def noise_inputs(c):
    return dict()


def noise_ref(c, inp, mutant=None):
    if mutant == "fast_inner_log":       # e carries an ABSOLUTE error 2^-22 (a fast log): an order-one error of g where e ~ 6e-8
        e = torch.from_numpy(R.exponential(c.seed, np.arange(c.R * c.V, dtype=np.uint64))).reshape(c.R, c.V)
        return dict(g=-torch.log(e + TR))
    return dict(g=gumbel64(c.seed, c.R, c.V))


def noise_bound(c, inp):
    g = noise_ref(c, inp)["g"]
    b = noise_err(g) if NOISE_FALLBACK is None else torch.full_like(g, NOISE_FALLBACK)
    return dict(g=Bd(b, U * g.abs(), 0.5))


def noise_emulate(c, inp, order):
    """the float64 contract rounded to fp32 ("seq"), or with the inner draw rounded to fp32 first ("pair64")"""
    if order == "seq":
        return dict(g=gumbel64(c.seed, c.R, c.V).to(F32).to(F64))
    e = torch.from_numpy(R.exponential(c.seed, np.arange(c.R * c.V, dtype=np.uint64))).reshape(c.R, c.V).to(F32).to(F64)
    return dict(g=(-torch.log(e)).to(F32).to(F64))


# ================================================================================================ what probabilities, product and backward share
P_MUTANTS = ("noise_row_base_dropped", "noise_missing_in_second_pass", "masked_in_denominator", "inv_temp_twice", "no_inv_temp")


def scores_like(g_, Rr, V):
    """cosine-like scores: N(0, 0.3) clipped to [-1, 1] (the recipe of tests/test_vq_modes_gpu.py)"""
    return (0.3 * torch.randn(Rr, V, generator=g_, dtype=F64)).clamp(-1, 1)


def live_of(V, ids):
    live = torch.ones(V, dtype=torch.bool)
    if len(ids):
        live[list(ids)] = False
    return live


def p_parts(x, g, live, temp, mutant=None):
    """fp64: s = x + g, mx = max_live s, den = sum_live exp((s - mx) / T), p = exp((s - mx) / T) / den on the live columns and 0 elsewhere; a row without a
    live column: mx = -inf, den = 0, p = 0.  With a mutant name the statement of that wrong kernel, or None where it cannot differ.
    -> dict(s, mx, den, p, it)"""
    Rr, V = x.shape
    it = 1 / f32v(temp)
    if mutant in ("inv_temp_twice", "no_inv_temp") and temp == 1.0:
        return None
    if mutant in ("noise_row_base_dropped", "noise_missing_in_second_pass") and g is None:
        return None
    if mutant == "noise_row_base_dropped" and Rr == 1:
        return None
    if mutant == "masked_in_denominator" and bool(live.all()):
        return None
    ite = it * it if mutant == "inv_temp_twice" else 1.0 if mutant == "no_inv_temp" else it
    if g is not None and mutant == "noise_row_base_dropped":
        g = g[:1].expand(Rr, V)
    s = x if g is None else x + g
    if not bool(live.any()):
        z = torch.zeros(Rr, V, dtype=F64)
        return dict(s=s, mx=torch.full((Rr,), float("-inf"), dtype=F64), den=torch.zeros(Rr, dtype=F64), p=z, it=it)
    mx = s.masked_fill(~live, float("-inf")).amax(-1, keepdim=True)
    s_den = x if mutant == "noise_missing_in_second_pass" else s
    e_den = torch.exp((s_den - mx) * ite)
    den = (e_den if mutant == "masked_in_denominator" else e_den * live).sum(-1, keepdim=True)
    p = torch.exp((s - mx) * ite) * live / den
    return dict(s=s, mx=mx.squeeze(-1), den=den.squeeze(-1), p=p, it=it)


def p_errors(q, g, live, V):
    """-> (rel [R, V]: relative error of every fp32 probability, d_s [R, V]: absolute error of the fp32 logit numerator x + g, eta [R, V]: the relative error of
    the single term e_v = exp((s_v - mx) / T) apart from the shift of mx -- exp's own TR + |a| 2^-23 and the argument's 3 U |a| + d_s / T) -- see the header.
    softmax_parts gives exp, the V-term sum, the reciprocal and the product."""
    s, it = q["s"], q["it"]
    zero = torch.zeros_like(s)
    if not bool(live.any()):
        return zero, zero, zero
    d_s = zero if g is None else torch.where(live, noise_err(g) + U * s.abs(), zero)
    am = (s * it).masked_fill(~live, float("-inf"))
    _, rel = softmax_parts(am, V)
    arg = torch.where(live, 3 * U * (am - am.amax(-1, keepdim=True)).abs() + d_s * it, zero)
    rel = torch.where(live, rel + arg + (q["p"] * arg).sum(-1, keepdim=True), zero)
    eta = torch.where(live, TR + (am - am.amax(-1, keepdim=True)).abs() * 2.0 ** -23 + arg, zero)
    return rel, d_s, eta


def p_emulate(x, g, live, temp, order):
    """fp32: -> (s, mx, e, den) with e = exp((s - mx) * inv_temp) on the live columns; the noise is the float64 contract rounded to fp32"""
    x = x.to(F32)
    s = x if g is None else x + g.to(F32)
    it = t32(1.0) / t32(temp)
    if not bool(live.any()):
        return s, torch.full((x.shape[0],), float("-inf"), dtype=F32), torch.zeros_like(s), torch.zeros(x.shape[0], dtype=F32)
    mx = s.masked_fill(~live, float("-inf")).amax(-1, keepdim=True)
    e = torch.where(live, torch.exp((s - mx) * it), torch.zeros((), dtype=F32))
    return s, mx.squeeze(-1), e, fsum(e, order)


# ================================================================================================ sc_vq_probs, and sc_vq_soft_embed's row_max / row_den
ProbCase = collections.namedtuple("ProbCase", "id R V temp nmask noise")
PROB_V, PROB_R, PROB_T, PROB_NMASK = (5, 255, 256, 257, 1031), (1, 7), (1.0, 0.5, 0.1), (0, 3, 8)


def prob_cases():
    return [ProbCase(f"probs-{Rr}x{V}-T{t:g}-mask{nm}-{'noise' if nz else 'plain'}", Rr, V, t, nm, nz)
            for V in PROB_V for Rr in PROB_R for t in PROB_T for nm in PROB_NMASK for nz in (False, True)]


def prob_inputs(c):
    """scores_like; with a mask the FIRST masked id of row 0 holds 9.0 (the row's largest raw score sits in a masked column)"""
    x = scores_like(gen("vqprobs", c.R, c.V), c.R, c.V)
    ids = vq_mask_ids(c)
    if ids:
        x[0, ids[0]] = 9.0
    return dict(x=rnd(x, F32), g=gumbel64(SEED, c.R, c.V) if c.noise else None)


def prob_ref(c, inp, mutant=None):
    q = p_parts(inp["x"], inp["g"], live_of(c.V, vq_mask_ids(c)), c.temp, mutant)
    return None if q is None else dict(p=q["p"], row_max=q["mx"], row_den=q["den"])


def prob_bound(c, inp):
    """p: p rel + FTZ (0 on the masked columns).  row_max: the maximum of fp32 values is exact -- without noise bound 0, with noise the largest d_s of the row.
    row_den = sum_v e_v: every term carries exp's TR + |a| 2^-23, the argument's 3 U |a| + (d_s(v) + d_max) / T, and the V-term sum V U."""
    live = live_of(c.V, vq_mask_ids(c))
    q = p_parts(inp["x"], inp["g"], live, c.temp)
    rel, d_s, eta = p_errors(q, inp["g"], live, c.V)
    p, den = q["p"], q["den"]
    e_p = torch.where(live, p * rel + FTZ, torch.zeros_like(p))
    d_mx = d_s.amax(-1)
    e = p * den.unsqueeze(-1)                                                     # exp((s - mx) / T), 0 on the masked columns
    term = torch.where(live, eta + d_mx.unsqueeze(-1) * q["it"], torch.zeros_like(p))
    e_den = (e * term).sum(-1) + c.V * U * den + U * den + (c.V * FTZ if bool(live.any()) else 0.0)
    st_mx = U * q["mx"].abs() if c.noise and bool(live.any()) else torch.zeros(c.R, dtype=F64)
    return dict(p=Bd(e_p, U * p, 0.5), row_max=Bd(d_mx, st_mx, 0.5 if c.noise else 1.0), row_den=Bd(e_den, U * den, 0.5))


def prob_emulate(c, inp, order):
    s, mx, e, den = p_emulate(inp["x"], inp["g"], live_of(c.V, vq_mask_ids(c)), c.temp, order)
    p = torch.where(den.unsqueeze(-1) > 0, e / den.unsqueeze(-1), torch.zeros((), dtype=F32))
    return dict(p=p.to(F64), row_max=mx.to(F64), row_den=den.to(F64))


# ================================================================================================ sc_vq_soft_embed: keywords
SoftCase = collections.namedtuple("SoftCase", "id R V E temp noise nsplits")
GRID_R, GRID_E = (1, 64, 65, 129, 200, 256), (64, 128, 192, 256, 320, 384, 512, 768)      # 256: R % 128 == 0 (the workload's 2048 rows are 16 full tiles)
GRID_NSPLIT = (1, 2, 5, 0, 64)            # 0 = auto; 64 is above the 11 / 33 steps of V = 333 / 1031: the clamp
SOFT_V, SOFT_T = (333, 1031), (1.0, 0.1)
SOFT_BIG = SoftCase("soft-129x49408x512-T0.1-noise-big", 129, 49408, 512, 0.1, True, (0,))
SOFT_MUTANTS = P_MUTANTS + ("table_lo_dropped", "last_step_short", "rows_64_127_take_rows_0_63", "wave_column_shifted")


def soft_cases():
    out = [SoftCase(f"soft-{Rr}x{V}x{E}-T{t:g}-{'noise' if nz else 'plain'}", Rr, V, E, t, nz, GRID_NSPLIT)
           for V in SOFT_V for E in GRID_E for Rr in GRID_R for t in SOFT_T for nz in (False, True)]
    return out + [SOFT_BIG]


@functools.lru_cache(maxsize=4)
def _emb(V, E):
    """the table: 0.02 (randn + 1.5 sign_e) -- CLIP's token-embedding scale with a per-column offset, so that a softmax-weighted mean of many rows stands clear
    of its bound (|ref| is of the order of the magnitude reference)"""
    g_ = gen("vqemb", V, E)
    sign = torch.where(torch.arange(E) % 2 == 0, 1.0, -1.0).to(F64)
    return rnd(0.02 * (torch.randn(V, E, generator=g_, dtype=F64) + 1.5 * sign), F32)


def planted(x, mask=R.MASK):
    """the rows of tests/test_vq_modes_gpu.py::_planted, as far as the row count goes"""
    Rr, V = x.shape
    if Rr > 0:
        x[0, 1] = 1.5                      # winner at the first unmasked column
    if Rr > 1:
        x[1, V - 1] = 1.5                  # winner at the last column (the short last step)
    if Rr > 2:
        x[2, :] = 0.25                     # all unmasked scores equal
        x[2, list(mask)] = -0.5
    if Rr > 3:
        x[3, 2] = 7.0                      # the largest raw score sits in a masked column
    if Rr > 4:
        x[4, 0] = 7.0
        x[4, 3] = 6.0
    return x


@functools.lru_cache(maxsize=4)
def _soft_scores(Rr, V):
    return rnd(planted(scores_like(gen("vqsoft", Rr, V), Rr, V)), F32)


def soft_inputs(c):
    return dict(x=_soft_scores(c.R, c.V), emb=_emb(c.V, c.E), g=gumbel64(SEED, c.R, c.V) if c.noise else None)


def soft_ref(c, inp, mutant=None):
    """keywords = softmax((x + g) / T over the unmasked sub-words) @ emb"""
    x, emb = inp["x"], inp["emb"]
    live = live_of(c.V, R.MASK)
    q = p_parts(x, inp["g"], live, c.temp, mutant if mutant in P_MUTANTS else None)
    if q is None:
        return None
    p = q["p"]
    if mutant == "table_lo_dropped":                       # hi . hi only
        return dict(kw=p.to(F32).to(BF).to(F64) @ emb.to(F32).to(BF).to(F64))
    if mutant == "last_step_short":
        p = p.clone()
        p[:, (nsteps(c.V) - 1) * SE_BK:] = 0
    if mutant == "rows_64_127_take_rows_0_63":
        if c.R <= 64:
            return None
        rows = torch.arange(c.R)
        p = p[torch.where(rows % SE_BM >= 64, rows - 64, rows)]
    kw = p @ emb
    if mutant == "wave_column_shifted":                    # et0 = (ez * 4 + (wn + 1) % 4) * NE
        w = 16 * soft_ne(c.E)
        col = torch.arange(c.E)
        blk, j = col // w, col % w
        kw = kw[:, ((blk // 4) * 4 + (blk % 4 + 1) % 4) * w + j]
    return dict(kw=kw)


def soft_bound_terms(c, inp):
    """-> (the bound of one chunk [R, E], what every further chunk adds [R, E], U |ref|): see soft_bound"""
    live = live_of(c.V, R.MASK)
    q = p_parts(inp["x"], inp["g"], live, c.temp)
    rel, _, _ = p_errors(q, inp["g"], live, c.V)
    p, ae = q["p"], inp["emb"].abs()
    mag = p @ ae
    st = U * (p @ inp["emb"]).abs()
    per_chunk = U * mag * (1 + 2.0 ** -7)
    return (p * (rel + U) + FTZ * live) @ ae + HILO * mag + 3 * SE_BK * nsteps(c.V) * per_chunk + st, per_chunk, st


def soft_bound(c, inp, ns=None):
    """sum_v |emb| (p rel + FTZ) for the probabilities (and U for the product with 1 / den in place of the quotient), HILO sum p |emb| for the (hi, lo) pairs and
    the dropped lo . lo term, (3 * 32 ceil(V / 32) + ns - 1) U sum p |emb| (1 + 2^-7: the three terms' own magnitude) for the accumulation and the finish
    kernel's adds; ns None: the most chunks any nsplit can give (64, or the steps)."""
    ns = min(64, nsteps(c.V)) if ns is None else ns
    one, per_chunk, st = soft_bound_terms(c, inp)
    return dict(kw=Bd(one + (ns - 1) * per_chunk, st, 0.5))


def hilo(t):
    hi = t.to(BF)
    return hi.to(F32), (t - hi.to(F32)).to(BF).to(F32)


def soft_emulate(c, inp, order):
    """P = e * (1 / den) in fp32, (hi, lo) bf16 pairs of P and of the table, the three products per 32-column step accumulated in fp32 -- the steps in ascending
    ("seq") or descending ("pair64") order"""
    live = live_of(c.V, R.MASK)
    s, mx, e, den = p_emulate(inp["x"], inp["g"], live, c.temp, order)
    P = e * (t32(1.0) / den).unsqueeze(-1)
    ph, pl = hilo(P)
    eh, el = hilo(inp["emb"].to(F32))
    acc = torch.zeros(c.R, c.E, dtype=F32)
    steps = range(nsteps(c.V))
    for k in (steps if order == "seq" else reversed(steps)):
        sl = slice(k * SE_BK, min((k + 1) * SE_BK, c.V))
        acc = acc + ph[:, sl] @ eh[sl]
        acc = acc + pl[:, sl] @ eh[sl]
        acc = acc + ph[:, sl] @ el[sl]
    return dict(kw=acc.to(F64))


# ================================================================================================ sc_vq_mode_bwd with noise
BwdCase = collections.namedtuple("BwdCase", "id R V temp nmask zero")
BWD_SHAPES, BWD_T, BWD_NMASK = ((1, 5), (7, 255), (7, 256), (7, 257), (3, 49408)), (0.1, 1.0), (0, 3, 8)
BWD_MUTANTS = P_MUTANTS + ("rowdot_z_with_cos",)
# At T = 0.1 the noise (spread 1.3 against the cosines' 0.25) makes most rows one-hot: dcos and both rowdots then vanish while the V-term sums' rounding does not.
# A case is well-posed when some of its rows are not (tools/vq_mode_bounds.py (a): rms >= 10x the mean bound); where the first draw of the inputs gives no such
# row the next one is taken -- a choice on the INPUTS, made on the host, before any kernel ran.
BWD_DRAW = {"modebwd-7x256-T0.1-mask0": 1}


def bwd_cases():
    """zero: the outputs that ARE zero up to their bound and are left out of the self-check's rms condition (still judged): a 49408-column row under noise is
    one-hot or close to it, so both rowdots vanish, while the rule for their V-term sums (V U = 2.9e-3 of the magnitude) does not.  What the 49408-column cases
    are for -- the noise index r * V + v far beyond 2^16, 193 strides per thread -- dcos shows element by element."""
    return [BwdCase(f"modebwd-{Rr}x{V}-T{t:g}-mask{nm}", Rr, V, t, nm, ("rowdot_cos", "rowdot_z") if V > 40000 else ())
            for (Rr, V) in BWD_SHAPES for t in BWD_T for nm in BWD_NMASK]


def bwd_inputs(c):
    """the vq_inputs recipe of tail_kernels_ref.py (cosines of unit vectors in 16 dimensions, dprob = randn + 4 cos) and the noise of SEED"""
    g_ = gen("vqmodebwd", c.id, BWD_DRAW.get(c.id, 0))
    nrm = lambda t: t / t.norm(dim=-1, keepdim=True)      # noqa: E731
    cos = rnd(nrm(torch.randn(c.R, 16, generator=g_, dtype=F64)) @ nrm(torch.randn(c.V, 16, generator=g_, dtype=F64)).t(), F32)
    return dict(cos=cos, dprob=rnd(torch.randn(c.R, c.V, generator=g_, dtype=F64) + 4 * cos, F32), g=gumbel64(SEED, c.R, c.V))


def _bwd_parts(c, inp, mutant=None):
    live = live_of(c.V, vq_mask_ids(c))
    q = p_parts(inp["cos"], inp["g"], live, c.temp, mutant if mutant in P_MUTANTS else None)
    if q is None:
        return None
    p, dp = q["p"], inp["dprob"]
    ite = q["it"] ** 2 if mutant == "inv_temp_twice" else 1.0 if mutant == "no_inv_temp" else q["it"]
    dot = (p * dp).sum(-1, keepdim=True)
    d = p * (dp - dot) * ite * live
    return live, q, dot, d


def bwd_ref(c, inp, mutant=None):
    """y = softmax((cos + g) / T) over the live sub-words; dcos = y (dprob - sum y dprob) / T, 0 on the masked ones; rowdot_cos = sum_v dcos cos;
    rowdot_z = sum_v dcos (cos + g)"""
    parts = _bwd_parts(c, inp, mutant)
    if parts is None:
        return None
    live, q, dot, d = parts
    z = inp["cos"] if mutant == "rowdot_z_with_cos" else inp["cos"] + (inp["g"][:1] if mutant == "noise_row_base_dropped" else inp["g"])
    return dict(dcos=d, rowdot_cos=(d * inp["cos"]).sum(-1), rowdot_z=(d * z).sum(-1))


def bwd_bound(c, inp):
    """vq_bound of tail_kernels_ref.py with the noise: the relative error of p takes d_s / T and its row mean (p_errors).  dot = sum(e dprob) / sum(e): relative
    errors eta_v of the terms e_v move the quotient by sum p_v eta_v (dprob_v - dot) / (1 + sum p eta) -- the common part of the errors cancels, and with noise at
    T = 0.1, where eta reaches 7e-5, that matters: sum p eta |dprob - dot| (1.001 for the second order) + V U (sum p |dprob| + |dot|) for the two V-term sums
    + (TR + U) |dot| for the quotient; dcos = p (dprob - dot) / T: p / T (e_dot + U |dprob - dot|) + |dcos| (rel + 3 U) and the flush;
    rowdot_cos: sum |cos| e_dcos + (V + 1) U sum |dcos cos|; rowdot_z: sum |cos + g| e_dcos + sum |dcos| d_s + (V + 1) U sum |dcos (cos + g)| -- each against
    its magnitude."""
    live, q, dot, d = _bwd_parts(c, inp)
    rel, d_s, eta = p_errors(q, inp["g"], live, c.V)
    p, it, dp, cos, s = q["p"], q["it"], inp["dprob"], inp["cos"], q["s"]
    pg = p * dp.abs()
    e_dot = (1.001 * (p * eta * (dp - dot).abs()).sum(-1, keepdim=True) + c.V * U * (pg.sum(-1, keepdim=True) + dot.abs()) + (TR + U) * dot.abs()
             + FTZ * dp.abs().sum(-1, keepdim=True))
    e_d = (p * it * (e_dot + U * (dp - dot).abs()) + d.abs() * (rel + 3 * U) + U * d.abs() + FTZ * (1 + (dp - dot).abs() * it)) * live
    rc, rz = (d * cos).sum(-1), (d * s).sum(-1)
    e_rc = (cos.abs() * e_d).sum(-1) + (c.V + 1) * U * (d * cos).abs().sum(-1) + U * rc.abs()
    e_rz = (s.abs() * e_d).sum(-1) + (d.abs() * d_s).sum(-1) + (c.V + 1) * U * (d * s).abs().sum(-1) + U * rz.abs()
    return dict(dcos=Bd(e_d, U * d.abs(), 0.5), rowdot_cos=Bd(e_rc, U * rc.abs(), 0.5), rowdot_z=Bd(e_rz, U * rz.abs(), 0.5))


def bwd_emulate(c, inp, order):
    live = live_of(c.V, vq_mask_ids(c))
    s, mx, e, den = p_emulate(inp["cos"], inp["g"], live, c.temp, order)
    cos, dp = inp["cos"].to(F32), inp["dprob"].to(F32)
    it = t32(1.0) / t32(c.temp)
    den = den.unsqueeze(-1)
    num = fsum(e * dp, order).unsqueeze(-1)
    d = torch.where(live, e / den * (dp - num / den) * it, torch.zeros((), dtype=F32))
    return dict(dcos=d.to(F64), rowdot_cos=fsum(d * cos, order).to(F64), rowdot_z=fsum(d * s, order).to(F64))


# ================================================================================================ sc_vq_noisy_argmax: planted ties and masks (exact)
ArgCase = collections.namedtuple("ArgCase", "id V ids")
ARG_V = 700
ARG_TIES = dict(later_wave=(70, 300), same_thread=(10, 266), one_wave=(5, 40), three=(70, 300, 600))      # column v sits in thread v % 256, wave (v % 256) // 64


def arg_cases():
    out = [ArgCase(f"argmax-V{ARG_V}-mask{nm}", ARG_V, tuple(vq_mask_ids(ProbCase(None, 0, ARG_V, 0.0, nm, False)))) for nm in (0, 3, 8)]
    return out + [ArgCase("argmax-V5-allmasked", 5, (0, 1, 2, 3, 4)), ArgCase("argmax-V5-mask0", 5, ())]


def arg_inputs(c):
    """rows 0..3: the ties of ARG_TIES at 0.75 over scores below 0.5; row 4: id 0 holds the largest score (masked wherever there is a mask); row 5: the largest at
    V - 1 and the second largest at 1; row 6: no ties.  V = 5: two rows of equal scores."""
    if c.V < 16:
        return dict(x=rnd(torch.full((2, c.V), 0.25, dtype=F64), F32))
    x = scores_like(gen("vqargmax", c.V), 7, c.V).clamp(-1, 0.5)
    for r, cols in enumerate(ARG_TIES.values()):
        x[r, list(cols)] = 0.75
    x[4, 0], x[4, 33] = 9.0, 0.875
    x[5, c.V - 1], x[5, 1] = 0.875, 0.75
    return dict(x=rnd(x, F32))


def arg_ref(c, inp, mutant=None):
    """targets[r] = the LOWEST unmasked index that attains the row's largest unmasked score; 0 for a row without an unmasked column"""
    x = inp["x"]
    live = live_of(c.V, c.ids)
    if not bool(live.any()):
        return None if mutant else dict(targets=torch.zeros(x.shape[0], dtype=F64))
    z = x.masked_fill(~live, float("-inf"))
    hit = z == z.amax(-1, keepdim=True)
    idx = torch.arange(c.V).expand_as(z)
    if mutant == "ties_to_highest_index":
        return dict(targets=torch.where(hit, idx, -1).amax(-1).to(F64))
    return dict(targets=torch.where(hit, idx, c.V).amin(-1).to(F64))


def arg_bound(c, inp):
    z = torch.zeros(inp["x"].shape[0], dtype=F64)
    return dict(targets=Bd(z, z, 1.0))


def arg_emulate(c, inp, order):
    """the kernel's own shape: 256 threads stride the row and keep the first of equals, the threads are then merged low to high ("seq") or high to low ("pair64")
    with the (value, index) rule"""
    x = inp["x"].to(F32)
    live = live_of(c.V, c.ids)
    out = []
    for r in range(x.shape[0]):
        best = []
        for t in range(256):
            b, bi = float("-inf"), 0x7fffffff
            for v in range(t, c.V, 256):
                if live[v] and (float(x[r, v]) > b or (float(x[r, v]) == b and v < bi)):
                    b, bi = float(x[r, v]), v
            best.append((b, bi))
        b, bi = float("-inf"), 0x7fffffff
        for ob, oi in (best if order == "seq" else reversed(best)):
            if ob > b or (ob == b and oi < bi):
                b, bi = ob, oi
        out.append(0 if bi == 0x7fffffff else bi)
    return dict(targets=torch.tensor(out, dtype=F64))


GROUPS = collections.OrderedDict((g.name, g) for g in (
    Group("noise", noise_cases, noise_inputs, noise_ref, noise_bound, noise_emulate, ("fast_inner_log",)),
    Group("probs", prob_cases, prob_inputs, prob_ref, prob_bound, prob_emulate, P_MUTANTS),
    Group("soft", soft_cases, soft_inputs, soft_ref, soft_bound, soft_emulate, SOFT_MUTANTS),
    Group("modebwd", bwd_cases, bwd_inputs, bwd_ref, bwd_bound, bwd_emulate, BWD_MUTANTS),
    Group("argmax", arg_cases, arg_inputs, arg_ref, arg_bound, arg_emulate, ("ties_to_highest_index",)),
))


# ================================================================================================ sc_vq_soft_table, restated (exact)
TABLE_V, TABLE_E = (5, 31, 32, 33, 333), (64, 192)
TABLE_FILL = 0x7fc1            # a bf16 NaN: what the buffer holds before the kernel runs


def table_emb(V, E):
    """randn over six decades (the lo half then spans bf16's exponents too), fp32"""
    g_ = gen("vqtable", V, E)
    return rnd(torch.randn(V, E, generator=g_, dtype=F64) * 10 ** (6 * torch.rand(V, E, generator=g_, dtype=F64) - 3), F32).to(F32)


def table_bits(emb):
    """table[half][vb][et][lane][j] = half(emb[32 vb + 8 (lane >> 4) + j][16 et + (lane & 15)]) as int16 bit patterns, flat; hi = bf16(x) round to nearest even,
    lo = bf16(x - hi); rows beyond V are +0"""
    V, E = emb.shape
    nb, ET = nsteps(V), E // 16
    pad = torch.zeros(nb * SE_BK, E, dtype=F32)
    pad[:V] = emb.to(F32)
    hi = pad.to(BF)
    lo = (pad - hi.to(F32)).to(BF)
    vb, et, lane, j = torch.meshgrid(torch.arange(nb), torch.arange(ET), torch.arange(64), torch.arange(8), indexing="ij")
    row, col = 32 * vb + 8 * (lane >> 4) + j, 16 * et + (lane & 15)
    return torch.cat([hi[row, col].reshape(-1), lo[row, col].reshape(-1)]).view(torch.int16)


def table_elems(V, E):
    return 2 * nsteps(V) * SE_BK * E


# ================================================================================================ one-hot / two-hot products (exact)
HotCase = collections.namedtuple("HotCase", "id kind R E temp shift")
HOT_V = 333
HOT_LOW, HOT_WIN, HOT_MASKED = -1000.0, 0.5, 5.0


def hot_table(V, E):
    """emb[v][e] = +- n 2^k with i = v E + e, n = 2^15 + (i mod 2^15) (16 significant bits), k = -20 - (i >> 15) % 4, the sign from bit 17 of i: every entry
    differs from every other, hi + lo is exact (the remainder of an 8-bit hi has at most 8 bits), and half the sum of two entries -- multiples of 2^-24 below
    2^-4 -- is exact in fp32 whatever the order of the adds"""
    assert V * E <= 2 ** 18
    i = torch.arange(V * E, dtype=torch.int64)
    n = (2 ** 15 + (i & 0x7fff)).to(F64)
    q = i >> 15
    val = n * torch.pow(torch.tensor(2.0, dtype=F64), (-20 - (q & 3)).to(F64)) * torch.where((q & 4) > 0, -1.0, 1.0).to(F64)
    return val.view(V, E)


def hot_winner_list(V=HOT_V, mask=R.MASK):
    """the first unmasked column, V - 1, both sides of every 32-column step boundary (every split boundary of every nsplit is one), then 32 consecutive columns
    (every v mod 32)"""
    w = [min(v for v in range(V) if v not in mask), V - 1]
    for k in range(1, nsteps(V)):
        w += [32 * k - 1, 32 * k]
    w += list(range(100, 132))
    out = []
    for v in w:
        if v not in out and v not in mask:
            out.append(v)
    return out


def hot_pair_list(V=HOT_V):
    """both sides of every step boundary, then pairs far apart"""
    return [(32 * k - 1, 32 * k) for k in range(1, nsteps(V))] + [(1, V - 1), (95, 288), (4, 192)]


def hot_cases():
    out = []
    for kind in ("one", "two"):
        for ei, E in enumerate(GRID_E):
            for ri, Rr in enumerate(GRID_R):
                out.append(HotCase(f"{kind}hot-{Rr}x{HOT_V}x{E}", kind, Rr, E, (1.0, 0.1)[(ei + ri) % 2], 7 * ei + 3 * ri))
    return out


def hot_winners(c):
    """per row: (a,) or (a, b)"""
    lst = [(v,) for v in hot_winner_list()] if c.kind == "one" else hot_pair_list()
    return [lst[(r + c.shift) % len(lst)] for r in range(c.R)]


def hot_inputs(c):
    """scores: HOT_LOW everywhere, HOT_WIN at the winners, HOT_MASKED (the row's largest raw score) in masked column 2"""
    x = torch.full((c.R, HOT_V), HOT_LOW, dtype=F64)
    for r, w in enumerate(hot_winners(c)):
        x[r, list(w)] = HOT_WIN
    x[:, 2] = HOT_MASKED
    return dict(x=x, emb=hot_table(HOT_V, c.E))


def hot_ref(c, inp):
    emb = inp["emb"]
    kw = torch.stack([emb[list(w)].sum(0) / len(w) for w in hot_winners(c)])
    return dict(kw=kw, row_max=torch.full((c.R,), HOT_WIN, dtype=F64), row_den=torch.full((c.R,), 1.0 if c.kind == "one" else 2.0, dtype=F64))


# ================================================================================================ the row with every column masked (exact)
ALLMASKED = ((5, (0, 1, 2, 3, 4)), (8, (0, 1, 2, 3, 4, 5, 6, 7)))          # (V, ids); sc_vq_soft_embed covers V >= 5, and a mask holds at most 8 ids

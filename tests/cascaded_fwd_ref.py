"""Plain fp64 statements, case lists, deterministic inputs, DERIVED per-element bounds, fp32 emulations and mutant statements of the FORWARD kernels of the cascaded branch
(csrc/cascaded.hip: sc_kw_affine, sc_cosine_scores, sc_cosine_refine[_masked], sc_vq_fwd, sc_gather_rows, sc_retrieval_ranks) and of the two analysis kernels
(csrc/analysis.hip: sc_topk_rows_f32, sc_attention_probs_fwd), and of the host chain ops.cosine_scores(exact=False) (sc_l2norm_fwd -> sc_split_hilo_bf16 -> sc_gemm_bf16 ->
sc_cosine_refine_masked), for tests/test_cascaded_fwd_parity_gpu.py and tools/cascaded_fwd_bounds.py.  A helper module, not a test; no kernel runs here.  The constants (U, TR),
the generator, the rounding helper, the guarded window, the judge and the two summation orders are those of tests/row_kernels_ref.py; Bd / Group are laid out as in
tests/tail_kernels_ref.py.  Every input is generated on the CPU from a fixed seed and ROUNDED TO THE KERNEL'S INPUT TYPE before the reference sees it.

The rules of the bounds are row_kernels_ref's: an fp32 sum of n terms n U sum|terms|; every other fp32 operation U; `/`, sqrtf, __expf, exp2f, logf TR each (the budgeted figure of
the suite); exp(a) carries |a| 2^-23 on top (the argument's roundings).  Outputs that are integers or copies are judged with bound 0: equality.

kwaffine   out = fma(x, scale[r % K], shift[r % K]): ONE rounding, U |ref|.
cosine     sc_cosine_scores.  inv = 1 / max(sqrt(q), eps) with q a lane-strided sum of E squares: n_q = ceil(E / 64) + 7 roundings on q, half of them on the square root, TR for
           sqrtf and TR for the division (inv_rel).  The dot is ONE fma chain of E terms in k order (the KC padding adds exact zeros): E U sum|a_k e_k|; two products finish it.
           bound = E U S inv_a inv_e + |ref| (inv_rel_a + inv_rel_e + 2 U), S = sum_k |a_k e_k|.  max(., eps) is 1-Lipschitz, so the clamp needs no term; eps is the fp32 value of
           1e-8 (the kernel's argument is a float).  "int" cases: entries in {0, +-1} with 4^k non-zeros per row -- q = 4^k, sqrt and the reciprocal exact, the dot an integer:
           every operation exact, judged bit for bit.
refine     sc_cosine_refine[_masked] alone, on a hand-made score matrix = fp32(fp64 cosine +- 3e-5): every UNMASKED entry whose input is >= fl32(max over the unmasked inputs -
           delta) ends as the one-row fp32 cosine -- dot and |e|^2 are 256-strided fma chains, a wave tree and three adds: n_d = ceil(E / 256) + 9, n_q = n_d + 1 --, every other
           entry keeps its input bit for bit (bound 0).  rf_wellposed asserts on the CPU that the candidate count of every row is the one the case is named for and that no input
           lies within RF_GAP of the threshold (the fp32 subtraction cannot flip a candidacy), and, in the "lead" cases, that a masked column leads every unmasked one by > 0.03.
chain      ops.cosine_scores(exact=False).  Away from the maximum the value is a_hi.e_hi + a_lo.e_hi + a_hi.e_lo of the normalised operands, hi = bf16(x), lo = bf16(x - hi):
           bf16 keeps 8 significant bits, so |lo| <= 2^-8 |x| and |x - hi - lo| <= 2^-16 |x|: the dropped a_lo.e_lo and the two representation errors are each <= 2^-16 S_n
           (S_n = sum|a_n e_n| <= 1), the MFMA's fp32 accumulation of 3 E terms 3 E U S_n, the two normalisations (sc_l2norm_fwd) inv_rel each:
           b3 = (3 * 2^-16 * (1 + 2^-7) + 3 E U) S_n + |ref| 2 inv_rel (4.6e-5 at S_n = 1; the dense cases stay below a tenth of it, the sparse ones reach a third).
           An entry that is surely a candidate (unmasked, fp64 cosine >= the unmasked fp64 maximum - delta + 2 max b3) carries the refine bound; every other entry b3 (an entry in
           the band of width 4 b3 around the threshold may be either, and the refine bound is the smaller one).  The arg-max over the unmasked ids must equal fp64's on every row:
           ch_wellposed asserts that fp64's winner leads the runner-up by more than twice the refine bound.
           What the refine buys on these inputs is MEASURED by ch_three_term (the split in fp64 with bf16 roundings): see REFINE_MARGIN_NOTE.
vq         sc_vq_fwd.  a = x - max, p = exp(a) / tot: e_a = TR + |a| 2^-23, e_p = e_a + sum_v p_v e_a(v) + n_s U + TR with n_s = ceil(V / 256) + 9 (256-strided chain, wave
           tree, three adds).  t = p log(p + c): dt = p e_p |L| + p (e_p + U) + (TR + U) |t|, L = log(p + c) (the rounding of p + c moves L by U, logf TR |L|).
           row entropy: n_s U sum|t| + sum dt; ent_per_t: (Bn U + TR) mean|rent| + mean d rent.  avg[v]: (rows_per_split + nsplit) U + TR on the sum, mean_r p e_p on the terms;
           prob perplexity exp(-P), P = sum avg log(avg + 1e-7) over 256-blocks (9 roundings) then nparts in order: stats[1] (TR + |P| 2^-23 + dP).  code perplexity
           exp(-(1 / R) sum_r log(cnt_r / R + 1e-7)): per row TR + U + TR |L|, n = ceil(R / 256) + 9, the division TR, the exponential as above.  Targets are exact by the
           statement (fp32 comparisons of the inputs; lowest unmasked index on ties); no decisiveness is needed because nothing is rounded before the comparison.
gather / ranks / topk: copies and integers, bound 0.  ranks = the position of the row's first positive in a STABLE descending sort of the fp64 scores (m without a positive);
           topk = the first K of a stable descending sort of the entries that compare (NaN never does: fewer than K comparable entries leave (-inf, -1); -inf compares and keeps
           its index -- torch.topk would rank NaN first, the reference never feeds one).
probs      sc_attention_probs_fwd.  The log2-domain score is an fma chain over hd of k_d (q_d c), c = scale log2 e: ds = (hd + 2) U sum|k q c|; p = exp2(s - max) / sum:
           e_p(j) = ln 2 (ds_j + ds_max + U |s_j - max|) + TR, the sum n U (n = ceil(L / 64) + 6) and sum_j p_j e_p(j), the reciprocal TR, the product U.
           Row sums: every p_j shares the reciprocal, so |sum - 1| <= n U + TR + 2 U.  Padded keys are exactly 0 (bound 0) and a fully padded batch row is all zeros.

REFINE_MARGIN_NOTE.  The three refine mutants (skipped / maximum over the masked columns too / first 128 candidates by index) are rejected by the `refine` group, whose unrefined
value carries the planted 3e-5.  Whether the REAL unrefined value -- the three-term split -- leaves the fp32 bound is a property of the inputs, and the chain group measures it
(ch_three_term: the split in fp64 with bf16 roundings; CH_MUTANTS).  The derived refine bound at |cos| ~ 1 is 2 inv_rel + n_d U ~ 2.4e-6 (four TR-budgeted operations).  On the
dense planted tables the split's error is a random sum: 0.5 .. 1.8 of that bound -- not a margin to rest on.  The sparse cases follow the recipe of the issue of record (three
non-zeros, integer entries of 9 .. 12 significant bits, the worst of 20000 seeded draws): with e = a the dropped term is sum lo^2 and the split errs by up to 1.7e-5, with the
0.05 masked lead by up to 1.5e-5 -- 6 .. 7 times the refine bound.  tools/cascaded_fwd_bounds.py prints the figure for every chain case and the mutants' margins are asserted
on the sparse ones (the figures are in profiles/cascaded_fwd_parity.txt)."""
import collections
import math

import numpy as np
import torch

import row_kernels_ref as R
from row_kernels_ref import F64, F32, BF, U, TR, PAST_VALUE, SENT32, gen, rnd, fsum, ORDERS, worst, Guarded, judge   # noqa: F401

Bd = collections.namedtuple("Bd", "bound store limit")
Group = collections.namedtuple("Group", "name cases inputs ref bound emulate mutants")
TINY = 2.0 ** -149
SLACK = 1.01
EPS = float(np.float32(1e-8))
DELTA = float(np.float32(1e-3))
C9, C7 = float(np.float32(1e-9)), float(np.float32(1e-7))
INF = float("inf")
LN2 = math.log(2.0)


def _exact(t):
    z = torch.zeros(t.shape, dtype=F64)
    return Bd(z, z, 1.0)


def _f32bd(b):
    return Bd(b, torch.zeros_like(b), 0.5)


def _unit(x):
    return x / (x * x).sum(-1, keepdim=True).sqrt()


def ksum(t, stride, order):
    """fp32 sum over the last dim as the kernels' blocks form it: element i belongs to thread i % stride, which adds its elements in turn ("seq": first to last, otherwise
    last to first); then a binary tree over the threads (the wave butterflies and the adds over the waves: the same depth)"""
    assert t.dtype == F32
    n = t.shape[-1]
    t = torch.nn.functional.pad(t, (0, (-n) % stride)).reshape(*t.shape[:-1], -1, stride)
    acc = torch.zeros(*t.shape[:-2], stride, dtype=F32)
    steps = range(t.shape[-2]) if order == "seq" else range(t.shape[-2] - 1, -1, -1)
    for i in steps:
        acc = acc + t[..., i, :]
    w = stride
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    return acc[..., 0]


def fma_chain(a32, b32, order):
    """sum_k a_k b_k over the last dim as ONE chain of fp32 fmas ("seq": first to last, otherwise last to first): the product is exact in fp64, the sum rounds to fp32"""
    acc = torch.zeros(torch.broadcast_shapes(a32.shape, b32.shape)[:-1], dtype=F32)
    n = a32.shape[-1]
    for k in (range(n) if order == "seq" else range(n - 1, -1, -1)):
        acc = (acc.to(F64) + a32[..., k].to(F64) * b32[..., k].to(F64)).to(F32)
    return acc


def unmasked(V, mask):
    um = torch.ones(V, dtype=torch.bool)
    for i in mask:
        if 0 <= i < V:
            um[i] = False
    return um


# ================================================================================================ sc_kw_affine
KACase = collections.namedtuple("KACase", "id rows K D")
KA_MUTANTS = ("k_is_row_div_K",)


def ka_cases():
    return [KACase("kwaffine/total1", 1, 1, 1), KACase("kwaffine/total255-K8", 15, 8, 17), KACase("kwaffine/total256-K8", 4, 8, 64),
            KACase("kwaffine/total257-K1", 1, 1, 257), KACase("kwaffine/total703-K8", 19, 8, 37)]


def ka_inputs(c):
    g = gen("kwaffine", c.id)
    return dict(x=rnd(torch.randn(c.rows, c.D, generator=g, dtype=F64), F32), scale=rnd(1 + 0.5 * torch.randn(c.K, c.D, generator=g, dtype=F64), F32),
                shift=rnd(torch.randn(c.K, c.D, generator=g, dtype=F64), F32))


def ka_ref(c, inp, mutant=None):
    r = torch.arange(c.rows)
    k = (r // c.K).clamp_max(c.K - 1) if mutant == "k_is_row_div_K" else r % c.K
    return dict(out=inp["x"] * inp["scale"][k] + inp["shift"][k])


def ka_bound(c, inp):
    b = U * ka_ref(c, inp)["out"].abs() + TINY
    return dict(out=Bd(b, b, 1.0))


def ka_emulate(c, inp, order):
    return dict(out=ka_ref(c, inp)["out"].to(F32).to(F64))          # the product of two fp32 values is exact in fp64: one rounding, as the fma


# ================================================================================================ sc_cosine_scores
CSCase = collections.namedtuple("CSCase", "id R V E kind")
CS_SIZES, CS_E = (1, 63, 64, 65, 130), (4, 20, 64, 516)
CS_MUTANTS = ("no_clamp", "rsqrt_q_plus_eps", "tile_tail_R", "tile_tail_V")


def cs_cases():
    real = [(1, 1, 4), (63, 65, 20), (64, 64, 64), (65, 63, 516), (130, 130, 20), (1, 130, 64), (130, 1, 4), (65, 64, 4)]
    ints = [(65, 130, 64), (130, 65, 516), (63, 63, 4), (64, 1, 20), (1, 64, 64)]
    return [CSCase(f"cosine/real-R{r}-V{v}-E{e}", r, v, e, "real") for r, v, e in real] + [CSCase(f"cosine/int-R{r}-V{v}-E{e}", r, v, e, "int") for r, v, e in ints]


def _cs_rows(g, n, E, kind):
    if kind == "int":
        kmax = int(math.log(E, 4) + 1e-9)
        x = torch.zeros(n, E, dtype=F64)
        for i in range(n):
            nz = 4 ** (i % (kmax + 1))
            pos = torch.randperm(E, generator=g)[:nz]
            x[i, pos] = torch.randint(0, 2, (nz,), generator=g).to(F64) * 2 - 1
        if n >= 3:
            x[n // 2] = 0
        return x
    x = torch.randn(n, E, generator=g, dtype=F64)
    sc = 2.0 ** torch.randint(-20, 21, (n, 1), generator=g).to(F64)
    if n >= 5:
        sc[2], sc[3] = 2.0 ** -20, 2.0 ** 20
    x = x * sc
    if n >= 3:
        x[0] = 0                                                                  # the eps clamp at q = 0
        x[1] = 1e-10 * torch.randn(E, generator=g, dtype=F64)                     # 0 < |x| < eps
    return rnd(x, F32)


def cs_inputs(c):
    g = gen("cosine", c.id)
    return dict(a=_cs_rows(g, c.R, c.E, c.kind), e=_cs_rows(g, c.V, c.E, c.kind))


def cos64(a, e, eps=EPS, mutant=None):
    na, ne = (a * a).sum(-1).sqrt(), (e * e).sum(-1).sqrt()
    if mutant == "no_clamp":
        ia, ie = 1 / na, 1 / ne
    elif mutant == "rsqrt_q_plus_eps":
        ia, ie = 1 / (na * na + eps).sqrt(), 1 / (ne * ne + eps).sqrt()
    else:
        ia, ie = 1 / na.clamp_min(eps), 1 / ne.clamp_min(eps)
    return (a @ e.t()) * ia[:, None] * ie[None, :]


def cs_ref(c, inp, mutant=None):
    out = cos64(inp["a"], inp["e"], mutant=mutant if mutant in ("no_clamp", "rsqrt_q_plus_eps") else None)
    if mutant == "tile_tail_R":                                                   # `gi >= R - 1`: the last row keeps what the buffer held
        out[-1, :] = SENT32
    if mutant == "tile_tail_V":
        out[:, -1] = SENT32
    return dict(out=out)


def inv_rel(n_q):
    """relative error of 1 / max(sqrt(q), eps), q an fp32 sum carrying n_q roundings"""
    return 0.5 * n_q * U + 2 * TR + U


def cos_bound(a, e, n_d, n_q):
    ref = cos64(a, e)
    ia, ie = 1 / (a * a).sum(-1).sqrt().clamp_min(EPS), 1 / (e * e).sum(-1).sqrt().clamp_min(EPS)
    S = (a.abs() @ e.abs().t()) * ia[:, None] * ie[None, :]
    return SLACK * (n_d * U * S + ref.abs() * (2 * inv_rel(n_q) + 2 * U)) + TINY


def cs_bound(c, inp):
    if c.kind == "int":
        return dict(out=_exact(torch.empty(c.R, c.V)))
    return dict(out=_f32bd(cos_bound(inp["a"], inp["e"], c.E, -(-c.E // 64) + 7)))


def _inv32(x32, order, stride):
    return 1.0 / torch.maximum(ksum(x32 * x32, stride, order).sqrt(), torch.tensor(EPS, dtype=F32))


def cos32(a, e, order, stride=None):
    """stride None: sc_cosine_scores (64-strided norms, the dot one fma chain); 256: the refine kernel's block sums"""
    a32, e32 = a.to(F32), e.to(F32)
    if not (a32.shape[0] and e32.shape[0]):
        return torch.zeros(a32.shape[0], e32.shape[0], dtype=F64)
    d = fma_chain(a32[:, None, :], e32[None, :, :], order) if stride is None else ksum(a32[:, None, :] * e32[None, :, :], stride, order)
    return (d * _inv32(a32, order, stride or 64)[:, None] * _inv32(e32, order, stride or 64)[None, :]).to(F64)


def cs_emulate(c, inp, order):
    return dict(out=cos32(inp["a"], inp["e"], order))


# ================================================================================================ sc_cosine_refine[_masked]
RFCase = collections.namedtuple("RFCase", "id R V E ncand delta mask lead")            # ncand None: every unmasked column; lead: the masked columns lead the field
RF_PERT, RF_GAP, RF_LEAD = 3e-5, 1e-6, 0.03
RF_MUTANTS = ("refine_skipped", "max_over_masked", "first_128_by_index")
MAXCAND = 128


def rf_cases():
    C, D, M = RFCase, DELTA, (0, 2, 3)
    return [C("refine/V5-E4-c1", 3, 5, 4, 1, D, (), False), C("refine/V5-E64-c2", 3, 5, 64, 2, D, (), False),
            C("refine/V256-E260-c127", 2, 256, 260, 127, D, (), False), C("refine/V257-E512-c128", 2, 257, 512, 128, D, (), False),
            C("refine/V257-E64-c129", 2, 257, 64, 129, D, (), False), C("refine/V1031-E260-c300", 2, 1031, 260, 300, D, (), False),
            C("refine/V256-E64-all", 2, 256, 64, None, D, (), False), C("refine/V1031-E512-all", 1, 1031, 512, None, D, (), False),
            C("refine/V257-E64-delta0", 3, 257, 64, 1, 0.0, (), False), C("refine/V5-E4-R0", 0, 5, 4, 1, D, (), False),
            C("refine/V5-E4-c1-mask0-lead", 3, 5, 4, 1, D, (0,), True), C("refine/V257-E64-c2-mask023-lead", 5, 257, 64, 2, D, M, True),
            C("refine/V1031-E512-c129-mask8-lead", 2, 1031, 512, 129, D, (0, 2, 3, 1030, 5000, 7, 64, 256), True),
            C("refine/V257-E260-all-mask023", 2, 257, 260, None, D, M, False)]


def planted_table(g, R_, V, E, cand, mask, lead, a_noise=0.02, c_noise=0.004, ladder=False):
    """a [R, E] around a unit direction u; e [V, E]: candidates around `centre` = u (lead: u2 with cos(u, u2) = 0.95, and the in-range masked columns ON u), the rest
    orthogonal to u plus at most 0.3 u: cos <= 0.45.  Row scales 2^-3 .. 2^3.  The candidates are centre + c_noise (a random unit vector), or with `ladder` centre + 0.02 j w_j
    for the j-th candidate, w_j a unit vector orthogonal to u and u2: candidate 0 IS the centre and wins every row, candidate j trails it by (0.02 j)^2 / 2 = 2e-4, 8e-4
    whatever the row (a's noise reaches it only through a_noise * 0.02 j)."""
    u = _unit(torch.randn(E, generator=g, dtype=F64))
    w0 = torch.randn(E, generator=g, dtype=F64)
    w0 = _unit(w0 - (w0 @ u) * u)

    def orth(n, both=False):
        w = torch.randn(n, E, generator=g, dtype=F64)
        w = w - (w @ u)[:, None] * u
        return _unit(w - (w @ w0)[:, None] * w0 if both else w)
    a = u + a_noise * _unit(torch.randn(R_, E, generator=g, dtype=F64))
    e = orth(V) + (0.6 * torch.rand(V, 1, generator=g, dtype=F64) - 0.3) * u
    centre = _unit(u + 0.33 * w0) if lead else u
    if ladder:
        e[cand] = centre + 0.02 * torch.arange(len(cand), dtype=F64)[torch.randperm(len(cand), generator=g)][:, None] * orth(len(cand), both=True)
    else:
        e[cand] = centre + c_noise * _unit(torch.randn(len(cand), E, generator=g, dtype=F64))
    if lead:
        for i in mask:
            if 0 <= i < V:
                e[i] = u
    e = e * 2.0 ** torch.randint(-3, 4, (V, 1), generator=g).to(F64)
    return rnd(a, F32), rnd(e, F32)


def rf_inputs(c):
    g = gen("refine", c.id)
    pool = unmasked(c.V, c.mask).nonzero().flatten()
    n = len(pool) if c.ncand is None else c.ncand
    pick = torch.randperm(len(pool), generator=g)[:n]
    if n >= 2:                                                                    # the first and the last unmasked column are candidates
        pick[0], pick[1] = 0, len(pool) - 1
        pick = torch.unique(pick)
        extra = [i for i in range(len(pool)) if i not in set(pick.tolist())][:n - len(pick)]
        pick = torch.cat([pick, torch.tensor(extra, dtype=pick.dtype)])
    cand = pool[pick.sort().values]
    a, e = planted_table(g, c.R, c.V, c.E, cand, c.mask, c.lead)
    sign = torch.randint(0, 2, (c.R, c.V), generator=g).to(F64) * 2 - 1
    return dict(a=a, e=e, scores=rnd(cos64(a, e) + RF_PERT * sign, F32), cand=cand)


def rf_candidates(c, scores, mask_aware=True):
    """-> bool [R, V]: what the kernel's own statement refines, from the fp32 inputs (threshold in fp32 as the kernel forms it)"""
    um = unmasked(c.V, c.mask)
    if scores.shape[0] == 0:
        return torch.zeros(0, c.V, dtype=torch.bool)
    cols = um if mask_aware else torch.ones_like(um)
    mx = scores[:, cols].max(1).values
    thr = (mx.to(F32) - torch.tensor(c.delta, dtype=F32)).to(F64)
    cd = scores >= thr[:, None]
    return cd & um[None, :] if mask_aware else cd


def rf_wellposed(c, inp):
    s, um = inp["scores"], unmasked(c.V, c.mask)
    if c.R == 0:
        return
    cd = rf_candidates(c, s)
    want = int(um.sum()) if c.ncand is None else c.ncand
    assert (cd.sum(1) == want).all() and (cd[:, inp["cand"]]).all(), (c.id, cd.sum(1).tolist(), want)
    thr = s[:, um].max(1).values - c.delta
    gap = (s - thr[:, None]).abs()
    if c.delta == 0:
        gap = gap + cd * 1.0                                                      # the maximum IS the threshold
    assert float(gap[:, um].min()) > RF_GAP, (c.id, float(gap[:, um].min()))
    if c.lead:
        assert float((s[:, ~um].min(1).values - s[:, um].max(1).values).min()) > RF_LEAD, c.id
    if c.ncand is not None and c.ncand > MAXCAND:
        assert bool((cd.cumsum(1)[:, -1] > MAXCAND).all())


def rf_ref(c, inp, mutant=None):
    s = inp["scores"]
    cd = rf_candidates(c, s, mask_aware=mutant != "max_over_masked")
    if mutant == "refine_skipped":
        cd = torch.zeros_like(cd)
    if mutant == "first_128_by_index":
        cd = cd & (cd.cumsum(1) <= MAXCAND)
    return dict(out=torch.where(cd, cos64(inp["a"], inp["e"]), s))


def rf_nd(E):
    return -(-E // 256) + 9


def rf_bound(c, inp):
    cd = rf_candidates(c, inp["scores"])
    b = cos_bound(inp["a"], inp["e"], rf_nd(c.E), rf_nd(c.E) + 1)
    return dict(out=_f32bd(torch.where(cd, b, torch.zeros_like(b))))


def rf_emulate(c, inp, order):
    cd = rf_candidates(c, inp["scores"])
    return dict(out=torch.where(cd, cos32(inp["a"], inp["e"], order, 256), inp["scores"]))


# ================================================================================================ ops.cosine_scores(exact=False) and the auto dispatch
CHCase = collections.namedtuple("CHCase", "id R V E mask lead exact kind")             # exact: what is passed to ops.cosine_scores (None: the dispatch rule decides)
CH_MUTANTS = ("refine_skipped", "max_over_masked")                                     # on the REAL unrefined value, the three-term split (ch_three_term)
AUTO_THRESHOLD = 1 << 22
SPARSE_NZ, SPARSE_PATTERNS, SPARSE_DRAWS = 3, 3, 20000


def exact_rule(R_, V, E):
    """ops.cosine_scores' dispatch, restated: the fp32 SIMT kernel unless the GEMM takes the shape and the problem is large"""
    return not (E % 64 == 0 and V % 4 == 0 and R_ * V >= AUTO_THRESHOLD)


def ch_cases():
    M, C_ = (0, 2, 3), CHCase
    return [C_("chain/R1-V4-E64", 1, 4, 64, (), False, False, "dense"), C_("chain/R5-V8-E64-mask023-lead", 5, 8, 64, M, True, False, "dense"),
            C_("chain/R65-V260-E64-mask023-lead", 65, 260, 64, M, True, False, "dense"), C_("chain/R3-V1028-E128", 3, 1028, 128, (), False, False, "dense"),
            C_("chain/sparse-R9-V260-E64", 9, 260, 64, (), False, False, "sparse"), C_("chain/sparse-R9-V260-E64-mask023-lead", 9, 260, 64, M, True, False, "sparse"),
            C_("chain/auto-R4096-V1028-E64-mask023-lead", 4096, 1028, 64, M, True, None, "dense")]


def _cos_rows(x, y):
    return (x * y).sum(-1) / ((x * x).sum(-1).sqrt() * (y * y).sum(-1).sqrt())


def _three_term_rows(x, y):
    """the three-term split of cos(x_i, y_i), row by row"""
    xn, yn = (x / (x * x).sum(-1, keepdim=True).sqrt()).to(F32).to(F64), (y / (y * y).sum(-1, keepdim=True).sqrt()).to(F32).to(F64)
    (xh, xl), (yh, yl) = _split(xn), _split(yn)
    return (xh * yh + xl * yh + xh * yl).sum(-1)


def sparse_pattern(g, lead):
    """(p, w, w2): keyword pattern, winner and runner-up sub-word patterns on SPARSE_NZ coordinates, integer entries of 9 .. 12 significant bits.  Without a lead w = p
    (cos = 1: the dropped a_lo.e_lo is sum lo^2, ONE sign); with a lead w = round(p + 0.33 |p| o), o a unit vector orthogonal to p (cos = 0.95: p itself, in a masked column,
    leads by 0.05).  Of SPARSE_DRAWS seeded draws the one whose three-term split errs most is kept -- a choice made on the inputs and the fp64 emulation of the split alone.
    w2 = w + a small integer step that lowers the fp64 cosine by 1.5e-5 .. 5e-5: more than twice the refine bound, less than the split's own error budget."""
    p = torch.randint(257, 4096, (SPARSE_DRAWS, SPARSE_NZ), generator=g).to(F64)
    w = p
    if lead:
        o = torch.randn(SPARSE_DRAWS, SPARSE_NZ, generator=g, dtype=F64)
        o = _unit(o - (o * p).sum(-1, keepdim=True) * p / (p * p).sum(-1, keepdim=True))
        w = (p + 0.33 * (p * p).sum(-1, keepdim=True).sqrt() * o).round()
    i = int((_three_term_rows(p, w) - _cos_rows(p, w)).abs().argmax())
    p, w = p[i], w[i]
    step = torch.randint(-40, 41, (4096, SPARSE_NZ), generator=g).to(F64)
    loss = _cos_rows(p[None, :], w[None, :]) - _cos_rows(p[None, :], w[None, :] + step)
    ok = ((loss > 1.5e-5) & (loss < 5e-5)).nonzero().flatten()
    assert len(ok), "no runner-up step in 4096 draws"
    return p, w, w + step[int(ok[0])]


def ch_inputs(c):
    g = gen("chain", c.id)
    pool = unmasked(c.V, c.mask).nonzero().flatten()
    if c.kind == "sparse":
        e = rnd(torch.randn(c.V, c.E, generator=g, dtype=F64), F32)
        a = torch.zeros(c.R, c.E, dtype=F64)
        coords = torch.randperm(c.E, generator=g)[:SPARSE_NZ * SPARSE_PATTERNS].view(SPARSE_PATTERNS, SPARSE_NZ)
        cols = pool[torch.randperm(len(pool), generator=g)[:2 * SPARSE_PATTERNS]].view(SPARSE_PATTERNS, 2)
        msk = [i for i in c.mask if 0 <= i < c.V]
        for i in range(SPARSE_PATTERNS):
            p, w, w2 = sparse_pattern(g, c.lead)
            for col, v in ((cols[i, 0], w), (cols[i, 1], w2)) + (((msk[i], p),) if c.lead else ()):
                e[col] = 0
                e[col, coords[i]] = v * 2.0 ** int(torch.randint(-3, 4, (1,), generator=g))
            for r in range(i, c.R, SPARSE_PATTERNS):
                a[r, coords[i]] = p * 2.0 ** int(torch.randint(-3, 4, (1,), generator=g))
        return dict(a=rnd(a, F32), e=rnd(e, F32), cand=cols.flatten().sort().values)
    ncand = min(3, len(pool))
    cand = pool[torch.randperm(len(pool), generator=g)[:ncand].sort().values]
    a, e = planted_table(g, c.R, c.V, c.E, cand, c.mask, c.lead, a_noise=0.005, ladder=True)
    return dict(a=a, e=e, cand=cand)


def ch_b3(c, inp):
    a, e = inp["a"], inp["e"]
    ia, ie = 1 / (a * a).sum(-1).sqrt().clamp_min(EPS), 1 / (e * e).sum(-1).sqrt().clamp_min(EPS)
    S = (a.abs() @ e.abs().t()) * ia[:, None] * ie[None, :]
    return SLACK * ((3 * 2.0 ** -16 * (1 + 2.0 ** -7) + 3 * c.E * U) * S + cos64(a, e).abs() * 2 * inv_rel(-(-c.E // 64) + 7)) + TINY


def ch_sure(c, inp):
    """-> bool [R, V]: the entries that every run refines"""
    ref, um, b3 = cos64(inp["a"], inp["e"]), unmasked(c.V, c.mask), ch_b3(c, inp)
    mx = ref[:, um].max(1, keepdim=True).values
    return (ref >= mx - DELTA + 2 * b3.max(1, keepdim=True).values) & um[None, :]


def ch_ref(c, inp, mutant=None):
    ref = cos64(inp["a"], inp["e"])
    if mutant is not None:                                                        # what the chain returns when the refine does nothing / looks at the masked columns too
        um, t3 = unmasked(c.V, c.mask), ch_three_term(c, inp)
        if mutant == "max_over_masked":
            if not c.lead:
                return None
            cd = (t3 >= t3.max(1, keepdim=True).values - DELTA)
            assert not bool((cd & um[None, :]).any())                             # the masked lead is 50 deltas: no unmasked entry is refined
            t3 = torch.where(cd, ref, t3)
        ref = t3
    xm = ref.clone()
    xm[:, ~unmasked(c.V, c.mask)] = -INF
    return dict(out=ref, argmax=xm.argmax(1).to(F64))


def ch_bound(c, inp):
    b32 = cos_bound(inp["a"], inp["e"], rf_nd(c.E), rf_nd(c.E) + 1)
    return dict(out=_f32bd(torch.where(ch_sure(c, inp), b32, ch_b3(c, inp))), argmax=_exact(torch.empty(c.R)))


def ch_wellposed(c, inp):
    ref, um = cos64(inp["a"], inp["e"]), unmasked(c.V, c.mask)
    b32 = cos_bound(inp["a"], inp["e"], rf_nd(c.E), rf_nd(c.E) + 1)
    xm = ref.clone()
    xm[:, ~um] = -INF
    top = xm.topk(min(2, int(um.sum())), dim=1).values
    if top.shape[1] == 2:
        assert bool(((top[:, 0] - top[:, 1]) > 2 * b32.max(1).values).all()), (c.id, float((top[:, 0] - top[:, 1]).min()), float(b32.max()))
    assert bool(ch_sure(c, inp)[torch.arange(c.R), xm.argmax(1)].all()), c.id
    if c.lead:
        assert float((ref[:, ~um].max(1).values - xm.max(1).values).min()) > RF_LEAD, c.id
    assert (c.exact is False) or exact_rule(c.R, c.V, c.E) is False, c.id


def _split(x64):
    x32 = x64.to(F32)
    hi = x32.to(BF).to(F32)
    lo = (x32 - hi).to(BF).to(F32)
    return hi.to(F64), lo.to(F64)


def ch_three_term(c, inp):
    """the unrefined value: a_hi.e_hi + a_lo.e_hi + a_hi.e_lo of the fp32-normalised operands, products and sum in fp64"""
    a, e = inp["a"], inp["e"]
    an = (a / (a * a).sum(-1, keepdim=True).sqrt().clamp_min(EPS)).to(F32).to(F64)
    en = (e / (e * e).sum(-1, keepdim=True).sqrt().clamp_min(EPS)).to(F32).to(F64)
    ah, al = _split(an)
    eh, el = _split(en)
    return ah @ eh.t() + al @ eh.t() + ah @ el.t()


def ch_emulate(c, inp, order):
    ref = ch_ref(c, inp)
    sure = ch_sure(c, inp)
    got = torch.where(sure, cos32(inp["a"], inp["e"], order, 256) if c.R * c.V <= 1 << 16 else ref["out"].to(F32).to(F64), ch_three_term(c, inp))
    xm = got.clone()
    xm[:, ~unmasked(c.V, c.mask)] = -INF
    return dict(out=got, argmax=xm.argmax(1).to(F64))


# ================================================================================================ sc_vq_fwd
VQCase = collections.namedtuple("VQCase", "id V R K mask")
VQ_MUTANTS = ("entropy_1e-7", "avg_over_Rm1", "code_ppl_without_mask", "ties_highest")


def vq_nsplit(R_):
    """csrc/cascaded.hip, restated"""
    return 32 if R_ >= 1024 else (8 if R_ >= 64 else 1)


def vq_workspace_floats(R_, V):
    return 3 * R_ + (V + 255) // 256 + V * (1 + vq_nsplit(R_))


def vq_cases():
    M = (0, 2, 3)
    return [VQCase("vq/V1-R1-K1-nomask", 1, 1, 1, ()), VQCase("vq/V7-R63-K1", 7, 63, 1, M), VQCase("vq/V255-R64-K8", 255, 64, 8, M),
            VQCase("vq/V256-R65-K1-maskVm1-idpastV", 256, 65, 1, (0, 255, 300)), VQCase("vq/V257-R64-K8-nomask", 257, 64, 8, ()),
            VQCase("vq/V7-R1024-K8", 7, 1024, 8, M), VQCase("vq/V1031-R8-K8-mask8", 1031, 8, 8, (0, 2, 3, 1030, 5, 700, 256, 63)),
            VQCase("vq/V7-R257-K257", 7, 257, 257, M), VQCase("vq/V49408-R8-K8", 49408, 8, 8, M)]


def vq_inputs(c):
    """rows r % 4: 0 a masked column holds the maximum; 1 an exact tie of two unmasked columns (and a masked one below them in index); 2 one-hot peaked (+30);
    3 plain.  One unmasked column is -inf on every row where V >= 7."""
    g = gen("vq", c.id)
    x = rnd(0.3 * torch.randn(c.R, c.V, generator=g, dtype=F64), F32)
    um = unmasked(c.V, c.mask)
    pool, msk = um.nonzero().flatten(), (~um).nonzero().flatten()
    ninf = int(pool[len(pool) // 2]) if c.V >= 7 else -1
    for r in range(c.R):
        kind = r % 4
        if kind == 0 and len(msk):
            x[r, msk] = 5.0
        elif kind == 1 and len(pool) >= 4:
            j = pool[torch.randperm(len(pool), generator=g)[:2]]
            j = j[j != ninf]
            x[r, j] = 2.5
            if len(msk):
                x[r, msk[0]] = 2.5
        elif kind == 2:
            x[r, pool[int(torch.randint(0, len(pool), (1,), generator=g))]] = 30.0
    if ninf >= 0:
        x[:, ninf] = -INF
        for r in range(2, c.R, 4):                                              # the peak may have landed on it
            if not torch.isfinite(x[r]).all() and float(x[r, um].max()) < 30:
                x[r, pool[0]] = 30.0
    return dict(x=x)


def _first_max(xm, highest=False):
    V = xm.shape[1]
    eq = xm == xm.max(1, keepdim=True).values
    w = torch.arange(1, V + 1) if highest else torch.arange(V, 0, -1)
    return (eq * w).argmax(1)


def _vq_parts(c, x, c_row=C9):
    um = unmasked(c.V, c.mask)
    xm = x.clone()
    xm[:, ~um] = -INF
    a = xm - xm.max(1, keepdim=True).values
    ex = a.exp()
    tot = ex.sum(1, keepdim=True)
    p = ex / tot
    Lr = (p + c_row).log()
    return um, xm, a, p, Lr


def vq_ref(c, inp, mutant=None):
    x = inp["x"]
    if mutant == "avg_over_Rm1" and c.R == 1:
        return None
    um, xm, a, p, Lr = _vq_parts(c, x, C7 if mutant == "entropy_1e-7" else C9)
    targets = _first_max(xm, mutant == "ties_highest")
    rent = -(p * Lr).sum(1)
    ent = rent.view(c.R // c.K, c.K).mean(0)
    avg = p.sum(0) / (c.R - 1 if mutant == "avg_over_Rm1" else c.R)
    P = (avg * (avg + C7).log())[um].sum()
    hsrc = _first_max(x) if mutant == "code_ppl_without_mask" else targets
    hp = torch.bincount(hsrc, minlength=c.V).to(F64) / c.R
    return dict(targets=targets.to(F64), stats=torch.stack([(-(hp * (hp + C7).log()).sum()).exp(), (-P).exp()]), ent=ent)


def vq_bound(c, inp):
    x = inp["x"]
    um, xm, a, p, Lr = _vq_parts(c, x)
    ref = vq_ref(c, inp)
    n_s = -(-c.V // 256) + 9
    live = p > 0
    e_a = torch.where(live, TR + torch.where(live, a, torch.zeros_like(a)).abs() * 2.0 ** -23, torch.zeros_like(a))
    e_p = e_a + (p * e_a).sum(1, keepdim=True) + n_s * U + TR
    t = p * Lr
    dt = p * e_p * Lr.abs() + p * (e_p + U) + (TR + U) * t.abs()
    d_rent = n_s * U * t.abs().sum(1) + dt.sum(1)
    rent = -t.sum(1)
    Bn = c.R // c.K
    b_ent = (Bn * U + TR) * rent.abs().view(Bn, c.K).mean(0) + d_rent.view(Bn, c.K).mean(0)
    nsplit = vq_nsplit(c.R)
    rps = -(-c.R // nsplit)
    avg = p.sum(0) / c.R
    d_avg = ((rps + nsplit) * U + TR) * avg + (p * e_p).sum(0) / c.R
    L2 = (avg + C7).log()
    term = avg * L2
    d_term = d_avg * L2.abs() + d_avg + U * avg + (TR + U) * term.abs()
    nparts = (c.V + 255) // 256
    P = term[um].sum()
    dP = (9 + nparts) * U * term[um].abs().sum() + d_term[um].sum()
    b1 = ref["stats"][1] * (TR + P.abs() * 2.0 ** -23 + dP)
    hp = torch.bincount(ref["targets"].long(), minlength=c.V).to(F64) / c.R
    Lh = (hp + C7).log()[ref["targets"].long()]
    n0 = -(-c.R // 256) + 9
    dA = n0 * U * Lh.abs().sum() + (TR + U + TR * Lh.abs()).sum()
    arg = -Lh.sum() / c.R
    b0 = ref["stats"][0] * (TR + arg.abs() * 2.0 ** -23 + dA / c.R + TR * arg.abs())
    return dict(targets=_exact(ref["targets"]), stats=_f32bd(SLACK * torch.stack([b0, b1]) + TINY), ent=_f32bd(SLACK * b_ent + TINY))


def vq_emulate(c, inp, order):
    x = inp["x"].to(F32)
    um = unmasked(c.V, c.mask)
    xm = x.clone()
    xm[:, ~um] = -INF
    targets = _first_max(xm.to(F64))
    ex = (xm - xm.max(1, keepdim=True).values).exp()
    tot = ksum(ex, 256, order).unsqueeze(1)
    p = ex / tot
    rent = -ksum(p * (p + torch.tensor(C9, dtype=F32)).log(), 256, order)
    Bn = c.R // c.K
    ent = fsum(rent.view(Bn, c.K).t().contiguous(), order) / Bn
    avg = fsum(p.t().contiguous(), order) / c.R
    term = avg * (avg + torch.tensor(C7, dtype=F32)).log()
    term = torch.where(um, term, torch.zeros_like(term))
    P = fsum(torch.stack([ksum(term[i:i + 256], 256, order) for i in range(0, c.V, 256)]), "seq")                 # one partial per 256-block, then in order
    cnt = torch.bincount(targets, minlength=c.V).to(F32)[targets]
    acc = ksum((cnt / c.R + torch.tensor(C7, dtype=F32)).log(), 256, order)
    return dict(targets=targets.to(F64), stats=torch.stack([(-acc / c.R).exp(), (-P).exp()]).to(F64), ent=ent.to(F64))


# ================================================================================================ sc_gather_rows
GTCase = collections.namedtuple("GTCase", "id R S E")
GT_MUTANTS = ("columns_past_256_dropped",)


def gt_cases():
    return [GTCase("gather/E1", 5, 3, 1), GTCase("gather/E255", 7, 4, 255), GTCase("gather/E256", 7, 4, 256), GTCase("gather/E257", 9, 4, 257), GTCase("gather/R0", 0, 3, 4)]


def gt_inputs(c):
    g = gen("gather", c.id)
    idx = torch.randint(0, c.S, (c.R,), generator=g)
    if c.R >= 3:
        idx[0], idx[1], idx[2] = c.S - 1, c.S - 1, 0                             # the last row, twice
    return dict(src=rnd(torch.randn(c.S, c.E, generator=g, dtype=F64), F32), idx=idx)


def gt_ref(c, inp, mutant=None):
    out = inp["src"][inp["idx"]].clone()
    if mutant == "columns_past_256_dropped":
        out[:, 256:] = SENT32
    return dict(out=out)


def gt_bound(c, inp):
    return dict(out=_exact(torch.empty(c.R, c.E)))


def gt_emulate(c, inp, order):
    return gt_ref(c, inp)


# ================================================================================================ sc_retrieval_ranks
RKCase = collections.namedtuple("RKCase", "id n m ld")
RK_MUTANTS = ("rank_counts_ge", "ids_by_low_word", "ties_to_higher_index")


def rk_cases():
    return [RKCase("ranks/n1-m1", 1, 1, 1), RKCase("ranks/n3-m63-ld70", 3, 63, 70), RKCase("ranks/n4-m64", 4, 64, 64), RKCase("ranks/n5-m65-ld72", 5, 65, 72),
            RKCase("ranks/n5-m300-ld301", 5, 300, 301), RKCase("ranks/n4-m300", 4, 300, 300)]


def rk_inputs(c):
    """scores in eighths of [-1, 1] (ties everywhere); candidate ids = low | high << 32 with four low words and three high words, so that ids that differ collide in
    their low words; row 1: an id no candidate carries; every other row: the id of a candidate, carried by several where m allows"""
    g = gen("ranks", c.id)
    score = torch.randint(-8, 9, (c.n, c.m), generator=g).to(F64) / 8
    cand = torch.randint(0, 4, (c.m,), generator=g) + (torch.randint(1, 4, (c.m,), generator=g) << 32)
    own = cand[torch.randint(0, c.m, (c.n,), generator=g)].clone()
    if c.n >= 3:
        own[1] = (own[1] & 0xffffffff) + (7 << 32)                              # the low word of a candidate, a high word of none
    return dict(score=score, cand=cand, own=own)


def rk_ref(c, inp, mutant=None):
    s, cand, own = inp["score"], inp["cand"], inp["own"]
    if mutant == "ids_by_low_word":
        cand, own = cand & 0xffffffff, own & 0xffffffff
    out = torch.full((c.n,), float(c.m), dtype=F64)
    for i in range(c.n):
        pos = (cand == own[i])
        if not bool(pos.any()):
            continue
        if mutant == "ties_to_higher_index":
            order = (c.m - 1 - torch.argsort(-s[i].flip(0), stable=True))
        else:
            order = torch.argsort(-s[i], stable=True)
        first = int(pos[order].nonzero()[0])
        out[i] = first
        if mutant == "rank_counts_ge":
            best = s[i][order[first]]
            out[i] = float((s[i] >= best).sum()) - 1
    return dict(rank=out)


def rk_bound(c, inp):
    return dict(rank=_exact(torch.empty(c.n)))


def rk_emulate(c, inp, order):
    return rk_ref(c, inp)


# ================================================================================================ sc_topk_rows_f32
TKCase = collections.namedtuple("TKCase", "id rows V K ld")
TK_MUTANTS = ("no_index_tie_break",)


def tk_cases():
    return [TKCase("topk/V1-K1-ld4", 2, 1, 1, 4), TKCase("topk/V255-K10", 3, 255, 10, 255), TKCase("topk/V255-K255-ld256", 3, 255, 255, 256),
            TKCase("topk/V256-K256-ld260", 3, 256, 256, 260), TKCase("topk/V257-K1", 3, 257, 1, 257), TKCase("topk/V257-K257-ld264", 3, 257, 257, 264),
            TKCase("topk/V1031-K10-ld1040", 3, 1031, 10, 1040), TKCase("topk/V256-K10", 3, 256, 10, 256)]


def tk_inputs(c):
    """values in quarters of [-2, 2] (duplicates everywhere, the row maximum planted on both sides of the wave and block borders); row 1: -inf from V / 2 on (they compare,
    in index order); row 2: NaN from 5 on where V > 5 (they do not: fewer than K comparable entries for K > 5)"""
    g = gen("topk", c.id)
    x = torch.randint(-8, 9, (c.rows, c.V), generator=g).to(F64) / 4
    for j in (63, 64, 255, 256, 1030):
        if j < c.V:
            x[0, j] = 3.0
    if c.rows > 1 and c.V >= 2:
        x[1, c.V // 2:] = -INF
    if c.rows > 2 and c.V > 5:
        x[2, 5:] = float("nan")
    return dict(x=x)


def tk_ref(c, inp, mutant=None):
    x = inp["x"]
    vals, idx = torch.full((c.rows, c.K), -INF, dtype=F64), torch.full((c.rows, c.K), -1.0, dtype=F64)
    for r in range(c.rows):
        ok = (~torch.isnan(x[r])).nonzero().flatten()
        v = x[r][ok]
        order = (len(v) - 1 - torch.argsort(-v.flip(0), stable=True)) if mutant == "no_index_tie_break" else torch.argsort(-v, stable=True)
        n = min(c.K, len(ok))
        vals[r, :n], idx[r, :n] = v[order[:n]], ok[order[:n]].to(F64)
    return dict(vals=vals, idx=idx)


def tk_bound(c, inp):
    return dict(vals=_exact(torch.empty(c.rows, c.K)), idx=_exact(torch.empty(c.rows, c.K)))


def tk_emulate(c, inp, order):
    return tk_ref(c, inp)


# ================================================================================================ sc_attention_probs_fwd
PBCase = collections.namedtuple("PBCase", "id B H L hd n_rows ld_extra pad peaked")
PB_MUTANTS = ("no_pad_mask", "scale_dropped")


def pb_cases():
    C = PBCase
    return [C("probs/hd8-L1-rows1", 1, 2, 1, 8, 1, 0, "none", False), C("probs/hd96-L63-rows5-ragged", 2, 2, 63, 96, 5, 8, "ragged", False),
            C("probs/hd8-L64-rowsL-fullpad", 2, 3, 64, 8, 64, 0, "full", False), C("probs/hd1024-L65-rows1-ragged", 2, 1, 65, 1024, 1, 16, "ragged", False),
            C("probs/hd96-L130-rows0", 1, 2, 130, 96, 0, 0, "none", False), C("probs/hd96-L130-rows5-peaked", 2, 2, 130, 96, 5, 8, "ragged", True),
            C("probs/hd8-L65-rowsL-none", 1, 2, 65, 8, 65, 8, "none", True)]


def pb_inputs(c):
    """q, k bf16 values [B, L, H, hd]; pad bool [B, L] or None (ragged: batch row b keeps L - 1 - 3 b keys... at least one; full: the last batch row is all padding);
    peaked: the queries are scaled so that single keys take nearly all the mass"""
    g = gen("probs", c.id)
    q = torch.randn(c.B, c.L, c.H, c.hd, generator=g, dtype=F64) * (6.0 if c.peaked else 1.0)
    k = torch.randn(c.B, c.L, c.H, c.hd, generator=g, dtype=F64)
    pad = None
    if c.pad != "none":
        pad = torch.zeros(c.B, c.L, dtype=torch.bool)
        for b in range(c.B):
            keep = max(1, c.L - 1 - 30 * b)
            pad[b, keep:] = True
        if c.pad == "full":
            pad[-1] = True
    return dict(q=rnd(q, BF), k=rnd(k, BF), pad=pad, scale=c.hd ** -0.5)


def _pb_scores(c, inp, scale):
    s = torch.einsum("bihd,bjhd->bhij", inp["q"][:, :c.n_rows], inp["k"]) * scale
    S = torch.einsum("bihd,bjhd->bhij", inp["q"][:, :c.n_rows].abs(), inp["k"].abs()) * abs(scale)
    return s, S


def _pb_softmax(s, pad):
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], -INF)
    mx = s.max(-1, keepdim=True).values
    dead = mx == -INF
    ex = (s - torch.where(dead, torch.zeros_like(mx), mx)).exp()
    p = ex / ex.sum(-1, keepdim=True).clamp_min(1e-300)
    return torch.where(dead, torch.zeros_like(p), p), s - torch.where(dead, torch.zeros_like(mx), mx)


def pb_ref(c, inp, mutant=None):
    s, _ = _pb_scores(c, inp, 1.0 if mutant == "scale_dropped" else inp["scale"])
    p, _ = _pb_softmax(s, None if mutant == "no_pad_mask" else inp["pad"])
    return dict(probs=p, rowsum=p.sum(-1))


def pb_bound(c, inp):
    s, S = _pb_scores(c, inp, inp["scale"])
    p, a = _pb_softmax(s, inp["pad"])
    ds = (c.hd + 2) * U * S / LN2                                                # log2 domain
    if inp["pad"] is not None:
        ds = ds.masked_fill(inp["pad"][:, None, None, :], 0.0)
    live = p > 0
    a2 = torch.where(live, a, torch.zeros_like(a)).abs() / LN2
    e = torch.where(live, LN2 * (ds + ds.max(-1, keepdim=True).values + U * a2) + TR, torch.zeros_like(p))
    n = -(-c.L // 64) + 6
    e_p = e + (p * e).sum(-1, keepdim=True) + n * U + TR + U
    alive = (p.sum(-1) > 0).to(F64)
    return dict(probs=_f32bd(SLACK * p * e_p + TINY * live), rowsum=_f32bd(SLACK * (n * U + TR + 2 * U) * alive + TINY * alive))


def pb_emulate(c, inp, order):
    c2 = torch.tensor(inp["scale"], dtype=F32) * torch.tensor(1.44269504088896341, dtype=F32)
    q = inp["q"][:, :c.n_rows].to(F32) * c2
    k = inp["k"].to(F32)
    qv, kv = q.permute(0, 2, 1, 3)[:, :, :, None, :], k.permute(0, 2, 1, 3)[:, :, None, :, :]      # -> [B, H, n_rows, L, hd]
    s = fma_chain(qv, kv, order) if c.n_rows else torch.zeros(c.B, c.H, 0, c.L, dtype=F32)
    if inp["pad"] is not None:
        s = s.masked_fill(inp["pad"][:, None, None, :], -INF)
    mx = s.max(-1, keepdim=True).values if s.numel() else s[..., :1]
    dead = mx == -INF
    ex = torch.exp2(s - torch.where(dead, torch.zeros_like(mx), mx))
    tot = ksum(ex, 64, order).unsqueeze(-1) if ex.numel() else ex[..., :1]
    p = torch.where(dead, torch.zeros_like(ex), ex * (1.0 / tot.clamp_min(1e-30)))
    return dict(probs=p.to(F64), rowsum=p.to(F64).sum(-1))


GROUPS = collections.OrderedDict((g.name, g) for g in (
    Group("kwaffine", ka_cases, ka_inputs, ka_ref, ka_bound, ka_emulate, KA_MUTANTS),
    Group("cosine", cs_cases, cs_inputs, cs_ref, cs_bound, cs_emulate, CS_MUTANTS),
    Group("refine", rf_cases, rf_inputs, rf_ref, rf_bound, rf_emulate, RF_MUTANTS),
    Group("chain", ch_cases, ch_inputs, ch_ref, ch_bound, ch_emulate, CH_MUTANTS),
    Group("vq", vq_cases, vq_inputs, vq_ref, vq_bound, vq_emulate, VQ_MUTANTS),
    Group("gather", gt_cases, gt_inputs, gt_ref, gt_bound, gt_emulate, GT_MUTANTS),
    Group("ranks", rk_cases, rk_inputs, rk_ref, rk_bound, rk_emulate, RK_MUTANTS),
    Group("topk", tk_cases, tk_inputs, tk_ref, tk_bound, tk_emulate, TK_MUTANTS),
    Group("probs", pb_cases, pb_inputs, pb_ref, pb_bound, pb_emulate, PB_MUTANTS),
))
WELLPOSED = {"refine": rf_wellposed, "chain": ch_wellposed}

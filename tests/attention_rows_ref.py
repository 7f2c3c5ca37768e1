"""Plain fp64 statement, case list, deterministic inputs, DERIVED per-element bound, fp32 emulation and mutant statements of the full-row attention kernel
(csrc/attention_rows.hip: sc_attention_rows_fwd), for tests/test_attention_rows_parity_gpu.py, tests/test_attention_rows_bounds_cpu.py and tools/attention_rows_bounds.py.
A helper module, not a test; no kernel runs here.  The constants (U, TR, BF_STORE), the generator, the rounding helper, the guarded window, the judge and the two summation
ORDERS are those of tests/row_kernels_ref.py; Bd / Group are laid out as in tests/cascaded_fwd_ref.py.  Every input is generated on the CPU from a fixed seed and ROUNDED TO
bf16 before the reference sees it.

Statement.  Per (b, h, i), in fp64 from the bf16 operands:  out[d] = sum_j P_j v[j, d],  P_j = 2^(s_j) / sum_j' 2^(s_j'),  s_j = c q_i . k_j  (log2 units) over the live keys
{j < L : mask[b, j] == 0}; c is the fp32 value the host passes to the kernel, fl32(fl32(scale) * 1.44269504088896341f).  A row without a live key is all zeros.  The reference
works on one batch entry at a time and INDEXES the live keys (it never multiplies a masked key by zero), so it sees neither a neighbour nor a masked key's contents.

The bound, term by term against the kernel (the rules are row_kernels_ref's: an fp32 sum of n terms n U sum|terms|, every other fp32 operation U, v_exp_f32 and the reciprocal TR):
    score     myq_d = fl(q_d c) (one rounding), then ONE fma chain over hd of k_d myq_d:  ds_j = (hd + 2) U sum_d |k_d q_d c|  log2 units.
    weight    the kernel holds, for key j of live chunk t, the float p_j = exp2(s_j - m_t) (m_t: the running maximum after chunk t) and multiplies it, through the accumulator and the
              running sum alike, by corr_t' = exp2(m_(t'-1) - m_t') of every LATER live chunk t'.  Against 2^(s_j - m_last) the product W_j is off by the relative
                  e_j = ln 2 (ds_j + U |s_j - m_last|) + TR (1 + the number of live chunks after t):
              the subtractions round their results (U |s_j - m_t| and U |m_(t'-1) - m_t'|: the distances add up to |s_j - m_last| because s_j <= m_t <= m_last), each exp2 costs
              TR, and a corr whose maximum did not rise is exp2(0) = 1 (counted all the same: at most 3 TR too much).  [The issue of record lists e_j without the corr factors;
              they do NOT cancel between keys of different chunks -- an early key carries more of them than a late one -- so they are added here.]  The maximum itself is only a
              shift: the same float m enters every weight, and any shift cancels in the quotient.
    quotient  numerator and denominator are sums over the SAME floats W_j, so a common factor cancels and what is left is  sum_j P_j e_j (|v_jd| + |ref_d|).
    numerator one fma per live key with a non-zero weight and one product with corr per live chunk:  (n_live + n_chunks) U sum_j P_j |v_jd|.
    denominator  per live chunk a 6-level butterfly (6 U on that chunk's part), the product with corr and the add (2 U on the running total):  (2 n_chunks + 6) U |ref_d|.
    finish    1.0f / run_sum: TR |ref_d|; acc * inv: U |ref_d|.
    range     a weight or a rescaled accumulator below 2^-126 may be flushed to zero, which is an ABSOLUTE error of at most 2^-126 of a quantity that is divided by a row sum
              >= 1 (the maximal key's weight is exactly 1):  (n_live + 2 n_chunks + 4) 2^-125 (1 + |v|_max + |ref_d|).  It carries the `underflow` and `jump` profiles, where whole
              chunks vanish (corr = exp2(-173) = 0), and is ~1e-35 everywhere.
    store     ONE bf16 store, round to nearest even (common.h: f2bf casts to __bf16): BF_STORE |ref_d|.
    bound = SLACK * (the fp32 terms) + store.  Nothing here is taken from what the kernel returns; the store dominates (4e-3 |ref| against ~1e-5 sum P |v|).
census    q = 0: every live score is fma(k, 0, 0) = 0 exactly, every weight exp2(0) = 1, corr = 1, the running sum is the integer n_live = 2^k, the accumulator an integer of
          magnitude <= 8 * 200, 1 / 2^k and the product exact: out = bf16(sum v / n_live), judged bit for bit (bound 0).

Inputs (three families per mask shape):
    sentinel  0.5 x randn q / k, randn v (tests/test_attention_fwd_parity_gpu.py::build_utt); the query's dims 0..7 hold the common component QC, so a key holding x * unit there
              scores x (natural units) against every query.  In every batch entry the LAST LIVE KEY BEFORE EACH MASKED RUN, the last live key and key 64 (when live) share about
              0.4 of the row between them -- level ln(n_live) - 0.3 - ln(their number) on top of the profile's own level -- and carry V = +-3 in a per-head sign pattern; every MASKED
              key scores 1.5 above the highest of them and carries V = -50.  One key too many or too few therefore moves every element of the row by O(1).
    poison    the same operands with NaN in the K and V rows of every masked key (the GPU test adds NaN guard rows around the buffers and NaN in the gap columns of the wide
              layout): the output must be finite and within the SAME bound.
    census    above; the mask is thinned to n_live = 2^k without touching a fully masked chunk.
Score profiles (on the common component, exact for every query: q[:8] = QC): plain; flat (k = 0: every score exactly 0); rise (+6.0 per 64-key chunk: every chunk rescales); fall
(-6.0 per chunk: corr = 1 throughout); jump (+120 natural = 173 log2 units at the last live chunk: corr underflows to 0 and the earlier accumulators must vanish); underflow (every
seventh live key 150 lower: its probability is exactly 0 in fp32 and the kernel skips it).

Mutant statements (CPU variants of the reference, judged on the sentinel family, on the rows they change): the first masked key admitted; the last live key dropped; key 64 dropped;
the mask row of batch entry b + 1 used; the running sum reset at a skipped chunk (changes only rows with a live chunk BEFORE the skipped one: a leading masked chunk has no state to
lose); the accumulator not rescaled when the maximum rises; log2 e left out of the scale; a fully masked row returning the mean of V."""
import collections
import functools
import math

import numpy as np
import torch

import row_kernels_ref as R
from row_kernels_ref import F64, F32, BF, U, TR, BF_STORE, gen, rnd, ORDERS, worst, Guarded, judge   # noqa: F401

Bd = collections.namedtuple("Bd", "bound store limit")
Group = collections.namedtuple("Group", "name cases inputs ref bound emulate mutants")
Case = collections.namedtuple("Case", "id base B H L hd mask profile family layout mbyte scale")
SLACK = 1.01
LN2 = math.log(2.0)
INF = float("inf")
NAN = float("nan")
LOG2E_F32 = np.float32(1.44269504088896341)
QC = 1.5
STEP, JUMP, SINK = 6.0, 120.0, 150.0              # natural units of the scaled score
MASKED_LEAD, MASKED_V, SENT_V = 1.5, -50.0, 3.0
MAX_HD, ROWS_PER_BLOCK, CHUNK = 1024, 4, 64
MUTANTS = ("first_masked_admitted", "last_live_dropped", "key64_dropped", "mask_of_next_b", "sum_reset_at_skipped_chunk", "acc_not_rescaled", "no_log2e", "dead_row_mean_v")
MASKS = ("none", "prefix", "holes", "only0", "onlylast", "only64", "first_chunk", "mid_chunk", "last_chunk", "one_full")
PROFILES = ("plain", "flat", "rise", "fall", "jump", "underflow")
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 200)
HEAD_DIMS = (8, 16, 32, 64, 72, 96, 128, 768, 1024)
WIDE_GAP = 8                                       # gap columns in front of q, k and v and behind v in the wide layout: ld_qkv = 3 H hd + 4 * WIDE_GAP


# ================================================================================================ masks
def mask_for(name, B, L):
    """bool [B, L] (True = padding) or None.  Every batch entry of a mask case has a mask of its own, so a row read from the wrong b shows."""
    if name == "none":
        return None
    pad = torch.zeros(B, L, dtype=torch.bool)
    last0 = CHUNK * ((L - 1) // CHUNK)
    for b in range(B):
        if name == "prefix":
            pad[b, max(1, L - 1 - 17 * b):] = True
        elif name == "holes":
            for j in ((0, 63, 64, 65, L - 1) if b % 2 == 0 else (1, 61, 67, L - 2)):
                if 0 <= j < L:
                    pad[b, j] = True
            if bool(pad[b].all()):
                pad[b, min(1, L - 1)] = False
        elif name == "only0":
            pad[b, 1 + b:] = True
        elif name == "onlylast":
            pad[b, :max(0, L - 1 - b)] = True
        elif name == "only64":
            pad[b] = True
            pad[b, 64] = False
            if b % 2:
                pad[b, 3] = False
        elif name == "first_chunk":
            pad[b, :CHUNK] = True
            if b % 2 and L > 101:
                pad[b, 100] = True
            elif b % 2:
                pad[b, 7] = False                                                # (a chunk with ONE live key next to a fully masked one)
        elif name == "mid_chunk":
            pad[b, CHUNK:2 * CHUNK] = True
            if b % 2:
                pad[b, 5] = True
        elif name == "last_chunk":
            pad[b, last0:] = True
            if b % 2 and last0 >= 2:
                pad[b, last0 - 1] = True                                         # the even entries' last live key
        elif name == "one_full":
            if b == 0:
                pad[b] = True
            elif b == 1:
                pad[b, L - 3:] = True
            else:
                pad[b, 1::5] = True
        else:
            raise KeyError(name)
    return pad


def census_mask(pad, B, L):
    """the mask thinned so that every batch entry keeps a power of two of live keys (every other live key is masked until the count fits); a fully masked chunk stays as it is"""
    pad = torch.zeros(B, L, dtype=torch.bool) if pad is None else pad.clone()
    for b in range(B):
        live = (~pad[b]).nonzero().flatten().tolist()
        if not live:
            continue
        drop = len(live) - (1 << (len(live).bit_length() - 1))
        for j in live[1::2][:drop]:
            pad[b, j] = True
    return pad


def live_chunks(pad_row, L):
    """the 64-key chunks with at least one live key"""
    return [t for t in range(-(-L // CHUNK)) if pad_row is None or not bool(pad_row[t * CHUNK:(t + 1) * CHUNK].all())]


def skipped_after_live(pad, B, L):
    """batch entries in which a fully masked chunk FOLLOWS a live one (the only place where the state of the online softmax crosses a skipped chunk)"""
    out = []
    for b in range(B if pad is not None else 0):
        lc = live_chunks(pad[b], L)
        if lc and any(t not in lc for t in range(lc[0], -(-L // CHUNK))):
            out.append(b)
    return out


# ================================================================================================ cases
def _case(base, B, H, L, hd, mask, profile="plain", family="sentinel", layout="packed", mbyte=1, scale=None):
    return Case(f"rows/{base}-{family}", base, B, H, L, hd, mask, profile, family, layout, mbyte, scale)


@functools.lru_cache(maxsize=None)
def cases():
    shapes = [  # base id, B, H, L, hd, mask, profile, layout, mbyte, scale, census twin
        ("L1-hd8-none", 2, 2, 1, 8, "none", "plain", "packed", 1, None, True),
        ("L2-hd16-onlylast", 2, 3, 2, 16, "onlylast", "plain", "packed", 1, None, False),
        ("L3-hd8-holes", 2, 2, 3, 8, "holes", "plain", "packed", 1, None, False),
        ("L4-hd32-prefix", 2, 2, 4, 32, "prefix", "plain", "packed", 1, None, True),
        ("L5-hd16-prefix", 3, 4, 5, 16, "prefix", "plain", "wide", 2, None, True),
        ("L5-hd1024-none", 2, 1, 5, 1024, "none", "plain", "packed", 1, None, False),
        ("L63-hd64-holes", 2, 2, 63, 64, "holes", "plain", "packed", 1, None, False),
        ("L63-hd8-none", 2, 3, 63, 8, "none", "flat", "packed", 1, None, False),
        ("L64-hd72-prefix", 2, 2, 64, 72, "prefix", "plain", "wide", 255, None, True),
        ("L64-hd768-only0", 2, 1, 64, 768, "only0", "plain", "packed", 1, None, False),
        ("L65-hd96-holes", 2, 2, 65, 96, "holes", "plain", "packed", "mix", None, True),
        ("L65-hd16-only64", 2, 2, 65, 16, "only64", "plain", "packed", 1, None, True),
        ("L65-hd8-first_chunk", 2, 2, 65, 8, "first_chunk", "plain", "packed", 1, None, True),
        ("L65-hd768-holes", 2, 1, 65, 768, "holes", "plain", "wide", 1, None, False),
        ("L65-hd1024-prefix", 2, 1, 65, 1024, "prefix", "plain", "packed", 1, None, True),
        ("L65-hd32-one_full", 3, 2, 65, 32, "one_full", "plain", "packed", 1, None, False),
        ("L65-hd64-last_chunk", 2, 2, 65, 64, "last_chunk", "plain", "packed", 1, None, True),
        ("L127-hd32-prefix", 2, 2, 127, 32, "prefix", "plain", "packed", 1, 0.2, False),
        ("L127-hd128-onlylast", 2, 2, 127, 128, "onlylast", "plain", "packed", 1, None, False),
        ("L128-hd16-holes", 2, 4, 128, 16, "holes", "plain", "packed", 1, None, False),
        ("L128-hd64-first_chunk", 2, 2, 128, 64, "first_chunk", "plain", "packed", 1, None, True),
        ("L129-hd72-mid_chunk", 2, 2, 129, 72, "mid_chunk", "plain", "packed", 1, None, True),
        ("L129-hd128-last_chunk", 2, 2, 129, 128, "last_chunk", "plain", "wide", 1, None, False),
        ("L129-hd8-only0", 2, 2, 129, 8, "only0", "plain", "packed", 1, None, False),
        ("L130-hd96-holes", 2, 2, 130, 96, "holes", "plain", "packed", 1, None, False),
        ("L130-hd32-only64", 2, 2, 130, 32, "only64", "plain", "packed", 1, None, False),
        ("L130-hd64-none", 2, 2, 130, 64, "none", "plain", "packed", 1, None, False),
        ("L130-hd16-one_full", 2, 2, 130, 16, "one_full", "plain", "packed", 1, None, False),
        ("L200-hd64-mid_chunk", 2, 2, 200, 64, "mid_chunk", "plain", "packed", 1, None, True),
        ("L200-hd128-holes", 3, 4, 200, 128, "holes", "plain", "packed", 1, None, False),
        ("L200-hd8-last_chunk", 2, 2, 200, 8, "last_chunk", "plain", "packed", 1, None, False),
        ("L200-hd96-prefix", 2, 2, 200, 96, "prefix", "plain", "packed", 1, None, False),
        # score profiles
        ("L130-hd32-holes-flat", 2, 2, 130, 32, "holes", "flat", "packed", 1, None, False),
        ("L200-hd32-none-rise", 1, 1, 200, 32, "none", "rise", "packed", 1, None, False),
        ("L128-hd72-holes-rise", 2, 2, 128, 72, "holes", "rise", "packed", 1, None, False),
        ("L130-hd16-last_chunk-rise", 2, 2, 130, 16, "last_chunk", "rise", "packed", 1, None, False),
        ("L200-hd16-mid_chunk-fall", 2, 1, 200, 16, "mid_chunk", "fall", "packed", 1, None, False),
        ("L200-hd32-none-fall", 1, 1, 200, 32, "none", "fall", "packed", 1, None, False),
        ("L130-hd64-holes-fall", 2, 1, 130, 64, "holes", "fall", "packed", 1, None, False),
        ("L200-hd64-none-jump", 1, 2, 200, 64, "none", "jump", "packed", 1, None, False),
        ("L130-hd96-prefix-jump", 2, 2, 130, 96, "prefix", "jump", "packed", 1, None, False),
        ("L130-hd32-holes-underflow", 2, 2, 130, 32, "holes", "underflow", "packed", 1, None, False),
        ("L65-hd128-none-underflow", 2, 2, 65, 128, "none", "underflow", "packed", 1, None, False),
    ]
    out = []
    for base, B, H, L, hd, mask, profile, layout, mbyte, scale, census in shapes:
        out.append(_case(base, B, H, L, hd, mask, profile, "sentinel", layout, mbyte, scale))
        if mask != "none":
            out.append(_case(base, B, H, L, hd, mask, profile, "poison", layout, mbyte, scale))
        if census:
            out.append(_case(base, B, H, L, hd, mask, "flat", "census", layout, mbyte, scale))
    assert len({c.id for c in out}) == len(out)
    return out


def case(cid):
    return {c.id: c for c in cases()}[cid]


# ================================================================================================ inputs
def v_sign(h, hd):
    """+-1 pattern of a sentinel key's V row: differs between any two heads h, h ^ 1 (tests/test_attention_fwd_parity_gpu.py)"""
    d = torch.arange(hd)
    return 1.0 - 2.0 * (((d >> (h % 5)) + h) & 1).double()


def scale_of(c):
    return c.hd ** -0.5 if c.scale is None else c.scale


def c_log2(scale):
    """the fp32 constant the host hands the kernel: float(scale) * 1.44269504088896341f"""
    return float(np.float32(scale) * LOG2E_F32)


def profile_offsets(c, pad_row):
    """natural-unit score offset of every key of one batch entry"""
    off = torch.zeros(c.L, dtype=F64)
    t = (torch.arange(c.L) // CHUNK).double()
    if c.profile == "rise":
        off = STEP * t
    elif c.profile == "fall":
        off = -STEP * t
    elif c.profile == "jump":
        lc = live_chunks(pad_row, c.L)
        if lc and lc[-1] >= 1:
            off = JUMP * (t >= lc[-1]).double()
    elif c.profile == "underflow":
        live = torch.arange(c.L) if pad_row is None else (~pad_row).nonzero().flatten()
        off[live[3::7]] = -SINK
    return off


def sentinel_keys(pad_row, L):
    """the last live key before each masked run, the last live key, and key 64 when live"""
    livef = [True] * L if pad_row is None else [not bool(x) for x in pad_row]
    keys = {j for j in range(L - 1) if livef[j] and not livef[j + 1]}
    if any(livef):
        keys.add(max(j for j in range(L) if livef[j]))
    if L > 64 and livef[64]:
        keys.add(64)
    return sorted(keys)


@functools.lru_cache(maxsize=4)
def inputs(c):
    """dict(q, k, v: fp64 [B, L, H, hd] of bf16 values (poison: NaN in the K / V rows of masked keys), pad: bool [B, L] | None, scale: float, c: float)"""
    g = gen("attention_rows", c.base, "census" if c.family == "census" else "real")
    B, L, H, hd = c.B, c.L, c.H, c.hd
    scale = scale_of(c)
    pad = mask_for(c.mask, B, L)
    if c.family == "census":
        pad = census_mask(pad, B, L)
        q = torch.zeros(B, L, H, hd, dtype=F64)
        k = torch.randn(B, L, H, hd, generator=g, dtype=F64)
        v = torch.randint(-8, 9, (B, L, H, hd), generator=g).double()
        return dict(q=q, k=rnd(k, BF), v=v, pad=pad, scale=scale, c=c_log2(scale))
    q = 0.5 * torch.randn(B, L, H, hd, generator=g, dtype=F64)
    k = 0.5 * torch.randn(B, L, H, hd, generator=g, dtype=F64)
    v = torch.randn(B, L, H, hd, generator=g, dtype=F64)
    q[..., :8] = QC + (0.5 * q[..., :8] if c.profile == "plain" else 0.0)
    unit = 1.0 / (scale * 8 * QC)
    for b in range(B):
        prow = None if pad is None else pad[b]
        if c.profile == "flat":
            k[b] = 0.0
            off = torch.zeros(L, dtype=F64)
        else:
            off = profile_offsets(c, prow)
            k[b, :, :, :8] += (off * unit)[:, None, None]
        sk = sentinel_keys(prow, L)
        n_live = L if prow is None else int((~prow).sum())
        level = math.log(max(n_live, 2)) - 0.3 - math.log(max(len(sk), 1))
        top = 0.0
        for j in sk:
            if c.profile != "flat":
                k[b, j, :, :8] = (level + float(off[j])) * unit
            top = max(top, level + float(off[j]))
            for h in range(H):
                v[b, j, h] = SENT_V * v_sign(h, hd)
        if prow is not None:
            if c.profile != "flat":
                k[b, prow, :, :8] = (max(top, level) + MASKED_LEAD) * unit
            v[b, prow] = MASKED_V
    q, k, v = rnd(q, BF), rnd(k, BF), rnd(v, BF)
    if c.family == "poison" and pad is not None:
        k[pad], v[pad] = NAN, NAN
    return dict(q=q, k=k, v=v, pad=pad, scale=scale, c=c_log2(scale))


# ================================================================================================ the statement
def live_keys(c, inp, b, mutant=None):
    pad = inp["pad"]
    if mutant == "mask_of_next_b" and pad is not None:
        b = (b + 1) % c.B
    live = list(range(c.L)) if pad is None else (~pad[b]).nonzero().flatten().tolist()
    if mutant == "first_masked_admitted" and pad is not None and bool(pad[b].any()):
        live = sorted(live + [int(pad[b].nonzero()[0])])
    if mutant == "last_live_dropped" and live:
        live = live[:-1]
    if mutant == "key64_dropped" and 64 in live:
        live.remove(64)
    return torch.tensor(live, dtype=torch.long)


def _scores(inp, b, live, cc):
    """log2-domain scores [H, L, n] of every query of batch entry b against its live keys, and sum_d |k_d q_d c|"""
    q, k = inp["q"][b], inp["k"][b, live]
    return cc * torch.einsum("ihd,jhd->hij", q, k), abs(cc) * torch.einsum("ihd,jhd->hij", q.abs(), k.abs())


def _online64(c, inp, b, live, cc, mutant):
    """the kernel's chunk-by-chunk recurrence in fp64, for the two mutants that live in it (and, unmutated, a restatement of the plain softmax: the tool compares them)"""
    H, L, hd = c.H, c.L, c.hd
    run_max, run_sum, acc = torch.full((H, L), -INF, dtype=F64), torch.zeros(H, L, dtype=F64), torch.zeros(H, L, hd, dtype=F64)
    for j0 in range(0, L, CHUNK):
        idx = live[(live >= j0) & (live < j0 + CHUNK)]
        if idx.numel() == 0:
            if mutant == "sum_reset_at_skipped_chunk":
                run_sum = torch.zeros_like(run_sum)
            continue
        s, _ = _scores(inp, b, idx, cc)
        nmax = torch.maximum(run_max, s.amax(-1))
        corr = torch.exp2(run_max - nmax)
        p = torch.exp2(s - nmax.unsqueeze(-1))
        run_sum = run_sum * corr + p.sum(-1)
        if mutant != "acc_not_rescaled":
            acc = acc * corr.unsqueeze(-1)
        acc = acc + torch.einsum("hij,jhd->hid", p, inp["v"][b, idx])
        run_max = nmax
    out = torch.where(run_sum.unsqueeze(-1) > 0, acc / run_sum.clamp_min(1e-300).unsqueeze(-1), torch.zeros_like(acc))
    return out.permute(1, 0, 2)


def ref(c, inp, mutant=None, online=False):
    """-> dict(out = fp64 [B, L, H, hd])"""
    out = torch.zeros(c.B, c.L, c.H, c.hd, dtype=F64)
    cc = float(np.float32(inp["scale"])) if mutant == "no_log2e" else inp["c"]
    for b in range(c.B):
        live = live_keys(c, inp, b, mutant)
        if live.numel() == 0:
            if mutant == "dead_row_mean_v":
                out[b] = inp["v"][b].mean(0, keepdim=True)
            continue
        if online or mutant in ("sum_reset_at_skipped_chunk", "acc_not_rescaled"):
            out[b] = _online64(c, inp, b, live, cc, mutant)
            continue
        s, _ = _scores(inp, b, live, cc)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        out[b] = torch.einsum("hij,jhd->ihd", p / p.sum(-1, keepdim=True), inp["v"][b, live])
    return dict(out=out)


def bound(c, inp):
    """-> dict(out = Bd(bound, store, limit)), every tensor [B, L, H, hd]; census: zeros (bit for bit)"""
    z = torch.zeros(c.B, c.L, c.H, c.hd, dtype=F64)
    if c.family == "census":
        return dict(out=Bd(z, z.clone(), 1.0))
    pre, r = z.clone(), ref(c, inp)["out"]
    for b in range(c.B):
        live = live_keys(c, inp, b)
        if live.numel() == 0:
            continue                                                             # zeros by definition: exact
        chunk_of = live // CHUNK
        chunks = sorted(set(chunk_of.tolist()))
        later = torch.tensor([sum(1 for t in chunks if t > int(tj)) for tj in chunk_of], dtype=F64)
        n_live, n_chunks = live.numel(), len(chunks)
        s, S = _scores(inp, b, live, inp["c"])
        a = s - s.amax(-1, keepdim=True)
        p = torch.exp2(a)
        P = p / p.sum(-1, keepdim=True)
        e = LN2 * ((c.hd + 2) * U * S + U * a.abs()) + TR * (1 + later)
        v = inp["v"][b, live]
        refb = r[b].permute(1, 0, 2)                                             # [H, L, hd]
        mag = torch.einsum("hij,jhd->hid", P, v.abs())
        quot = torch.einsum("hij,jhd->hid", P * e, v.abs()) + (P * e).sum(-1, keepdim=True) * refb.abs()
        rng = (n_live + 2 * n_chunks + 4) * 2.0 ** -125 * (1 + float(v.abs().max()) + refb.abs())
        t = quot + (n_live + n_chunks) * U * mag + ((2 * n_chunks + 6) * U + TR + U) * refb.abs() + rng
        pre[b] = t.permute(1, 0, 2)
    store = BF_STORE * r.abs()
    return dict(out=Bd(SLACK * pre + store, store, 1.0))


# ================================================================================================ fp32 emulation
def _fma(acc32, a32, b32):
    return (acc32.to(F64) + a32.to(F64) * b32.to(F64)).to(F32)


def _wave_sum(p32, lanes, order):
    """sum of a chunk's weights: lane = key - j0, dead lanes 0; "seq": lane 0 upwards, otherwise the kernel's butterfly (a binary tree over the 64 lanes)"""
    full = torch.zeros(*p32.shape[:-1], CHUNK, dtype=F32)
    full[..., lanes] = p32
    if order == "seq":
        s = torch.zeros(p32.shape[:-1], dtype=F32)
        for i in range(CHUNK):
            s = s + full[..., i]
        return s
    w = CHUNK
    while w > 1:
        w //= 2
        full = full[..., :w] + full[..., w:2 * w]
    return full[..., 0]


def emulate(c, inp, order, store=True):
    """the kernel's arithmetic in torch fp32, chunk by chunk: fl(q c), the score as one fma chain over hd, the online rescale, the all-padding skip, the zero-probability
    skip, the reciprocal, one bf16 store (store=False: the fp32 value in front of it).  "seq": the kernel's own orders; otherwise the fma chain and the keys of a chunk run backwards and the chunk sum is the butterfly."""
    H, L, hd = c.H, c.L, c.hd
    out = torch.zeros(c.B, L, H, hd, dtype=F64)
    c32 = torch.tensor(inp["c"], dtype=F32)
    for b in range(c.B):
        live = live_keys(c, inp, b)
        myq = (inp["q"][b].to(F32) * c32).permute(1, 0, 2)                        # [H, L, hd]
        run_max, run_sum, acc = torch.full((H, L), -INF, dtype=F32), torch.zeros(H, L, dtype=F32), torch.zeros(H, L, hd, dtype=F32)
        for j0 in range(0, L, CHUNK):
            idx = live[(live >= j0) & (live < j0 + CHUNK)]
            if idx.numel() == 0:
                continue                                                         # a chunk of padding only
            k32 = inp["k"][b, idx].to(F32).permute(1, 0, 2)                      # [H, n, hd]
            v32 = inp["v"][b, idx].to(F32).permute(1, 0, 2)
            s = torch.zeros(H, L, idx.numel(), dtype=F32)
            for d in (range(hd) if order == "seq" else range(hd - 1, -1, -1)):
                s = _fma(s, k32[:, None, :, d], myq[:, :, None, d])
            nmax = torch.maximum(run_max, s.amax(-1))
            corr = torch.exp2(run_max - nmax)
            p = torch.exp2(s - nmax.unsqueeze(-1))
            run_sum = run_sum * corr + _wave_sum(p, idx - j0, order)
            run_max = nmax
            acc = acc * corr.unsqueeze(-1)
            for jj in (range(idx.numel()) if order == "seq" else range(idx.numel() - 1, -1, -1)):
                pj = p[:, :, jj].unsqueeze(-1)
                acc = torch.where(pj == 0, acc, _fma(acc, pj, v32[:, None, jj, :]))
        inv = torch.where(run_sum > 0, 1.0 / run_sum.clamp_min(1e-45), torch.zeros_like(run_sum))
        o = acc * inv.unsqueeze(-1)
        out[b] = (o.to(BF) if store else o).to(F64).permute(1, 0, 2)
    return dict(out=out)


def census_expected(c, inp):
    """bf16(sum of the live v / n_live) per batch entry, the same for every query and zero where no key is live"""
    out = torch.zeros(c.B, c.L, c.H, c.hd, dtype=F64)
    for b in range(c.B):
        live = live_keys(c, inp, b)
        if live.numel():
            out[b] = rnd(inp["v"][b, live].sum(0) / live.numel(), BF).unsqueeze(0)
    return out


GROUPS = collections.OrderedDict(rows=Group("rows", cases, inputs, ref, bound, emulate, MUTANTS))


# ================================================================================================ comparisons with the neighbouring kernels and the modules
CrossCase = collections.namedtuple("CrossCase", "id B H L hd mask")
PROBS_CASES = tuple(CrossCase(f"probs-hd{hd}-L{L}", 2, 2, L, hd, "holes") for hd in (8, 96) for L in (65, 130))
HD_CASES = tuple(CrossCase(f"hd-hd{hd}-L{L}", 2, 2, L, hd, "prefix") for hd in (64, 96, 128) for L in (65, 129))


def cross_case(x):
    """the sentinel case a comparison runs on"""
    return _case(x.id, x.B, x.H, x.L, x.hd, x.mask)


def prefix_lengths(pad):
    lens = (~pad).sum(1)
    assert all(bool((~pad[b, :int(lens[b])]).all()) for b in range(pad.shape[0]))
    return [int(n) for n in lens]


# ================================================================================================ the modules built on the kernel (TransformerModels.py)
ModCase = collections.namedtuple("ModCase", "id kind d nhead n_layers norm_first B L ff")
MOD_B, MOD_L, MOD_D, MOD_FF = 3, 70, 128, 256
MOD_CASES = tuple(ModCase(f"encoder-n{n}-{'pre' if nf else 'post'}", "encoder", MOD_D, 4, n, nf, MOD_B, MOD_L, MOD_FF) for n in (1, 2) for nf in (False, True)) + \
    tuple(ModCase(f"mha-h{h}", "mha", MOD_D, h, 1, False, MOD_B, MOD_L, 0) for h in (1, 4))
LAYER_PARAMS = (("self_attn.in_proj_weight", 3, 1), ("self_attn.in_proj_bias", 3, 0), ("self_attn.out_proj.weight", 1, 1), ("self_attn.out_proj.bias", 1, 0),
                ("linear1.weight", "ff", 1), ("linear1.bias", "ff", 0), ("linear2.weight", 1, "ff"), ("linear2.bias", 1, 0))


def mod_mask(B, L):
    """a key-padding mask WITHOUT prefix structure: holes in the middle, another pattern in every batch entry, key 0 (the CLS position) always live"""
    pad = torch.zeros(B, L, dtype=torch.bool)
    pad[0, 20:30] = True
    pad[0, 64] = True
    if B > 1:
        pad[1, 5] = True
        pad[1, 33:41] = True
        pad[1, 65:] = True
    if B > 2:
        pad[2, 41::2] = True
    assert not bool(pad[:, 0].any())
    return pad


def mod_inputs(m):
    """dict(src fp64 [B, L, d] of fp32 values, pad bool [B, L], params: name -> fp64 tensor of fp32 values, named as the torch modules name them)"""
    g = gen("attention_rows_module", m.id)
    d = m.d
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)   # noqa: E731
    params = {}

    def weights(prefix, rows, cols):
        rows, cols = (m.ff if r == "ff" else r * d if r else 0 for r in (rows, cols))
        params[prefix] = rnd(rn(rows, cols) / cols ** 0.5 if cols else 0.1 * rn(rows), F32)

    def norm(prefix):
        params[prefix + ".weight"], params[prefix + ".bias"] = rnd(1 + 0.1 * rn(d), F32), rnd(0.1 * rn(d), F32)
    if m.kind == "encoder":
        for i in range(m.n_layers):
            for name, r, c in LAYER_PARAMS:
                weights(f"model.layers.{i}.{name}", r, c)
            norm(f"model.layers.{i}.norm1")
            norm(f"model.layers.{i}.norm2")
        norm("model.norm")
    else:
        for name, r, c in LAYER_PARAMS[:4]:
            weights("multihead_attn_layer." + name[len("self_attn."):], r, c)
        norm("attentionBlock_Norm")
    return dict(src=rnd(rn(m.B, m.L, d), F32), pad=mod_mask(m.B, m.L), params=params)


def _ln64(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    return (x - mu) / ((x - mu) ** 2).mean(-1, keepdim=True).add(eps).sqrt() * g + b


def mod_ref(m, inp, model=False):
    """The fp64 restatement of TransformerEncoder.extract_hidden_states_and_output / MultiheadAttentionAndNorm.forward on rows [B L, d]: bf16 weights, fp32 biases and norms,
    a bf16 rounding wherever the Python chain hands bf16 to the next kernel (x.to(bf16), a LayerNorm with a bf16 output); the attention is THIS module's statement.
    model=True: the MODEL of a correct chain -- the attention output and the 16-bit GEMM outputs (q|k|v, the GELU layer) rounded to bf16 as well, as those kernels document.
    -> dict(out [B, L, d], hidden: list over layers of the layer's output [B, L, d])"""
    B, L, d, H = m.B, m.L, m.d, m.nhead
    P = inp["params"]
    rb = lambda t: rnd(t, BF)                                 # noqa: E731
    ro = rb if model else (lambda t: t)
    lin = lambda x, name: x @ rb(P[name + "weight"]).t() + P[name + "bias"]   # noqa: E731

    def attend(qkv):
        q, k, v = (qkv[:, j * d:(j + 1) * d].reshape(B, L, H, d // H) for j in range(3))
        c = _case("module", B, H, L, d // H, "none")
        return ref(c, dict(q=q, k=k, v=v, pad=inp["pad"], scale=scale_of(c), c=c_log2(scale_of(c))))["out"].reshape(B * L, d)
    x = inp["src"].reshape(B * L, d)
    if m.kind == "mha":
        qkv = ro(lin(rb(x), "multihead_attn_layer.in_proj_"))
        y = lin(ro(attend(qkv)), "multihead_attn_layer.out_proj.") + x
        return dict(out=_ln64(y, P["attentionBlock_Norm.weight"], P["attentionBlock_Norm.bias"]).view(B, L, d), hidden=[])
    hidden = []
    for i in range(m.n_layers):
        p = f"model.layers.{i}."
        n1, n2 = (P[p + "norm1.weight"], P[p + "norm1.bias"]), (P[p + "norm2.weight"], P[p + "norm2.bias"])
        if m.norm_first:
            qkv = ro(lin(rb(_ln64(x, *n1)), p + "self_attn.in_proj_"))
            x1 = lin(ro(attend(qkv)), p + "self_attn.out_proj.") + x
            h = ro(R.gelu64(lin(rb(_ln64(x1, *n2)), p + "linear1.")))
            x = lin(h, p + "linear2.") + x1
        else:
            qkv = ro(lin(rb(x), p + "self_attn.in_proj_"))
            x1 = _ln64(lin(ro(attend(qkv)), p + "self_attn.out_proj.") + x, *n1)
            h = ro(R.gelu64(lin(rb(x1), p + "linear1.")))
            x = _ln64(lin(h, p + "linear2.") + x1, *n2)
        hidden.append(x.view(B, L, d))
    return dict(out=_ln64(x, P["model.norm.weight"], P["model.norm.bias"]).view(B, L, d), hidden=hidden)


def row_metric(got, want):
    """per row: max|got - want| / max|want| over the last dim (tests/test_attention_fwd_parity_gpu.py)"""
    err, scale = (got - want).abs().amax(-1), want.abs().amax(-1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, INF), torch.zeros_like(err)))


def mod_model(m):
    """-> (MODEL: the worst row metric of the modelled chain over the output and every hidden state, the smallest max|ref| of any of their rows)"""
    inp = mod_inputs(m)
    r, mo = mod_ref(m, inp), mod_ref(m, inp, model=True)
    pairs = [(mo["out"], r["out"])] + list(zip(mo["hidden"], r["hidden"]))
    return max(float(row_metric(a, b).max()) for a, b in pairs), min(float(b.abs().amax(-1).min()) for _, b in pairs)

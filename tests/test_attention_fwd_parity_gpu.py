"""Kernel-level parity of the flash attention FORWARDS: `sc_attention_fwd` (plain and causal, bf16 and IEEE half), `sc_attention_fwd_dropout` (plain and causal),
`sc_attention_fwd_packed` (with and without dropout) and `sc_attention_hd_fwd` (head_dim 64 / 96 / 128, and the Tq = 1 strided-query fp32-output form).

Every reference is fp64 torch on the CPU, computed per (utterance, head) from the same bf16 / half operands, one utterance at a time: it never sees a neighbour.

Metric and bound (the convention of tests/test_packed_frontend_gpu.py).  Per query row and head: max|got - ref| / max|ref| over the head's output columns.  Bound:
4 x MODEL + 1e-3, MODEL being the same metric for a CPU model of a correct kernel on exactly the inputs of that case (`tools/attention_bounds.py` prints every
value; the constants are the MODEL dict below).  The model applies the kernels' documented roundings and nothing else: operands as given, scores / maxima / row sums
in high precision, probabilities rounded to the operand format AFTER the dropout mask and its 1 / (1 - p) rescale and BEFORE P.V, the row sum taken over the
unrounded, undropped probabilities, one rounding of the output to the output format (none for SC_ATTN_HD_OUT_F32).  The lazy rescale of the online softmax
(SC_ATTN_LAZY_LOG2 = 8: the reference maximum lags the running maximum by up to 8 log2 units) is NOT modelled and need not be: bf16 / half rounding is relative and
P <= 2^8 stays in the range of both formats, so rounding exp2(s - m_lagging) has the same relative error as rounding exp2(s - m_true); the row sum uses the same
reference maximum, so the quotient is unchanged (tools/attention_bounds.py checks that the tile-by-tile lazy recurrence restates the plain softmax to 1e-12).
The factor 4 covers what the model leaves out (fp32 MFMA summation order, v_exp_f32), the 1e-3 floor rows whose reference is tiny -- the tool checks that no row
here has max|ref| < 1e-2, so the floor never carries a row.  Every test also meets the absolute tolerance of its older twin in tests/test_kernels_gpu.py /
test_attention_hd_gpu.py / test_f16_operands_gpu.py (2e-2 bf16, 2e-3 half).  Modelled values and the mutant table: EXPERIMENTS.md ("Attention forwards: per-row parity").

Inputs: 0.5 x randn q / k (0.25 x on the 8 dims that carry the common query component), randn v, PLUS sentinels (build_utt), so that a mask that is off by one moves every row by O(1) of its maximum:
  * length sentinels: the last valid key klens[b] - 1 scores ln(klens[b]) - 0.3 above the crowd for every query (about a third of the row's probability) and
    carries V = +-3 in a per-head sign pattern; the first invalid key klens[b] scores 1.5 higher still and carries V = -50;
  * diagonal sentinels (causal cases): query i carries the combination of its own key and key i + 1 that scores ln(i + 2) + 1 on key i (around half of the row)
    and 1.25 x that on key i + 1;
  * staircase heads (h % 4 == 2): the score level rises per 64-key tile by 5.1 (even utterances: under 8 log2 units = 5.545, the lazy rescale alternates) or 6.0
    (odd utterances: every tile rescales); jump heads (h % 4 == 3): one rise of 12 at the last valid tile.  The dropout cases have plain heads only.
No row is excluded anywhere in this file: every test asserts it compared B x T x H rows (padded queries attend to the valid keys too)."""
import ctypes
import dataclasses
import functools
import math

import pytest
import torch

from test_dropout_gpu import _keep_attn, _keep_attn_packed

BF = torch.bfloat16
HALF = torch.float16
F64 = torch.float64
DT = {"bf16": BF, "f16": HALF}
TWIN_TOL = {"bf16": 2e-2, "f16": 2e-3}
QC = 1.5                       # common component of every query on dims 0..7 (what the length sentinels and the staircase act on)
STEP_UNDER, STEP_OVER, JUMP = 5.1, 6.0, 12.0        # natural units of the scaled score; 8 log2 units = 5.545


def bound_of(model_err):
    return 4.0 * model_err + 1e-3


def rfmt(t, dt):
    """store of an fp64 value in format `dt` (None: fp32), back in fp64"""
    t = t.to(torch.float32)
    return (t if dt is None else t.to(dt)).to(F64)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def row_metric(got, ref):
    """per row (all leading dims): max|got - ref| / max|ref| over the last dim; a row whose reference is all zero must be zero exactly (metric 0) or counts as inf."""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


# ================================================================================================ cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    group: str                  # fwd | causal | drop | packed | hd | hdq1
    dtype: str                  # bf16 | f16
    rows: tuple                 # query / key rows per utterance (uniform layouts: all equal)
    klens: tuple
    H: int = 4
    hd: int = 64
    scale: float = 0.125
    causal: bool = False
    p: float = 0.0
    seed: int = 0               # dropout seed
    wide: bool = False          # separate q / k / v pointers into a wider buffer, ld_out > D

    @property
    def T(self):
        return max(self.rows)

    @property
    def B(self):
        return len(self.rows)


def klens_for(T, i=0):
    """T, 1, a value at a 64-key tile edge (64 k - 1 / 64 k / 64 k + 1, rotating with i) and a mid-tile value -- those that exist below T."""
    out = [T, 1]
    k = (T - 1) // 64
    edges = [e for e in (64 * k - 1, 64 * k, 64 * k + 1) if 1 < e < T]
    if edges:
        out.append(edges[i % len(edges)])
    mid = (T // 2) // 64 * 64 + 29
    if 1 < mid < T:
        out.append(mid)
    elif T > 3:
        out.append(T // 2 + 1)
    return tuple(out)


FWD_T = (1, 63, 64, 65, 128, 129, 256, 257, 319, 384, 385, 499, 500, 529)
CAUSAL_T = (1, 2, 16, 63, 64, 65, 77, 127, 128, 129, 255, 256, 257, 300, 512, 529)
DROP_T = (64, 65, 131, 257, 300, 499)
PACKED_ROWS = (500, 100, 129, 256, 257, 300, 384, 385, 1, 128)          # test_attention_query_row_split_packed_ragged: both sides of every block edge, plus 1
PACKED_KLENS = (500, 97, 129, 193, 257, 1, 320, 383, 1, 64)
HD_GRID = ((1, (1, 1)), (63, (63, 1, 62)), (64, (64, 63, 1)), (65, (65, 64, 2)), (129, (129, 65, 128)), (200, (200, 13, 127)), (500, (500, 437, 64, 65)))


@functools.lru_cache(maxsize=None)
def all_cases():
    cs = []
    for i, T in enumerate(FWD_T):
        kl = klens_for(T, i)
        for dt in ("bf16", "f16"):
            # H = 3: B * H not a multiple of 8 (the XCD unit mapping); T = 128: 12 heads once; T = 319: a non-default scale; T = 385: wide rows
            H = 12 if T == 128 else (3 if i % 3 == 1 else 4)
            cs.append(Case(f"fwd-{dt}-T{T}", "fwd", dt, (T,) * len(kl), kl, H=H, scale=0.2 if T == 319 else 0.125, wide=(T == 385)))
    for i, T in enumerate(CAUSAL_T):
        kl = klens_for(T, i)
        for dt in ("bf16", "f16"):
            H = 3 if i % 3 == 1 else 4
            cs.append(Case(f"causal-{dt}-T{T}", "causal", dt, (T,) * len(kl), (T,) * len(kl), H=H, causal=True))
            cs.append(Case(f"causal-klens-{dt}-T{T}", "causal", dt, (T,) * len(kl), kl, H=H, causal=True))
    for i, T in enumerate(DROP_T):
        kl = klens_for(T, i)
        for p in (0.1, 0.25):
            for causal in (False, True):
                cs.append(Case(f"drop-{'causal-' if causal else ''}p{p}-T{T}", "drop", "bf16", (T,) * len(kl), kl, causal=causal, p=p, seed=4242 + T))
    for dt in ("bf16", "f16"):
        cs.append(Case(f"packed-{dt}", "packed", dt, PACKED_ROWS, PACKED_KLENS))
    cs.append(Case("packed-drop-p0.1", "packed", "bf16", PACKED_ROWS, PACKED_KLENS, p=0.1, seed=1234))
    for hd in (64, 96, 128):
        for L, lens in HD_GRID:
            cs.append(Case(f"hd{hd}-L{L}", "hd", "bf16", (L,) * len(lens), lens, hd=hd, scale=hd ** -0.5))
    cs.append(Case("hdq1-hd96", "hdq1", "bf16", (301,) * 5, (301, 1, 64, 65, 200), H=8, hd=96, scale=96 ** -0.5))
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


def case(cid):
    return next(c for c in all_cases() if c.id == cid)


def ids_of(group, pred=lambda c: True):
    return [c.id for c in all_cases() if c.group == group and pred(c)]


# ================================================================================================ inputs and CPU references (no GPU below this line until the tests)
def v_sign(h, hd):
    """+-1 pattern of the last-valid key's V row: differs between any two heads h, h ^ 1."""
    d = torch.arange(hd)
    return 1.0 - 2.0 * (((d >> (h % 5)) + h) & 1).double()


def build_utt(c, b, gen):
    """One utterance's q, k, v [T_b, H, hd] in the case's operand format: randn plus the sentinels of the file header."""
    T, kl, H, hd = c.rows[b], min(max(c.klens[b], 0), c.rows[b]), c.H, c.hd
    unit = 1.0 / (c.scale * 8 * QC)                   # a key holding x * unit on dims 0..7 scores x against the common query component
    q = 0.5 * torch.randn(T, H, hd, generator=gen, dtype=F64)
    k = 0.5 * torch.randn(T, H, hd, generator=gen, dtype=F64)
    v = torch.randn(T, H, hd, generator=gen, dtype=F64)
    q[:, :, :8] = QC + 0.5 * q[:, :, :8]
    # length sentinels
    a = math.log(max(kl, 2)) - 0.3
    if kl >= 1:
        k[kl - 1, :, :8] = a * unit
        for h in range(H):
            v[kl - 1, h] = 3.0 * v_sign(h, hd)
    if kl < T:
        k[kl, :, :8] = (a + 1.5) * unit
        v[kl] = -50.0
    # staircase / jump heads (exact common component, so the step is the same for every query)
    tile = torch.arange(T) // 64
    last_tile = (max(kl, 1) - 1) // 64
    for h in range(H if c.p == 0.0 else 0):           # not under dropout: a row whose few dominant keys are all dropped would be left with a reference of ~1e-6
        if h % 4 == 2:
            q[:, h, :8] = QC
            k[:, h, :8] += (tile.double() * (STEP_UNDER if b % 2 == 0 else STEP_OVER) * unit)[:, None]
        elif h % 4 == 3 and last_tile >= 1:
            q[:, h, :8] = QC
            k[:, h, :8] += ((tile >= last_tile).double() * JUMP * unit)[:, None]
    # diagonal sentinels on dims 8..: query i gets the combination of its own key and key i + 1 that scores ln(i + 2) + 1 on the first and 1.25 x that on the second
    # (a 2 x 2 solve per row, so the two do not disturb each other; what the length sentinels add on dims 0..7 is taken off the target)
    if c.causal:
        kk = k[:, :, 8:]
        extra = torch.zeros(T + 1, dtype=F64)
        if kl >= 1:
            extra[kl - 1] = a
        extra[kl] = a + 1.5
        s_i = torch.log(torch.arange(T, dtype=F64) + 2.0) + 1.0
        n2 = (kk * kk).sum(-1)                                     # [T, H]
        cr = torch.cat([(kk[:-1] * kk[1:]).sum(-1), torch.zeros(1, H, dtype=F64)])
        nn = torch.cat([n2[1:], torch.ones(1, H, dtype=F64)])
        t0 = ((s_i - extra[:T]) / c.scale)[:, None].expand(T, H)
        t1 = ((1.25 * s_i - extra[1:]) / c.scale)[:, None].expand(T, H).clone()
        t1[-1] = 0.0
        det = n2 * nn - cr * cr
        al, be = (t0 * nn - t1 * cr) / det, (t1 * n2 - t0 * cr) / det
        q[:, :, 8:] += al[:, :, None] * kk
        q[:-1, :, 8:] += be[:-1, :, None] * kk[1:]
    dt = DT[c.dtype]
    return q.to(torch.float32).to(dt), k.to(torch.float32).to(dt), v.to(torch.float32).to(dt)


@functools.lru_cache(maxsize=8)
def case_inputs(cid):
    """-> list over utterances of (q, k, v) [T_b, H, hd]"""
    c = case(cid)
    gen = _g(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % (2 ** 31))
    return [build_utt(c, b, gen) for b in range(c.B)]


def keep_masks(c):
    """list over utterances of the dropout keep mask [H, T_b, T_b] (1 = kept), or None"""
    if c.p == 0.0:
        return [None] * c.B
    if c.group == "packed":
        off = offsets(c.rows)
        return [_keep_attn_packed(c.seed, off[b], c.H, c.rows[b], c.T, c.p) for b in range(c.B)]
    m = _keep_attn(c.seed, c.B, c.H, c.T, c.p)
    return [m[b] for b in range(c.B)]


def offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


def attn_ref(q, k, v, kl, scale, causal=False, keep=None, p=0.0, p_fmt=None, out_fmt="none", diag=0, key_limit=None, drop_rescale=True, sum_dropped=False):
    """One utterance: q [Tq, H, hd], k / v [Tk, H, hd] -> fp64 [Tq, H, hd] = softmax(scale q k^T over keys < kl [and <= query + diag]) v.
    keep [H, Tq, Tk]: dropout mask on the probabilities (rescaled by 1 / (1 - p)); the row sum keeps every probability.
    p_fmt / out_fmt: the MODEL's roundings (probabilities after dropout; the output; "none" = the reference, None = fp32).
    diag / key_limit [Tq] / drop_rescale / sum_dropped: MUTANTS only (tools/attention_bounds.py)."""
    Tq, Tk = q.shape[0], k.shape[0]
    qd, kd, vd = (t.double().permute(1, 0, 2) for t in (q, k, v))
    kl = min(max(int(kl), 0), Tk)
    if kl == 0:
        return torch.zeros(Tq, q.shape[1], q.shape[2], dtype=F64)
    s = scale * (qd @ kd.transpose(-1, -2))
    j = torch.arange(Tk)[None, :]
    i = torch.arange(Tq)[:, None]
    valid = (j < kl).expand(Tq, Tk)
    if causal:
        valid = valid & (j <= i + diag)
    if key_limit is not None:
        valid = valid & (j < key_limit[:, None])
    s = s.masked_fill(~valid[None], float("-inf"))
    P = torch.exp(s - s.amax(-1, keepdim=True))
    Pd = P
    if keep is not None:
        Pd = P * keep.double() * (1.0 / (1.0 - p) if drop_rescale else 1.0)
    l = (Pd if sum_dropped else P).sum(-1, keepdim=True)
    if p_fmt is not None:
        Pd = rfmt(Pd, p_fmt)
    o = (Pd @ vd) / l
    if out_fmt != "none":
        o = rfmt(o, out_fmt)
    return o.permute(1, 0, 2).contiguous()


def case_reference(c, model=False, ins=None, keeps=None, **mut):
    """list over utterances of the fp64 reference [T_b, H, hd] (model=True: the CPU model of a correct kernel).  ins / keeps / **mut: MUTANTS only."""
    ins = case_inputs(c.id) if ins is None else ins
    keeps = keep_masks(c) if keeps is None else keeps
    dt = DT[c.dtype]
    out = []
    for b, (q, k, v) in enumerate(ins):
        if c.group == "hdq1":
            q = q[:1]
        kw = dict(p_fmt=dt, out_fmt=None if c.group == "hdq1" else dt) if model else {}
        kl = mut.get("klens", c.klens)[b]
        rest = {n: (x[b] if isinstance(x, (list, tuple)) else x) for n, x in mut.items() if n != "klens"}
        out.append(attn_ref(q, k, v, kl, c.scale, c.causal, keeps[b] if c.group != "hdq1" else None, c.p, **kw, **rest))
    return out


# ---- modelled error of a correct kernel per case (per-row max|err| / max|ref|, maximum over all rows of the case): `python tools/attention_bounds.py --emit`
MODEL = {"fwd-bf16-T1": 0.00e+00, "fwd-f16-T1": 0.00e+00, "fwd-bf16-T63": 3.83e-03, "fwd-f16-T63": 4.29e-04, "fwd-bf16-T64": 3.57e-03, "fwd-f16-T64": 4.55e-04,
    "fwd-bf16-T65": 3.61e-03, "fwd-f16-T65": 4.67e-04, "fwd-bf16-T128": 3.92e-03, "fwd-f16-T128": 4.98e-04, "fwd-bf16-T129": 3.79e-03,
    "fwd-f16-T129": 4.85e-04, "fwd-bf16-T256": 3.85e-03, "fwd-f16-T256": 4.87e-04, "fwd-bf16-T257": 3.82e-03, "fwd-f16-T257": 4.85e-04,
    "fwd-bf16-T319": 3.87e-03, "fwd-f16-T319": 4.84e-04, "fwd-bf16-T384": 3.90e-03, "fwd-f16-T384": 4.81e-04, "fwd-bf16-T385": 3.90e-03,
    "fwd-f16-T385": 4.85e-04, "fwd-bf16-T499": 3.93e-03, "fwd-f16-T499": 4.93e-04, "fwd-bf16-T500": 3.92e-03, "fwd-f16-T500": 4.88e-04,
    "fwd-bf16-T529": 3.92e-03, "fwd-f16-T529": 4.94e-04, "causal-bf16-T1": 0.00e+00, "causal-klens-bf16-T1": 0.00e+00, "causal-f16-T1": 0.00e+00,
    "causal-klens-f16-T1": 0.00e+00, "causal-bf16-T2": 2.90e-03, "causal-klens-bf16-T2": 2.65e-03, "causal-f16-T2": 3.50e-04, "causal-klens-f16-T2": 3.52e-04,
    "causal-bf16-T16": 3.66e-03, "causal-klens-bf16-T16": 4.15e-03, "causal-f16-T16": 4.71e-04, "causal-klens-f16-T16": 4.38e-04, "causal-bf16-T63": 3.77e-03,
    "causal-klens-bf16-T63": 3.98e-03, "causal-f16-T63": 4.91e-04, "causal-klens-f16-T63": 4.74e-04, "causal-bf16-T64": 4.02e-03,
    "causal-klens-bf16-T64": 4.69e-03, "causal-f16-T64": 4.76e-04, "causal-klens-f16-T64": 4.68e-04, "causal-bf16-T65": 3.98e-03,
    "causal-klens-bf16-T65": 3.84e-03, "causal-f16-T65": 5.36e-04, "causal-klens-f16-T65": 4.86e-04, "causal-bf16-T77": 3.91e-03,
    "causal-klens-bf16-T77": 4.31e-03, "causal-f16-T77": 5.58e-04, "causal-klens-f16-T77": 5.46e-04, "causal-bf16-T127": 4.06e-03,
    "causal-klens-bf16-T127": 4.62e-03, "causal-f16-T127": 5.72e-04, "causal-klens-f16-T127": 5.29e-04, "causal-bf16-T128": 3.93e-03,
    "causal-klens-bf16-T128": 3.99e-03, "causal-f16-T128": 5.43e-04, "causal-klens-f16-T128": 5.32e-04, "causal-bf16-T129": 4.26e-03,
    "causal-klens-bf16-T129": 4.33e-03, "causal-f16-T129": 4.81e-04, "causal-klens-f16-T129": 5.69e-04, "causal-bf16-T255": 4.32e-03,
    "causal-klens-bf16-T255": 4.33e-03, "causal-f16-T255": 5.02e-04, "causal-klens-f16-T255": 6.01e-04, "causal-bf16-T256": 3.95e-03,
    "causal-klens-bf16-T256": 4.05e-03, "causal-f16-T256": 5.04e-04, "causal-klens-f16-T256": 4.97e-04, "causal-bf16-T257": 4.11e-03,
    "causal-klens-bf16-T257": 4.15e-03, "causal-f16-T257": 5.04e-04, "causal-klens-f16-T257": 6.71e-04, "causal-bf16-T300": 4.71e-03,
    "causal-klens-bf16-T300": 4.44e-03, "causal-f16-T300": 5.54e-04, "causal-klens-f16-T300": 5.21e-04, "causal-bf16-T512": 5.49e-03,
    "causal-klens-bf16-T512": 5.07e-03, "causal-f16-T512": 5.72e-04, "causal-klens-f16-T512": 6.10e-04, "causal-bf16-T529": 4.35e-03,
    "causal-klens-bf16-T529": 4.69e-03, "causal-f16-T529": 6.82e-04, "causal-klens-f16-T529": 6.23e-04, "drop-p0.1-T64": 5.15e-03,
    "drop-causal-p0.1-T64": 5.18e-03, "drop-p0.25-T64": 5.91e-03, "drop-causal-p0.25-T64": 5.84e-03, "drop-p0.1-T65": 5.29e-03,
    "drop-causal-p0.1-T65": 5.50e-03, "drop-p0.25-T65": 5.60e-03, "drop-causal-p0.25-T65": 6.33e-03, "drop-p0.1-T131": 5.30e-03,
    "drop-causal-p0.1-T131": 5.39e-03, "drop-p0.25-T131": 5.69e-03, "drop-causal-p0.25-T131": 5.88e-03, "drop-p0.1-T257": 5.36e-03,
    "drop-causal-p0.1-T257": 5.51e-03, "drop-p0.25-T257": 5.73e-03, "drop-causal-p0.25-T257": 6.03e-03, "drop-p0.1-T300": 5.39e-03,
    "drop-causal-p0.1-T300": 6.44e-03, "drop-p0.25-T300": 5.68e-03, "drop-causal-p0.25-T300": 7.12e-03, "drop-p0.1-T499": 5.35e-03,
    "drop-causal-p0.1-T499": 7.13e-03, "drop-p0.25-T499": 5.80e-03, "drop-causal-p0.25-T499": 6.25e-03, "packed-bf16": 4.04e-03, "packed-f16": 4.88e-04,
    "packed-drop-p0.1": 5.40e-03, "hd64-L1": 0.00e+00, "hd64-L63": 3.86e-03, "hd64-L64": 3.53e-03, "hd64-L65": 4.09e-03, "hd64-L129": 3.79e-03,
    "hd64-L200": 3.87e-03, "hd64-L500": 3.93e-03, "hd96-L1": 0.00e+00, "hd96-L63": 3.79e-03, "hd96-L64": 3.91e-03, "hd96-L65": 3.92e-03, "hd96-L129": 3.80e-03,
    "hd96-L200": 3.92e-03, "hd96-L500": 3.85e-03, "hd128-L1": 0.00e+00, "hd128-L63": 3.69e-03, "hd128-L64": 3.67e-03, "hd128-L65": 4.14e-03,
    "hd128-L129": 3.88e-03, "hd128-L200": 3.93e-03, "hd128-L500": 3.86e-03, "hdq1-hd96": 5.92e-04,
}


# ================================================================================================ GPU side
def pack_qkv(ins):
    """[(q, k, v) [T_b, H, hd]] -> [sum T_b, 3 * H * hd] (q | k | v)"""
    return torch.cat([torch.cat([t.reshape(t.shape[0], -1) for t in qkv], 1) for qkv in ins], 0).contiguous()


def split_out(out, c):
    off = offsets(c.rows)
    return [out[off[b]: off[b + 1]].view(c.rows[b], c.H, c.hd) for b in range(c.B)]


def _kl(c, klens=None):
    return torch.tensor(list(c.klens if klens is None else klens), dtype=torch.int32, device="cuda")


def run_fwd(c, ins, klens=None, p=None, seed=None, causal=None):
    """sc_attention_fwd / _dropout / _packed on the case's layout -> host [sum T_b, H * 64]."""
    from speechclip_amd import _lib, ops
    qkv = pack_qkv(ins).cuda()
    p = c.p if p is None else p
    seed = c.seed if seed is None else seed
    causal = c.causal if causal is None else causal
    D = c.H * 64
    if c.group == "packed":
        off = torch.tensor(offsets(c.rows), dtype=torch.int32, device="cuda")
        return ops.attention_packed(qkv, c.B, c.T, c.H, _kl(c, klens), off, drop_p=p, seed=seed).cpu()
    if p == 0.0 and seed == 0:
        return ops.attention(qkv, c.B, c.T, c.H, _kl(c, klens), scale=c.scale, causal=causal).cpu()
    assert c.dtype == "bf16" and c.scale == 0.125
    if not causal:
        return ops.attention_dropout(qkv, c.B, c.T, c.H, _kl(c, klens), p, seed).cpu()
    out = torch.empty(c.B * c.T, D, device="cuda", dtype=BF)          # dropout + causal: no ops wrapper, the C entry directly
    rc = _lib.lib().sc_attention_fwd_dropout(qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, out.data_ptr(), _kl(c, klens).data_ptr(), c.B, c.H, c.T, 64,
                                             3 * D, D, c.scale, 1, float(p), seed & 0xffffffff, ops.stream())
    assert rc == 0, _lib.lib().sc_last_error()
    torch.cuda.synchronize()
    return out.cpu()


def check_case(c, got, ref, what=None):
    """got / ref: lists over utterances of [T_b, H, hd].  Every row of every head within the case's bound and within the older twin's absolute tolerance."""
    what = what or c.id
    model = MODEL[c.id]
    bound = bound_of(model)
    n_rows, worst, where = 0, 0.0, None
    for b, (g_, r_) in enumerate(zip(got, ref)):
        assert g_.shape == r_.shape and torch.isfinite(g_.float()).all(), (what, b)
        m = row_metric(g_, r_)
        n_rows += m.numel()
        if m.max().item() >= worst:
            worst = m.max().item()
            t, h = divmod(int(m.argmax()), m.shape[1])
            where = (b, t, h)
    expected = (c.B if c.group == "hdq1" else sum(c.rows)) * c.H          # from the case alone: every query row the layout holds
    excluded = expected - n_rows
    print(f"{what}: {n_rows} (row, head) pairs compared, {excluded} excluded; worst row metric {worst:.3e} at (utterance, row, head) {where} "
          f"(model {model:.2e}, bound {bound:.2e})")
    assert excluded == 0
    assert worst <= bound, (what, "utterance / row / head", where, "metric", worst, "bound", bound)
    tol = TWIN_TOL[c.dtype]
    for b, (g_, r_) in enumerate(zip(got, ref)):
        torch.testing.assert_close(g_.double(), r_, atol=tol, rtol=tol, msg=lambda s: f"{what} utterance {b}: {s}")
    return worst


pytestmark = pytest.mark.gpu


# ---- 1. sc_attention_fwd, non-causal
@pytest.mark.parametrize("cid", ids_of("fwd", lambda c: not c.wide))
def test_attention_fwd_every_row_vs_fp64(cid):
    c = case(cid)
    got = run_fwd(c, case_inputs(cid))
    check_case(c, split_out(got, c), case_reference(c))


@pytest.mark.parametrize("cid", ids_of("fwd", lambda c: c.wide))
def test_attention_fwd_wide_rows_separate_pointers(cid):
    """ld_qkv > 3 D and ld_out > D: q, k, v at separate (16-byte aligned) column offsets of one wider buffer, out inside a wider buffer whose other columns are
    pre-filled and must come back untouched."""
    from speechclip_amd import _lib, ops
    c = case(cid)
    ins = case_inputs(cid)
    D, M = c.H * 64, c.B * c.T
    W, WO = 3 * D + 56, D + 24
    qo, ko, vo, oo = 8, D + 24, 2 * D + 40, 16
    buf = torch.full((M, W), 7.0, dtype=DT[c.dtype])
    for col, i in ((qo, 0), (ko, 1), (vo, 2)):
        buf[:, col: col + D] = torch.cat([x[i].reshape(x[i].shape[0], D) for x in ins], 0)
    buf = buf.cuda()
    out = torch.full((M, WO), -3.0, dtype=DT[c.dtype], device="cuda")
    flags = ops.ATTN_F16 if c.dtype == "f16" else 0
    rc = _lib.lib().sc_attention_fwd(buf.data_ptr() + 2 * qo, buf.data_ptr() + 2 * ko, buf.data_ptr() + 2 * vo, out.data_ptr() + 2 * oo, _kl(c).data_ptr(), c.B, c.H, c.T, 64,
                                     W, WO, c.scale, flags, ops.stream())
    assert rc == 0, _lib.lib().sc_last_error()
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[:, :oo] == -3.0).all() and (out[:, oo + D:] == -3.0).all()
    got = out[:, oo: oo + D].contiguous()
    check_case(c, split_out(got, c), case_reference(c))
    assert torch.equal(got, run_fwd(c, ins))                                    # and the same bits as the packed q|k|v layout


# ---- 2. sc_attention_fwd, causal
@pytest.mark.parametrize("cid", ids_of("causal"))
def test_attention_fwd_causal_every_row_vs_fp64(cid):
    """SC_ATTN_CAUSAL at T on both sides of 64 / 128 / 256 (4- and 8-wave blocks, one to three query blocks, the diagonal crossing key-tile edges inside a block), without
    and with klens (valid keys below, at and above a block's last query: both terms of the key-tile count bind).  Row 0 attends to key 0 alone: out == v[0] bit for bit."""
    c = case(cid)
    ins = case_inputs(cid)
    got = split_out(run_fwd(c, ins), c)
    check_case(c, got, case_reference(c))
    for b, (q, k, v) in enumerate(ins):
        assert torch.equal(got[b][0], v[0]), (cid, b)


# ---- 3. sc_attention_fwd_dropout
@pytest.mark.parametrize("cid", ids_of("drop"))
def test_attention_fwd_dropout_host_mask_every_row_vs_fp64(cid):
    """Against the fp64 reference with the host-restated mask (test_dropout_gpu._keep_attn), plain and causal (the C entry directly: ops has no wrapper); the mask is
    really applied (far from the undropped reference), p = 0 is the plain kernel bit for bit, two seeds differ."""
    c = case(cid)
    ins = case_inputs(cid)
    raw = run_fwd(c, ins)
    got = split_out(raw, c)
    worst = check_case(c, got, case_reference(c))
    plain = dataclasses.replace(c, p=0.0)
    undropped = case_reference(plain)
    far = max(row_metric(g_, r_).max().item() for g_, r_ in zip(got, undropped))
    assert far > 10 * bound_of(MODEL[c.id]) and far > 10 * worst, (cid, far)
    assert torch.equal(run_fwd(c, ins, p=0.0, seed=5), run_fwd(c, ins, p=0.0, seed=0))
    assert not torch.equal(run_fwd(c, ins, seed=c.seed + 1), raw)


# ---- 4. sc_attention_fwd_packed
@pytest.mark.parametrize("cid", ids_of("packed"))
def test_attention_fwd_packed_every_row_vs_fp64(cid):
    """Ragged row counts on both sides of every block edge, per utterance against its own reference; with dropout against the host mask restated for the PACKED index
    (row = (row_off[b] + query) * H + h, pair stride ceil(Tmax / 2): test_dropout_gpu._keep_attn_packed)."""
    c = case(cid)
    got = run_fwd(c, case_inputs(cid))
    check_case(c, split_out(got, c), case_reference(c))


@pytest.mark.parametrize("cid", ["packed-bf16", "packed-drop-p0.1"])
def test_attention_fwd_packed_neighbours_do_not_reach_own_rows(cid):
    """Contamination control: every OTHER utterance's q / k / v rows replaced by +-1e4 -- the rows of the utterance left alone are bitwise unchanged, each in turn."""
    c = case(cid)
    ins = case_inputs(cid)
    base = split_out(run_fwd(c, ins), c)
    for keep in range(c.B):
        loud = [x if b == keep else tuple(torch.full_like(t, 1e4 if (b + i) % 2 else -1e4) for i, t in enumerate(x)) for b, x in enumerate(ins)]
        got = split_out(run_fwd(c, loud), c)
        assert torch.equal(got[keep], base[keep]), (cid, keep)
        assert all(torch.isfinite(g_.float()).all() for g_ in got)
        assert any(not torch.equal(got[b], base[b]) for b in range(c.B) if b != keep)          # the control is live


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("T", [257, 500])
def test_attention_fwd_uniform_equals_packed_with_uniform_offsets(T, dtype):
    """sc_attention_fwd (row_off = NULL; T = 257: the 8-wave launch plus the 4-wave tail launch of the query-row split, T = 500: one launch) == sc_attention_fwd_packed
    with row_off[b] = b * T (always one 8-wave launch), bit for bit: a row's arithmetic does not depend on the shape of the block that holds it."""
    c = case(f"fwd-{dtype}-T{T}")
    ins = case_inputs(c.id)
    assert torch.equal(run_fwd(c, ins), run_fwd(dataclasses.replace(c, group="packed"), ins))


# ---- 5. sc_attention_hd_fwd
@pytest.mark.parametrize("cid", ids_of("hd"))
def test_attention_hd_every_row_vs_fp64(cid):
    from speechclip_amd import ops
    c = case(cid)
    qkv = pack_qkv(case_inputs(cid)).cuda()
    got = ops.attention_hd_qkv(qkv, c.B, c.T, c.H, _kl(c)).cpu()
    check_case(c, split_out(got, c), case_reference(c))


def test_attention_hd_cls_row_form_fp32_out_vs_fp64():
    """Tq = 1, strided query, K / V rows of [k | v], fp32 output: the model has no output rounding."""
    from speechclip_amd import ops
    c = case("hdq1-hd96")
    ins = case_inputs(c.id)
    D, L = c.H * c.hd, c.T
    q = torch.stack([x[0][0].reshape(D) for x in ins]).cuda()
    kv = torch.cat([torch.cat([x[1].reshape(L, D), x[2].reshape(L, D)], 1) for x in ins], 0).cuda()
    out = ops.attention_hd(q, kv, kv[:, D:], c.B, c.H, 1, L, c.hd, (D, D), (L * 2 * D, 2 * D), _kl(c), out_f32=True).cpu()
    assert out.dtype == torch.float32
    check_case(c, [out[b].view(1, c.H, c.hd) for b in range(c.B)], case_reference(c))


# ---- 6. what lies past klens[b]
@pytest.mark.parametrize("cid", ["fwd-bf16-T319", "fwd-f16-T319", "fwd-bf16-T129", "packed-bf16", "packed-f16"])
def test_rows_past_the_key_length_do_not_matter_when_finite(cid):
    """Q / K / V rows at t >= klens[b] replaced by the largest round finite values of the format (1e4 bf16, 6e4 half): the K / V rows of the last partial tile are
    loaded and multiplied by P = 0, and 0 x finite = 0 exactly, so the rows < klens[b] are BITWISE unchanged.  (Non-finite V there is outside the contract:
    include/speechclip_hip.h, sc_attention_fwd.)"""
    c = case(cid)
    ins = case_inputs(cid)
    big = 1e4 if c.dtype == "bf16" else 6e4
    base = split_out(run_fwd(c, ins), c)
    loud = []
    for b, x in enumerate(ins):
        y = tuple(t.clone() for t in x)
        for i, t in enumerate(y):
            t[c.klens[b]:] = big if i != 1 else -big
        loud.append(y)
    got = split_out(run_fwd(c, loud), c)
    n = 0
    for b in range(c.B):
        kl = c.klens[b]
        assert torch.equal(got[b][:kl], base[b][:kl]), (cid, b)
        assert torch.isfinite(got[b].float()).all()
        n += kl * c.H
    assert any(kl < r for kl, r in zip(c.klens, c.rows))
    print(f"{cid}: {n} (row, head) pairs bitwise unchanged with +-{big:g} past the key length")


@pytest.mark.parametrize("cid", ["fwd-bf16-T129", "fwd-f16-T500", "packed-bf16"])
def test_key_length_zero_gives_zero_rows_and_above_T_is_T(cid):
    c = case(cid)
    ins = case_inputs(cid)
    base = split_out(run_fwd(c, ins), c)
    kl0 = list(c.klens)
    kl0[0], kl0[-1] = 0, 0
    got = split_out(run_fwd(c, ins, klens=kl0), c)
    for b in range(c.B):
        if kl0[b] == 0:
            assert (got[b] == 0).all() and torch.isfinite(got[b].float()).all(), (cid, b)      # the inv = 0 exit: exactly zero, not NaN
        else:
            assert torch.equal(got[b], base[b])
    full = [r for r in c.rows]
    over = [r + 5 + 64 * b for b, r in enumerate(c.rows)]
    assert torch.equal(run_fwd(c, ins, klens=over), run_fwd(c, ins, klens=full))

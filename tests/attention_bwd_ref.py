"""Plain fp64 statements, case lists, seeded inputs, DERIVED per-element bounds, the slope check, an fp32 emulation and the mutants of the fused attention
backward (csrc/attention_bwd.hip: sc_attention_bwd_packed, sc_attention_hd_bwd) and of the P / dS image chain of the padded layout (csrc/train_hubert.hip:
sc_attn_bwd_probs, sc_attn_softmax_bwd*; group "image") for tests/test_attention_bwd_parity_gpu.py and tools/attention_bwd_bounds.py.
A helper module, not a test; no kernel runs here.  The rules of the bounds are those at the top of tests/row_kernels_ref.py; DESIGN.md ("Attention backward:
parity") derives every term used below.

Per (utterance, head) unit, keys j < klen, queries i < nq = min(klen, Tq), m = keep / (1 - p) (1 without dropout):
    P = softmax(scale Q K^T)    Pd = P m    dP = dO V^T    dS = scale P (m dP - delta)    dQ = dS K    dK = dS^T Q    dV = Pd^T dO
    delta, TRUE form:     delta_i = sum_j Pd_ij dP_ij       (sc_attention_hd_bwd when it drops; the truth for every path)
    delta, STORED-O form: delta_i = dO_i . O_i, O as passed  (sc_attention_bwd_packed always, sc_attention_hd_bwd without dropout)
Every other row of every output is exactly 0.

Inputs (build_utt; the builder idea of tests/test_attention_fwd_parity_gpu.py): 0.5 randn q / k, randn v / dO, all rounded to bf16 before the reference sees them, PLUS
  * the last valid key scores ln(klen) - 0.3 above the crowd and carries V = +-3 in a sign pattern that differs between heads h and h ^ 1; the first invalid key scores
    1.5 higher still and carries V = -50 and +-20 on the other dims of its K row; the last participating query carries dO = +-3, the first query that takes no part
    dO = 50 and a q row of +-20: a mask that is off by one moves whole rows by O(1) of their size;
  * peaked heads (h % 3 == 2): q and k scaled by 4, so rows concentrate and m dP - delta cancels;
  * offset cases: +60 on every score (the |a| 2^-23 term of the exponent argument)."""
import dataclasses
import functools
import math

import numpy as np
import torch

from row_kernels_ref import BF, BF_STORE, F32, F64, TR, U, gen, rnd, store_bound, worst   # noqa: F401
from test_attention_fwd_parity_gpu import klens_for, v_sign
from test_dropout_gpu import _keep_attn, _keep_attn_packed, _keep_rows

LOG2E, LN2 = 1.4426950408889634, math.log(2.0)
QC = 1.5
SLOPE_MIN = 4096                       # the slope check applies to operands with at least this many participating elements
OPS = ("dq", "dk", "dv")


def f32v(x):
    return float(np.float32(x))


# ================================================================================================ cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    group: str                  # packed (row_off) | uniform (row_off = NULL) | hd (Tq == Tk) | hdq1 (Tq == 1) | image (the P / dS image chain of the padded layout)
    rows: tuple                 # key rows per utterance
    klens: tuple
    H: int = 2
    hd: int = 64
    scale: float = 0.125
    p: float = 0.0
    seed: int = 0
    wide: bool = False          # packed / uniform: ld wider than the data; hd: dq | dk | dv in separate buffers with their own strides
    o_src: str = "cpu"          # cpu: O = bf16(o_true) with the restated mask; fwd: O from the project's forward kernel
    offset: float = 0.0         # common score offset
    null_klens: bool = False

    @property
    def T(self):
        return max(self.rows)

    @property
    def B(self):
        return len(self.rows)

    @property
    def form(self):
        return "true" if self.group in ("hd", "hdq1") and self.p > 0 else "stored"

    def tq(self, b):
        return 1 if self.group == "hdq1" else self.rows[b]

    def kl(self, b):
        return min(max(self.klens[b], 0), self.rows[b])

    def nq(self, b):
        return self.nq_of(b, self.kl(b))

    def nq_of(self, b, kl):
        if self.group == "image":          # the image chain computes EVERY query row of an utterance that has a valid key (a training step hands it dO = 0 there)
            return self.rows[b] if kl else 0
        return min(kl, self.tq(b))

    @property
    def Lp(self):
        return -(-self.T // 64) * 64


PACKED_ROWS = (2, 64, 65, 66, 131, 40, 1, 129)
PACKED_KLENS = (1, 63, 64, 65, 131, 30, 1, 128)
UNIFORM_T = (1, 63, 64, 65, 131, 200)
HD_L = (1, 63, 64, 65, 129, 200)
HDQ1_TK = (1, 64, 65, 131)
IMAGE_T = (1, 63, 64, 65, 131)


def hd_klens(L):
    """L, 0, 1 and both sides of every 64-key tile edge below L (at most 7 utterances)"""
    out = [L, 0, 1]
    for e in (63, 64, 65, 127, 128, 129):
        if 1 < e < L and len(out) < 7:
            out.append(e)
    return tuple(dict.fromkeys(out))


@functools.lru_cache(maxsize=None)
def all_cases():
    C, cs = Case, []
    for p in (0.0, 0.1, 0.25):
        for o_src in ("cpu", "fwd"):
            if o_src == "fwd" and p == 0.25:
                continue
            cs.append(C(f"packed-p{p}-{o_src}", "packed", PACKED_ROWS, PACKED_KLENS, H=3 if o_src == "cpu" else 2, p=p, seed=1234 + int(100 * p), o_src=o_src))
    cs.append(C("packed-H12", "packed", PACKED_ROWS, PACKED_KLENS, H=12))
    cs.append(C("packed-offset60", "packed", PACKED_ROWS, PACKED_KLENS, H=3, offset=60.0))
    for i, T in enumerate(UNIFORM_T):
        kl = klens_for(T, i)
        for p in (0.0, 0.1):
            cs.append(C(f"uniform-T{T}-p{p}", "uniform", (T,) * len(kl), kl, H=3 if i % 2 else 2, p=p, seed=77 + T, wide=i % 2 == 1,
                        o_src="fwd" if (T, p) in ((131, 0.1), (200, 0.0)) else "cpu"))
    n = 0
    for hd in (64, 96, 128):
        for L in HD_L:
            kl = hd_klens(L)
            for p in (0.0, 0.1, 0.25):
                cs.append(C(f"hd{hd}-L{L}-p{p}", "hd", (L,) * len(kl), kl, H=3 if n % 3 else 2, hd=hd, scale=hd ** -0.5, p=p, seed=4242 + L + hd, wide=n % 2 == 1,
                            o_src="fwd" if L in (65, 200) and p != 0.25 else "cpu"))
                n += 1
    cs.append(C("hd96-L65-scale0.2", "hd", (65,) * 4, (65, 64, 1, 30), H=3, hd=96, scale=0.2))
    cs.append(C("hd128-L70-nullklens", "hd", (70, 70), (70, 70), H=3, hd=128, scale=128 ** -0.5, null_klens=True, wide=True))
    cs.append(C("hd96-L129-offset60", "hd", (129,) * 4, (129, 128, 65, 1), H=3, hd=96, scale=96 ** -0.5, offset=60.0, p=0.1, seed=9))
    for hd in (64, 96, 128):
        for i, Tk in enumerate(HDQ1_TK):
            kl = tuple(dict.fromkeys(k for k in (Tk, 1, 0, 63, 64, 65, 30) if k <= Tk))
            for p in (0.0, 0.1):
                cs.append(C(f"hdq1-hd{hd}-Tk{Tk}-p{p}", "hdq1", (Tk,) * len(kl), kl, H=3 if i % 2 else 2, hd=hd, scale=hd ** -0.5, p=p, seed=31 + Tk + hd,
                            o_src="fwd" if Tk == 131 else "cpu"))
    for i, T in enumerate(IMAGE_T):
        kl = klens_for(T, i)
        for p in (0.0, 0.25):
            cs.append(C(f"image-T{T}-p{p}", "image", (T,) * len(kl), kl, H=3, p=p, seed=500 + T))
    assert len({c.id for c in cs}) == len(cs)
    return tuple(cs)


N_CASES = {"packed": 7, "uniform": 12, "hd": 57, "hdq1": 24, "image": 10}
# what tests/test_attention_bwd_bounds_cpu.py runs: one case per group and per delta form
REDUCED = ("packed-p0.1-cpu", "uniform-T65-p0.0", "hd96-L65-p0.1", "hdq1-hd128-Tk65-p0.1", "image-T65-p0.25")


def case(cid):
    return next(c for c in all_cases() if c.id == cid)


def ids_of(*groups):
    return [c.id for c in all_cases() if c.group in groups]


def offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


# ================================================================================================ inputs
def build_utt(c, b, g):
    """-> q, dO [Tq, H, hd], k, v [T, H, hd]: fp64 tensors of bf16 values"""
    T, Tq, kl, nq, H, hd = c.rows[b], c.tq(b), c.kl(b), c.nq(b), c.H, c.hd
    unit = 1.0 / (c.scale * 8 * QC)                  # a key holding x * unit on dims 0..7 scores x against the common query component
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    sign = lambda *s: 1.0 - 2.0 * (r(*s) < 0).double()          # noqa: E731
    q, k, v, dO = 0.5 * r(Tq, H, hd), 0.5 * r(T, H, hd), r(T, H, hd), r(Tq, H, hd)
    for h in range(H):
        if h % 3 == 2:
            q[:, h] *= 4.0
            k[:, h] *= 4.0
    q[:, :, :8] = QC + 0.25 * r(Tq, H, 8)
    a = math.log(max(kl, 2)) - 0.3
    if kl >= 1:
        k[kl - 1, :, :8] = a * unit
        for h in range(H):
            v[kl - 1, h] = 3.0 * v_sign(h, hd)
    if kl < T:
        k[kl, :, :8] = (a + 1.5) * unit
        k[kl, :, 8:] = 20.0 * sign(H, hd - 8)
        v[kl] = -50.0
    if nq >= 1:
        dO[nq - 1] = 3.0 * sign(H, hd)
    if nq < Tq:
        dO[nq] = 50.0
        q[nq] = 20.0 * sign(H, hd)
    if c.offset:
        k[:, :, :8] += c.offset * unit
    return tuple(rnd(t, BF) for t in (q, k, v, dO))


@functools.lru_cache(maxsize=4)
def case_inputs(cid):
    c = case(cid)
    g = gen("attention_bwd", cid)
    return [build_utt(c, b, g) for b in range(c.B)]


def keep_masks(c, stride=None, pitch_own=False, swap_halves=False):
    """list over utterances of the forward's keep mask [H, Tq, T] (fp64, 1 = kept), None without dropout.  stride / pitch_own / swap_halves: MUTANTS only."""
    if c.p == 0.0:
        return [None] * c.B
    out = []
    off = offsets(c.rows)
    for b in range(c.B):
        T, H = c.rows[b], c.H
        if c.group == "packed":
            pitch = T if pitch_own else c.T
            if stride is None and not pitch_own:
                m = _keep_attn_packed(c.seed, off[b], H, T, c.T, c.p)
            else:
                ids = (off[b] + np.arange(T))[None, :] * H + np.arange(H)[:, None]
                m = _keep_rows(c.seed, ids.reshape(-1), T, pitch // 2 if stride == "floor" else (pitch + 1) // 2, c.p).view(H, T, T)
        else:
            Tq = c.tq(b)
            ids = ((b * H + np.arange(H))[:, None] * T + np.arange(Tq)[None, :]).reshape(-1)
            m = _keep_rows(c.seed, ids, T, T // 2 if stride == "floor" else (T + 1) // 2, c.p).view(H, Tq, T)
        m = m.double()
        if swap_halves:
            idx = torch.arange(T) ^ 1
            idx[idx >= T] = T - 1
            m = m[..., idx]
        out.append(m)
    return out


# the row form above IS the uniform restatement _keep_attn, and the packed one _keep_attn_packed (checked once, at import, on small shapes)
assert torch.equal(_keep_attn(5, 2, 2, 5, 0.25), _keep_rows(5, np.arange(20), 5, 3, 0.25).view(2, 2, 5, 5))
assert torch.equal(_keep_attn_packed(5, 3, 2, 4, 7, 0.25), _keep_rows(5, ((3 + np.arange(4))[None, :] * 2 + np.arange(2)[:, None]).reshape(-1), 4, 4, 0.25).view(2, 4, 4))


# ================================================================================================ the operation and its bounds, one (utterance) = H units at a time
def hm(t):
    """[n, H, hd] -> [H, n, hd]"""
    return t.permute(1, 0, 2)


def unit_ref(q, k, v, dO, O, m, scale, form, model=False, mut=None, pack=None, s=None, dP=None):
    """q, dO, O [H, nq, hd], k, v [H, kl, hd] fp64; m [H, nq, kl] = keep / (1 - p) or None.  -> dict of the statement's tensors.
    model: the bf16 roundings of a correct kernel (Pd and dS as MFMA operands, the three outputs).  s / dP: the raw scores and dP GIVEN (the fp32 images
    sc_attn_softmax_bwd* take).  mut / pack: MUTANTS only."""
    rb = (pack or (lambda t: rnd(t, BF))) if model else (lambda t: t)
    s = q @ k.transpose(-1, -2) if s is None else s
    P = torch.softmax(scale * s * (LN2 if mut == "natural_log" else 1.0), -1)
    if mut == "lse_last_block" and k.shape[1] > 16:
        nb = (k.shape[1] - 1) // 16 * 16
        P = torch.exp(scale * s - torch.logsumexp(scale * s[..., :nb], -1, keepdim=True))
    one = torch.ones_like(P)
    mm = one if m is None else m
    Pd = P * (one if mut == "no_m_on_P" else mm)
    dP = dO @ v.transpose(-1, -2) if dP is None else dP
    x = dP * (one if mut == "no_m_on_dP" else mm)
    delta_true = (P * mm * dP).sum(-1)
    delta = delta_true if form == "true" else (dO * O).sum(-1)
    if mut == "delta_undropped":
        delta = (P * dP).sum(-1)
    if mut == "delta_next_row":
        delta = torch.roll(delta, -1, -1)
    dS = scale * P * (x - delta[..., None]) * {"no_scale": 1.0 / scale, "scale_twice": scale}.get(mut, 1.0)
    dSr, Pdr = rb(dS), rb(Pd)
    dSk = dSr
    if mut == "ds_not_transposed":
        n = max(dSr.shape[-2:])
        sq = torch.zeros(dSr.shape[0], n, n, dtype=F64)
        sq[:, :dSr.shape[1], :dSr.shape[2]] = dSr
        dSk = sq.transpose(-1, -2)[:, :dSr.shape[1], :dSr.shape[2]]
    return dict(s=s, P=P, Pd=Pd, dP=dP, x=x, delta=delta, delta_true=delta_true, dS=dS, dq=rb(dSr @ k), dk=rb(dSk.transpose(-1, -2) @ q),
                dv=rb(Pdr.transpose(-1, -2) @ dO), o_true=P * mm @ v)


def unit_bounds(u, q, k, v, dO, O, m, scale, form, shared=False, image=None):
    """Per-element bounds of one utterance's units (DESIGN.md derives each line).  -> {op: (b32, bbf, var)}, e_lse, e_delta, lse (log2 units), {op: sum(ref^2 var)}.
    shared (Tq == 1): the last is summed per ROUNDING, not per element -- the one rounding of Pd_j or dS_j reaches the hd elements of row j with equal signs
    (dV_je dO_e = Pd_j dO_e^2), which the elementwise quadrature undercounts by up to sqrt(hd).
    image = (Lp, given): the image chain -- p = __expf(S scale - max) * (1 / den) in natural units, the outputs GEMMs with K = Lp; given: S and dP were handed over
    as fp32 images (no MFMA error of their own); a sixth result holds the bounds of the P and dS images themselves."""
    hd, kl, nq = q.shape[-1], k.shape[1], q.shape[1]
    P, Pd, dS, x, delta = u["P"], u["Pd"], u["dS"], u["x"], u["delta"]
    aq, ak, av, ad = q.abs(), k.abs(), v.abs(), dO.abs()
    c = scale * LOG2E
    sc = c * u["s"]
    e_sc = c * hd * U * (aq @ ak.transpose(-1, -2)) + 3 * U * sc.abs()          # the MFMA sum; the product with scale_log2e and that constant's own two roundings
    M = sc.amax(-1, keepdim=True)
    lt = torch.exp2(sc - M).sum(-1)
    lse = M[..., 0] + torch.log2(lt)
    nkb = -(-kl // 16)
    r_lt = kl * U + (nkb + 2) * (TR + 2 * U) + TR + LN2 * U * (P * (M - sc)).sum(-1)          # relative error of the row sum
    e_lse = (P * e_sc).sum(-1) + r_lt / LN2 + TR * torch.log2(lt) + U * lse.abs()
    a = sc - lse[..., None]
    rel_p = LN2 * (e_sc + e_lse[..., None] + U * a.abs()) + TR
    e_dP = hd * U * (ad @ av.transpose(-1, -2))
    if image is not None:
        # __expf(x) = v_exp_f32(x log2 e): the product S scale, the subtraction of the maximum and the product with log2 e each round the ARGUMENT; an error of
        # a score moves p_j by itself and by the p-weighted mean (the maximum cancels between numerator and row sum); den: kl terms, one exp each, the online
        # rescales of sc_attn_bwd_probs; 1 / den (TR) and the product with it
        S = scale * u["s"]
        e_S = (0.0 if image[1] else scale * hd * U * (aq @ ak.transpose(-1, -2))) + U * S.abs()
        Mn = S.amax(-1, keepdim=True)
        e_arg = e_S + 3 * U * (Mn - S)
        rel_p = e_arg + (P * e_arg).sum(-1, keepdim=True) + 2 * TR + (kl + 1) * U + (nkb + 2) * (TR + 3 * U) + TR + U
        if image[1]:
            e_dP = torch.zeros_like(e_dP)
        kl = nq = image[0]          # the length of the GEMMs' accumulation
    mm = torch.ones_like(P) if m is None else m
    if form == "stored":
        e_delta = hd * U * (dO * O).abs().sum(-1)
        e_x = mm * e_dP + (0.0 if m is None else U) * x.abs()
        e_dS = (rel_p + 3 * U) * dS.abs() + scale * P * (e_x + e_delta[..., None])
        e_delta_ws = e_delta
    else:
        # delta = sum_j e_j x_j / sum_j e_j from the SAME exponentials e_j and the SAME x_j = fl(m dP_j) the sweeps recompute: an error of a weight acts on
        # |x_j - delta|, an error of dP_j enters m dP_j - delta on both sides
        rho = LN2 * (e_sc + (P * e_sc).sum(-1, keepdim=True) + U * (M - sc)) + TR
        r_tot = (2 * (kl + nkb + 2) + 1) * U + TR
        e_dt = (P * rho * (x - delta[..., None]).abs()).sum(-1) + r_tot * (P * x.abs()).sum(-1)
        tsum = (Pd * e_dP).sum(-1, keepdim=True)
        e_dS = (rel_p + 3 * U) * dS.abs() + scale * P * (mm * e_dP * (1 - P) + (tsum - Pd * e_dP).clamp_min(0) + e_dt[..., None])
        e_delta_ws = e_dt + tsum[..., 0] + U * (P * x.abs()).sum(-1)
    aS, aSt, Pt = dS.abs(), dS.abs().transpose(-1, -2), Pd.transpose(-1, -2)
    out = {}
    mag = aS @ ak
    out["dq"] = (e_dS @ ak + kl * U * mag, BF_STORE * (mag + u["dq"].abs()), BF_STORE ** 2 / 3 * ((dS * dS) @ (k * k) + u["dq"] ** 2))
    mag = aSt @ aq
    out["dk"] = (e_dS.transpose(-1, -2) @ aq + nq * U * mag, BF_STORE * (mag + u["dk"].abs()),
                 BF_STORE ** 2 / 3 * ((dS * dS).transpose(-1, -2) @ (q * q) + u["dk"] ** 2))
    mag = Pt @ ad
    out["dv"] = (((rel_p + U) * Pd).transpose(-1, -2) @ ad + nq * U * mag, BF_STORE * (mag + u["dv"].abs()),
                 BF_STORE ** 2 / 3 * ((Pd * Pd).transpose(-1, -2) @ (dO * dO) + u["dv"] ** 2))
    vs = {o: float((u[o] ** 2 * out[o][2]).sum()) for o in OPS}
    if shared:
        c2 = BF_STORE ** 2 / 3
        vs = {"dq": c2 * float(((dS * (u["dq"] @ k.transpose(-1, -2))) ** 2).sum() + (u["dq"] ** 4).sum()),
              "dk": c2 * float(((dS * (q @ u["dk"].transpose(-1, -2))) ** 2).sum() + (u["dk"] ** 4).sum()),
              "dv": c2 * float(((Pd * (dO @ u["dv"].transpose(-1, -2))) ** 2).sum() + (u["dv"] ** 4).sum())}
    if image is not None:
        return out, e_lse, e_delta_ws, lse, vs, {"P": ((rel_p + U) * Pd, BF_STORE * Pd), "dS": (e_dS, BF_STORE * dS.abs())}
    return out, e_lse, e_delta_ws, lse, vs


def delta_term(u, q, k, dO, O, scale):
    """what Delta_i = dO_i . (O_stored,i - o_true,i) adds to the dq and dk bounds when a stored-O path is judged against the truth"""
    D = (dO * (O - u["o_true"])).sum(-1).abs()[..., None]           # [H, nq, 1]
    return {"dq": scale * (u["P"] * D) @ k.abs(), "dk": scale * (u["P"] * D).transpose(-1, -2) @ q.abs()}


@dataclasses.dataclass
class CaseRef:
    """per utterance lists; outputs [Tq or T, H, hd] with zeros on the rows that take no part; bounds likewise (0 there: exact)"""
    ref: dict
    b32: dict
    bbf: dict
    var: dict
    truth: dict
    extra: dict
    lse: list
    delta: list
    e_lse: list
    e_delta: list
    O: list
    units: list
    vsum: dict
    img: list = None


def _zeros(c, b, op):
    return torch.zeros(c.tq(b) if op == "dq" else c.rows[b], c.H, c.hd, dtype=F64)


def slices(c, b, ins):
    q, k, v, dO = ins[b]
    nq, kl = c.nq(b), c.kl(b)
    return hm(q[:nq]), hm(k[:kl]), hm(v[:kl]), hm(dO[:nq])


def cpu_O(c, ins=None, keeps=None):
    """O = bf16(o_true) per utterance [Tq, H, hd] (zeros on the rows that take no part)"""
    ins = case_inputs(c.id) if ins is None else ins
    keeps = keep_masks(c) if keeps is None else keeps
    ks = 1.0 / (1.0 - f32v(c.p))
    out = []
    for b in range(c.B):
        o = torch.zeros(c.tq(b), c.H, c.hd, dtype=F64)
        nq, kl = c.nq(b), c.kl(b)
        if nq:
            q, k, v, _ = slices(c, b, ins)
            P = torch.softmax(f32v(c.scale) * (q @ k.transpose(-1, -2)), -1)
            if keeps[b] is not None:
                P = P * keeps[b][:, :nq, :kl] * ks
            o[:nq] = hm(rnd(P @ v, BF))
        out.append(o)
    return out


def case_reference(c, O=None, ins=None, given=False):
    """The statement the case's path computes (form = c.form) with its bounds, and the truth with the Delta term.  O: per utterance [Tq, H, hd] as passed to the kernel."""
    ins = case_inputs(c.id) if ins is None else ins
    keeps = keep_masks(c)
    O = cpu_O(c, ins, keeps) if O is None else O
    scale, ks = f32v(c.scale), 1.0 / (1.0 - f32v(c.p))
    R = CaseRef({o: [] for o in OPS}, {o: [] for o in OPS}, {o: [] for o in OPS}, {o: [] for o in OPS}, {o: [] for o in OPS}, {o: [] for o in OPS}, [], [], [], [], O, [], {o: 0.0 for o in OPS})
    R.img = []
    for b in range(c.B):
        nq, kl, Tq = c.nq(b), c.kl(b), c.tq(b)
        z = {o: [_zeros(c, b, o) for _ in range(6)] for o in OPS}
        im = {n_: [torch.zeros(c.H, c.Lp, c.Lp, dtype=F64) for _ in range(3)] for n_ in ("P", "dS")} if c.group == "image" else None
        st = [torch.zeros(c.H, Tq, dtype=F64) for _ in range(4)]
        u = None
        if nq:
            q, k, v, dO = slices(c, b, ins)
            Ob = hm(O[b][:nq])
            m = None if keeps[b] is None else keeps[b][:, :nq, :kl] * ks
            sg, dPg = (rnd(q @ k.transpose(-1, -2), F32), rnd(dO @ v.transpose(-1, -2), F32)) if given else (None, None)
            u = unit_ref(q, k, v, dO, Ob, m, scale, c.form, s=sg, dP=dPg)
            res = unit_bounds(u, q, k, v, dO, Ob, m, scale, c.form, shared=c.group == "hdq1", image=(c.Lp, given) if im else None)
            bd, e_lse, e_delta, lse, vs = res[:5]
            if im:
                im["P"][0][:, :nq, :kl], im["dS"][0][:, :nq, :kl] = u["Pd"], u["dS"]
                for n_ in ("P", "dS"):
                    im[n_][1][:, :nq, :kl], im[n_][2][:, :nq, :kl] = res[5][n_]
            for o in OPS:
                R.vsum[o] += vs[o]
            ut = u if c.form == "true" else unit_ref(q, k, v, dO, Ob, m, scale, "true")
            dt = delta_term(u, q, k, dO, Ob, scale) if c.form == "stored" else {}
            for o in OPS:
                n = nq if o == "dq" else kl
                z[o][0][:n], z[o][1][:n], z[o][2][:n], z[o][3][:n], z[o][4][:n] = hm(u[o]), hm(bd[o][0]), hm(bd[o][1]), hm(bd[o][2]), hm(ut[o])
                if o in dt:
                    z[o][5][:n] = hm(dt[o])
            st[0][:, :nq], st[1][:, :nq], st[2][:, :nq], st[3][:, :nq] = lse, u["delta"], e_lse, e_delta
        for o in OPS:
            for dst, t in zip((R.ref, R.b32, R.bbf, R.var, R.truth, R.extra), z[o]):
                dst[o].append(t)
        R.lse.append(st[0]); R.delta.append(st[1]); R.e_lse.append(st[2]); R.e_delta.append(st[3])
        R.units.append(u)
        R.img.append(im)
    return R


def participating(c, op):
    return sum((c.nq(b) if op == "dq" else c.kl(b)) for b in range(c.B) if c.nq(b)) * c.H * c.hd


def n_elements(c, op):
    return sum((c.tq(b) if op == "dq" else c.rows[b]) for b in range(c.B)) * c.H * c.hd


def cat(xs):
    return torch.cat([x.reshape(-1) for x in xs])


def judge_op(what, got, ref, b32, bbf, extra=None):
    """got / ref / bounds: lists over utterances.  Every element against b32 + bbf [+ extra]; -> (worst ratio, elements judged, share of `extra` in the bound)"""
    g, r = cat(got), cat(ref)
    bound = cat(b32) + cat(bbf) + (0 if extra is None else cat(extra))
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), what
    w, i = worst((g - r).abs(), bound)
    share = float(cat(extra).sum() / bound.sum().clamp_min(1e-300)) if extra is not None else 0.0
    print(f"{what:56s} worst err/bound {w:8.4f} over {g.numel()} elements" + (f", Delta share of the bound {share:.3f}" if extra is not None else ""))
    return w, g.numel(), share, (i, float(g[i]), float(r[i]), float(bound[i]))


def slope_check(got, ref, b32, vsum):
    """-> (|slope - 1|, threshold); vsum = sum(ref^2 var) of the case and operand.  The rows that take no part have ref = 0 and add nothing to any of the sums."""
    g, r, b = cat(got), cat(ref), cat(b32)
    s2 = float((r * r).sum())
    slope = float((g * r).sum()) / s2
    thr = 6.0 * math.sqrt(vsum) / s2 + float((r.abs() * b).sum()) / s2
    return abs(slope - 1.0), thr


def part_rows(c, op, xs):
    """the participating rows of per-utterance tensors [rows, H, hd]"""
    return [x[: (c.nq(b) if op == "dq" else c.kl(b))] if c.nq(b) else x[:0] for b, x in enumerate(xs)]


# ================================================================================================ a correct kernel, modelled: fp64 + bf16 roundings, or fp32 at its rounding points
def trunc_bf(t):
    return (t.to(F32).view(torch.int32) & -65536).view(F32).to(F64)


def _f32_unit(q, k, v, dO, O, m, scale, form, rev):
    """fp32 emulation of the three kernels at their rounding points: scores and dP as fp32 products of the bf16 operands, the online softmax statistics over
    16-key blocks, exp2(s c - lse), P / dS rounded to bf16, the outputs accumulated 64-row tile by tile.  rev: every walk reversed."""
    f = lambda t: t.to(F32)      # noqa: E731
    q, k, v, dO, O = f(q), f(k), f(v), f(dO), f(O)
    flip = (lambda t: t.flip(-1)) if rev else (lambda t: t)
    H, nq, kl = q.shape[0], q.shape[1], k.shape[1]
    c32 = torch.tensor(np.float32(np.float32(scale) * np.float32(1.44269504088896341)))
    sc32 = torch.tensor(np.float32(scale))
    s = (flip(q) @ flip(k).transpose(-1, -2)) * c32
    dP = flip(dO) @ flip(v).transpose(-1, -2)
    x = dP if m is None else dP * f(m)
    mx = torch.full((H, nq), float("-inf"), dtype=F32)
    l = torch.zeros(H, nq, dtype=F32)
    da = torch.zeros(H, nq, dtype=F32)
    blocks = list(range(0, kl, 16))
    for j0 in (reversed(blocks) if rev else blocks):
        sb, xb = s[..., j0:j0 + 16], x[..., j0:j0 + 16]
        bm = torch.maximum(mx, sb.amax(-1))
        e = torch.exp2(sb - bm[..., None])
        resc = torch.exp2(mx - bm)
        l = l * resc + e.sum(-1)
        da = da * resc + (e * xb).sum(-1)
        mx = bm
    lse = mx + torch.log2(l)
    delta = da / l if form == "true" else (flip(dO) * flip(O)).sum(-1)
    p = torch.exp2(s - lse[..., None])
    dS = (p * (x - delta[..., None]) * sc32).to(BF).to(F32)
    Pd = (p if m is None else p * f(m)).to(BF).to(F32)

    def tiled(a, b_):          # a [H, n, r], b_ [H, r, hd]: sum over r in 64-row tiles
        acc = torch.zeros(a.shape[0], a.shape[1], b_.shape[-1], dtype=F32)
        tiles = list(range(0, a.shape[-1], 64))
        for t0 in (reversed(tiles) if rev else tiles):
            acc = acc + a[..., t0:t0 + 64] @ b_[:, t0:t0 + 64]
        return acc.to(BF).to(F64)
    return dict(dq=tiled(dS, k), dk=tiled(dS.transpose(-1, -2), q), dv=tiled(Pd.transpose(-1, -2), dO), lse=lse.to(F64), delta=delta.to(F64))


MUTANTS = ("klen_plus1", "klen_minus1", "nq_plus1", "nq_minus1", "lse_last_block", "natural_log", "no_scale", "scale_twice", "v_heads_swapped", "dO_heads_swapped",
           "ds_not_transposed", "delta_next_row", "delta_undropped", "delta_stored_in_hd", "no_m_on_P", "no_m_on_dP", "mask_halves_swapped", "pair_stride_floor",
           "mask_pitch_own", "row_off_bTmax", "q_stride_of_k")
SLOPE_MUTANTS = ("keep_scale_bf16", "trunc_pack")
# where a mutant can show at all
def single_kept(c):
    """utterances of a true-form case whose one valid key is kept on some head"""
    if c.form != "true":
        return []
    keeps = keep_masks(c)
    return [b for b in range(c.B) if c.kl(b) == 1 and bool(keeps[b][:, 0, 0].any())]


def single_key_check(c, R, ins=None):
    """One kept key under dropout, true form: m dP - delta cancels exactly in fp32, so the dq and dk bounds there hold only the tiny fp32 terms -- asserted to lie
    below 1e-4 of what the stored-O form would leave, BF_STORE sum|dO v| scale |k| (|q| for dk), so that a return to the stored-O delta must leave the bound.
    -> number of (utterance, head) units checked"""
    ins = case_inputs(c.id) if ins is None else ins
    keeps, n = keep_masks(c), 0
    for b in single_kept(c):
        q, k, v, dO = ins[b]
        for h in range(c.H):
            if not bool(keeps[b][h, 0, 0]):
                continue
            lim = 1e-4 * BF_STORE * float((dO[0, h] * v[0, h]).abs().sum()) * f32v(c.scale)
            for op, other in (("dq", k[0, h]), ("dk", q[0, h])):
                bound = (R.b32[op][b] + R.bbf[op][b])[0, h]
                assert bool((R.bbf[op][b][0, h] == 0).all()) and bool((bound < lim * other.abs()).all()), (c.id, b, h, op, float((bound / (lim * other.abs())).max()))
            n += 1
    return n


NEEDS = {"delta_undropped": lambda c: c.p > 0, "delta_stored_in_hd": lambda c: bool(single_kept(c)), "no_m_on_P": lambda c: c.p > 0,
         "no_m_on_dP": lambda c: c.p > 0, "mask_halves_swapped": lambda c: c.p > 0, "pair_stride_floor": lambda c: c.p > 0 and c.T % 2 == 1 and c.group != "hdq1",
         "mask_pitch_own": lambda c: c.p > 0 and c.group == "packed", "row_off_bTmax": lambda c: c.group == "packed", "q_stride_of_k": lambda c: c.group == "hdq1",
         "nq_plus1": lambda c: c.group != "hdq1", "nq_minus1": lambda c: c.group != "hdq1", "keep_scale_bf16": lambda c: c.p > 0,
         "delta_next_row": lambda c: c.group != "hdq1", "ds_not_transposed": lambda c: c.group != "hdq1"}


def case_model(c, mode="model", mut=None, ins=None, O=None):
    """dq / dk / dv of the whole case [per utterance: rows, H, hd] as a correct kernel (mode model | f32 | f32rev) or a MUTANT of it (fp64 + bf16 roundings) would write them"""
    base = case_inputs(c.id) if ins is None else ins
    ins = base
    O = cpu_O(c, base) if O is None else O
    keeps = keep_masks(c, stride="floor" if mut == "pair_stride_floor" else None, pitch_own=mut == "mask_pitch_own", swap_halves=mut == "mask_halves_swapped")
    scale, ks = f32v(c.scale), 1.0 / (1.0 - f32v(c.p))
    if mut == "keep_scale_bf16":
        ks = float(rnd(torch.tensor(ks), BF))
    if mut == "row_off_bTmax":          # utterance b read from (and its O / dO rows taken at) row b * Tmax of the packed rows, as far as the buffer goes
        allr = [torch.cat([x[i] for x in base]) for i in range(4)]
        allO = torch.cat(O)
        tot = allr[0].shape[0]
        ins, O2 = [], []
        for b in range(c.B):
            r0 = min(b * c.T, tot - c.rows[b])
            ins.append(tuple(t[r0:r0 + c.rows[b]] for t in allr))
            O2.append(allO[r0:r0 + c.rows[b]])
        O = O2
    if mut == "q_stride_of_k":          # Tq = 1: utterance b's query read at b * (the key buffer's utterance stride), modulo the [B, D] query buffer
        qa = torch.stack([x[0][0] for x in base]).reshape(-1)
        D = c.H * c.hd
        ins = []
        for b in range(c.B):
            o0 = (b * c.rows[b] * 2 * D) % qa.numel()
            qb = torch.cat([qa, qa])[o0:o0 + D].view(1, c.H, c.hd)
            ins.append((qb,) + tuple(base[b][1:]))
    out = {o: [] for o in OPS}
    out["lse"], out["delta"] = [], []
    for b in range(c.B):
        kl, Tq, T = c.kl(b), c.tq(b), c.rows[b]
        kl = {"klen_plus1": min(kl + 1, T), "klen_minus1": max(kl - 1, 0)}.get(mut, kl)
        nq = c.nq_of(b, kl)
        nq = {"nq_plus1": min(nq + 1, Tq), "nq_minus1": max(nq - 1, 0)}.get(mut, nq)
        res = {o: _zeros(c, b, o) for o in OPS}
        st = [torch.zeros(c.H, Tq, dtype=F64), torch.zeros(c.H, Tq, dtype=F64)]
        if nq and kl:
            q, k, v, dO = ins[b]
            q, k, v, dO, Ob = hm(q[:nq]), hm(k[:kl]), hm(v[:kl]), hm(dO[:nq]), hm(O[b][:nq])
            swap = [h ^ 1 if (h ^ 1) < c.H else h for h in range(c.H)]
            if mut == "v_heads_swapped":
                v = v[swap]
            if mut == "dO_heads_swapped":
                dO = dO[swap]
            m = None if keeps[b] is None else keeps[b][:, :nq, :kl] * ks
            form = "stored" if mut == "delta_stored_in_hd" else c.form
            if mode == "model":
                u = unit_ref(q, k, v, dO, Ob, m, scale, form, model=True, mut=mut, pack=trunc_bf if mut == "trunc_pack" else None)
            else:
                u = _f32_unit(q, k, v, dO, Ob, m, scale, form, mode == "f32rev")
                st[0][:, :nq], st[1][:, :nq] = u["lse"], u["delta"]
            res["dq"][:nq], res["dk"][:kl], res["dv"][:kl] = hm(u["dq"]), hm(u["dk"]), hm(u["dv"])
        for o in OPS:
            out[o].append(res[o])
        out["lse"].append(st[0]); out["delta"].append(st[1])
    return out


def sentinel_mass(c, R):
    """mean probability of the last valid key over the queries of the plain heads, per utterance with klen >= 3"""
    out = []
    for b, u in enumerate(R.units):
        if u is not None and c.kl(b) >= 3:
            out += [float(u["P"][h, :, -1].mean()) for h in range(c.H) if h % 3 != 2]
    return out


IMAGE_MUTANTS = ("pad_column_holds_p", "inv_over_all_keys")


def image_model(c, mut=None, given=False):
    """the P and dS images [B][H, Lp, Lp] as a correct sc_attn_bwd_probs (fp64 + the bf16 store) or an image MUTANT writes them"""
    ins, keeps = case_inputs(c.id), keep_masks(c)
    O = cpu_O(c, ins, keeps)
    scale, ks = f32v(c.scale), 1.0 / (1.0 - f32v(c.p))
    out = []
    for b in range(c.B):
        nq, kl, T = c.nq(b), c.kl(b), c.rows[b]
        P, dS = torch.zeros(c.H, c.Lp, c.Lp, dtype=F64), torch.zeros(c.H, c.Lp, c.Lp, dtype=F64)
        if nq:
            q, k, v, dO = slices(c, b, ins)
            m = None if keeps[b] is None else keeps[b][:, :nq, :kl] * ks
            u = unit_ref(q, k, v, dO, hm(O[b][:nq]), m, scale, "stored")
            Pd, ds = u["Pd"], u["dS"]
            if mut is not None and kl < T:
                S = scale * (q @ hm(ins[b][1]).transpose(-1, -2))          # every key row of the utterance
                if mut == "pad_column_holds_p":
                    P[:, :nq, kl] = rnd(torch.exp(S[..., kl] - torch.logsumexp(S[..., :kl], -1)), BF)
                if mut == "inv_over_all_keys":
                    r = torch.exp(torch.logsumexp(S[..., :kl], -1) - torch.logsumexp(S, -1))[..., None]
                    Pd, ds = Pd * r, ds * r
            P[:, :nq, :kl], dS[:, :nq, :kl] = rnd(Pd, BF), rnd(ds, BF)
        out.append({"P": P, "dS": dS})
    return out

"""Shared by the image-tower training tests (test_vit_train_*.py): the two tiny towers, their fp64 oracle twins, and the plain fp64 statements and
DERIVED bounds of the two kernels of csrc/train_vit.hip.

Bounds (u = 2^-24, the unit round-off of fp32; every rule is first order in u):
    a bf16 store                        2^-8 |value stored| (8 significand bits, round to nearest; the stored value carries its own fp32 error e:
                                        |bf16(x + e) - x| <= 2^-8 |x| + (1 + 2^-8) |e|)
    an fp32 sum of n terms              n u sum|terms|      (any order), plus the terms' own errors
    an fp32 product / sum of two        u |result|, plus the operands' errors times the partner
    rsqrtf, the reciprocal              4 u relative
sc_vit_embed_bwd recomputes the LayerNorm row in fp32, so the bound carries the errors of the row mean, the variance, rstd and xhat into dx; the statements
below follow the kernel's algebra step by step and `embed_bwd_bounds` adds the rules up along them.  Nothing in it is fitted to an output.
"""
import dataclasses

import torch

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
EPS = 1e-5
SENT16, SENT32 = -24576.0, 2.0 ** 100        # sentinels of the guarded output buffers (exact in bf16 / in f32)
GUARD = 64

TOWERS = {          # name -> (image_resolution, vision_patch): ntok, K = 3 p^2, Kpad
    "T17": (56, 14),     # 17 tokens, K 588 -> Kpad 640: the padded-K cut of the conv gradient; fewer rows than one attention tile
    "T65": (64, 8),      # 65 tokens, K 192 (unpadded): one row past a 64-row tile
}
B_IMG = 4
SEED = 20


def tower_config(name):
    from speechclip_amd.module.clip_model import ClipConfig
    r, p = TOWERS[name]
    return ClipConfig(image_resolution=r, vision_patch=p, vision_width=128, vision_layers=2, embed_dim=64, context_length=77, vocab_size=512,
                      text_width=64, text_heads=1, text_layers=2)


def make_tower(name, trainable=True):
    """(ClipModel on the CPU with perturbed LayerNorms / biases so that no gradient is trivially zero, its fp64 oracle twin, image f32 [4, 3, R, R], w f64 [4, 64])."""
    from oracle.clip_ref import ClipRef, ClipRefConfig
    from speechclip_amd.module.clip_official import ClipModel
    cfg = tower_config(name)
    torch.manual_seed(SEED)
    model = ClipModel("ViT-B/32", image_encoder_trainable=trainable, clip_config=cfg)
    g = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for k, p in model.model.visual.named_parameters():
            if "ln_" in k or k.endswith(".bias") or k.endswith("in_proj_bias"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    ref = ClipRef(ClipRefConfig(**dataclasses.asdict(cfg))).double()
    ref.load_state_dict({k: v.double() for k, v in model.model.state_dict().items()})
    image = torch.randn(B_IMG, 3, cfg.image_resolution, cfg.image_resolution, generator=g)
    w = torch.randn(B_IMG, cfg.embed_dim, generator=g, dtype=F64)
    return model, ref, image, w


def oracle_visual_grads(ref, image, w):
    """fp64 autograd of sum(encode_image(image) * w) w.r.t. every `visual` tensor -> (feat, {name: grad})."""
    for p in ref.parameters():
        p.requires_grad_(False)
        p.grad = None
    for p in ref.visual.parameters():
        p.requires_grad_(True)
    with torch.enable_grad():
        feat = ref.encode_image(image.double())
        (feat * w).sum().backward()
    return feat.detach(), {k: p.grad.clone() for k, p in ref.visual.named_parameters()}


def cos_ratio(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return torch.nn.functional.cosine_similarity(got[None], ref[None]).item(), got.norm().item() / ref.norm().item()


class Guarded:
    """a flat window of n elements, `off` elements past the guard, inside a sentinel-filled buffer"""

    def __init__(self, n, dt, off=0):
        self.n, self.off, self.sent = n, off, SENT32 if dt == F32 else SENT16
        self.buf = torch.full((2 * GUARD + off + n,), self.sent, dtype=dt, device="cuda")
        self.win = self.buf[GUARD + off:GUARD + off + n]

    def check(self, what):
        flat = self.buf.cpu().to(F64)
        lo = GUARD + self.off
        assert bool((flat[:lo] == self.sent).all()) and bool((flat[lo + self.n:] == self.sent).all()), (what, "wrote outside its output region")
        return flat[lo:lo + self.n].clone()


# ================================================================================================ sc_quickgelu_bwd_bf16
def every_bf16_in(lo, hi):
    """every bf16 value in [lo, hi] (both signs of zero, denormals included) as f64"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF).to(F64)
    return v[torch.isfinite(v) & (v >= lo) & (v <= hi)]


def quickgelu_bwd_ref(u, dh):
    s = torch.sigmoid(1.702 * u)
    return dh * (s + 1.702 * u * s * (1 - s))


def quickgelu_bwd_bound(ref, dh):
    """2^-8 |ref| for the bf16 store + 2^-20 |dh| = 16 u |dh|: the fp32 error of dh q'(u), |q'| < 1.2 (exp, reciprocal and the cancelling sum near q' = 0)"""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -20 * dh.abs()


# ================================================================================================ sc_vit_embed_bwd
EMBED_SHAPES = [(4, 17, 128), (3, 65, 128), (2, 5, 1024), (1, 2, 64)]


def embed_bwd_inputs(B, ntok, D, seed=0):
    """f64 tensors holding bf16-exact `patch` and f32-exact dx / cls / pos / gamma (gamma around 1, dx with a non-zero column mean)"""
    g = torch.Generator().manual_seed(1000 * ntok + D + seed)
    r = lambda *s: torch.randn(*s, generator=g)            # noqa: E731
    patch = (0.8 * r(B * (ntok - 1), D) + 0.1).to(BF).to(F64)
    cls, pos = (0.5 * r(D)).to(F64), (0.4 * r(ntok, D)).to(F64)
    gamma = (1.0 + 0.3 * r(D)).to(F64)
    dx = (0.05 * r(B * ntok, D) + 0.01).to(F64)
    return dict(dx=dx, patch=patch, cls=cls, pos=pos, gamma=gamma, B=B, ntok=ntok, D=D)


def embed_bwd_ref(dx, patch, cls, pos, gamma, B, ntok, D, dt=F64, mutant=None):
    """The adjoint of x0 = LN_pre([cls | patch] + pos) in precision `dt` -> dict(dpatch [B*(ntok-1), D], dpos [ntok, D], dgamma [D], dbeta [D]) plus the
    intermediates the bound needs.  mutant: 'no_mean' (mean term dropped from dx), 'dpos_no_cls' (dpos misses the class row), 'dgamma_dy' (dy for dy xhat)."""
    dx, patch, cls, pos, gamma = (t.to(dt) for t in (dx, patch, cls, pos, gamma))
    v = torch.cat([cls.expand(B, 1, D), patch.view(B, ntok - 1, D)], 1) + pos
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + EPS).rsqrt()
    xh = d * rstd
    dy = dx.view(B, ntok, D)
    gv = dy * gamma
    s1 = gv.mean(-1, keepdim=True)
    s2 = (gv * xh).mean(-1, keepdim=True)
    dv = rstd * (gv - (0 if mutant == "no_mean" else s1) - xh * s2)
    dpos = dv.sum(0)
    if mutant == "dpos_no_cls":
        dpos = dpos.clone()
        dpos[0] = 0
    dgamma = (dy if mutant == "dgamma_dy" else dy * xh).sum((0, 1))
    return dict(dpatch=dv[:, 1:].reshape(B * (ntok - 1), D), dpos=dpos, dgamma=dgamma, dbeta=dy.sum((0, 1)),
                _=dict(v=v, mean=mean, d=d, var=var, rstd=rstd, xh=xh, dy=dy, gv=gv, s1=s1, s2=s2, dv=dv))


def embed_bwd_bounds(ref, gamma, B, ntok, D):
    """Per-element bounds of the four outputs from the module docstring's rules, along the kernel's steps (fp64 intermediates of embed_bwd_ref)."""
    t = ref["_"]
    v, mean, d, var, rstd, xh, dy, gv, s1, s2, dv = (t[k].abs() for k in ("v", "mean", "d", "var", "rstd", "xh", "dy", "gv", "s1", "s2", "dv"))
    m = lambda x: x.mean(-1, keepdim=True)                   # noqa: E731
    ev = U * v                                               # v = base + pos
    em = D * U * m(v) + m(ev) + U * mean                     # row mean: a sum of D terms, then the division
    ed = ev + em + U * d                                     # d = v - mean
    evar = m(2 * d * ed) + (D + 3) * U * var                 # sum of D squares (each d^2: 2 |d| ed + u d^2), the division, + eps
    rr = evar / (2 * (var + EPS)) + 4 * U                    # relative error of rstd
    exh = ed * rstd + xh * (rr + U)                          # xhat = d rstd
    eg = U * gv                                              # g = dy gamma
    es1 = D * U * m(gv) + m(eg) + U * s1
    tt = gv * xh
    et = gv * exh + xh * eg + U * tt
    es2 = D * U * m(tt) + m(et) + U * s2
    xs = xh * s2
    einner = eg + es1 + xh * es2 + s2 * exh + U * xs + 2 * U * (gv + s1 + xs)     # g - s1 - xhat s2
    edv = rstd * einner + dv * (rr + U)                      # dv = rstd (...)
    term = dy * xh
    eterm = dy * exh + U * term
    n = B * ntok
    return dict(dpatch=(edv * (1 + 2.0 ** -8) + 2.0 ** -8 * dv)[:, 1:].reshape(B * (ntok - 1), D),
                dpos=edv.sum(0) + B * U * dv.sum(0),
                dgamma=eterm.sum((0, 1)) + n * U * term.sum((0, 1)),
                dbeta=n * U * dy.sum((0, 1)) + torch.zeros(D, dtype=F64))


def worst_ratio(got, ref, bound):
    """max err / bound and its flat index; a zero bound passes only with a zero error"""
    err = (got.to(F64).reshape(ref.shape) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r, i = ratio.reshape(-1).max(0)
    return r.item(), int(i)

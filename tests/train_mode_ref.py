"""Plain fp64 restatements of the TRAIN-MODE paths (dropout sites of the frozen encoder, of the fine-tuning nodes and of the pooling head) for
tests/test_train_mode_parity_gpu.py and tools/train_mode_bounds.py.  A helper module, not a test; no kernel runs here.  tests/train_nodes_ref.py builds on it
(the pre-LN body, the layer mix, the branch stack and the image tower, for tests/test_train_nodes_parity_gpu.py).

Every function is torch autograd in fp64 on the CPU, one utterance at a time (it never sees a neighbour).  Masks come in as TENSORS that already hold
keep / (1 - p), so a mutant is just another mask (or one of the few `wiring` switches).  The keep bits themselves are the restatements of
tests/test_dropout_gpu.py (_keep, _keep_rows, _keep_attn, _keep_attn_packed); the hash is not restated here.

model=True turns the same graph into the CPU MODEL OF A CORRECT IMPLEMENTATION: every tensor the product stores as bf16 (fp32 where it stores fp32) passes
through a rounding node that rounds the VALUE in the forward and the GRADIENT in the backward -- the gradient of a stored tensor is exactly the bf16 tensor
the product's backward stores for it.  The nodes (named by the product's tensor in the comments below):
    rs   stored in the forward AND its gradient stored in the backward          (qkv/dqkv, att/datt, y1/dy1r, x1/dx1, hm/dhm, y2/dy2r, out/dh ...)
    rf   stored / rounded in the forward only                                    (the probabilities, 16-bit weights)
    rb   only the gradient is stored                                             (dS of the attention backward, dh_in, dz, dx6)
What the model leaves out (covered by the factor 4 of the bound): fp32 accumulation order, the polynomial GELU / v_exp_f32, the attention backward's
delta = dO . O taken from the stored bf16 output instead of sum P dP, and the second rounding where the product adds two bf16 gradients."""
import numpy as np
import torch
import torch.nn.functional as F

from test_dropout_gpu import _keep, _keep_attn, _keep_attn_packed, _keep_rows   # noqa: F401  (re-exported for the test and the tool)

F64 = torch.float64
BF = torch.bfloat16
LAYER_NAMES = "q_w q_b k_w k_b v_w v_b o_w o_b ln1_w ln1_b fc1_w fc1_b fc2_w fc2_b ln2_w ln2_b".split()
FRONT_FEATURES_XOR, FRONT_HIDDEN_XOR = 0x2545F491, 0x61C88647          # train_front.py: the two site seeds of the front-end node
NODE_SEED_MUL, NODE_SEED_ADD = 2654435761, 97                          # speech_encoder_plus.py: the layer node's seed from the forward's seed


def r16(t):
    """bf16 store of an fp64 value, back in fp64"""
    return t.to(torch.float32).to(BF).to(F64)


def r32(t):
    return t.to(torch.float32).to(F64)


def bound_of(model_err):
    return 4.0 * model_err + 1e-3


def row_metric(got, ref):
    """per row (all leading dims): max|got - ref| / max|ref| over the last dim; a row whose reference is all zero must be zero exactly (metric 0) or counts as inf."""
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    err = (got - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def tensor_metric(got, ref):
    """parameter-shaped gradients: max|got - ref| / max|ref| over the whole tensor"""
    return row_metric(got.reshape(-1), ref.reshape(-1)).item()


# ================================================================================================ rounding and mask nodes
class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return fwd(x) if fwd is not None else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (ctx.bwd(g) if ctx.bwd is not None else g), None, None


class _Mask(torch.autograd.Function):
    """x * m in the forward, g * mb in the backward (mb is m unless a MUTANT re-applies another mask)."""
    @staticmethod
    def forward(ctx, x, m, mb):
        ctx.save_for_backward(mb)
        return x * m

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class _GeluStored(torch.autograd.Function):
    """gelu(u) of the accumulator in the forward; the backward recomputes u and STORES it in bf16 before gelu' (train_hubert.py: `u = ops.gemm(x1, W1, b1)`)."""
    @staticmethod
    def forward(ctx, u, rnd):
        ctx.save_for_backward(rnd(u) if rnd is not None else u)
        return F.gelu(u)

    @staticmethod
    def backward(ctx, g):
        u, = ctx.saved_tensors
        return g * (0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5), None


class _SoftmaxDrop(torch.autograd.Function):
    """(p, pp) = (softmax(s), p * m).  from_dropped: MUTANT -- the softmax backward taken with the DROPPED probabilities, ds = pp (dp - sum pp dp)."""
    @staticmethod
    def forward(ctx, s, m, from_dropped):
        p = torch.softmax(s, -1)
        ctx.save_for_backward(p, m)
        ctx.from_dropped = from_dropped
        return p, p * m

    @staticmethod
    def backward(ctx, gp, gpp):
        p, m = ctx.saved_tensors
        dp = gp + gpp * m
        q = p * m if ctx.from_dropped else p
        return q * (dp - (q * dp).sum(-1, keepdim=True)), None, None


class Rounder:
    """model=False: every node is the identity.  fmt: the storage format of the 16-bit tensors (r16) or of an fp32 path (r32)."""

    def __init__(self, model, fmt=r16):
        self.model, self.fmt = bool(model), fmt

    def rs(self, x, fmt=None):
        return _Round.apply(x, fmt or self.fmt, fmt or self.fmt) if self.model else x

    def rf(self, x, fmt=None):
        return _Round.apply(x, fmt or self.fmt, None) if self.model else x

    def rb(self, x, fmt=None):
        return _Round.apply(x, None, fmt or self.fmt) if self.model else x

    def w16(self, w):
        """a 16-bit weight operand (the fp32 master copy keeps the gradient)"""
        return self.rf(w, r16)

    def gelu(self, u):
        return _GeluStored.apply(u, r16 if self.model else None)


def mask(x, m, mb=None):
    return x if m is None else _Mask.apply(x, m, m if mb is None else mb)


# ================================================================================================ seeds and keep masks
def site_seeds(seed, count):
    """`count` site seeds from one forward's seed, in forward order: the LCG of train_hubert._site_seeds / hubert.py next_seed."""
    s0, out = int(seed) & 0x7fffffff, []
    for _ in range(count):
        s0 = (s0 * 1103515245 + 12345) & 0x7fffffff
        out.append(s0)
    return out


def elem_mask(seed, row0, rows, cols, p, rescale=True):
    """sc_dropout_bf16 on rows [row0, row0 + rows) of a [., cols] tensor: element index row * cols + col.  -> fp64 [rows, cols] holding keep / (1 - p)."""
    if p <= 0:
        return None
    k = _keep(seed, np.arange(row0 * cols, (row0 + rows) * cols), p).view(rows, cols).to(F64)
    return k / (1 - p) if rescale else k


def attn_mask(seed, layout, b, H, n, p, rescale=True, packed_base=None, packed_stride=None):
    """The probability mask of utterance b, queries / keys < n.  layout = dict(B, Tp) (uniform rows) or dict(row_off, Tmax) (packed rows).
    packed_base / packed_stride: MUTANTS -- another first row / another pair stride of the packed mask.  -> fp64 [H, n, n]"""
    if p <= 0:
        return None
    if "row_off" in layout:
        base = layout["row_off"][b] if packed_base is None else packed_base
        stride = (layout["Tmax"] + 1) // 2 if packed_stride is None else packed_stride
        ids = (base + np.arange(n))[None, :] * H + np.arange(H)[:, None]
        k = _keep_rows(seed, ids.reshape(-1), n, stride, p).view(H, n, n)
        if packed_base is None and packed_stride is None:
            assert torch.equal(k, _keep_attn_packed(seed, base, H, n, layout["Tmax"], p))
    else:
        Tp = layout["Tp"]
        ids = ((b * H + np.arange(H))[:, None] * Tp + np.arange(n)[None, :]).reshape(-1)
        k = _keep_rows(seed, ids, n, (Tp + 1) // 2, p).view(H, n, n)
    k = k.to(F64)
    return k / (1 - p) if rescale else k


def first_row(layout, b):
    return layout["row_off"][b] if "row_off" in layout else b * layout["Tp"]


def layer_masks(seeds4, layout, b, n, d, ffn, H, rates, **attn_kw):
    """The four masks of one post-LN layer for the first n rows of utterance b: dict(attn, d1, d2, d3), None where the rate is 0."""
    sa, s1, s2, s3 = seeds4
    r0 = first_row(layout, b)
    return dict(attn=attn_mask(sa, layout, b, H, n, rates["attention"], **attn_kw), d1=elem_mask(s1, r0, n, d, rates["hidden"]),
                d2=elem_mask(s2, r0, n, ffn, rates["activation"]), d3=elem_mask(s3, r0, n, d, rates["hidden"]))


# ================================================================================================ the fairseq post-LN layer
def post_ln_layer(x, params, lens, masks=None, model=False, eps=1e-5, bwd_masks=None, wiring=(), fused_ln=False, heads=None):
    """x fp64 [B, T, d]; params: the 16 tensors of train_hubert.layer_params (fp64); lens: valid keys per utterance (keys >= lens[b] are masked, every query
    row is computed); masks: dict(attn [B, H, T, T], d1 [B, T, d], d2 [B, T, ffn], d3 [B, T, d]) of keep / (1 - p), None = no dropout at that site.
    x = LN(x + dropout1(attn(x)));  x = LN(x + dropout3(fc2(dropout2(gelu(fc1 x)))))    (heads: None = head_dim 64).  Stack it by feeding the output back in.
    bwd_masks: MUTANT -- masks the backward applies instead.  wiring: MUTANTS -- "residual_masked" (the mask also on the residual path), "res2_from_h" (the second
    residual taken from the layer's input instead of LayerNorm 1's output: tests/infer_nodes_ref.py).
    fused_ln: the frozen encoder at d = 768 (sc_dropout_add_layernorm_bf16): residual + dropout(x) is not stored before the LayerNorm."""
    R = Rounder(model)
    masks = masks or {}
    bm = bwd_masks or {}
    qw, qb, kw, kb, vw, vb, ow, ob, g1, b1n, w1, b1, w2, b2, g2, b2n = params
    B, T, d = x.shape
    H = heads or d // 64
    hd = d // H
    wqkv = torch.cat([R.w16(qw), R.w16(kw), R.w16(vw)], 0)
    qkv = R.rs(x @ wqkv.t() + torch.cat([qb, kb, vb]))                                 # qkv (forward) / dqkv (backward)
    q, k, v = [t.view(B, T, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    s = R.rb((q @ k.transpose(-1, -2)) * hd ** -0.5)                                    # dS: the bf16 score gradient of the attention backward
    dead = torch.arange(T)[None, :] >= torch.as_tensor(lens).view(B, 1)
    pr = torch.softmax(s.masked_fill(dead[:, None, None, :], float("-inf")), -1)
    pd = R.rf(mask(pr, masks.get("attn"), bm.get("attn")))                             # the probabilities in the operand format, AFTER mask and rescale
    att = R.rs((pd @ v).transpose(1, 2).reshape(B, T, d))                               # att / datt
    sub = "residual_masked" in wiring
    o = att @ R.w16(ow).t() + ob
    if masks.get("d1") is None:
        y1 = o + x                                                                      # the residual rides in the GEMM's epilogue
    else:
        o = R.rs(o)                                                                     # out_proj's bf16 output / dy1 (the masked gradient)
        y1 = mask(o + x, masks["d1"], bm.get("d1")) if sub else mask(o, masks["d1"], bm.get("d1")) + x
    if not fused_ln:
        y1 = R.rs(y1)                                                                   # y1 / dy1r (LayerNorm 1's input and its gradient)
    x1 = R.rs(F.layer_norm(y1, (d,), g1, b1n, eps))                                     # x1 / dx1
    hm = R.rs(R.gelu(x1 @ R.w16(w1).t() + b1))                                          # hm / du's input (u itself is recomputed and stored in the backward: du)
    if masks.get("d2") is not None:
        hm = R.rs(mask(hm, masks["d2"], bm.get("d2")))                                  # hm after dropout2 (in place) / dhm
    f = hm @ R.w16(w2).t() + b2
    if masks.get("d3") is None:
        y2 = f + (x if "res2_from_h" in wiring else x1)
    else:
        f = R.rs(f)                                                                     # fc2's bf16 output / dy2 (the masked gradient)
        y2 = mask(f + x1, masks["d3"], bm.get("d3")) if sub else mask(f, masks["d3"], bm.get("d3")) + x1
    if not fused_ln:
        y2 = R.rs(y2)                                                                   # y2 / dy2r
    return R.rs(F.layer_norm(y2, (d,), g2, b2n, eps))                                   # the layer's output / the gradient it receives


def layer_node(xs, layers, lens, masks, dhidden, train, model=False, bwd_masks=None, wiring=(), pre_ln=False, act="gelu"):
    """train_hubert.HubertLayersTrainFn over a list of utterances: xs[b] fp64 [T_b, d]; layers[li]: 16 fp64 tensors; lens[b] valid keys; masks[li][b] (layer_masks,
    or None: no dropout); dhidden[li][b] fp64 [T_b, d]: the gradient of hidden state li.  Any number of layers, any `train` tuple (a frozen layer still passes the
    gradient down).  pre_ln: the pre-LN body on an fp32 stream (train_nodes_ref.pre_ln_layer, activation `act`); there the sum of the stream gradient and the direct
    gradient of a hidden state is stored in bf16 once more (sc_axpy_bf16).  wiring: the bodies' MUTANTS plus "no_direct" (the direct gradient of hidden[li - 1]
    not added).  -> dict(hidden[li][b], dh_in[b], grads[li] = 16 tensors or None where train[li] is False)."""
    R = Rounder(model)
    n = len(layers)
    if pre_ln:
        from train_nodes_ref import pre_ln_layer
    P = [[p.detach().clone().requires_grad_(True) for p in lp] for lp in layers]
    leaves = [x.detach().clone().requires_grad_(True) for x in xs]
    hidden = [[None] * len(xs) for _ in range(n)]
    loss = 0.0
    for b, x in enumerate(leaves):
        h = R.rb(x)[None]                                                               # dh_in: bf16
        for li in range(n):
            if pre_ln:
                out = R.rb(pre_ln_layer(h, P[li], [lens[b]], masks[li][b], model, act, wiring=wiring))      # the join with the direct gradient, stored in bf16
            else:
                out = post_ln_layer(h, P[li], [lens[b]], masks[li][b], model, bwd_masks=None if bwd_masks is None else bwd_masks[li][b], wiring=wiring)
            hidden[li][b] = out[0]
            if li == n - 1 or "no_direct" not in wiring:
                loss = loss + (out[0] * dhidden[li][b]).sum()
            h = R.rb(out)                                                               # dh of the layer above, stored before the direct gradient is added
    flat = [p for li in range(n) if train[li] for p in P[li]]
    got = torch.autograd.grad(loss, leaves + flat, allow_unused=True)
    dh_in, rest = list(got[:len(xs)]), list(got[len(xs):])
    grads = []
    for li in range(n):
        grads.append([rest.pop(0) for _ in range(16)] if train[li] else None)
    return dict(hidden=[[h.detach() for h in hs] for hs in hidden], dh_in=dh_in, grads=grads)


# ================================================================================================ the front stretch (conv stack output -> hidden state 0)
def fold_weight_norm(g, v):
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def front_stretch(x6, valid, params, masks, G, Kw, model=False, grad_mult=1.0, bwd_masks=None, eps=1e-5, node=True):
    """x6 fp64 [rows, C]: ONE utterance's own conv-stack output, the same tensor the node sees; rows >= valid are masked in front of the positional conv.
    params = dict(flw, flb, pw, pb, pg, pv, pbias, elw, elb) (feature LayerNorm, projection, weight-normalised positional conv, encoder LayerNorm);
    masks = dict(features, hidden) of keep / (1 - p) [rows, d] or None.  The conv stack below has no dropout.
    feats = LN(x6) -> xp = dropout_input(proj(feats)) -> s = mask(xp) + gelu(pos_conv(mask(xp)) + bias) -> h0 = dropout(LN(s)).
    node: the training node (sc_posconv_finish_train stores u and s); False: the frozen engine's positional conv, which stores the conv slab and the result only.
    bwd_masks: MUTANT -- the masks the backward re-applies."""
    R = Rounder(model)
    masks = masks or {}
    bm = bwd_masks or {}
    rows, C = x6.shape
    p = params
    d = p["pw"].shape[0]
    x6 = R.rb(x6)                                                                       # dx6: the bf16 gradient handed to the conv stack ...
    if grad_mult != 1.0:
        x6 = R.rb(_Round.apply(x6, None, lambda g: g * grad_mult))                      # ... scaled by feature_grad_mult after it was stored once
    feats = R.rs(F.layer_norm(x6, (C,), p["flw"], p["flb"], eps))                       # feats / dfeats
    xp = R.rs(feats @ R.w16(p["pw"]).t() + p["pb"])                                     # xp / dxp after the features mask
    if masks.get("features") is not None:
        xp = R.rs(mask(xp, masks["features"], bm.get("features")))                      # xp after dropout_input (in place) / dxp before the mask
    live = (torch.arange(rows) < valid).to(F64)[:, None]
    xm = xp * live
    wfold = R.w16(fold_weight_norm(p["pg"], p["pv"]))                                   # the folded bf16 conv operand
    conv = R.rf(F.conv1d(xm.t()[None], wfold, None, padding=Kw // 2, groups=G)[0, :, :rows].t())      # the conv slab, bf16
    u = conv + p["pbias"]
    if node:
        u = R.rs(u)                                                                     # u (pre-activation, stored) / du
    s = xm + F.gelu(u)
    if node:
        s = R.rs(s)                                                                     # s / ds
    h0 = R.rs(F.layer_norm(s, (d,), p["elw"], p["elb"], eps))                           # h0 / the masked dh0
    if masks.get("hidden") is not None:
        h0 = R.rs(mask(h0, masks["hidden"], bm.get("hidden")))                          # hidden state 0 IS the dropped tensor
    return h0


def front_masks(seed_features, seed_hidden, layout, b, n, d, rates, rescale=True):
    r0 = first_row(layout, b)
    return dict(features=elem_mask(seed_features, r0, n, d, rates["features"], rescale), hidden=elem_mask(seed_hidden, r0, n, d, rates["hidden"], rescale))


# ================================================================================================ the pooling head
def pool_head(x, cls, u, beta, lens, NQ, H, keep, p, hidden=None, alpha=None, normalize=False, model=False, from_dropped=False, dalpha_without_ds=False):
    """`_pool_reference` of tests/test_train_kernels_gpu.py in fp64 with the layer mix in front of it.
    x fp64 [B, T, D]: the frames the kernels read (bf16 values).  With hidden [n, B, T, D] and alpha [n] (softmax weights) the frames are the mix
    sum_n alpha_n [LN](hidden_n) stored as bf16: x must hold exactly that store, and the gradient reaches alpha THROUGH it (straight-through), so d alpha comes
    from autograd.  cls [NQ, D], u [R, D], beta [R], R = NQ * H; scores z.u_r + beta_r over [CLS ; frames < lens[b]], softmax, dropout (keep [B, R, NQ + T] of
    0 / 1, rescaled by 1 / (1 - p) here), weighted sums.  An utterance with lens[b] = 0 pools the CLS keys alone.
    model=True: everything the kernels store is fp32 (scores, p, pp, xbar and every gradient) except dz, which is bf16.
    MUTANTS: from_dropped (ds from the dropped probabilities), dalpha_without_ds (d alpha from dz without its ds . u term).
    -> (p [B, R, NQ + T], pp, xbar [B, R, D])"""
    R32 = Rounder(model, r32)
    B, T, D = x.shape
    Rr = NQ * H
    x = _Round.apply(x, None, r16) if model else x                                      # dz: bf16 (sc_cls_pool_dz)
    xv = xs = x
    if hidden is not None:
        hsrc = F.layer_norm(hidden, (D,)) if normalize else hidden
        mix = torch.einsum("bn,nbtd->btd", alpha if alpha.dim() == 2 else alpha.expand(B, -1), hsrc)      # alpha [B, n]: d alpha per utterance, as the kernel writes it
        thru = mix - mix.detach()                                                       # value 0, gradient d mix
        xv = x + thru
        xs = x if dalpha_without_ds else x + thru
    zv = torch.cat([cls.unsqueeze(0).expand(B, NQ, D), xv], 1)                          # [B, NQ + T, D]
    zs = torch.cat([cls.unsqueeze(0).expand(B, NQ, D), xs], 1)
    s = R32.rs(torch.einsum("bkd,rd->brk", zs, u) + beta.view(1, Rr, 1))                # scores (fp32 inputs of the kernel) / ds
    valid = torch.arange(NQ + T).view(1, 1, -1) < (torch.as_tensor(lens).view(B, 1, 1) + NQ)
    m = torch.ones(B, Rr, NQ + T, dtype=F64) if keep is None else keep.to(F64) / (1 - p)
    pr, pp = _SoftmaxDrop.apply(s.masked_fill(~valid, float("-inf")), m, from_dropped)
    pr, pp = R32.rf(pr), R32.rf(pp)                                                     # p, pp: fp32
    return pr, pp, R32.rs(torch.einsum("brk,bkd->brd", pp, zv))                         # xbar / dzbar: fp32


def pool_keep(seed, B, R, n_keys, stride, p, lens=None, NQ=0, share_rows=False):
    """The pooling head's mask: element index (b * R + r) * stride + key, stride = NQ + T in the product.  MUTANTS: lens (stride NQ + lens[b]), share_rows (no r term)."""
    if p <= 0:
        return None
    out = torch.empty(B, R, n_keys)
    for b in range(B):
        st = stride if lens is None else NQ + int(lens[b])
        for r in range(R):
            out[b, r] = _keep(seed, (b * R + (0 if share_rows else r)) * st + np.arange(n_keys), p)
    return out


# ================================================================================================ the frozen encoder in train mode
def conv_stack(enc, wav_b, length, model=False, conv0_fused=True, wave_len=None, gn_frames=None):
    """The conv feature extractor of module.hubert.HubertModel `enc` on ONE utterance's own zero-padded wave [lmax] -> fp64 [T, C] (GroupNorm statistics over
    the padded length, as the engine computes them).  model=True: bf16 conv 1-6 weights and a bf16 store of every layer's output; a "layer_norm" extractor also
    stores the conv output in bf16 in front of its LayerNorm (layer 0 only when conv0_fused is False: the fused kernel keeps it in registers).
    MUTANTS: wave_len -- the wave LayerNorm (cfg.normalize) over this many samples instead of the utterance's own `length`; gn_frames -- the GroupNorm statistics
    over the first gn_frames frames (the utterance's own) instead of all frames of the padded length."""
    cfg = enc.cfg
    st = r16 if model else (lambda t: t)
    w16 = (lambda t: r16(t.detach())) if model else (lambda t: t.detach().double())
    d64 = lambda t: None if t is None else t.detach().double()      # noqa: E731
    x = wav_b.double().clone()
    if cfg.normalize:
        n = length if wave_len is None else wave_len
        x[:n] = F.layer_norm(x[:n], (n,))
        x[length:] = 0                                          # the padding stays zero (sc_wave_layernorm writes zeros there)
    y = None
    for i, blk in enumerate(enc.feature_extractor.conv_layers):
        c = getattr(blk, "0")
        y = F.conv1d(x[None, None] if i == 0 else y, d64(c.weight) if i == 0 else w16(c.weight), d64(getattr(c, "bias", None)), stride=cfg.conv_layers[i][2])
        if cfg.extractor_mode == "layer_norm":
            ln = getattr(getattr(blk, "2"), "1")
            if i > 0 or not conv0_fused:
                y = st(y)
            y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), d64(ln.weight), d64(ln.bias), 1e-5).transpose(1, 2)
        elif i == 0:
            gn = getattr(blk, "2")
            if gn_frames is None:
                y = F.group_norm(y, y.shape[1], d64(gn.weight), d64(gn.bias), 1e-5)
            else:
                own = y[..., :gn_frames]
                y = (y - own.mean(-1, keepdim=True)) / (own.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt() * d64(gn.weight)[None, :, None] + d64(gn.bias)[None, :, None]
        y = st(F.gelu(y))
    return y[0].t().contiguous()


def front_params_of(enc):
    d64 = lambda t: t.detach().double()      # noqa: E731
    pc = getattr(enc.encoder.pos_conv, "0")
    return dict(flw=d64(enc.layer_norm.weight), flb=d64(enc.layer_norm.bias), pw=d64(enc.post_extract_proj.weight), pb=d64(enc.post_extract_proj.bias),
                pg=d64(pc.weight_g), pv=d64(pc.weight_v), pbias=d64(pc.bias), elw=d64(enc.encoder.layer_norm.weight), elb=d64(enc.encoder.layer_norm.bias))


def layer_params_of(lyr):
    from speechclip_amd.train_hubert import layer_params
    return [p.detach().double() for p in layer_params(lyr)]


def frozen_seed_plan(seed, n_layers, rates, four_always=False):
    """Site seeds in the order hubert.py draws them: features, hidden state 0 (each only when its rate > 0), then per layer attention, dropout1,
    [dropout2 only when the activation rate > 0], dropout3.  four_always: MUTANT -- four seeds per layer whatever the activation rate.
    -> (features seed | None, hidden seed | None, [(sa, s1, s2 | None, s3)] per layer)"""
    per = 4 if (rates["activation"] > 0 or four_always) else 3
    seeds = site_seeds(seed, 2 + per * n_layers)
    sf = seeds.pop(0) if rates["features"] > 0 else None
    sh = seeds.pop(0) if rates["hidden"] > 0 else None
    layers = []
    for _ in range(n_layers):
        sa, s1 = seeds.pop(0), seeds.pop(0)
        s2 = seeds.pop(0) if per == 4 else None
        layers.append((sa, s1, s2, seeds.pop(0)))
    return sf, sh, layers


def frozen_encoder_train(enc, wav, lens, seed, rates, pack=None, model=False, plan=None, wiring=(), swap13=False):
    """The whole post-LN encoder forward in train mode from the product's own weights (`enc`: module.hubert.HubertModel on the CPU): every hidden state on the
    valid frames of every utterance.  wav [B, lmax] zero-padded, lens: samples; rates: enc.dropout_rates(); pack: enc.packed_geometry(...) or None (rows b * Tp + t).
    plan / swap13 / wiring: MUTANTS (another seed plan, dropout1 and dropout3 seeds swapped, post_ln_layer's wiring).
    -> hidden[b] = list of n_layers + 1 fp64 [valid_b, d]"""
    cfg = enc.cfg
    assert not cfg.layer_norm_first
    B, lmax = wav.shape
    T0, T, P0, Tp = enc.frame_geometry(lmax)
    valid = enc.valid_frames(lens, lmax, T)
    layout = dict(row_off=pack["row_off"], Tmax=pack["rows_max"]) if pack is not None else dict(B=B, Tp=Tp)
    d, ffn, H = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_attention_heads
    sf, sh, lseeds = plan or frozen_seed_plan(seed, cfg.encoder_layers, rates)
    fp = front_params_of(enc)
    lp = [layer_params_of(l) for l in enc.encoder.layers]
    out = []
    with torch.no_grad():
        for b in range(B):
            n = valid[b]
            x6 = conv_stack(enc, wav[b], int(lens[b]), model)[:n]
            fm = front_masks(sf or 0, sh or 0, layout, b, n, d, dict(features=rates["features"] if sf is not None else 0.0, hidden=rates["hidden"] if sh is not None else 0.0))
            h = front_stretch(x6, n, fp, fm, cfg.conv_pos_groups, cfg.conv_pos, model, node=False)
            hs = [h]
            for li, (sa, s1, s2, s3) in enumerate(lseeds):
                if swap13:
                    s1, s3 = s3, s1
                lr = dict(rates, activation=rates["activation"] if s2 is not None else 0.0)
                m = layer_masks((sa, s1, s2 or 0, s3), layout, b, n, d, ffn, H, lr)
                h = post_ln_layer(h[None], lp[li], [n], m, model, wiring=wiring, fused_ln=(d == 768))[0]
                hs.append(h)
            out.append(hs)
    return out

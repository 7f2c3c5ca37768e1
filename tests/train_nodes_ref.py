"""Plain fp64 restatements of the TRAINING NODES that chain the kernels (train_hubert.py pre-LN bodies and WeightedSumTrainFn, train_branch.BranchStackTrainFn)
for tests/test_train_nodes_parity_gpu.py and tools/train_node_bounds.py.  A helper module, not a test; no kernel runs here.

The conventions are those of tests/train_mode_ref.py, whose Rounder / mask / metrics / bound_of this module imports: fp64 torch autograd on the CPU, one utterance
at a time; masks come in as tensors of keep / (1 - p); model=True puts a rounding node wherever the product stores bf16 (fp32 where it stores fp32); a MUTANT is one
of the `wiring` switches named in each docstring.  train_mode_ref.layer_node(..., pre_ln=True) stacks `pre_ln_layer` below.

One step the older model leaves to the factor 4 of the bound is modelled here, because the zero rule on the k-bias slices sees nothing else: without dropout the
attention backwards take the softmax's row term from the stored bf16 output, delta = dO . O (`_AttnStored`)."""
import numpy as np
import torch
import torch.nn.functional as F

from train_mode_ref import F64, Rounder, _keep_rows, _Round, attn_mask, elem_mask, mask, post_ln_layer, r16, r32   # noqa: F401

BRANCH_NAMES = "in_w in_b out_w out_b n1_w n1_b l1_w l1_b l2_w l2_b n2_w n2_b".split()


# ================================================================================================ nodes
class _LNStored(torch.autograd.Function):
    """LayerNorm whose BACKWARD recomputes the row statistics from the copy of its input the product saved: rnd = r16 for the bf16 copies of the fp32 stream
    (h16, xmid16), None where the product keeps the fp32 rows.  w / b None: the affine-free form.  from_out: MUTANT -- the backward is fed the LayerNorm's own
    (stored) OUTPUT in place of the stream copy."""
    @staticmethod
    def forward(ctx, x, w, b, eps, rnd, from_out):
        y = F.layer_norm(x, (x.shape[-1],), w, b, eps)
        src = y if from_out else x
        ctx.x = (rnd(src) if rnd is not None else src).detach()
        ctx.w, ctx.eps = None if w is None else w.detach(), eps
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.x, ctx.w
        d = x - x.mean(-1, keepdim=True)
        rstd = (d.pow(2).mean(-1, keepdim=True) + ctx.eps).rsqrt()
        xh = d * rstd
        gw = g if w is None else g * w
        dx = rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))
        lead = tuple(range(g.dim() - 1))
        return dx, None if w is None else (g * xh).sum(lead), None if w is None else g.sum(lead), None, None, None


class _ActStored(torch.autograd.Function):
    """act(u) of the accumulator in the forward; the backward recomputes u, STORES it in bf16 (rnd) and applies the derivative of `bwd` ("gelu": erf-GELU,
    "quickgelu": u sigmoid(1.702 u)).  bwd != fwd: MUTANT -- the other activation's derivative."""
    @staticmethod
    def forward(ctx, u, rnd, fwd, bwd):
        ctx.save_for_backward(rnd(u) if rnd is not None else u)
        ctx.bwd = bwd
        return F.gelu(u) if fwd == "gelu" else u * torch.sigmoid(1.702 * u)

    @staticmethod
    def backward(ctx, g):
        u, = ctx.saved_tensors
        if ctx.bwd == "gelu":
            return g * (0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5), None, None, None
        s = torch.sigmoid(1.702 * u)
        return g * (s + 1.702 * u * s * (1 - s)), None, None, None


def _cut(x):
    """the value without its gradient path (MUTANTS that drop a residual join)"""
    return x.detach()


class _AttnStored(torch.autograd.Function):
    """o = bf16(bf16(softmax(s) m) v) per head from the masked scores s [..., Tq, Tk], v [..., Tk, hd], m = keep / (1 - p) or None.  rnd = r16 (the model) stores
    the probabilities in the operand format, the output and its gradient in bf16.  delta_stored: the backward takes the softmax's row term from the STORED output,
    delta = dO . O, as the attention backwards do without dropout (csrc/attention_bwd.hip: DELTA_PDP false), instead of sum_k P_k dP_k; in fp64 the two agree."""
    @staticmethod
    def forward(ctx, s, v, m, rnd, delta_stored):
        p = torch.softmax(s, -1)
        pm = p if m is None else p * m
        pd = rnd(pm) if rnd is not None else pm
        o = pd @ v
        o = rnd(o) if rnd is not None else o
        ctx.save_for_backward(p, pm, pd, v, o)
        ctx.m, ctx.rnd, ctx.delta_stored = m, rnd, delta_stored
        return o

    @staticmethod
    def backward(ctx, g):
        p, pm, pd, v, o = ctx.saved_tensors
        g = ctx.rnd(g) if ctx.rnd is not None else g                                    # datt, bf16
        dpd = g @ v.transpose(-1, -2)
        delta = (g * o).sum(-1, keepdim=True) if ctx.delta_stored else (pm * dpd).sum(-1, keepdim=True)      # from the fp32 P: cancels exactly
        return p * ((dpd if ctx.m is None else dpd * ctx.m) - delta), pd.transpose(-1, -2) @ g, None, None, None


def _attention(R, qkv, B, T, H, lens, m_attn, delta_stored=True, causal=False):
    """q | k | v [B, T, 3d] -> att [B, T, d]: keys >= lens[b] masked, every query computed; the rounding points of train_mode_ref.post_ln_layer.
    causal: query i also masks the keys > i (the text tower).  The 16-bit stores take the Rounder's format (bf16, or IEEE half for the frozen pre-LN encoder)."""
    d = qkv.shape[-1] // 3
    hd = d // H
    q, k, v = [t.view(B, T, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1)]
    s = R.rb((q @ k.transpose(-1, -2)) * hd ** -0.5)                                    # dS: the bf16 score gradient of the attention backward
    dead = (torch.arange(T)[None, :] >= torch.as_tensor(lens).view(B, 1))[:, None, None, :]
    if causal:
        dead = dead | (torch.arange(T)[None, :] > torch.arange(T)[:, None] + (int(causal) - 1))          # causal = 2: MUTANT, key i + 1 admitted
    o = _AttnStored.apply(s.masked_fill(dead, float("-inf")), v, m_attn, R.fmt if R.model else None, delta_stored)      # P, att / datt
    return o.transpose(1, 2).reshape(B, T, d)


# ================================================================================================ the pre-LN layer body
def pre_ln_layer(x, params, lens, masks=None, model=False, act="gelu", eps=1e-5, wiring=(), heads=None, causal=False, fmt=r16):
    """train_hubert._layer_fwd_pre_ln / _layer_bwd_pre_ln.  x fp64 [B, T, d]: the fp32 residual stream; params: the 16 tensors of train_hubert.layer_params;
    lens: valid keys per utterance; masks: dict(attn, d1, d2, d3) of keep / (1 - p) or None (train_mode_ref.layer_masks); heads: None = d / 64.
        x += dropout1(out_proj(attn(LN1 x)));  x += dropout3(fc2(dropout2(act(fc1(LN2 x)))))
    The stream is stored in fp32; t1, q | k | v, the probabilities, att, t2, hm and the recomputed u in bf16.  Both LayerNorm backwards read the bf16 copy of the
    stream (h16, xmid16) and store a bf16 gradient; each residual join (sc_axpy_bf16) stores the sum in bf16 again.
    wiring (MUTANTS): "no_join_mid" / "no_join_h" (a residual join dropped: dxm without g / dh without dxm), "ln_from_out" (the LayerNorm backward fed t1 / t2),
    "act_bwd_swapped" (the other activation's derivative), "res_after_ln" (both residuals taken behind the LayerNorm: t1 / t2 instead of the stream).
    causal: the text tower's mask (query i sees keys <= i below lens[b]).  fmt: the format of every 16-bit store and weight operand -- r16, or the IEEE-half store of
    the frozen pre-LN encoder layers (tests/infer_nodes_ref.py); forward-only wirings of the inference references are documented there."""
    R = Rounder(model, fmt)
    masks = masks or {}
    qw, qb, kw, kb, vw, vb, ow, ob, g1, b1n, w1, b1, w2, b2, g2, b2n = params
    B, T, d = x.shape
    H = heads or d // 64
    rnd = getattr(fmt, "plain", fmt) if model else None          # what only a backward reads (saved copies) goes past a probing format
    ln = lambda t, w, b: _LNStored.apply(R.rb(t), w, b, eps, rnd, "ln_from_out" in wiring)      # noqa: E731   R.rb: the bf16 dx the LayerNorm backward stores
    other = "quickgelu" if act == "gelu" else "gelu"
    h = R.rb(R.rf(x, r32))                                                              # the stream (fp32) / dh after the join, bf16
    t1 = R.rs(ln(h, g1, b1n))                                                           # t1 / dt1
    wqkv = torch.cat([R.rf(qw), R.rf(kw), R.rf(vw)], 0)
    qkv = R.rs(t1 @ wqkv.t() + torch.cat([qb, kb, vb]))                                 # qkv / dqkv
    # the head_dim 64 backwards of train_hubert.py always take delta from the stored output, the head-dim kernel (heads given) whenever it does not drop
    att = _attention(R, qkv, B, T, H, lens, masks.get("attn"), heads is None or masks.get("attn") is None, causal)
    o = att @ R.rf(ow).t() + ob
    if masks.get("d1") is not None:
        o = R.rs(mask(R.rs(o), masks["d1"]))                                            # out_proj's bf16 output, dropped in place / dy1 = the masked dxm
    xmid = R.rb(R.rf((_cut(h) if "no_join_h" in wiring else t1 if "res_after_ln" in wiring else h) + o, r32))      # xmid (fp32) / dxm after the join, bf16
    t2 = R.rs(ln(xmid, g2, b2n))                                                        # t2 / dt2
    hm = R.rs(_ActStored.apply(t2 @ R.rf(w1).t() + b1, rnd, act, other if "act_bwd_swapped" in wiring else act))      # hm / dhm; u recomputed and stored
    if masks.get("d2") is not None:
        hm = R.rs(mask(hm, masks["d2"]))
    f = hm @ R.rf(w2).t() + b2
    if masks.get("d3") is not None:
        f = R.rs(mask(R.rs(f), masks["d3"]))                                            # fc2's bf16 output, dropped in place / dy2 = the masked g
    return R.rf((_cut(xmid) if "no_join_mid" in wiring else t2 if "res_after_ln" in wiring else xmid) + f, r32)      # the layer's output (fp32); its gradient arrives in bf16


# ================================================================================================ the layer mix
def weighted_sum_node(hidden, w, normalize, dmixed, model=False, wiring=()):
    """train_hubert.WeightedSumTrainFn: hidden fp64 [n, M, D] (bf16 values), w fp64 [n] (pre-softmax), dmixed fp64 [M, D] (bf16 values).
    mixed = bf16(sum_l softmax(w)_l [LN](hidden_l)); the backward stores softmax(w)_l dmixed in bf16 per state and, with `normalize`, runs the affine-free
    LayerNorm backward on the bf16 copy of the state, storing bf16 again.  wiring: "skip_ln_bwd" (MUTANT: that LayerNorm backward left out).
    -> dict(mixed [M, D], dhidden [n, M, D])"""
    R = Rounder(model)
    hl = hidden.detach().clone().requires_grad_(True)
    a = torch.softmax(w, 0)
    src = hl
    if normalize:
        if "skip_ln_bwd" in wiring:
            src = hl + (F.layer_norm(hl, (hl.shape[-1],), None, None, 1e-5) - hl).detach()
        else:
            src = _LNStored.apply(R.rb(hl), None, None, 1e-5, r16 if model else None, False)
    mixed = R.rf((a.view(-1, 1, 1) * R.rb(src)).sum(0))
    dh, = torch.autograd.grad((mixed * dmixed).sum(), [hl])
    return dict(mixed=mixed.detach(), dhidden=dh)


# ================================================================================================ the stacked parallel branch
def last_attn_mask(seed, b, H, Lq, n, p):
    """The probability mask of the last layer's ONE query per utterance (csrc/attention_hd.hip: drop_row = (b H + h) Tk + query with query 0 and Tk = Lq,
    ceil(Tk / 2) pairs per row).  -> fp64 [H, 1, n] of keep / (1 - p)"""
    if p <= 0:
        return None
    return _keep_rows(seed, (b * H + np.arange(H)) * Lq, n, (Lq + 1) // 2, p).view(H, 1, n).to(F64) / (1 - p)


def branch_masks(seeds, B, Lq, lens1, D, ffn, H, p, reuse_last=None):
    """masks[li][b] of BranchStackTrainFn for n = len(seeds) / 4 layers: the full layers' masks on the first lens1[b] rows of utterance b of the [B, Lq] layout
    (train_mode_ref.layer_masks), the last layer's on the B CLS rows (sc_dropout_f32: element b * cols + c).
    reuse_last = site 1 | 2 | 3: MUTANT -- that dropout site of the last layer draws from the previous site's seed."""
    if p <= 0:
        return None
    from train_mode_ref import layer_masks
    n = len(seeds) // 4
    rates = dict(hidden=p, attention=p, activation=p)
    out = []
    for li in range(n):
        s4 = list(seeds[4 * li:4 * li + 4])
        if li < n - 1:
            out.append([layer_masks(s4, dict(B=B, Tp=Lq), b, lens1[b], D, ffn, H, rates) for b in range(B)])
            continue
        if reuse_last is not None:
            s4[reuse_last] = s4[reuse_last - 1]
        out.append([dict(attn=last_attn_mask(s4[0], b, H, Lq, lens1[b], p), d1=elem_mask(s4[1], b, 1, D, p), d2=elem_mask(s4[2], b, 1, ffn, p),
                         d3=elem_mask(s4[3], b, 1, D, p)) for b in range(B)])
    return out


def _sixteen(p12, D):
    iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = p12
    return [iw[:D], ib[:D], iw[D:2 * D], ib[D:2 * D], iw[2 * D:], ib[2 * D:], ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b]


def branch_stack_node(cls, frames, audio_len, params, heads, pre_ln, masks, dout, model=False, eps=1e-5, wiring=()):
    """train_branch.BranchStackTrainFn.  cls fp64 [D]; frames[b] fp64 [T, D] (bf16 values); params: 12 tensors per layer (BRANCH_NAMES) then the final norm's
    weight and bias; masks: `branch_masks` or None; dout fp64 [B, D].
    Layers 0 .. n-2 on every row of [CLS; frames < len] with keys < len + 1 (post_ln_layer / pre_ln_layer); the last layer as train_branch.py's docstring states
    it: K | V of all rows and the CLS query stored in bf16, the attention output in bf16, then out-proj, LayerNorms, FFN and the final norm (eps 1e-5) on the CLS
    row in fp32.  The gradient of the rows is bf16: [dk | dv] W_kv stored for every row, row 0 stored again after dq W_q and the residual gradient joined it.
    wiring (MUTANTS): "klen_len" (keys < len), "no_dq" (the CLS row without dq W_q), "no_dy" (without the residual gradient), "no_dg1" (pre-LN: the all-row dg1
    not added into dn1w), plus pre_ln_layer's.
    -> dict(out [B, D], dcls [D], dframes[b] [len_b, D], grads: 12 n + 2 tensors)"""
    R = Rounder(model)
    H = heads
    n = (len(params) - 2) // 12
    D = cls.shape[0]
    hd = D // H
    P = [p.detach().clone().requires_grad_(True) for p in params]
    cl = cls.detach().clone().requires_grad_(True)
    fl = [f[:int(l)].detach().clone().requires_grad_(True) for f, l in zip(frames, audio_len)]
    rnd = r16 if model else None
    outs, loss = [], 0.0
    for b, f in enumerate(fl):
        nb = f.shape[0] + 1
        lens = [nb - 1 if "klen_len" in wiring else nb]
        c0 = cl if pre_ln else R.rf(cl)                                                 # post-LN rows are bf16
        h = R.rb(torch.cat([c0[None], f], 0))[None]                                    # [1, nb, D]; dcls / dframes come out of a bf16 buffer
        for li in range(n - 1):
            p16 = _sixteen(P[12 * li:12 * li + 12], D)
            m = None if masks is None else masks[li][b]
            if pre_ln:
                h = pre_ln_layer(h, p16, lens, m, model, eps=eps, wiring=wiring, heads=H)
            else:
                h = R.rb(post_ln_layer(h, p16, lens, m, model, eps, heads=H))
        # ---- the last layer
        iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = P[12 * (n - 1):12 * n]
        nfw, nfb = P[-2:]
        m = (masks[n - 1][b] if masks is not None else None) or {}
        h = R.rb(R.rf(h[0], r32) if pre_ln else h[0])                                   # row 0 is stored once more after dxc joined it
        xc = h[:1]
        if pre_ln:
            a_all = R.rs(_LNStored.apply(R.rb(h), _cut(n1w) if "no_dg1" in wiring else n1w, n1b, eps, rnd, "ln_from_out" in wiring))
            ac = R.rs(F.layer_norm(xc, (D,), n1w, n1b, eps), r32)
        else:
            a_all, ac = R.rb(h), xc
        kv = R.rs(a_all @ R.w16(iw[D:]).t() + ib[D:])                                   # k | v, bf16 / dk | dv
        qc = R.rs((_cut(ac) if "no_dq" in wiring else ac) @ iw[:D].t() + ib[:D])        # the CLS query, bf16 / dq
        q = qc.view(1, H, hd).transpose(0, 1)                                           # [H, 1, hd]
        k, v = [t.view(nb, H, hd).transpose(0, 1) for t in kv.split(D, dim=-1)]         # [H, nb, hd]
        s = R.rb((q @ k.transpose(-1, -2)) * hd ** -0.5)
        if lens[0] < nb:
            s = s.masked_fill(torch.arange(nb)[None, None, :] >= lens[0], float("-inf"))
        att = _AttnStored.apply(s, v, m.get("attn"), rnd, m.get("attn") is None).transpose(0, 1).reshape(1, D)      # att16 / datt16
        R32 = Rounder(model, r32)
        so = R32.rs(mask(att @ ow.t() + ob, m.get("d1")))
        y = R32.rs(so + (_cut(xc) if "no_dy" in wiring else xc))
        x1 = R32.rs(F.layer_norm(y, (D,), n2w, n2b, eps) if pre_ln else F.layer_norm(y, (D,), n1w, n1b, eps))
        hm = R32.rs(mask(F.gelu(R32.rs(x1 @ l1w.t() + l1b)), m.get("d2")))
        ff = R32.rs(mask(hm @ l2w.t() + l2b, m.get("d3")))
        y2 = R32.rs(ff + (y if pre_ln else x1))
        x2 = y2 if pre_ln else R32.rs(F.layer_norm(y2, (D,), n2w, n2b, eps))
        res = R32.rs(F.layer_norm(x2, (D,), nfw, nfb, 1e-5))
        outs.append(res[0])
        loss = loss + (res[0] * dout[b]).sum()
    got = torch.autograd.grad(loss, [cl] + fl + P)
    B = len(fl)
    return dict(out=torch.stack(outs).detach(), dcls=got[0], dframes=list(got[1:1 + B]), grads=list(got[1 + B:]))


# ================================================================================================ the image tower
class _MatmulStored16(torch.autograd.Function):
    """x @ bf16(w) in the forward (the eval GEMM's 16-bit operand copy); the fp32 head of the backward reads the fp32 master: dx = g w^T, dw = x^T g."""
    @staticmethod
    def forward(ctx, x, w, model):
        ctx.save_for_backward(x, w)
        return x @ (r16(w) if model else w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g @ w.t(), x.t() @ g, None


def image_tower_node(image, params, cfg, w, model=False, wiring=()):
    """train_vit.ImageTowerTrainFn.  image fp64 [B, 3, R, R]; params: name -> fp64 tensor for the 32 tensors of `visual` (its named_parameters); cfg = dict(patch,
    heads, layers, eps); w fp64 [B, E]: the gradient of the feature.
    Stem: the patch GEMM on the bf16 patch columns and the bf16 kernel, output stored in bf16 (patch / dpatch); LN_pre([cls | patch] + pos) in fp32, recomputed in
    fp32 by the backward.  Blocks: pre_ln_layer with QuickGELU, no key mask.  Head: ln_post of the fp32 class rows stored in bf16, proj as a 16-bit operand with an
    fp32 output; its backward in fp32 from the fp32 master of proj; the class-row gradient enters a zero bf16 stream gradient.
    wiring (MUTANTS): "seed_row1" (that gradient seeded on row 1), "dcls_cut" (class_embedding's gradient without the class row's share), plus pre_ln_layer's;
    of the forward (tests/infer_nodes_ref.py): "post_row1" (ln_post on row 1 instead of the class row), "no_ln_pre" (ln_pre left out).
    -> dict(feat [B, E], grads: name -> tensor)"""
    R = Rounder(model)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    B = image.shape[0]
    W = P["conv1.weight"].shape[0]
    eps = cfg["eps"]
    patch = F.conv2d(R.rf(image), R.w16(P["conv1.weight"]), None, stride=cfg["patch"])
    patch = R.rs(patch.reshape(B, W, -1).permute(0, 2, 1))                              # patch / dpatch, bf16
    ce = P["class_embedding"]
    v = torch.cat([(_cut(ce) if "dcls_cut" in wiring else ce).expand(B, 1, W), patch], 1) + P["positional_embedding"]
    x = R.rf(v if "no_ln_pre" in wiring else F.layer_norm(v, (W,), P["ln_pre.weight"], P["ln_pre.bias"], eps), r32)
    for li in range(cfg["layers"]):
        pre = f"transformer.resblocks.{li}."
        iw, ib = P[pre + "attn.in_proj_weight"], P[pre + "attn.in_proj_bias"]
        p16 = [iw[:W], ib[:W], iw[W:2 * W], ib[W:2 * W], iw[2 * W:], ib[2 * W:], P[pre + "attn.out_proj.weight"], P[pre + "attn.out_proj.bias"],
               P[pre + "ln_1.weight"], P[pre + "ln_1.bias"], P[pre + "mlp.c_fc.weight"], P[pre + "mlp.c_fc.bias"], P[pre + "mlp.c_proj.weight"],
               P[pre + "mlp.c_proj.bias"], P[pre + "ln_2.weight"], P[pre + "ln_2.bias"]]
        x = pre_ln_layer(x, p16, [x.shape[1]] * B, None, model, "quickgelu", eps, wiring, cfg["heads"])
    x = R.rb(x)                                                                         # the stream gradient the class rows are written into: bf16
    rows = x[:, 0]
    if "seed_row1" in wiring:
        rows = rows.detach() + (x[:, 1] - x[:, 1].detach())
    if "post_row1" in wiring:
        rows = x[:, 1]
    ncls = R.rf(F.layer_norm(rows, (W,), P["ln_post.weight"], P["ln_post.bias"], eps))  # ln_post's output, bf16
    feat = R.rf(_MatmulStored16.apply(ncls, P["proj"], model), r32)
    names = list(P)
    got = torch.autograd.grad((feat * w).sum(), [P[k] for k in names], allow_unused=True)
    return dict(feat=feat.detach(), grads={k: (torch.zeros_like(P[k]) if g is None else g) for k, g in zip(names, got)})

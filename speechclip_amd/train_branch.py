"""Training the stacked parallel branch (`TransformerEncoder` with n_layers >= 2 or norm_first) on MI355X.

`BranchStackTrainFn` is ONE autograd node for norm(layers([CLS; frames]))[:, 0], the differentiable counterpart of
`TransformerEncoder._forward_cls_stack`:
  layers 0 .. n-2   every row of [CLS; frames] ([B, T + 1] rows, key lengths len + 1) on the layer bodies of train_hubert.py (post-LN on bf16 rows,
                    pre-LN on an fp32 residual stream) with the head_dim 64 / 96 / 128 attention pair ops.attention_hd_qkv / attention_hd_qkv_bwd
                    (sc_attention_hd_fwd / sc_attention_hd_bwd) in place of the head_dim 64 one.  nn.TransformerEncoderLayer is the fairseq layer's
                    graph with one packed in_proj and all four dropout rates equal to `dropout`.
  layer n-1         K | V of all rows from one bf16 GEMM, Q of the B CLS rows, attention with Tq = 1 (bf16 output), then out-proj, LayerNorms, FFN
                    and the final norm of the B CLS rows in fp32 (sc_sgemm, fp32 LayerNorm: the pieces of ParallelBranchTrainFn's CLS rows).
                    Backward: the fp32 tail, sc_attention_hd_bwd with Tq = 1 -> dq [B, D], dk | dv [B (T + 1), 2D]; dx = [dk | dv] W_kv for every row,
                    row 0 of each utterance also takes dq W_q and the residual gradient; in_proj gradients from the q part (B rows) and the k | v
                    part (all rows).
Dropout (train mode): rate p at the four sites of every layer -- attention probabilities inside the kernels, sc_dropout_bf16 on the rows of the full
layers, sc_dropout_f32 on the fp32 CLS rows of the last layer.  Site seeds come from one forward seed (`_site_seeds`); the backward regenerates every
mask and stores none.  A padded position is masked as a key in every layer, so its rows never reach a CLS row and its gradient is exactly zero.
"""
import torch

from . import ops
from .train_hubert import (BF, _f32, _layer_bwd_post_ln, _layer_bwd_pre_ln, _layer_fwd_post_ln, _layer_fwd_pre_ln, _param_grads, _site_seeds, _w16,
                           wgrad)

PER_LAYER = 12     # in_w in_b out_w out_b n1_w n1_b l1_w l1_b l2_w l2_b n2_w n2_b


def stack_params(model):
    """The node's parameter list of a `_EncoderStack`: PER_LAYER tensors per layer, then the final norm's weight and bias."""
    out = []
    for L in model.layers:
        a = L.self_attn
        out += [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, L.norm1.weight, L.norm1.bias, L.linear1.weight, L.linear1.bias,
                L.linear2.weight, L.linear2.bias, L.norm2.weight, L.norm2.bias]
    return out + [model.norm.weight, model.norm.bias]


def _hd_fwd(pk, qkv, M, B, Tp, H, valid_i32, drop=None):
    p, s = drop if drop is not None else (0.0, 0)
    return ops.attention_hd_qkv(qkv[:M], B, Tp, H, valid_i32, drop_p=p, seed=s)


def _hd_bwd(pk, qkv, att, datt, B, Tp, H, valid_i32, drop=None):
    p, s = drop if drop is not None else (0.0, 0)
    return ops.attention_hd_qkv_bwd(qkv[:B * Tp], att, datt, B, Tp, H, valid_i32, drop_p=p, seed=s)


ATTN_HD = (_hd_fwd, _hd_bwd)


def _hubert_order(p, D):
    """One layer's PER_LAYER tensors -> the 16 of the layer bodies (q_w q_b k_w k_b v_w v_b o_w o_b ln1 fc1 fc2 ln2)."""
    iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = p
    return [iw[:D], ib[:D], iw[D:2 * D], ib[D:2 * D], iw[2 * D:], ib[2 * D:], ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b]


class BranchStackTrainFn(torch.autograd.Function):
    """out f32 [B, D] = norm(layers([CLS; frames]))[:, 0].
    args: meta (dict: heads, eps, pre_ln, drop_p, seed), cls [1, 1, D], frames bf16 [B, T, D], audio_len int [B], then PER_LAYER tensors per layer
    and the final norm's weight and bias (`stack_params`)."""

    @staticmethod
    def forward(ctx, meta, cls, frames, audio_len, *params):
        H, eps, pre_ln, pd = int(meta["heads"]), float(meta["eps"]), bool(meta["pre_ln"]), float(meta["drop_p"])
        n = (len(params) - 2) // PER_LAYER
        assert len(params) == n * PER_LAYER + 2 and n >= 1
        B, T, D = frames.shape
        Lq, M, hd = T + 1, B * (T + 1), D // H
        dev = frames.device
        klens = (audio_len.to(device=dev, dtype=torch.int32) + 1).contiguous()
        drop = dict(hidden=pd, attention=pd, activation=pd, seed=int(meta["seed"])) if pd > 0 else None
        seeds = _site_seeds(drop["seed"], 4 * n) if drop is not None else [0] * (4 * n)
        shape = (B, Lq, H, eps)
        x = torch.empty(B, Lq, D, device=dev, dtype=torch.float32 if pre_ln else BF)
        x[:, 0] = cls.detach().reshape(D)
        x[:, 1:] = frames.detach()
        h = x.view(M, D)
        layer = _layer_fwd_pre_ln if pre_ln else _layer_fwd_post_ln
        saved = []
        for li in range(n - 1):
            p16 = _hubert_order(params[li * PER_LAYER:(li + 1) * PER_LAYER], D)
            out = torch.empty_like(h)
            saved += layer(h, _w16(params[li * PER_LAYER]), _f32(params[li * PER_LAYER + 1]), p16[6:], None, shape, klens, out, drop,
                           seeds[4 * li:4 * li + 4], ATTN_HD)
            h = out
        # ---- last layer: K | V of every row, one CLS query per utterance, the B CLS rows in fp32
        iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = params[(n - 1) * PER_LAYER:n * PER_LAYER]
        nfw, nfb = params[-2:]
        sa, s1, s2, s3 = seeds[4 * (n - 1):]
        xc = h.view(B, Lq, D)[:, 0].float().contiguous()
        if pre_ln:
            h16 = h.to(BF)                                                                    # LayerNorm input of the backward
            a_all = ops.layernorm(h, _f32(n1w), _f32(n1b), eps)
            ac = ops.layernorm(xc, _f32(n1w), _f32(n1b), eps, out_f32=True)
        else:
            h16, a_all, ac = h, h, xc
        Win, bin_ = _f32(iw), _f32(ib)
        kv = ops.gemm(a_all, _w16(iw[D:]), bin_[D:].contiguous())                             # bf16 [M, 2D] = k | v
        qc = ops.sgemm(ac, Win[:D], transb=True, bias=bin_[:D].contiguous()).to(BF)           # [B, D]
        att16 = ops.attention_hd(qc, kv, kv[:, D:], B, H, 1, Lq, hd, (D, D), (Lq * 2 * D, 2 * D), klens, drop_p=pd, seed=sa)
        att = att16.view(B, D).float()
        so = ops.sgemm(att, _f32(ow), transb=True, bias=_f32(ob))
        if pd > 0:
            ops.dropout_f32(so, pd, s1, out=so)
        y = so + xc                                            # post-LN: LN1's input; pre-LN: the residual stream after attention
        x1 = ops.layernorm(y, _f32(n2w), _f32(n2b), eps, out_f32=True) if pre_ln else ops.layernorm(y, _f32(n1w), _f32(n1b), eps, out_f32=True)
        z1 = ops.sgemm(x1, _f32(l1w), transb=True, bias=_f32(l1b))
        hm = ops.gelu_f32(z1)
        if pd > 0:
            ops.dropout_f32(hm, pd, s2, out=hm)
        ff = ops.sgemm(hm, _f32(l2w), transb=True, bias=_f32(l2b))
        if pd > 0:
            ops.dropout_f32(ff, pd, s3, out=ff)
        y2 = ff + (y if pre_ln else x1)
        x2 = y2 if pre_ln else ops.layernorm(y2, _f32(n2w), _f32(n2b), eps, out_f32=True)
        res = ops.layernorm(x2, _f32(nfw), _f32(nfb), 1e-5, out_f32=True)
        ctx.meta = dict(H=H, eps=eps, pre_ln=pre_ln, pd=pd, n=n, B=B, T=T, D=D, seeds=seeds, drop=drop)
        ctx.klens = klens
        ctx.save_for_backward(*saved, xc, h16, a_all, ac, kv, qc, att16, y, x1, z1, hm, y2, x2, *[p.detach() for p in params])
        return res

    @staticmethod
    def backward(ctx, dout):
        m = ctx.meta
        H, eps, pre_ln, pd, n, B, T, D, seeds, drop = (m[k] for k in ("H", "eps", "pre_ln", "pd", "n", "B", "T", "D", "seeds", "drop"))
        Lq, M, hd = T + 1, B * (T + 1), D // H
        klens = ctx.klens
        shape = (B, Lq, H, eps)
        t = ctx.saved_tensors
        na = 7 * (n - 1)
        acts, (xc, h16, a_all, ac, kv, qc, att16, y, x1, z1, hm, y2, x2), params = t[:na], t[na:na + 13], t[na + 13:]
        dev = dout.device
        z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)   # noqa: E731
        grads = [None] * len(params)
        base = (n - 1) * PER_LAYER
        iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = params[base:base + PER_LAYER]
        sa, s1, s2, s3 = seeds[4 * (n - 1):]
        dout = dout.float().contiguous()
        # ---- the fp32 tail of the last layer
        dnfw, dnfb, dn1w, dn1b, dn2w, dn2b = z(D), z(D), z(D), z(D), z(D), z(D)
        dx2 = ops.layernorm_bwd(x2, dout, _f32(params[-2]), dnfw, dnfb, 1e-5)
        dy2 = dx2 if pre_ln else ops.layernorm_bwd(y2, dx2, _f32(n2w), dn2w, dn2b, eps)
        dff = ops.dropout_f32(dy2, pd, s3) if pd > 0 else dy2
        dl2w, dl2b = ops.sgemm(dff, hm, transa=True), ops.colsum(dff)
        dhm = ops.sgemm(dff, _f32(l2w))
        if pd > 0:
            ops.dropout_f32(dhm, pd, s2, out=dhm)
        ops.gelu_bwd_(z1, dhm)                                                                # dhm is now dz1
        dl1w, dl1b = ops.sgemm(dhm, x1, transa=True), ops.colsum(dhm)
        if pre_ln:       # x1 = LN2(y), y2 = y + ff
            dy = ops.layernorm_bwd(y, ops.sgemm(dhm, _f32(l1w)), _f32(n2w), dn2w, dn2b, eps) + dy2
        else:            # x1 = LN1(y), y2 = x1 + ff
            dy = ops.layernorm_bwd(y, ops.sgemm(dhm, _f32(l1w), beta=1.0, out=dy2.clone()), _f32(n1w), dn1w, dn1b, eps)
        dso = ops.dropout_f32(dy, pd, s1) if pd > 0 else dy                                   # y = xc + dropout1(att Wo^T + bo)
        att = att16.view(B, D).float()
        dow, dob = ops.sgemm(dso, att, transa=True), ops.colsum(dso)
        datt16 = ops.sgemm(dso, _f32(ow)).to(BF).view(B, 1, D)
        # ---- attention, Tq = 1
        dq, dk, dv = ops.attention_hd_bwd(qc, kv, kv[:, D:], att16, datt16, B, H, 1, Lq, hd, (D, D), (Lq * 2 * D, 2 * D), klens, pd, sa)
        dkv = torch.as_strided(dk, (M, 2 * D), (2 * D, 1))                                    # dk | dv: one buffer
        dq32 = dq.view(B, D).float()
        Win = _f32(iw)
        diw, dib = torch.empty(3 * D, D, device=dev, dtype=torch.float32), torch.empty(3 * D, device=dev, dtype=torch.float32)
        ops.sgemm(dq32, ac, transa=True, out=diw[:D])
        ops.colsum(dq32, out=dib[:D])
        diw[D:] = wgrad(dkv, a_all)
        ops.colsum_bf16(dkv, out=dib[D:])
        dac = ops.sgemm(dq32, Win[:D].contiguous())                                           # [B, D]: the CLS rows as queries
        g = ops.gemm(dkv, _w16(iw[D:].t()))                                                   # [M, D]: every row as key / value
        if pre_ln:       # a_all = LN1(h), ac = LN1(xc); y = xc + ...
            g, dg1, db1 = ops.layernorm_bwd_bf16(h16, g, _f32(n1w), eps, True)
            dxc = ops.layernorm_bwd(xc, dac, _f32(n1w), dn1w, dn1b, eps) + dy
            dn1w += dg1
            dn1b += db1
        else:
            dxc = dac + dy
        g3 = g.view(B, Lq, D)
        g3[:, 0] = (g3[:, 0].float() + dxc).to(BF)
        grads[base:base + PER_LAYER] = [diw, dib, dow, dob, dn1w, dn1b, dl1w, dl1b, dl2w, dl2b, dn2w, dn2b]
        grads[-2], grads[-1] = dnfw, dnfb
        # ---- layers n-2 .. 0 on every row
        layer = _layer_bwd_pre_ln if pre_ln else _layer_bwd_post_ln
        for li in range(n - 2, -1, -1):
            p16 = _hubert_order(params[li * PER_LAYER:(li + 1) * PER_LAYER], D)
            g, pieces = layer(g, acts[7 * li:7 * li + 7], p16, None, shape, klens, True, drop, seeds[4 * li:4 * li + 4], ATTN_HD)
            g16 = [None] * 16
            _param_grads(g16, 0, *pieces)
            grads[li * PER_LAYER:(li + 1) * PER_LAYER] = [torch.cat([g16[0], g16[2], g16[4]], 0), torch.cat([g16[1], g16[3], g16[5]], 0)] + g16[6:]
        g3 = g.view(B, Lq, D)
        dcls = ops.colsum(g3[:, 0].float().contiguous()).view(1, 1, D) if ctx.needs_input_grad[1] else None
        dframes = g3[:, 1:].contiguous() if ctx.needs_input_grad[2] else None
        return (None, dcls, dframes, None, *grads)

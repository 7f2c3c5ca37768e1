"""Fine-tuning the CLIP image tower on MI355X (`clip.image_encoder_trainable: true`).

Reference: `ClipModel(image_encoder_trainable=True)` leaves `model.visual` trainable (avssl/module/clip_official.py `freeze_models`,
`trainable_params`; avssl/model/kwClip.py `getTrainableParams`), so `loss.backward()` differentiates `CLIP.encode_image`.

`ImageTowerTrainFn` is that function as ONE autograd node: patchify -> patch GEMM -> LN_pre([cls | patch] + pos) -> N pre-LN QuickGELU blocks ->
ln_post on the class rows -> proj.  The forward runs the eval path's kernels at the eval path's rounding points (its output is bitwise the eval
`encode_image`); the blocks are the pre-LN layer bodies of train_hubert.py with the QuickGELU activation pair and the ViT attention pair
(`ops.attention` forward, the fused head-dim-64 `ops.attention_hd_qkv_bwd` backward: no key mask, no dropout, no atomics).
  saved per block   the 7 tensors of `_layer_fwd_pre_ln`: bf16 copies of the stream in front of ln_1 and ln_2, ln_1's / ln_2's outputs, q | k | v, the
                    attention output and the MLP's hidden activations
  saved once        the patch columns and the patch GEMM's output (bf16), the class rows of the final stream (f32) and their ln_post output (bf16)
  recomputed        fc1's pre-activation (one GEMM per block), every LayerNorm's row statistics, attention scores and probabilities per tile, and the
                    whole of LN_pre's row in sc_vit_embed_bwd
  precision         the stream gradient is bf16 between blocks (as for HuBERT-large), parameter gradients fp32 (split-K wgrad, two-stage column sums);
                    the head (proj, ln_post on B rows) is fp32: ops.sgemm, ops.layernorm_bwd
"""
from typing import List

import torch

from . import ops
from .train_hubert import ACT_QUICKGELU_PAIR, BF, _f32, _layer_bwd_pre_ln, _layer_fwd_pre_ln, _w16, wgrad

PER_BLOCK = 12     # in_proj_weight in_proj_bias out_proj.weight out_proj.bias ln_1.weight ln_1.bias c_fc.weight c_fc.bias c_proj.weight c_proj.bias ln_2.weight ln_2.bias
N_STEM = 5         # conv1.weight class_embedding positional_embedding ln_pre.weight ln_pre.bias


def block_params(blk) -> List[torch.nn.Parameter]:
    a, m = blk.attn, blk.mlp
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, blk.ln_1.weight, blk.ln_1.bias, m.c_fc.weight, m.c_fc.bias,
            m.c_proj.weight, m.c_proj.bias, blk.ln_2.weight, blk.ln_2.bias]


def visual_params(visual) -> List[torch.nn.Parameter]:
    """Every tensor of `model.visual`, in the node's argument order: the stem, 12 per block, ln_post and proj."""
    out = [visual.conv1.weight, visual.class_embedding, visual.positional_embedding, visual.ln_pre.weight, visual.ln_pre.bias]
    for blk in visual.transformer.resblocks:
        out += block_params(blk)
    return out + [visual.ln_post.weight, visual.ln_post.bias, visual.proj]


def _vit_attn_fwd(pk, qkv, M, B, L, H, valid_i32, drop=None):
    assert pk is None and drop is None
    return ops.attention(qkv[:M], B, L, H, None)             # the eval tower's kernel (clip_model.run_tower)


def _vit_attn_bwd(pk, qkv, att, datt, B, L, H, valid_i32, drop=None):
    assert pk is None and drop is None
    return ops.attention_hd_qkv_bwd(qkv[:B * L], att, datt, B, L, H)


ATTN_VIT = (_vit_attn_fwd, _vit_attn_bwd)


def _layer_args(p, d):
    """A ViT block's 12 tensors as the 16 the layer bodies take: q / k / v are row slices (views) of the one in_proj pair."""
    iw, ib, ow, ob, g1, b1, w1, c1, w2, c2, g2, b2 = p
    return [iw[:d], ib[:d], iw[d:2 * d], ib[d:2 * d], iw[2 * d:], ib[2 * d:], ow, ob, g1, b1, w1, c1, w2, c2, g2, b2]


class ImageTowerTrainFn(torch.autograd.Function):
    """feat f32 [B, embed_dim] = CLIP.encode_image(image) with gradients for every tensor of `model.visual` (none for the image).
    args: meta (patch, ntok, heads, eps), image f32 [B, 3, R, R], then visual_params(visual).

    More than one rank: every rank evaluates the same global loss on the gathered features and differentiates it with respect to its LOCAL image rows
    only -- train_tail.PackedGatherFn's backward hands this node the rank's own slice of d loss / d image_feat -- so the parameter gradients returned
    here are the rank's partial sums; train_tail.FusedAdam adds them over the ranks before its step."""

    @staticmethod
    def forward(ctx, meta, image, *params):
        p, ntok, H, eps = meta["patch"], meta["ntok"], meta["heads"], meta["eps"]
        conv_w, cls_e, pos, gpre, bpre = params[:N_STEM]
        gpost, bpost, proj = params[-3:]
        blocks = params[N_STEM:-3]
        n = len(blocks) // PER_BLOCK
        dev = image.device
        B, W = image.shape[0], conv_w.shape[0]
        K = 3 * p * p
        Kpad = (K + 63) // 64 * 64
        assert W == H * 64 and tuple(pos.shape) == (ntok, W)
        w16 = torch.zeros(W, Kpad, device=dev, dtype=BF)
        w16[:, :K] = conv_w.detach().reshape(W, K).to(BF)
        cols = ops.vit_patchify(image.detach().float().contiguous(), p, Kpad)
        patch = ops.gemm(cols, w16)
        x = ops.vit_embed(patch, _f32(cls_e), _f32(pos), _f32(gpre), _f32(bpre), B, ntok, W, eps)
        shape = (B, ntok, H, eps)
        saved = []
        for li in range(n):
            bp = blocks[li * PER_BLOCK:(li + 1) * PER_BLOCK]
            out = torch.empty_like(x)
            saved += _layer_fwd_pre_ln(x, _w16(bp[0]), _f32(bp[1]), bp[2:], None, shape, None, out, None, (), attn=ATTN_VIT, act=ACT_QUICKGELU_PAIR)
            x = out
        rows = x.view(B, ntok, W)[:, 0].contiguous()                       # the class rows of the final stream (f32)
        ncls = ops.layernorm(x, _f32(gpost), _f32(bpost), eps, rows=B, D=W, ld_in=ntok * W)
        feat = ops.gemm(ncls, proj.detach().t().to(BF).contiguous(), out_f32=True)
        ctx.meta, ctx.n, ctx.dims = meta, n, (B, W, K)
        ctx.save_for_backward(cols, patch, rows, ncls, *saved, *[t.detach() for t in params])
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        meta, n = ctx.meta, ctx.n
        p, ntok, H, eps = meta["patch"], meta["ntok"], meta["heads"], meta["eps"]
        B, W, K = ctx.dims
        cols, patch, rows, ncls, *rest = ctx.saved_tensors
        acts, params = rest[:7 * n], rest[7 * n:]
        conv_w, cls_e, pos, gpre, bpre = params[:N_STEM]
        gpost, bpost, proj = params[-3:]
        blocks = params[N_STEM:-3]
        dev = rows.device
        grads = [None] * len(params)
        # head, fp32: feat = ln_post(class rows) @ proj
        dfeat = dfeat.float().contiguous()
        grads[-1] = ops.sgemm(ncls.float(), dfeat, transa=True)                               # [W, E] = n^T dfeat
        dn = ops.sgemm(dfeat, _f32(proj), transb=True)                                         # [B, W] = dfeat proj^T
        grads[-3] = torch.zeros(W, device=dev, dtype=torch.float32)
        grads[-2] = torch.zeros(W, device=dev, dtype=torch.float32)
        drows = ops.layernorm_bwd(rows, dn, _f32(gpost), grads[-3], grads[-2], eps)
        g = torch.zeros(B * ntok, W, device=dev, dtype=BF)                                     # d loss / d (final stream): the class rows only
        g.view(B, ntok, W)[:, 0] = drows.to(BF)
        shape = (B, ntok, H, eps)
        for li in range(n - 1, -1, -1):
            bp = blocks[li * PER_BLOCK:(li + 1) * PER_BLOCK]
            g, (dqkv, x_qkv, dyo, att, du, x_fc1, dy2, hm, dg1, db1, dg2, db2) = _layer_bwd_pre_ln(
                g, acts[7 * li:7 * li + 7], _layer_args(bp, W), None, shape, None, True, None, (0, 0, 0, 0), attn=ATTN_VIT, act=ACT_QUICKGELU_PAIR)
            grads[N_STEM + li * PER_BLOCK:N_STEM + (li + 1) * PER_BLOCK] = [
                wgrad(dqkv, x_qkv), ops.colsum_bf16(dqkv), wgrad(dyo, att), ops.colsum_bf16(dyo), dg1, db1,      # the q / k / v slices land in ONE in_proj tensor
                wgrad(du, x_fc1), ops.colsum_bf16(du), wgrad(dy2, hm), ops.colsum_bf16(dy2), dg2, db2]
        dpatch, dpos, dcls, dgpre, dbpre = ops.vit_embed_bwd(g.float(), patch, _f32(cls_e), _f32(pos), _f32(gpre), B, ntok, W, eps)
        dconv = wgrad(dpatch, cols)[:, :K].reshape(W, 3, p, p)                                 # [W, Kpad]: the zero-padded columns are cut
        grads[:N_STEM] = [dconv, dcls.clone(), dpos, dgpre, dbpre]                            # dcls is row 0 of dpos: two parameters, two buffers
        return (None, None, *grads)


def encode_image_train(clip, image: torch.Tensor) -> torch.Tensor:
    """CLIP.encode_image on the differentiable path (clip: module.clip_model.CLIP)."""
    assert image.is_cuda, "the image tower trains on the HIP kernels only (no CPU fallback)"
    v = clip.visual
    meta = dict(patch=v.patch, ntok=(v.input_resolution // v.patch) ** 2 + 1, heads=v.transformer.heads, eps=1e-5)
    return ImageTowerTrainFn.apply(meta, image, *visual_params(v))

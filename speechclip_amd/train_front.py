"""Training the HuBERT front end on MI355X: `audio_encoder.trainable: true` WITHOUT `reinit_layers` / `unfreeze_layers`
(avssl/module/speech_encoder_plus.py:399-401 -- `freeze_model` is simply not called, so the conv feature extractor, `post_extract_proj`,
`layer_norm`, the positional conv and every transformer layer train; [3P fairseq] `HubertModel.forward_features` multiplies the gradient that
enters the feature extractor by `feature_grad_mult`, 0.1 in the released base checkpoint).

`HubertFrontTrainFn` = wave -> hidden state 0 (the input of transformer layer 0) as ONE autograd node, post-LN / GroupNorm models (HuBERT-base):
  forward   the eval path's kernels (sc_conv0_fwd, conv-as-GEMM with fused GELU, LayerNorm, projection, sc_posconv_conv), keeping the layer outputs,
            plus sc_posconv_finish_train (pre-activation and LayerNorm input of the positional-conv tail)
  backward  encoder LayerNorm      sc_layernorm_bwd_bf16
            positional conv        dX: the SAME grouped conv on the time-reversed gradient with in/out channels swapped (sc_posconv_conv +
                                   sc_posconv_dgrad_finish); dW: per group, split-K sc_gemm_bf16_batched over the transposed sliding-window
                                   view (sc_posconv_pack + sc_transpose_bf16); weight-norm (g, v) from dW in fp32 on the [d, d/G, Kw] tensors
            projection, feature LN sc_gemm_bf16 on the transposed weight, train_hubert.wgrad, sc_layernorm_bwd_bf16
            conv layers 6..1       pre-activation recomputed (sc_gemm_bf16 without the GELU), sc_gelu_bwd_bf16, dW = split-K TN GEMM over the
                                   overlapping-row view, dX = one GEMM per group of taps written straight into the channels-last input gradient
                                   (taps 0..s-1 tile it exactly; tap s.. accumulate through the residual epilogue, in place)
            conv layer 0           sc_conv0_bwd (GroupNorm + GELU + conv from the wave)
meta["drop"] = dict(features, hidden, seed) applies the two dropouts fairseq has on this stretch in train mode (dropout_input on the projected
features, F.dropout on hidden state 0) with counter-based masks the backward regenerates.

ONE code path serves padded and padding-free batches.  The padded layout is the packed one with row_off[b] = b * Tp and rows_b = Tp; `_layout` states
either as a `Layout` once per node, and every per-utterance kernel takes it: conv layer 0 and the positional conv through `_conv0_forward` / `_posconv`, the
others (sc_posconv_finish_train, sc_reverse_rows_bf16, sc_posconv_dgrad_finish, sc_conv0_bwd / sc_conv0_wgrad and their *_packed entries, one kernel each)
through the `row_off_i32` of their `ops` wrapper.  The only other layout choice is between the two weight-gradient builders of the positional conv, which
keep their own split-K geometry.  Every GEMM, LayerNorm, GELU and dropout is row-wise and runs on all rows as it is (the dropout masks are indexed by position
in the layout in use): on packed rows the conv stack sees ONE utterance of scale0 * total frames.
meta["pack"] = dict(row_off, rows_max, total, scale0) (module/hubert.py: packed_geometry; row_off as B + 1 device ints) selects the padding-free layout:
utterance b owns rows [row_off[b], row_off[b + 1]) at transformer level and scale_l times that range at conv layer l.  The gradient stays inside its
utterance: dxp is non-zero on rows < valid_b only, and output frame F - 1 reaches 64 F + 15 <= 64 (F + 1) layer-0 frames, so the halo row and the rows that
read a neighbour's samples (finite junk in the forward) meet an exactly zero gradient at every conv level.
"""
from collections import namedtuple

import torch

from . import ops
from .ops import ACT_GELU, ACT_NONE
from .train_hubert import _pack_of, wgrad

BF = torch.bfloat16
N_FRONT = 18   # conv0 w, gn w, gn b, conv1..6 w, feat-LN w b, proj w b, pos g v bias, enc-LN w b


def front_params(enc) -> list:
    """The trainable tensors of the front end of module.hubert.HubertModel, in HubertFrontTrainFn's order (base / GroupNorm extractor)."""
    convs = enc.feature_extractor.conv_layers
    assert enc.cfg.extractor_mode == "default" and not enc.cfg.conv_bias and not enc.cfg.layer_norm_first and len(convs) == 7
    gn = getattr(convs[0], "2")
    pc = getattr(enc.encoder.pos_conv, "0")
    return ([getattr(convs[0], "0").weight, gn.weight, gn.bias] + [getattr(convs[i], "0").weight for i in range(1, 7)] +
            [enc.layer_norm.weight, enc.layer_norm.bias, enc.post_extract_proj.weight, enc.post_extract_proj.bias,
             pc.weight_g, pc.weight_v, pc.bias, enc.encoder.layer_norm.weight, enc.encoder.layer_norm.bias])


def _f32(t):
    return t.detach().float().contiguous()


def _conv_w16(w):
    """[out, in, k] -> bf16 [out, k*in] (K index = tap*C + c_in), the conv-as-GEMM operand."""
    return w.detach().permute(0, 2, 1).reshape(w.shape[0], -1).to(BF).contiguous()


def _fold_weight_norm(g, v):
    v = v.detach().float()
    n = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    return g.detach().float() * v / n, n


def _pos_operands(wfold, G, Kw):
    """folded weight f32 [d, d/G, Kw] -> (forward operand, adjoint operand) bf16 [G, cg, Kw*cg], K index = tap*cg + c_in."""
    d, cg, _ = wfold.shape
    w4 = wfold.view(G, cg, cg, Kw)                                   # [g, out, in, tap]
    fwd = w4.permute(0, 1, 3, 2).reshape(G, cg, Kw * cg).to(BF).contiguous()
    adj = w4.permute(0, 2, 3, 1).reshape(G, cg, Kw * cg).to(BF).contiguous()      # roles of in / out swapped
    return fwd, adj


def _posconv_wgrad_groups(xg, x_group, x_utt, du, du_utt, rows, batch, Tq, S, D, G, Kw):
    """The per-group part of both weight-gradient builders.  `batch` utterances of `rows` rows: group g of the window slab xg at element g * x_group, utterances
    x_utt elements apart; columns g * cg .. of du bf16 [., D], utterances du_utt elements apart.  Per group: both operands transposed to K-major with every
    utterance padded to Tq rows, split-K batched GEMM over S chunks of K = batch * Tq, column sum of the partials, permuted to f32 [out, in, tap]."""
    cg = D // G
    dev = du.device
    Ktot = batch * Tq
    chunk = Ktot // S
    xvT = torch.empty(Kw * cg, Ktot, device=dev, dtype=BF)
    duT = torch.empty(cg, Ktot, device=dev, dtype=BF)
    part = torch.empty(S, Kw * cg, cg, device=dev, dtype=torch.float32)
    out = torch.empty(D, cg, Kw, device=dev, dtype=torch.float32)
    du = du.view(-1)
    for g in range(G):
        ops.transpose_bf16(xg[g * x_group:], cg, x_utt, rows, Kw * cg, batch, rows_padded=Tq, out=xvT, ld_out=Ktot, stride_out=Tq)
        ops.transpose_bf16(du[g * cg:], D, du_utt, rows, cg, batch, rows_padded=Tq, out=duT, ld_out=Ktot, stride_out=Tq)
        ops.gemm_batched(xvT, Ktot, chunk, duT, chunk, S, part, cg, Kw * cg * cg, None, Kw * cg, cg, chunk, S, ldw=Ktot)
        tot = part[0] if S == 1 else ops.colsum(part.view(S, Kw * cg * cg)).view(Kw * cg, cg)      # [(tap, in), out]
        out[g * cg:(g + 1) * cg] = tot.view(Kw, cg, cg).permute(2, 1, 0)
    return out


def posconv_wgrad(du, xp, valid_i32, B, Tp, D, G, Kw):
    """dW of the grouped positional conv in the folded weight's layout: f32 [D, D/G, Kw] = sum_{b,t} du[b,t,out] * mask(xp)[b, t + tap - Kw/2, in]."""
    cg = D // G
    Tq = -(-Tp // 64) * 64
    S = max(s for s in (16, 8, 4, 2, 1) if B % s == 0)
    xg = ops.posconv_pack(xp, valid_i32, B, Tp, D, G, Kw)              # [B, G, Tp + Kw, cg]
    return _posconv_wgrad_groups(xg, (Tp + Kw) * cg, G * (Tp + Kw) * cg, du, Tp * D, Tp, B, Tq, S, D, G, Kw)


def posconv_wgrad_packed(du, xp, valid_i32, rows_i32, off_i32, B, total, D, G, Kw):
    """posconv_wgrad on packed rows (du, xp bf16 [total, D]).  The window slab keeps Kw zero rows between utterances (sc_posconv_pack_gapped) and du takes the
    same gapped row numbering, so both operands are ONE [rows, cols] matrix (one "utterance" of Ktot rows for the shared per-group chain); the split count
    depends on the row count only, so the summation order is fixed for a given batch."""
    cg = D // G
    Rg = total + B * Kw                                                 # gapped rows: utterance b starts at row_off[b] + b * Kw
    S = max(s for s in (16, 8, 4, 2, 1) if s == 1 or Rg >= 512 * s)
    Ktot = -(-Rg // (64 * S)) * 64 * S
    xg = ops.posconv_pack_gapped(xp, valid_i32, off_i32, B, total, D, G, Kw, Kw // 2, Ktot + Kw)       # [G, Ktot + Kw, cg], masked input, Kw/2 zero rows in front
    dug = ops.posconv_pack_gapped(du, rows_i32, off_i32, B, total, D, 1, Kw, 0, Ktot)                  # [Ktot, D], zero rows in the gaps and behind the batch
    return _posconv_wgrad_groups(xg, (Ktot + Kw) * cg, 0, dug, 0, Ktot, 1, Ktot, S, D, G, Kw)


def _rows_with_slack(n_rows, cols, dev):
    """[n_rows + 8, cols] bf16 whose 8 slack rows are zero (the conv-as-GEMM views over-read / the overlapping tap accumulates into them); the body is
    written in full by the producing GEMM, so it is not filled first."""
    t = torch.empty(n_rows + 8, cols, device=dev, dtype=BF)
    t[n_rows:].zero_()
    return t


def conv_layer_backward(xin, w, du_i, B, rows_out, dim, k, s, C):
    """Conv-as-GEMM layer, gradient du_i bf16 [B*rows_out, dim] of its (pre-activation) output -> (dW f32 [dim, C, k], dX bf16 [B*rows_in + 8, C])."""
    Mi = B * rows_out
    rows_in = rows_out * s
    w16 = _conv_w16(w)
    xview = torch.as_strided(xin, (Mi, k * C), (s * C, 1))
    dW = wgrad(du_i, xview).view(dim, k, C).permute(0, 2, 1).contiguous()
    wT = w16.t().contiguous()                                                    # [k*C, dim]
    dx = _rows_with_slack(B * rows_in, C, xin.device)
    ops.gemm(du_i, wT[:s * C], out=dx[:s * Mi].view(Mi, s * C))                  # taps 0 .. s-1 tile the input rows exactly
    for j in range(s, k):                                                        # overlapping taps: accumulate in place
        tgt = torch.as_strided(dx, (Mi, C), (s * C, 1), storage_offset=j * C)
        ops.gemm(du_i, wT[j * C:(j + 1) * C], residual=tgt, out=tgt)
    return dW, dx


# The row layout of one node.  B utterances; the conv stack and every row-wise kernel see Bc "utterances" of `rows` transformer rows (`rows0` conv-layer-0
# rows, scale0 per transformer row) each: (B, Tp, P0) padded, (1, total, scale0 * total) packed.  off = row_off as device ints (None: padded, the layout
# row_off[b] = b * rows); rows_max = the longest utterance's rows.
Layout = namedtuple("Layout", "B Bc rows rows_max off rows0 scale0")


def _layout(meta, B, dev):
    Tp, P0 = meta["Tp"], meta["P0"]
    pk = _pack_of(meta, dev)
    if pk is None:
        return Layout(B, B, Tp, Tp, None, P0, P0 // Tp)
    off, rows_max, total, scale0 = pk
    assert scale0 * Tp == P0
    return Layout(B, 1, total, rows_max, off, scale0 * total, scale0)


def _conv0_forward(lay, wav, w, T0, **kw):
    """conv layer 0 -> bf16 [Bc * rows0 + 8, C], zero-filled where the kernel does not write (alignment padding, the 8 slack rows)."""
    if lay.off is None:
        return ops.conv0(wav, w, T0, lay.rows0, **kw)
    out = torch.zeros(lay.rows0 + 8, w.shape[0], device=wav.device, dtype=BF)
    return ops.conv0_packed(wav, w, T0, lay.off, lay.scale0, lay.rows_max, lay.rows, out=out, **kw)


def _posconv(lay, x, lim_i32, wg, d, G, Kw):
    """The grouped positional conv of x bf16 [Bc * rows, d] (rows >= lim[b] of utterance b read as zero) -> conv slabs, utterance b = [G][rows_b][d/G]."""
    if lay.off is None:
        return ops.posconv_conv(x, lim_i32, wg, lay.B, lay.rows, d, G, Kw)
    return ops.posconv_conv_packed(x, lim_i32, lay.off, wg, lay.B, lay.rows_max, lay.rows, d, G, Kw)


def posconv_tail_backward(lay, ds, u, xp, valid, pg, pv, d, G, Kw):
    """s = mask(xp) + gelu(u), u = grouped_conv(mask(xp)) + bias, weight-normalised weight (g, v): gradient ds of s ->
    (dxp bf16 [Bc * rows, d], dg, dv, dbias)."""
    B = lay.B
    du = ops.gelu_bwd_bf16(u, ds)
    dbias = ops.colsum_bf16(du)
    wfold, norm = _fold_weight_norm(pg, pv)
    _, wg_adj = _pos_operands(wfold, G, Kw)
    # dX: the same conv with the adjoint operand on du, time reversed inside each utterance's own rows (all of them count: no mask on the gradient)
    rows_b = ops.dev_ints([lay.rows] * B, torch.int32, ds.device) if lay.off is None else (lay.off[1:] - lay.off[:-1]).contiguous()
    convT = _posconv(lay, ops.reverse_rows_bf16(du, B, lay.rows, d, lay.off), rows_b, wg_adj, d, G, Kw)
    dxp = ops.posconv_dgrad_finish(convT, ds, valid, B, lay.rows, d, G, lay.off)
    if lay.off is None:        # gradient of the FOLDED weight
        dwf = posconv_wgrad(du, xp, valid, B, lay.rows, d, G, Kw)
    else:
        dwf = posconv_wgrad_packed(du, xp, valid, rows_b, lay.off, B, lay.rows, d, G, Kw)
    v = pv.detach().float()
    dot = (dwf * v).sum(dim=(0, 1), keepdim=True)                     # weight-norm: w = g v / |v|  (norm over dims 0, 1 per tap)
    gf = pg.detach().float()
    return dxp, (dot / norm).to(pg.dtype), (gf / norm * dwf - gf * dot / norm.pow(3) * v).to(pv.dtype), dbias


def _tail_forward(lay, meta, x6, valid_i32, flw, flb, pw, pb, pg, pv, pbias):
    """The stretch both nodes share: x6 bf16 [Bc * rows, C] (conv stack output) -> feats = LN(x6) -> xp = [dropout] proj(feats) -> u = pos_conv(mask(xp)) + bias,
    s = mask(xp) + gelu(u).  -> (feats, xp, u, s)"""
    d, G, Kw = meta["d"], meta["G"], meta["Kw"]
    feats = ops.layernorm(x6, _f32(flw), _f32(flb))
    xp = ops.gemm(feats, pw.detach().to(BF).contiguous(), _f32(pb))
    drop = meta.get("drop")          # dict(features, hidden, seed): dropout_input on the projected features, F.dropout on hidden state 0
    if drop is not None and drop["features"] > 0:
        ops.dropout_bf16(xp, drop["features"], drop["seed"] ^ 0x2545F491, out=xp)
    wfold, _ = _fold_weight_norm(pg, pv)
    wg, _ = _pos_operands(wfold, G, Kw)
    conv = _posconv(lay, xp, valid_i32, wg, d, G, Kw)
    u, s_ = ops.posconv_finish_train(xp, valid_i32, conv, _f32(pbias), lay.B, lay.rows, d, G, lay.off)
    return feats, xp, u, s_


def _tail_backward(lay, meta, ds, u, xp, feats, x6, valid, flw, pw, pg, pv):
    """Backward of _tail_forward from ds (gradient of s) -> (gradient entering the conv stack bf16 [Bc * rows, C], scaled by grad_mult,
    [d feat-LN w, b, d proj w, b, d pos g, v, bias])."""
    drop = meta.get("drop")
    # ---- s = mask(xp) + gelu(u),  u = conv(mask(xp)) + bias
    dxp, dpg, dpv, dpbias = posconv_tail_backward(lay, ds, u, xp, valid, pg, pv, meta["d"], meta["G"], meta["Kw"])
    if drop is not None and drop["features"] > 0:
        ops.dropout_bf16(dxp, drop["features"], drop["seed"] ^ 0x2545F491, out=dxp)      # saved xp is the dropped tensor; its gradient takes the same mask
    if meta.get("trace") is not None:
        meta["trace"]["dxp"] = dxp
    # ---- xp = [dropout] (feats W^T + b) ; feats = LN(x6)
    dfeats = ops.gemm(dxp, pw.detach().t().to(BF).contiguous())
    dpw, dpb = wgrad(dxp, feats), ops.colsum_bf16(dxp)
    g, dflw, dflb = ops.layernorm_bwd_bf16(x6, dfeats, _f32(flw), 1e-5)
    mult = float(meta["grad_mult"])
    if mult != 1.0:      # [3P fairseq] GradMultiply on the feature extractor's output
        g = ops.axpy_bf16(torch.zeros_like(g), g, mult)
    return g, [dflw, dflb, dpw, dpb, dpg, dpv, dpbias]


class HubertFrontTrainFn(torch.autograd.Function):
    """h0 bf16 [Bc * rows, d] = LN(mask(x) + gelu(pos_conv(mask(x)))) with x = proj(LN(conv stack(wav))).
    args: meta (conv_layers, T0, P0, Tp, d, G, Kw, grad_mult, train: compute parameter gradients), wav f32 [B, L], valid_i32 [B], N_FRONT tensors."""

    @staticmethod
    def forward(ctx, meta, wav, valid_i32, *params):
        assert len(params) == N_FRONT
        c0w, gnw, gnb = params[:3]
        cws = params[3:9]
        elw, elb = params[16:]
        cl, T0 = meta["conv_layers"], meta["T0"]
        dev = wav.device
        C = cl[0][0]
        lay = _layout(meta, wav.shape[0], dev)
        Bc, rows = lay.Bc, lay.rows0
        x = _conv0_forward(lay, wav, _f32(c0w).reshape(C, -1), T0, gn_gamma=_f32(gnw), gn_beta=_f32(gnb))
        acts = [x]
        for (dim, k, s), w in zip(cl[1:], cws):
            rows //= s
            y = _rows_with_slack(Bc * rows, dim, dev)
            ops.gemm(x, _conv_w16(w), None, ACT_GELU, out=y[:Bc * rows], M=Bc * rows, K=k * C, lda=s * C)
            acts.append(y)
            x, C = y, dim
        assert rows == lay.rows
        feats, xp, u, s_ = _tail_forward(lay, meta, x[:Bc * rows], valid_i32, *params[9:16])
        h0 = ops.layernorm(s_, _f32(elw), _f32(elb), 1e-5)
        drop = meta.get("drop")
        if drop is not None and drop["hidden"] > 0:
            h0 = ops.dropout_bf16(h0, drop["hidden"], drop["seed"] ^ 0x61C88647)
        ctx.meta = meta
        ctx.valid = valid_i32
        ctx.save_for_backward(wav, *acts, feats, xp, u, s_, *[p.detach() for p in params])
        return h0

    @staticmethod
    def backward(ctx, dh0):
        meta = ctx.meta
        cl, T0 = meta["conv_layers"], meta["T0"]
        t = ctx.saved_tensors
        wav, acts, (feats, xp, u, s_), params = t[0], t[1:8], t[8:12], t[12:]
        c0w, gnw, gnb = params[:3]
        cws = params[3:9]
        flw, flb, pw, pb, pg, pv, pbias, elw, elb = params[9:]
        lay = _layout(meta, wav.shape[0], wav.device)
        Bc = lay.Bc
        grads = [None] * N_FRONT
        drop = meta.get("drop")
        dh0 = dh0.to(BF).contiguous()
        if drop is not None and drop["hidden"] > 0:
            dh0 = ops.dropout_bf16(dh0, drop["hidden"], drop["seed"] ^ 0x61C88647)
        # ---- h0 = [dropout] LN(s)
        ds, grads[16], grads[17] = ops.layernorm_bwd_bf16(s_, dh0, _f32(elw), 1e-5)
        g, grads[9:16] = _tail_backward(lay, meta, ds, u, xp, feats, acts[6][:Bc * lay.rows], ctx.valid, flw, pw, pg, pv)
        del ds
        # ---- conv layers 6 .. 1
        rows_out = lay.rows
        for i in range(6, 0, -1):
            dim, k, s = cl[i]
            C = cl[i - 1][0]
            xin = acts[i - 1]
            Mi = Bc * rows_out
            rows_in = rows_out * s
            w16 = _conv_w16(cws[i - 1])
            upre = ops.gemm(xin, w16, None, ACT_NONE, M=Mi, K=k * C, lda=s * C)        # pre-activation, recomputed
            du_i = ops.gelu_bwd_bf16(upre, g)
            del upre
            grads[3 + i - 1], dx = conv_layer_backward(xin, cws[i - 1], du_i, Bc, rows_out, dim, k, s, C)
            g = dx[:Bc * rows_in]
            rows_out = rows_in
            del du_i
            if meta.get("trace") is not None:      # tests: the input gradient of every conv level
                meta["trace"]["dx%d" % (i - 1)] = g
        assert rows_out == lay.rows0
        # ---- conv layer 0 from the wave
        C0 = cl[0][0]
        dw0, grads[1], grads[2], part = ops.conv0_bwd(wav, _f32(c0w).reshape(C0, -1), _f32(gnw), _f32(gnb), g.contiguous(), T0, lay.rows0,
                                                      row_off_i32=lay.off, row_scale=lay.scale0)
        grads[0] = dw0.view_as(c0w)
        if meta.get("trace") is not None:
            meta["trace"]["conv0_part"] = part
        return (None, None, None, *grads)


N_FRONT_LN = 35   # 7 x (conv w, conv b, ln w, ln b), feat-LN w b, proj w b, pos g v bias


def front_params_ln(enc) -> list:
    """Front-end tensors of a LayerNorm-extractor / pre-LN model (HuBERT-large) in HubertFrontLNTrainFn's order.  `encoder.layer_norm` is not among
    them: with layer_norm_first the reference applies it to the encoder's final `x` only, which the hidden states never see (speech_encoder_plus.py:101)."""
    convs = enc.feature_extractor.conv_layers
    assert enc.cfg.extractor_mode == "layer_norm" and enc.cfg.conv_bias and enc.cfg.layer_norm_first and len(convs) == 7
    out = []
    for blk in convs:
        c, ln = getattr(blk, "0"), getattr(getattr(blk, "2"), "1")
        out += [c.weight, c.bias, ln.weight, ln.bias]
    pc = getattr(enc.encoder.pos_conv, "0")
    return out + [enc.layer_norm.weight, enc.layer_norm.bias, enc.post_extract_proj.weight, enc.post_extract_proj.bias, pc.weight_g, pc.weight_v, pc.bias]


class HubertFrontLNTrainFn(torch.autograd.Function):
    """The same node for the LayerNorm extractor + pre-LN encoder (HuBERT-large): every conv layer is conv + bias -> LayerNorm(C) -> GELU, the wave is
    layer-normalised per utterance first (no parameters), and hidden state 0 = mask(x) + gelu(pos_conv(mask(x))) WITHOUT a LayerNorm, in fp32.
    The large checkpoint has no dropouts and feature_grad_mult = 1."""

    @staticmethod
    def forward(ctx, meta, wav, lens_i32, valid_i32, *params):
        assert len(params) == N_FRONT_LN
        cl, T0 = meta["conv_layers"], meta["T0"]
        assert meta.get("drop") is None, "the LayerNorm-extractor model has no dropouts"
        dev = wav.device
        if meta["normalize"]:
            wav = ops.wave_layernorm(wav.contiguous(), lens_i32)
        C = cl[0][0]
        w0, b0, g0, be0 = params[:4]
        lay = _layout(meta, wav.shape[0], dev)
        Bc, rows = lay.Bc, lay.rows0
        u = _conv0_forward(lay, wav, _f32(w0).reshape(C, -1), T0, bias=_f32(b0))              # conv + bias; rows the kernel does not write are zeros
        pre, acts = [u], []
        x = torch.zeros_like(u)
        ops.layernorm(u[:Bc * rows], _f32(g0), _f32(be0), gelu=True, out=x[:Bc * rows])
        acts.append(x)
        for li, (dim, k, s) in enumerate(cl[1:], start=1):
            w, b, g, be = params[4 * li:4 * li + 4]
            rows //= s
            u = _rows_with_slack(Bc * rows, dim, dev)
            ops.gemm(x, _conv_w16(w), _f32(b), ACT_NONE, out=u[:Bc * rows], M=Bc * rows, K=k * C, lda=s * C)
            y = _rows_with_slack(Bc * rows, dim, dev)
            ops.layernorm(u[:Bc * rows], _f32(g), _f32(be), gelu=True, out=y[:Bc * rows])
            pre.append(u)
            acts.append(y)
            x, C = y, dim
        assert rows == lay.rows
        feats, xp, upos, s_ = _tail_forward(lay, meta, x[:Bc * rows], valid_i32, *params[28:])
        ctx.meta = meta
        ctx.valid = valid_i32
        ctx.save_for_backward(wav, *pre, *acts, feats, xp, upos, *[p.detach() for p in params])
        return s_.float()                                                                     # hidden state 0 of a pre-LN model lives on the fp32 stream

    @staticmethod
    def backward(ctx, dh0):
        meta = ctx.meta
        cl, T0 = meta["conv_layers"], meta["T0"]
        t = ctx.saved_tensors
        wav, pre, acts, (feats, xp, upos), params = t[0], t[1:8], t[8:15], t[15:18], t[18:]
        flw, flb, pw, pb, pg, pv, pbias = params[28:]
        lay = _layout(meta, wav.shape[0], wav.device)
        Bc = lay.Bc
        grads = [None] * N_FRONT_LN
        g, grads[28:] = _tail_backward(lay, meta, dh0.to(BF).contiguous(), upos, xp, feats, acts[6][:Bc * lay.rows], ctx.valid, flw, pw, pg, pv)
        rows_out = lay.rows
        for li in range(6, -1, -1):
            dim, k, s = cl[li]
            w, b, gam, bet = params[4 * li:4 * li + 4]
            u = pre[li][:Bc * rows_out]
            z = ops.layernorm(u, _f32(gam), _f32(bet))                                        # the GELU's argument, recomputed
            dz = ops.gelu_bwd_bf16(z, g.contiguous())
            del z
            du, grads[4 * li + 2], grads[4 * li + 3] = ops.layernorm_bwd_bf16(u, dz, _f32(gam), 1e-5)
            del dz
            if li == 0:
                dw0, grads[1], part = ops.conv0_wgrad(wav, du.contiguous(), cl[0][0], T0, lay.rows0, row_off_i32=lay.off, row_scale=lay.scale0)
                grads[0] = dw0.view_as(w)
                if meta.get("trace") is not None:
                    meta["trace"]["conv0_part"] = part
                break
            C = cl[li - 1][0]
            grads[4 * li + 1] = ops.colsum_bf16(du)
            grads[4 * li], dx = conv_layer_backward(acts[li - 1], w, du, Bc, rows_out, dim, k, s, C)
            rows_out = rows_out * s
            g = dx[:Bc * rows_out]
            if meta.get("trace") is not None:
                meta["trace"]["dx%d" % (li - 1)] = g
        return (None, None, None, None, *grads)

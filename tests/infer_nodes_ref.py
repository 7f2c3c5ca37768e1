"""Plain fp64 restatements of the EVAL-MODE host drivers (module/hubert.py extract_all_layers, the encoder wrapper's layer mix and hidden-state normalisation,
the image tower's forward) for tests/test_infer_nodes_parity_gpu.py and tools/infer_node_bounds.py.  A helper module, not a test; no kernel runs here.

The bodies are those of tests/train_mode_ref.py (conv_stack, front_stretch(node=False), post_ln_layer without masks) and tests/train_nodes_ref.py (pre_ln_layer,
the forward half of image_tower_node); what is new here is the wiring around them: which state lands in which slot, what the pre-LN model stores in front of its
layers, the layer mix and the two hidden-state normalisations.  One utterance at a time, from the product's own weights: the reference never sees a neighbour,
and the only padding it sees is the utterance's own zero samples.

model: False (fp64), "bf16" or "f16" -- the CPU model of a correct implementation with the layers' 16-bit stores (LayerNorm outputs, q | k | v, P, the attention
output, fc1's output, the layer weights) in that format; the residual stream and xmid of a pre-LN model are fp32.  Post-LN models exist in bf16 only.
`probe` (a dict) receives the largest magnitude handed to a 16-bit store of the layers, for the half-range case.
wiring: the MUTANTS, one wrong wiring each, listed in tools/infer_node_bounds.py."""
import torch
import torch.nn.functional as F

from train_mode_ref import F64, bound_of, conv_stack, front_params_of, front_stretch, fold_weight_norm, layer_params_of, post_ln_layer, r16, r32, row_metric, tensor_metric   # noqa: F401
from train_nodes_ref import image_tower_node, pre_ln_layer   # noqa: F401

HALF_MAX = 65504.0


def rh(t):
    """IEEE-half store (round to nearest even, unsaturated) of an fp64 value, back in fp64"""
    return t.to(torch.float32).to(torch.float16).to(F64)


def fmt_of(model, probe=None):
    """-> (model on?, the 16-bit store of the layers)"""
    if not model:
        return False, r16
    assert model in ("bf16", "f16"), model
    f = rh if model == "f16" else r16
    if probe is None:
        return True, f

    def probed(t):
        probe["max"] = max(probe.get("max", 0.0), t.detach().abs().max().item())
        return f(t)
    probed.plain = f
    return True, probed


def front_pre_ln(x6, valid, p, G, Kw, model=False, eps=1e-5):
    """Hidden state 0 of a PRE-LN model: train_mode_ref.front_stretch(node=False) without the encoder LayerNorm, stored in fp32 (the positional-conv kernel
    writes the fp32 stream; encoder.layer_norm only touches the final x, which no caller reads)."""
    st = r16 if model else (lambda t: t)
    rows, C = x6.shape
    feats = st(F.layer_norm(x6, (C,), p["flw"], p["flb"], eps))
    xp = st(feats @ st(p["pw"]).t() + p["pb"])
    xm = xp * (torch.arange(rows) < valid).to(F64)[:, None]
    conv = st(F.conv1d(xm.t()[None], st(fold_weight_norm(p["pg"], p["pv"])), None, padding=Kw // 2, groups=G)[0, :, :rows].t())
    s = xm + F.gelu(conv + p["pbias"])
    return r32(s) if model else s


def _swap_ln(P):
    P = list(P)
    P[8], P[9], P[14], P[15] = P[14], P[15], P[8], P[9]
    return P


def encoder_eval(enc, wav, lens, pack=None, drop_layers=(), stop_layer=None, model=False, rows="valid", conv0_fused=True, wiring=(), probe=None, h0=None):
    """module.hubert.HubertModel.extract_all_layers in eval, from the product's own weights (`enc` on the CPU): for every utterance the list of hidden states on
    its valid frames (rows="all": on all T frames of its own zero-padded wave, what the padded layout holds; method2 averages over them).  wav [B, lmax]
    zero-padded, lens: samples.  pack: the packed geometry or None -- the result does not depend on it, that IS the statement.  drop_layers: the listed layers
    leave no state; stop_layer = L: states 0 .. L.  h0[b] fp64 [valid_b, d]: state 0 is GIVEN (the driver's own, or the CPU model's) and only the layers run --
    the front end is bf16 whatever the layers' format, so its error hides what the operand format of the layers changes.
    wiring (MUTANTS): "ln_swapped" (ln1 / ln2 affines exchanged), "res_after_ln" (pre-LN), "res2_from_h" (post-LN), "enc_ln_flipped" (the encoder LayerNorm
    missing on state 0 of a post-LN model, present on a pre-LN one), "wave_ln_padded", "gn_own_len", "halo_key" (the row behind the valid frames admitted as a
    key), "key_mask_short" (one valid key less), "keep_dropped" (a dropped layer still runs and keeps its slot).
    -> hidden[b] = list of fp64 [rows_b, d]"""
    cfg = enc.cfg
    pre = bool(cfg.layer_norm_first)
    on, fmt = fmt_of(model, probe)
    assert pre or model in (False, "bf16"), "post-LN layers store bf16"
    B, lmax = wav.shape
    T0, T, P0, Tp = enc.frame_geometry(lmax)
    valid = enc.valid_frames(lens, lmax, T)
    fp = front_params_of(enc)
    lp = [layer_params_of(l) for l in enc.encoder.layers]
    if "ln_swapped" in wiring:
        lp = [_swap_ln(P) for P in lp]
    H, G, Kw = cfg.encoder_attention_heads, cfg.conv_pos_groups, cfg.conv_pos
    body_wiring = tuple(w for w in wiring if w in ("res_after_ln", "res2_from_h"))
    out = []
    with torch.no_grad():
        for b in range(B):
            n = valid[b]
            if h0 is not None:
                assert rows == "valid" and not wiring and h0[b].shape[0] == n
            take = T if rows == "all" else min(n + 1, T) if "halo_key" in wiring else n
            own0 = (int(lens[b]) - cfg.conv_layers[0][1]) // cfg.conv_layers[0][2] + 1
            if h0 is not None:
                h = h0[b].to(F64)
            else:
                x6 = conv_stack(enc, wav[b], int(lens[b]), on, conv0_fused, wave_len=lmax if "wave_ln_padded" in wiring else None,
                                gn_frames=max(own0, 1) if "gn_own_len" in wiring else None)[:take]
                with_ln = pre == ("enc_ln_flipped" in wiring)
                h = front_stretch(x6, n, fp, None, G, Kw, on, node=False) if with_ln else front_pre_ln(x6, n, fp, G, Kw, on)
            keys = [take if "halo_key" in wiring else n - 1 if ("key_mask_short" in wiring and n > 1) else n]
            hs = [h]
            for i, P in enumerate(lp):
                if stop_layer is not None and i >= stop_layer:
                    break
                if i in drop_layers and "keep_dropped" not in wiring:
                    continue
                if pre:
                    h = pre_ln_layer(h[None], P, keys, None, on, "gelu", wiring=body_wiring, heads=H, fmt=fmt)[0]
                else:
                    h = post_ln_layer(h[None], P, keys, None, on, wiring=body_wiring, heads=H)[0]
                hs.append(h)
            if "keep_dropped" in wiring:
                hs = hs[:len(hs) - len([i for i in drop_layers if stop_layer is None or i < stop_layer])]
            out.append([t[:T if rows == "all" else n] for t in hs])
    return out


def mix_eval(hidden, w, normalize, model=False, wiring=()):
    """The layer mix (sc_weighted_sum_fwd): hidden fp64 [n, rows, d] (the stored states), w fp64 [n] (pre-softmax) -> sum_l softmax(w)_l [LN](hidden_l), the
    affine-free LayerNorm (eps 1e-5) per state with `normalize`; stored in bf16.
    wiring (MUTANTS): "w_shifted" (the weights moved by one state), "ln_on_mix" (the LayerNorm on the mixed output instead of per state),
    "softmax_more" (the softmax taken over one weight more than there are states)."""
    n, d = hidden.shape[0], hidden.shape[-1]
    if "softmax_more" in wiring:
        a = torch.softmax(torch.cat([w, w[-1:]]), 0)[:n]
    else:
        a = torch.softmax(w, 0)
    if "w_shifted" in wiring:
        a = torch.roll(a, 1, 0)
    src = F.layer_norm(hidden, (d,), None, None, 1e-5) if normalize and "ln_on_mix" not in wiring else hidden
    mixed = (a.view(-1, 1, 1) * src).sum(0)
    if normalize and "ln_on_mix" in wiring:
        mixed = F.layer_norm(mixed, (d,), None, None, 1e-5)
    return r16(mixed) if model else mixed


def hidden_normalize(hidden, T, method, store=None):
    """speech_encoder_plus.py:572-592 on ONE utterance's states, hidden fp64 [n, rows, d] with rows >= T for method2: method1 = every frame x / (||x|| + 1e-8);
    method2 = every frame of a state divided by the mean of ||x|| over its first T frames (all frames of the padded batch, padded frames included).
    store: the format the states are overwritten in (the model), None = fp64."""
    nrm = hidden.norm(dim=-1, keepdim=True)
    if method == "method1":
        out = hidden / (nrm + 1e-8)
    else:
        assert method == "method2" and hidden.shape[1] >= T
        out = hidden / nrm[:, :T].mean(1, keepdim=True)
    return store(out) if store is not None else out


def image_tower_eval(image, params, cfg, model=False, wiring=()):
    """CLIP.encode_image: the forward of train_nodes_ref.image_tower_node (the same kernels at the same rounding points).  -> feat fp64 [B, E]"""
    return image_tower_node(image, params, cfg, torch.zeros(image.shape[0], params["proj"].shape[1], dtype=F64), model, wiring)["feat"]


# ================================================================================================ the parallel branch
def _split16(p12, D):
    iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = p12
    return [iw[:D], ib[:D], iw[D:2 * D], ib[D:2 * D], iw[2 * D:], ib[2 * D:], ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b]


def _attend(q, k, v, dead, model, out32=False):
    """[H, Tq, hd] x [H, Tk, hd]: fp32 softmax, probabilities in bf16 into the product, output stored in bf16 (fp32 where the kernel writes fp32)"""
    st = r16 if model else (lambda t: t)
    s = (q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    p = st(torch.softmax(s.masked_fill(dead, float("-inf")), -1))
    o = p @ v
    return (r32(o) if out32 else r16(o)) if model else o


def post_ln_rows_layer(x, p16, dead, heads, model=False, eps=1e-5):
    """TransformerEncoder._layer_rows, post-LN: nn.TransformerEncoderLayer on fp32 ROWS x [T, d] -- unlike the encoder's post-LN body the stream between the
    kernels is fp32 (residual GEMMs and LayerNorms write fp32); bf16: the GEMM operands x, att, x1, the q | k | v, the probabilities, the GELU output."""
    st, s32 = (r16, r32) if model else ((lambda t: t),) * 2
    qw, qb, kw, kb, vw, vb, ow, ob, g1, b1n, w1, b1, w2, b2, g2, b2n = p16
    T, d = x.shape
    hd = d // heads
    qkv = st(st(x) @ torch.cat([st(qw), st(kw), st(vw)], 0).t() + torch.cat([qb, kb, vb]))
    q, k, v = [t.view(T, heads, hd).transpose(0, 1) for t in qkv.split(d, dim=-1)]
    att = _attend(q, k, v, dead, model).transpose(0, 1).reshape(T, d)
    y = s32(att @ st(ow).t() + ob + x)
    x1 = s32(F.layer_norm(y, (d,), g1, b1n, eps))
    h = st(F.gelu(st(x1) @ st(w1).t() + b1))
    y2 = s32(h @ st(w2).t() + b2 + x1)
    return s32(F.layer_norm(y2, (d,), g2, b2n, eps))


def branch_eval(cls, frames, lens, params, heads, pre_ln, n_layers, model=False, wiring=(), eps=1e-5):
    """kw_modules.TransformerModels.TransformerEncoder in eval.  cls fp64 [D]; frames[b] fp64 [T, D] (bf16 values); params: 12 tensors per layer
    (train_nodes_ref.BRANCH_NAMES) then the final norm's weight and bias.  One utterance at a time on the rows [CLS; frames < len], every one of them a key.
    -> (cls_rows [B, D]: forward_cls -- the algebraic CLS-rows head for one post-LN layer, else layers 0 .. n-2 on every row and the last layer on the CLS row;
        full[b] [len_b + 1, D]: the full-row forward, every layer and the final norm on every row).  In fp64 the CLS row of `full` IS cls_rows (asserted), and both
    are torch.nn.TransformerEncoder in double (tools/infer_node_bounds.py).  The model's rounding points follow the two drivers, which differ.
    wiring (MUTANTS): "no_final_norm", "cls_key_masked" (key 0 masked for the utterance of length 1)."""
    st, s32 = (r16, r32) if model else ((lambda t: t),) * 2
    D, H = cls.shape[0], heads
    hd = D // H
    nfw, nfb = params[-2:]
    final = (lambda t: t) if "no_final_norm" in wiring else (lambda t: s32(F.layer_norm(t, (D,), nfw, nfb, 1e-5)))
    cls_rows, full = [], []
    for b, f in enumerate(frames):
        nb = int(lens[b]) + 1
        x0 = torch.cat([cls[None], f[:nb - 1]], 0)
        dead = torch.zeros(nb, dtype=torch.bool)
        if "cls_key_masked" in wiring and nb == 2:
            dead[0] = True

        def rows_layer(x, li):
            p16 = _split16(params[12 * li:12 * li + 12], D)
            if pre_ln:
                if dead.any():          # pre_ln_layer masks keys by a length: the one mutant that masks key 0 runs the body on the frame row alone for its keys
                    raise NotImplementedError
                return pre_ln_layer(x[None], p16, [nb], None, model, "gelu", eps, heads=H)[0]
            return post_ln_rows_layer(x, p16, dead, H, model, eps)
        # ---- the full-row forward
        x = s32(x0)
        for li in range(n_layers):
            x = rows_layer(x, li)
        full.append(final(x))
        # ---- forward_cls
        x = s32(x0)
        for li in range(n_layers - 1):
            x = rows_layer(x, li)
        iw, ib, ow, ob, n1w, n1b, l1w, l1b, l2w, l2b, n2w, n2b = params[12 * (n_layers - 1):12 * n_layers]
        xc = x[:1]
        if n_layers == 1 and not pre_ln:
            # the algebraic head (sc_cls_pool_fwd): u_h = scale Wk_h^T q_h and the CLS token in bf16, the frames as they are; scores, softmax, the pooled sums and
            # the value projection at fp32 grade (hi | lo split operands)
            q = ((xc @ iw[:D].t() + ib[:D]) * hd ** -0.5).view(H, hd)
            wk, bk = iw[D:2 * D].view(H, hd, D), ib[D:2 * D].view(H, hd)
            u = st(torch.einsum("hk,hkd->hd", q, wk))
            z = torch.cat([st(xc), x[1:]], 0)
            s = s32(z @ u.t() + (q * bk).sum(-1)).t()                                   # [H, nb]
            p = s32(torch.softmax(s.masked_fill(dead[None], float("-inf")), -1))
            xbar = s32(p @ z)                                                           # [H, D]
            att = s32(torch.einsum("hd,hkd->hk", xbar, iw[2 * D:].view(H, hd, D)) + ib[2 * D:].view(H, hd)).reshape(1, D)
        else:
            if pre_ln:
                a_all, ac = st(F.layer_norm(x, (D,), n1w, n1b, eps)), s32(F.layer_norm(xc, (D,), n1w, n1b, eps))
            else:
                a_all, ac = st(x), xc
            kv = st(a_all @ st(iw[D:]).t() + ib[D:])
            qc = st(ac @ iw[:D].t() + ib[:D])
            k, v = [t.view(nb, H, hd).transpose(0, 1) for t in kv.split(D, dim=-1)]
            att = _attend(qc.view(1, H, hd).transpose(0, 1), k, v, dead, model, out32=True).transpose(0, 1).reshape(1, D)
        y = s32(att @ ow.t() + ob + xc)
        if pre_ln:
            a2 = s32(F.layer_norm(y, (D,), n2w, n2b, eps))
            out = s32(s32(F.gelu(a2 @ l1w.t() + l1b)) @ l2w.t() + l2b + y)
        else:
            x1 = s32(F.layer_norm(y, (D,), n1w, n1b, eps))
            out = s32(F.layer_norm(s32(s32(F.gelu(x1 @ l1w.t() + l1b)) @ l2w.t() + l2b + x1), (D,), n2w, n2b, eps))
        cls_rows.append(final(out)[0])
        if not model:
            assert (cls_rows[-1] - full[-1][0]).abs().max().item() <= 1e-10 * full[-1][0].abs().max().item(), "fp64: the CLS row of the full-row forward is forward_cls"
    return torch.stack(cls_rows), full


# ================================================================================================ the text tower
def text_tower_eval(clip, ids, model=False, wiring=()):
    """CLIP.encode_text_ids / _encode_text_embeddings_eval from the product's own weights (`clip`: module.clip_model.CLIP on the CPU), one caption at a time: token
    plus position embedding (fp32), the causal pre-LN QuickGELU blocks on the positions 0 .. EOT (EOT = argmax of the ids), ln_final on the EOT row (stored in
    bf16), the projection as a 16-bit operand with an fp32 output.  A row depends on no later position, so the padded driver computes the same rows.
    wiring (MUTANTS): "eot_off" (the row in front of the EOT row taken), "causal_plus1" (key i + 1 admitted), "pos_by_packed_row" (the positional embedding
    indexed by the packed row instead of the position).
    -> (feat fp64 [B, E], stream[b] fp64 [EOT_b + 1, W]: the residual stream entering ln_final)"""
    st, s32 = (r16, r32) if model else ((lambda t: t),) * 2
    d64 = lambda t: t.detach().double()      # noqa: E731
    tok, pos = d64(clip.token_embedding.weight), d64(clip.positional_embedding)
    W, H = tok.shape[1], clip.transformer.heads
    blocks = []
    for blk in clip.transformer.resblocks:
        iw, ib = d64(blk.attn.in_proj_weight), d64(blk.attn.in_proj_bias)
        blocks.append([iw[:W], ib[:W], iw[W:2 * W], ib[W:2 * W], iw[2 * W:], ib[2 * W:], d64(blk.attn.out_proj.weight), d64(blk.attn.out_proj.bias), d64(blk.ln_1.weight),
                       d64(blk.ln_1.bias), d64(blk.mlp.c_fc.weight), d64(blk.mlp.c_fc.bias), d64(blk.mlp.c_proj.weight), d64(blk.mlp.c_proj.bias), d64(blk.ln_2.weight),
                       d64(blk.ln_2.bias)])
    feats, streams, off = [], [], 0
    with torch.no_grad():
        for b in range(ids.shape[0]):
            n = int(ids[b].argmax()) + 1
            where = (off + torch.arange(n)) % pos.shape[0] if "pos_by_packed_row" in wiring else torch.arange(n)
            off += n
            x = s32(tok[ids[b, :n]] + pos[where])
            for p16 in blocks:
                x = pre_ln_layer(x[None], p16, [n], None, bool(model), "quickgelu", heads=H, causal=2 if "causal_plus1" in wiring else True)[0]
            streams.append(x)
            row = x[max(n - 2, 0) if "eot_off" in wiring else n - 1]
            nrm = st(F.layer_norm(row, (W,), d64(clip.ln_final.weight), d64(clip.ln_final.bias), 1e-5))
            feats.append(s32(nrm @ st(d64(clip.text_projection))))
    return torch.stack(feats), streams

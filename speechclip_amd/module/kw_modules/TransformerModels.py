"""CLS-pooling heads (avssl/module/kw_modules/TransformerModels.py:48-135) on the HIP kernels.

`TransformerEncoder` (parallel branch: n post-LN or pre-LN encoder layers + final LayerNorm) and
`MultiheadAttentionAndNorm` (cascaded branch: LN(MHA(x) + x)) keep the reference's constructor arguments and
`state_dict` key names (`model.layers.0.self_attn.in_proj_weight`, `model.norm.*`,
`multihead_attn_layer.*`, `attentionBlock_Norm.*`).  The reference evaluates every row of
[CLS ; frames] and then keeps only the CLS rows (kwClip.py:1099, :879); here only the CLS rows are computed
(`forward_cls`): K/V for all frames, Q / attention / FFN / LayerNorm for the NQ learned tokens only.  A branch deeper than one layer (or
pre-LN) runs layers 0..n-2 on every row of [CLS; frames] and the last layer on the CLS rows only (`_forward_cls_stack`).
"""
import os
import weakref

import torch
import torch.nn as nn

from ... import ops
from ...ops import ACT_GELU

__all__ = ["TransformerEncoder", "MultiheadAttentionAndNorm"]
BF = torch.bfloat16


def _frames_view(audio_feat: torch.Tensor):
    """[B,T,D] (possibly a [:, :T] slice of a [B,Tp,D] buffer) -> (rows2d [B*Tp, D], Tp) without copying."""
    B, T, D = audio_feat.shape
    if audio_feat.stride(2) == 1 and audio_feat.stride(1) == D and audio_feat.stride(0) % D == 0 and audio_feat.dtype == BF:
        Tp = audio_feat.stride(0) // D if B > 1 else T
        if audio_feat.untyped_storage().nbytes() // 2 - audio_feat.storage_offset() >= B * Tp * D or Tp == T:
            return torch.as_strided(audio_feat, (B * Tp, D), (D, 1)), Tp
    x = audio_feat.to(BF).contiguous()
    return x.view(B * T, D), T


_POOL_CACHE = {}
_CAST_CACHE = {}


def cached_cast(t: torch.Tensor, dtype) -> torch.Tensor:
    """Detached, contiguous copy of parameter `t` in `dtype`, rebuilt only when the parameter changes (torch's in-place version counter
    moves on torch optimizer steps / load_state_dict; ops.param_epoch() moves on FusedAdam steps, which write through raw pointers): the
    eval forward does not re-cast the frozen branch weights on every call."""
    key = (t.data_ptr(), dtype)
    ver = (t._version, ops.param_epoch(t), t.device, tuple(t.shape))
    hit = _CAST_CACHE.get(key)
    if hit is not None and hit[0] == ver and hit[2]() is t:      # same tensor OBJECT: a freed tensor's address can be reused
        return hit[1]
    out = t.detach().to(dtype).contiguous()
    if len(_CAST_CACHE) > 4096:
        _CAST_CACHE.clear()
    _CAST_CACHE[key] = (ver, out, weakref.ref(t))
    return out


def _w3(w32: torch.Tensor) -> torch.Tensor:
    """[W_hi | W_hi | W_lo] bf16 [N, 3K] of an fp32 weight [N, K]: with the activation as (a_hi | a_lo | a_hi) (sc_split_hilo_bf16, nblk = 3) ONE
    bf16 MFMA GEMM of depth 3K adds a_hi W_hi + a_lo W_hi + a_hi W_lo = a W to ~16 bits on BOTH operands (the a_lo W_lo term is 2^-16 relative)."""
    hi = w32.to(BF)
    lo = (w32 - hi.float()).to(BF)
    return torch.cat([hi, hi, lo], dim=1).contiguous()


def cached_w3(t: torch.Tensor) -> torch.Tensor:
    """_w3 of an nn.Linear weight, cached like cached_cast."""
    key = (t.data_ptr(), "w3")
    ver = (t._version, ops.param_epoch(t), t.device, tuple(t.shape))
    hit = _CAST_CACHE.get(key)
    if hit is not None and hit[0] == ver and hit[2]() is t:
        return hit[1]
    out = _w3(t.detach().float())
    _CAST_CACHE[key] = (ver, out, weakref.ref(t))
    return out


def hp_linear(a32: torch.Tensor, weight: torch.Tensor, bias, act: int = 0, residual=None) -> torch.Tensor:
    """f32 [M, N] = act(a32 @ W^T + b) (+ residual) at fp32-grade precision on the bf16 MFMA GEMM: activation and weight are both split into bf16
    (hi, lo) halves and ONE GEMM of depth 3K adds the three significant products in fp32 (see _w3).  Used for the B x NQ CLS rows of the pooling
    heads only (< 0.1 % of the step): on the benchmark batch (T = 499, white-noise utterances) the embeddings of different utterances differ by
    1e-2 of their norm, so both the per-utterance noise of a bf16-rounded activation (2e-3) and the common shift of bf16-rounded weights
    (2e-3) are visible in the centred-cosine parity of the embedding (tests/test_headline_parity_gpu.py); the reference runs these rows in fp32."""
    b = None if bias is None else cached_cast(bias, torch.float32)
    N, K = weight.shape
    if (3 * K) % 64 or N % 4:        # shapes the MFMA GEMM does not take (reduced test dimensions): the fp32 SIMT product (no split-K at these sizes)
        y = ops.sgemm(a32.contiguous(), cached_cast(weight, torch.float32), transb=True, bias=b)
        if act == ACT_GELU:
            y = ops.gelu_f32(y)
        elif act:
            raise NotImplementedError("hp_linear: activation %d on the sgemm fallback" % act)
        return y if residual is None else y + residual
    if K >= 2048 and a32.shape[0] <= 1024 and K % 256 == 0 and act in (0, ACT_GELU):
        # few rows, deep K (linear2 of the branch layer: 256 x 768 x (3 x 3072) is three 256 x 256 tiles walking 144 k-steps each, 104 us): a
        # DETERMINISTIC split-K -- K chunks as a batched GEMM into fp32 partials, summed in fixed order (sc_sgemm's own split-K uses atomics)
        return ops.gemm_splitk(ops.split_hilo(a32, 3), cached_w3(weight), 768 if (3 * K) % 768 == 0 else 256, b, act, residual)
    return ops.gemm(ops.split_hilo(a32, 3), cached_w3(weight), b, act, residual, out_f32=True)


HEAD_PRECISE = os.environ.get("SC_HEAD_PRECISE", "1") != "0"      # 0: the round-3 head (bf16 activations between the CLS-row GEMMs), for A/B timing


def _pool_operands(cls, in_w, in_b, heads):
    """Parameter-only preprocessing of the algebraic CLS pooling (cached per parameter version, like weight-norm folding):
    u_r = scale * Wk_h^T Q_{q,h},  beta_r = scale * Q_{q,h} . bk_h  for r = (q, h);  Q = Wq cls + bq."""
    key = (cls.data_ptr(), in_w.data_ptr(), in_b.data_ptr(), heads)
    ver = (cls._version, in_w._version, in_b._version, ops.param_epoch(cls, in_w, in_b), cls.device)
    hit = _POOL_CACHE.get(key)
    if hit is not None and hit[0] == ver and all(r() is o for r, o in zip(hit[2], (cls, in_w, in_b))):   # object identity, not just addresses
        return hit[1]
    with torch.no_grad():
        NQ, D = cls.shape[-2], cls.shape[-1]
        hd = D // heads
        c = cls.detach().reshape(NQ, D).float()
        w, b = in_w.detach().float(), in_b.detach().float()
        # the matrix products run on sc_sgemm / sc_sgemm_batched (fp32 SIMT, this library): no vendor BLAS kernel on the product path, not even in
        # the cached parameter preprocessing (`@` / einsum on device tensors launched Tensile kernels)
        q = ops.sgemm(c.contiguous(), w[:D].contiguous(), transb=True, bias=b[:D].contiguous(), alpha=1.0)          # [NQ, D] = c Wq^T + bq
        q = (q * hd ** -0.5).contiguous()
        # u[q, h, :] = q[q, h, :] . Wk_h  (Wk_h = rows [h hd, (h+1) hd) of w[D:2D]): `heads` products [NQ, hd] x [hd, D], strided views of q / Wk / u
        wk = w[D:2 * D].contiguous()
        u = torch.empty(NQ, heads * D, device=c.device, dtype=torch.float32)
        ops.sgemm_batched(NQ, D, hd, q, D, hd, wk, D, hd * D, u, heads * D, D, heads)
        u = u.view(NQ * heads, D)
        beta = (q.view(NQ, heads, hd) * b[D:2 * D].view(1, heads, hd)).sum(-1).reshape(NQ * heads).contiguous()
        c16 = c.to(BF)
        wv16 = w[2 * D:].to(BF).contiguous()
        u16 = u.to(BF).contiguous()
        ops_ = dict(u16=u16, beta=beta, cls16=c16.contiguous(), wv=wv16, wv3=_w3(w[2 * D:]), bv=b[2 * D:].contiguous(),
                    cls_scores=ops.sgemm(c16.float().contiguous(), u16.float().contiguous(), transb=True, bias=beta))                    # [NQ, R]
    if len(_POOL_CACHE) > 256:
        _POOL_CACHE.clear()
    _POOL_CACHE[key] = (ver, ops_, tuple(weakref.ref(o) for o in (cls, in_w, in_b)))
    return ops_


def _cls_attention_block(cls: torch.Tensor, audio_feat: torch.Tensor, audio_len: torch.Tensor, in_w, in_b, heads: int, precise: bool = False):
    """CLS-rows-only attention in its algebraic form (sc_cls_pool_fwd): scores x.u_r + beta_r over [CLS tokens ; valid frames],
    softmax, probability-weighted frame sums, then the per-head value projection as a small batched GEMM.  K/V of the frames
    are never materialised.  Returns [B*NQ, D] (the concatenated head outputs, before out_proj): f32 when `precise`, else bf16."""
    B = audio_feat.shape[0]
    NQ, D = cls.shape[-2], cls.shape[-1]
    hd, R = D // heads, NQ * heads
    rows, Tp = _frames_view(audio_feat)
    P = _pool_operands(cls, in_w, in_b, heads)
    lens = audio_len.to(device=rows.device, dtype=torch.int32).contiguous()
    scores = ops.gemm(rows, P["u16"], P["beta"], out_f32=True)                              # [B*Tp, R] = x . u_r + beta_r
    if precise:
        # pooled sums as (hi | lo | hi) bf16 blocks, value projection as a depth-3D GEMM against [Wv_hi | Wv_hi | Wv_lo], fp32 out: neither the
        # pooled vector nor the weight is rounded to 8 bits
        xbar3 = ops.cls_pool(rows, P["cls16"], scores, P["cls_scores"], lens, B, Tp, NQ, R, D, split=3)   # bf16 [B, R, 3D]
        out = torch.empty(B * NQ, D, device=rows.device, dtype=torch.float32)
        ops.gemm_batched(xbar3, R * 3 * D, 3 * D, P["wv3"], hd * 3 * D, heads, out, NQ * D, hd, P["bv"], B, hd, 3 * D, R)
        return out
    xbar = ops.cls_pool(rows, P["cls16"], scores, P["cls_scores"], lens, B, Tp, NQ, R, D)   # bf16 [B, R, D]
    out = torch.empty(B * NQ, D, device=rows.device, dtype=BF)
    ops.gemm_batched(xbar, R * D, D, P["wv"], hd * D, heads, out, NQ * D, hd, P["bv"], B, hd, D, R)
    return out


class _EncoderStack(nn.Module):
    def __init__(self, layer_args, n_layers, d_model):
        super().__init__()
        self.layers = nn.ModuleList([nn.TransformerEncoderLayer(**layer_args) for _ in range(n_layers)])
        self.norm = nn.LayerNorm(d_model, eps=1e-5)


class TransformerEncoder(nn.Module):
    def __init__(self, n_layers: int = 1, d_model: int = 768, nhead: int = 8, dim_feedforward: int = 3072, dropout: float = 0.1,
                 activation: str = "gelu", layer_norm_eps: float = 1e-5, batch_first: bool = True, norm_first: bool = False) -> None:
        super().__init__()
        if activation != "gelu" or not batch_first:
            raise NotImplementedError("MI355X parallel branch supports GELU layers with batch_first=True")
        if n_layers < 1:
            raise ValueError(f"TransformerEncoder: n_layers={n_layers} must be >= 1")
        # n_layers == 1 post-LN (the shipped shape) keeps the algebraic CLS-rows head; any other depth / order runs the stack
        # (full-row layers 0..n-2 on sc_attention_hd_fwd, CLS rows of the last layer), which takes the head dims of that kernel
        self.stacked = n_layers != 1 or norm_first
        if self.stacked and (d_model % nhead or d_model // nhead not in ops.ATTN_HD_DIMS):
            raise NotImplementedError(f"MI355X parallel branch with n_layers={n_layers}, norm_first={norm_first}: head_dim "
                                      f"{d_model / nhead:g} (d_model {d_model} / nhead {nhead}) is not in the supported set {{64, 96, 128}}")
        self.nhead, self.eps, self.n_layers, self.norm_first = nhead, layer_norm_eps, n_layers, norm_first
        self.model = _EncoderStack(dict(d_model=d_model, nhead=nhead, dim_feedforward=dim_feedforward, dropout=dropout,
                                        activation=activation, layer_norm_eps=layer_norm_eps, batch_first=batch_first,
                                        norm_first=norm_first), n_layers, d_model)

    def forward_cls(self, cls: torch.Tensor, audio_feat: torch.Tensor, audio_len: torch.Tensor) -> torch.Tensor:
        """cls [1,1,D]; audio_feat bf16 [B,T,D]; audio_len [B] (valid frames, without the CLS).  -> f32 [B, D]: row 0 of norm(layers([CLS; x]))
        -- what kwClip.py:1097-1099 keeps.  The one-layer post-LN head returns bf16 with SC_HEAD_PRECISE=0; the stack (`_forward_cls_stack`)
        ignores SC_HEAD_PRECISE and always returns f32."""
        if self.stacked:
            return self._forward_cls_stack(cls, audio_feat, audio_len)
        L = self.model.layers[0]
        sa = L.self_attn
        D = cls.shape[-1]
        f32 = lambda t: cached_cast(t, torch.float32)  # noqa: E731
        w16 = lambda t: cached_cast(t, BF)             # noqa: E731
        if HEAD_PRECISE:
            # the CLS row stays fp32 from the pooled sums to the embedding (the reference runs this branch in fp32 / autocast with fp32 LayerNorms):
            # every Linear is a (hi | lo)-split GEMM (hp_linear), LayerNorms fp32 in / fp32 out.  B rows: < 0.1 % of the step.
            att = _cls_attention_block(cls, audio_feat, audio_len, sa.in_proj_weight, sa.in_proj_bias, self.nhead, precise=True)
            y = hp_linear(att, sa.out_proj.weight, sa.out_proj.bias, residual=f32(cls).reshape(1, D).expand(att.shape[0], D))   # x + SA(x), CLS rows
            x1 = ops.layernorm(y, f32(L.norm1.weight), f32(L.norm1.bias), self.eps, out_f32=True)
            h = hp_linear(x1, L.linear1.weight, L.linear1.bias, ACT_GELU)
            y2 = hp_linear(h, L.linear2.weight, L.linear2.bias, residual=x1)
            x2 = ops.layernorm(y2, f32(L.norm2.weight), f32(L.norm2.bias), self.eps, out_f32=True)
            return ops.layernorm(x2, f32(self.model.norm.weight), f32(self.model.norm.bias), 1e-5, out_f32=True)
        att = _cls_attention_block(cls, audio_feat, audio_len, sa.in_proj_weight, sa.in_proj_bias, self.nhead)
        y = ops.gemm(att, w16(sa.out_proj.weight), f32(sa.out_proj.bias), residual=f32(cls).reshape(1, D).expand(att.shape[0], D),
                     out_f32=True)                                                       # x + SA(x), CLS rows
        x1 = ops.layernorm(y, f32(L.norm1.weight), f32(L.norm1.bias), self.eps, out_f32=True)
        x1b = ops.layernorm(y, f32(L.norm1.weight), f32(L.norm1.bias), self.eps)
        h = ops.gemm(x1b, w16(L.linear1.weight), f32(L.linear1.bias), ACT_GELU)
        y2 = ops.gemm(h, w16(L.linear2.weight), f32(L.linear2.bias), residual=x1, out_f32=True)
        x2 = ops.layernorm(y2, f32(L.norm2.weight), f32(L.norm2.bias), self.eps, out_f32=True)
        return ops.layernorm(x2, f32(self.model.norm.weight), f32(self.model.norm.bias), 1e-5)

    def forward_cls_train(self, cls: torch.Tensor, audio_feat: torch.Tensor, audio_len: torch.Tensor, seed: int = None) -> torch.Tensor:
        """The differentiable counterpart of `forward_cls` for the stack (n_layers >= 2 or norm_first): f32 [B, D] with gradients to `cls`,
        `audio_feat` (when it requires one) and every parameter of `self.model`, as ONE autograd node (train_branch.BranchStackTrainFn).  Dropout
        (rate `dropout` at the four sites of every layer) is active iff `self.training`; `seed` = None draws one from torch's generator."""
        if not self.stacked:
            raise NotImplementedError("forward_cls_train: the one-layer post-LN head trains through ParallelBranchTrainFn (its algebraic path)")
        from ...train_branch import BranchStackTrainFn, stack_params
        pd = float(self.model.layers[0].dropout.p) if self.training else 0.0
        if pd > 0 and seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        meta = dict(heads=self.nhead, eps=self.eps, pre_ln=self.norm_first, drop_p=pd, seed=int(seed or 0))
        return BranchStackTrainFn.apply(meta, cls, audio_feat.to(BF), audio_len, *stack_params(self.model))

    # ---- stack path (n_layers >= 2 or norm_first): layers 0..n-2 on every row of [CLS; frames] (padded [B, T + 1, d] rows, key lengths
    #      len + 1), then the last layer on the B CLS rows only: K / V of all rows, per-utterance CLS query.  Eval-mode arithmetic, no autograd.
    @torch.no_grad()
    def _forward_cls_stack(self, cls: torch.Tensor, audio_feat: torch.Tensor, audio_len: torch.Tensor) -> torch.Tensor:
        """-> f32 [B, D]: row 0 of norm(layers([CLS; x])).  Precision of the CLS rows: the last layer's out-proj, FFN and LayerNorms are
        fp32-grade (hp_linear), as in the one-layer head; its attention is bf16-grade -- query rounded to bf16, K / V from the bf16 GEMM, bf16
        probabilities into the MFMA, fp32 softmax and accumulation.  The one-layer head keeps the pooled value sums at fp32 grade; here the
        frames reaching the last layer have already been through bf16 full-row layers, so that step would not make the row fp32-grade."""
        B, T, D = audio_feat.shape
        Lq = T + 1
        x = torch.empty(B, Lq, D, device=audio_feat.device, dtype=torch.float32)
        x[:, 0] = cls.detach().reshape(D)
        x[:, 1:] = audio_feat.detach()
        x = x.view(B * Lq, D)
        klens = (audio_len.to(device=audio_feat.device, dtype=torch.int32) + 1).contiguous()
        hd = D // self.nhead
        attend = lambda qkv: ops.attention_hd_qkv(qkv, B, Lq, self.nhead, klens)   # noqa: E731
        for i in range(self.n_layers - 1):
            x = self._layer_rows(x, None, B, Lq, i, attend)
        # last layer, CLS rows only, fp32-grade (hp_linear) like forward_cls: K / V of every row feed one query per utterance
        L = self.model.layers[-1]
        sa = L.self_attn
        f32 = lambda t: cached_cast(t, torch.float32)  # noqa: E731
        xc = x.view(B, Lq, D)[:, 0].contiguous()
        if self.norm_first:
            a_all = ops.layernorm(x, f32(L.norm1.weight), f32(L.norm1.bias), self.eps)
            ac = ops.layernorm(xc, f32(L.norm1.weight), f32(L.norm1.bias), self.eps, out_f32=True)
        else:
            a_all, ac = x.to(BF), xc
        kv = ops.gemm(a_all, cached_cast(sa.in_proj_weight, BF)[D:], f32(sa.in_proj_bias)[D:])              # bf16 [B*Lq, 2D] = k | v
        qc = hp_linear(ac, sa.in_proj_weight, sa.in_proj_bias)[:, :D].to(BF).contiguous()                   # [B, D] (B rows: all of in_proj)
        att = ops.attention_hd(qc, kv, kv[:, D:], B, self.nhead, 1, Lq, hd, (D, D), (Lq * 2 * D, 2 * D), klens, out_f32=True).view(B, D)
        if self.norm_first:
            x1 = hp_linear(att, sa.out_proj.weight, sa.out_proj.bias, residual=xc)
            a2 = ops.layernorm(x1, f32(L.norm2.weight), f32(L.norm2.bias), self.eps, out_f32=True)
            y = hp_linear(hp_linear(a2, L.linear1.weight, L.linear1.bias, ACT_GELU), L.linear2.weight, L.linear2.bias, residual=x1)
        else:
            y = hp_linear(att, sa.out_proj.weight, sa.out_proj.bias, residual=xc)
            x1 = ops.layernorm(y, f32(L.norm1.weight), f32(L.norm1.bias), self.eps, out_f32=True)
            y2 = hp_linear(hp_linear(x1, L.linear1.weight, L.linear1.bias, ACT_GELU), L.linear2.weight, L.linear2.bias, residual=x1)
            y = ops.layernorm(y2, f32(L.norm2.weight), f32(L.norm2.bias), self.eps, out_f32=True)
        return ops.layernorm(y, f32(self.model.norm.weight), f32(self.model.norm.bias), 1e-5, out_f32=True)

    # ---- full-row path (TransformerModels.py:77-96): every position of [CLS; frames], any boolean key-padding mask.  Off the hot path
    #      (forward_cls is what KW_ParallelBranch.forward runs); eval-mode arithmetic (no dropout), no autograd.
    @torch.no_grad()
    def _layer_rows(self, x32: torch.Tensor, key_padding_mask, B: int, Lq: int, i: int = 0, attend=None) -> torch.Tensor:
        """nn.TransformerEncoderLayer i (post-LN, or pre-LN with norm_first) on fp32 rows [B*L, D] -> fp32 rows.  `attend(qkv)` -> bf16 [B*L, D]
        (default: attention_rows with the boolean key-padding mask)."""
        L = self.model.layers[i]
        sa = L.self_attn
        D = x32.shape[-1]
        f32 = lambda t: cached_cast(t, torch.float32)  # noqa: E731
        w16 = lambda t: cached_cast(t, BF)             # noqa: E731
        if attend is None:
            attend = lambda qkv: ops.attention_rows(qkv, B, Lq, self.nhead, D // self.nhead, key_padding_mask)   # noqa: E731
        if self.norm_first:         # x + SA(LN1(x)), then + FF(LN2(.))
            qkv = ops.gemm(ops.layernorm(x32, f32(L.norm1.weight), f32(L.norm1.bias), self.eps), w16(sa.in_proj_weight), f32(sa.in_proj_bias))
            x1 = ops.gemm(attend(qkv), w16(sa.out_proj.weight), f32(sa.out_proj.bias), residual=x32, out_f32=True)
            h = ops.gemm(ops.layernorm(x1, f32(L.norm2.weight), f32(L.norm2.bias), self.eps), w16(L.linear1.weight), f32(L.linear1.bias), ACT_GELU)
            return ops.gemm(h, w16(L.linear2.weight), f32(L.linear2.bias), residual=x1, out_f32=True)
        qkv = ops.gemm(x32.to(BF), w16(sa.in_proj_weight), f32(sa.in_proj_bias))
        att = attend(qkv)
        y = ops.gemm(att, w16(sa.out_proj.weight), f32(sa.out_proj.bias), residual=x32, out_f32=True)
        x1 = ops.layernorm(y, f32(L.norm1.weight), f32(L.norm1.bias), self.eps, out_f32=True)
        h = ops.gemm(x1.to(BF), w16(L.linear1.weight), f32(L.linear1.bias), ACT_GELU)
        y2 = ops.gemm(h, w16(L.linear2.weight), f32(L.linear2.bias), residual=x1, out_f32=True)
        return ops.layernorm(y2, f32(L.norm2.weight), f32(L.norm2.bias), self.eps, out_f32=True)

    @torch.no_grad()
    def forward(self, src: torch.Tensor, key_padding_mask: torch.Tensor = None):
        """src [B, L, D] -> fp32 [B, L, D] = norm(layer(src)) for every position (rows at padded positions are computed like any other
        query row, as torch's non-fused path does)."""
        return self.extract_hidden_states_and_output(src, key_padding_mask)[0]

    @torch.no_grad()
    def extract_hidden_states_and_output(self, src, key_padding_mask=None):
        B, Lq, D = src.shape
        x = src.detach().float().contiguous().view(B * Lq, D)
        hidden = [x.view(B, Lq, D)]
        for i in range(len(self.model.layers)):
            x = self._layer_rows(x, key_padding_mask, B, Lq, i)
            hidden.append(x.view(B, Lq, D))
        out = ops.layernorm(x, cached_cast(self.model.norm.weight, torch.float32), cached_cast(self.model.norm.bias, torch.float32), 1e-5, out_f32=True)
        return out.view(B, Lq, D), tuple(hidden)

    def extract_hidden_states(self, src: torch.Tensor, key_padding_mask: torch.Tensor = None):
        """(input of every layer ..., output of the last layer BEFORE the final norm) -- nnTransformerEncoder.extract_hidden_states
        (TransformerModels.py:16-44), element [1] as TransformerModels.py:83-96 returns it."""
        return self.extract_hidden_states_and_output(src, key_padding_mask)[1]


class MultiheadAttentionAndNorm(nn.Module):
    def __init__(self, d_model: int = 768, nhead: int = 8, dropout: float = 0.1, layer_norm_eps: float = 1e-5,
                 batch_first: bool = True, **kwargs) -> None:
        super().__init__()
        self.nhead, self.eps = nhead, layer_norm_eps
        self.multihead_attn_layer = nn.MultiheadAttention(d_model, num_heads=nhead, dropout=dropout, batch_first=batch_first)
        self.attentionBlock_Norm = nn.LayerNorm(d_model, eps=layer_norm_eps)

    def forward_cls(self, cls: torch.Tensor, audio_feat: torch.Tensor, audio_len: torch.Tensor) -> torch.Tensor:
        """cls [1,K,D] -> f32 [B, K, D] (bf16 with SC_HEAD_PRECISE=0): rows 0..K-1 of LN(MHA([CLS;x]) + [CLS;x])  (kwClip.py:877-881)."""
        m = self.multihead_attn_layer
        NQ, D = cls.shape[-2], cls.shape[-1]
        B = audio_feat.shape[0]
        res = cls.detach().float().reshape(1, NQ, D).expand(B, NQ, D).reshape(B * NQ, D).contiguous()
        n = self.attentionBlock_Norm
        if HEAD_PRECISE:          # fp32 keyword rows (see TransformerEncoder.forward_cls)
            att = _cls_attention_block(cls, audio_feat, audio_len, m.in_proj_weight, m.in_proj_bias, self.nhead, precise=True)
            y = hp_linear(att, m.out_proj.weight, m.out_proj.bias, residual=res)
            return ops.layernorm(y, cached_cast(n.weight, torch.float32), cached_cast(n.bias, torch.float32), self.eps, out_f32=True).view(B, NQ, D)
        att = _cls_attention_block(cls, audio_feat, audio_len, m.in_proj_weight, m.in_proj_bias, self.nhead)
        y = ops.gemm(att, cached_cast(m.out_proj.weight, BF), cached_cast(m.out_proj.bias, torch.float32), residual=res, out_f32=True)
        return ops.layernorm(y, cached_cast(n.weight, torch.float32), cached_cast(n.bias, torch.float32), self.eps).view(B, NQ, D)

    @torch.no_grad()
    def forward(self, src: torch.Tensor, key_padding_mask: torch.Tensor = None):
        """Full-row LN(MHA(src) + src) (TransformerModels.py:119-125): src [B, L, D] -> fp32 [B, L, D].  Off the hot path (forward_cls is what
        KW_CascadedBranch.forward runs); eval-mode arithmetic, no autograd."""
        m = self.multihead_attn_layer
        B, Lq, D = src.shape
        x = src.detach().float().contiguous().view(B * Lq, D)
        qkv = ops.gemm(x.to(BF), cached_cast(m.in_proj_weight, BF), cached_cast(m.in_proj_bias, torch.float32))
        att = ops.attention_rows(qkv, B, Lq, self.nhead, D // self.nhead, key_padding_mask)
        y = ops.gemm(att, cached_cast(m.out_proj.weight, BF), cached_cast(m.out_proj.bias, torch.float32), residual=x, out_f32=True)
        n = self.attentionBlock_Norm
        return ops.layernorm(y, cached_cast(n.weight, torch.float32), cached_cast(n.bias, torch.float32), self.eps, out_f32=True).view(B, Lq, D)

    def extract_hidden_states(self, src: torch.Tensor, key_padding_mask: torch.Tensor = None):
        """TransformerModels.py:127-128."""
        return tuple([src, self.forward(src, key_padding_mask)])

    @torch.no_grad()
    def extract_attention_map(self, src: torch.Tensor, key_padding_mask: torch.Tensor = None, query_rows: int = None):
        """TransformerModels.py:130-135: (LN(MHA(src) + src) fp32 [B, L, D], per-head attention probabilities fp32 [B, H, L, L]) -- torch's
        need_weights=True, average_attn_weights=False.  `query_rows=n` (an extension; the reference has no such argument) keeps the first n
        query rows of the map only: [B, H, n, L], which is all getAttentionMap reads (kwClip.py:941-949)."""
        m = self.multihead_attn_layer
        B, Lq, D = src.shape
        x = src.detach().float().contiguous().view(B * Lq, D)
        qkv = ops.gemm(x.to(BF), cached_cast(m.in_proj_weight, BF), cached_cast(m.in_proj_bias, torch.float32))
        hd = D // self.nhead
        att = ops.attention_rows(qkv, B, Lq, self.nhead, hd, key_padding_mask)
        probs = ops.attention_probs(qkv, B, Lq, self.nhead, hd, key_padding_mask, n_rows=query_rows)
        y = ops.gemm(att, cached_cast(m.out_proj.weight, BF), cached_cast(m.out_proj.bias, torch.float32), residual=x, out_f32=True)
        n = self.attentionBlock_Norm
        out = ops.layernorm(y, cached_cast(n.weight, torch.float32), cached_cast(n.bias, torch.float32), self.eps, out_f32=True).view(B, Lq, D)
        return out, probs

"""Tensor-level wrappers over the C ABI (include/speechclip_hip.h).

Only plumbing lives here: argument checks, output allocation, pointer extraction.  All arithmetic
happens inside libspeechclip_hip.so.  Every wrapper requires CUDA(HIP) tensors.
"""
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_GELU, ACT_NONE, ACT_QUICKGELU, ATTN_CAUSAL, ATTN_F16, ATTN_HD_OUT_F32, GEMM_F16, GEMM_OUT_F32, check, lib, ptr, stream

bf16 = torch.bfloat16

# Optional HIP-event instrumentation of the dominant kernel (bench.py roofline leg): when PROFILE is a list, every
# sc_gemm_bf16 launch appends (start_event, end_event, flops, shape_tag) recorded on the launch stream.
PROFILE = None
# HBM-bound segments (conv layer 0, LayerNorm, layer mix): when PROFILE_HBM is a list, each launch appends
# (start, end, algorithmic bytes, tag, stream) -- bench.py reports their GB/s against the 8 TB/s HBM peak
PROFILE_HBM = None


class _HbmSpan:
    __slots__ = ("tag", "nbytes", "e0")

    def __init__(self, tag, nbytes):
        self.tag, self.nbytes, self.e0 = tag, nbytes, None

    def __enter__(self):
        if PROFILE_HBM is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if self.e0 is not None and PROFILE_HBM is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROFILE_HBM.append((self.e0, e1, float(self.nbytes), self.tag, torch.cuda.current_stream().cuda_stream))
        return False
PROFILE_TAG = "speech"   # which part of the step is launching ("speech" / "image" / "head"): set by KWClip_GeneralTransformer.forward, stored as entry[5]
PROFILE_SIDE = []     # (start, end) HIP events of every side-stream window (the image tower running beside the speech tower) while PROFILE is on

_GEMM_WS = {}
# The plain GEMMs (QKV / out-proj / fc2 / ViT projections) run on the hand-written gemm256_kernel like everything else.  hipBLASLt behind
# the same entry (csrc/vendor_gemm.hip) is a COMPARATOR only: SC_GEMM_VENDOR=1 in the environment, or set_vendor_gemm(True) at run time
# (bench.py measures it beside the headline number); it is never on by default.
import os as _os
_VENDOR_GEMM = [_os.environ.get("SC_GEMM_VENDOR", "0") == "1"]


def set_vendor_gemm(enabled: bool) -> None:
    """Switch the vendor-library comparator path for plain GEMMs on / off (registers / drops the library workspace)."""
    _VENDOR_GEMM[0] = bool(enabled)
    if not enabled and _GEMM_WS:
        torch.cuda.synchronize()
        check(lib().sc_set_gemm_workspace(None, 0), "sc_set_gemm_workspace")
        _GEMM_WS.clear()


def vendor_gemm_enabled() -> bool:
    return _VENDOR_GEMM[0]


def _ensure_gemm_workspace(dev):
    """Comparator path only: one 64 MiB scratch buffer per process (one process per GPU) for the library (sc_set_gemm_workspace)."""
    if _VENDOR_GEMM[0] and dev not in _GEMM_WS:
        ws = torch.empty(64 << 20, device=dev, dtype=torch.uint8)
        check(lib().sc_set_gemm_workspace(ptr(ws), ws.numel()), "sc_set_gemm_workspace")
        _GEMM_WS.clear()          # the library keeps ONE registration: a process that hops devices re-registers
        _GEMM_WS[dev] = ws


# Parameter epoch: bumped by every optimizer step that writes parameters through raw pointers (train_tail.FusedAdam -> sc_adam_step does not
# move torch's per-tensor version counter).  Every parameter-derived cache (bf16 weight casts, pooling operands, cosine / VQ tables) carries
# it in its key, so an eval forward after training steps never sees pre-step weights.
_PARAM_EPOCH = [0]


def param_epoch(*tensors) -> int:
    """Current epoch; with tensors given, -1 if none of them is trainable (a frozen tensor cannot be written by an optimizer step, so its
    derived tables -- the 49408-row sub-word tables -- are not rebuilt after every step)."""
    if tensors and not any(t.requires_grad for t in tensors):
        return -1
    return _PARAM_EPOCH[0]


def bump_param_epoch() -> None:
    _PARAM_EPOCH[0] += 1


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SpeechClipHipError("speechclip_amd ops need device tensors (no CPU fallback)")


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
         residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_f32: bool = False,
         M: Optional[int] = None, K: Optional[int] = None, lda: Optional[int] = None) -> torch.Tensor:
    """out[M,N] = act(a[M,K] @ w[N,K]^T + bias) + residual.  `M/K/lda` override the logical A view
    (overlapping rows: conv-as-GEMM)."""
    _need_cuda(a, w)
    # operand format: bf16, or IEEE half for both operands (SC_GEMM_F16: the frozen pre-LN encoder layers; 16-bit outputs / residuals are half too)
    f16 = a.dtype == torch.float16
    op16 = torch.float16 if f16 else bf16
    assert a.dtype == op16 and w.dtype == op16 and w.dim() == 2 and w.is_contiguous(), (a.dtype, w.dtype)
    N, Kw = w.shape
    if M is None:
        assert a.dim() == 2 and a.stride(1) == 1
        M, K, lda = a.shape[0], a.shape[1], a.stride(0)
    assert K == Kw, (K, Kw)
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32 if out_f32 else op16)
    assert out.stride(-1) == 1 and out.dtype == (torch.float32 if out_f32 else op16)
    if residual is not None:
        assert residual.dtype == out.dtype and residual.stride(-1) == 1
    flags = act | (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_F16 if f16 else 0)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _ensure_gemm_workspace(a.device)
    check(lib().sc_gemm_bf16(ptr(a), lda, ptr(w), w.stride(0), ptr(out), out.stride(-2), ptr(bias), ptr(residual),
                             residual.stride(-2) if residual is not None else 0, M, N, K, flags, stream()), "sc_gemm_bf16")
    if PROFILE is not None:
        e1.record()
        PROFILE.append((e0, e1, 2.0 * M * N * K, (M, N, K, act, residual is not None, out_f32, int(lib().sc_gemm_last_path())),
                        torch.cuda.current_stream().cuda_stream, PROFILE_TAG))
    return out


def gemm_batched(a, lda, stride_a, w, stride_w, w_mod, out, ldc, stride_c, bias, M, N, K, batch, act=ACT_NONE, ldw=None):
    """`batch` products out_z[M,N] = a_z[M,K] w_{z % w_mod}[N,K]^T (+ bias); operand z at base + z * stride (elements); `a`, `w`, `out` may be
    views whose data_ptr is operand 0.  out dtype f32 => fp32 outputs."""
    _need_cuda(a, w, out)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    flags = act | (GEMM_OUT_F32 if out.dtype == torch.float32 else 0)
    check(lib().sc_gemm_bf16_batched(ptr(a), lda, stride_a, ptr(w), K if ldw is None else ldw, stride_w, w_mod, ptr(out), ldc, stride_c, ptr(bias),
                                     M, N, K, batch, flags, stream()), "sc_gemm_bf16_batched")
    if PROFILE is not None:
        e1.record()
        PROFILE.append((e0, e1, 2.0 * M * N * K * batch, (M, N, K, act, False, False, 0, batch),   # tag[6] = path (0 hand-written), tag[7] = batch
                        torch.cuda.current_stream().cuda_stream, PROFILE_TAG))
    return out


LN_IN_F32, LN_OUT_F32, LN_GELU, LN_OUT_F16 = 1, 2, 4, 8


def layernorm(x, gamma, beta, eps=1e-5, out=None, out_f32=False, gelu=False, rows=None, D=None, ld_in=None):
    """Row LayerNorm.  x: [..., D] (bf16 or f32, last dim contiguous); optional strided-row view via rows/D/ld_in."""
    _need_cuda(x)
    if rows is None:
        D = x.shape[-1]
        x2 = x.reshape(-1, D) if x.is_contiguous() else x
        assert x2.dim() == 2 and x2.stride(1) == 1
        rows, ld_in = x2.shape[0], x2.stride(0)
        shape = x.shape
    else:
        shape = (rows, D)
    ld_out = D
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32 if out_f32 else bf16)
    elif out.is_contiguous():
        assert out.numel() == rows * D, (tuple(out.shape), rows, D)
    else:                                    # a strided out: [rows, D] with its own row pitch
        assert out.dim() == 2 and tuple(out.shape) == (rows, D) and out.stride(1) == 1, (tuple(out.shape), out.stride(), rows, D)
        ld_out = out.stride(0)
    flags = (LN_IN_F32 if x.dtype == torch.float32 else 0) | (LN_OUT_F32 if out.dtype == torch.float32 else 0) | (LN_GELU if gelu else 0)
    if out.dtype == torch.float16:           # IEEE-half operand format of the pre-LN encoder layers (fp32 residual stream in)
        assert x.dtype == torch.float32
        flags |= LN_OUT_F16
    assert x.dtype in (bf16, torch.float32) and out.dtype in (bf16, torch.float16, torch.float32)
    with _HbmSpan("layernorm", rows * D * (x.element_size() + out.element_size())):
        check(lib().sc_layernorm(ptr(x), ld_in, ptr(gamma), ptr(beta), ptr(out), ld_out, rows, D, eps, flags, stream()), "sc_layernorm")
    return out


def weighted_sum(hidden, weights, normalize=False, eps=1e-5):
    """hidden: [n, rows, D] contiguous (bf16 or f32); weights f32 [n] (pre-softmax).  Returns bf16 [rows, D]."""
    _need_cuda(hidden, weights)
    n, rows, D = hidden.shape
    assert hidden.is_contiguous() and weights.dtype == torch.float32
    out = torch.empty(rows, D, device=hidden.device, dtype=bf16)
    flags = (1 if normalize else 0) | (2 if hidden.dtype == torch.float32 else 0)
    with _HbmSpan("layer_mix", rows * D * (n * hidden.element_size() + 2)):
        check(lib().sc_weighted_sum_fwd(ptr(hidden), rows * D, ptr(weights), ptr(out), n, rows, D, flags, eps, stream()), "sc_weighted_sum_fwd")
    return out


def hidden_normalize_(hidden, T, method):
    """In place: hidden [n, B, Tp, D] (bf16 / f32, contiguous) normalised as speech_encoder_plus.py:572-592 does for normalize_type "method1" / "method2"."""
    _need_cuda(hidden)
    assert hidden.dim() == 4 and hidden.is_contiguous() and hidden.dtype in (bf16, torch.float32) and method in ("method1", "method2")
    n, B, Tp, D = hidden.shape
    m = 1 if method == "method1" else 2
    ws = torch.empty(n * B * (Tp + 1), device=hidden.device, dtype=torch.float32) if m == 2 else None
    check(lib().sc_hidden_normalize(ptr(hidden), int(hidden.dtype == torch.float32), n, B, Tp, int(T), D, m, ptr(ws), stream()), "sc_hidden_normalize")
    return hidden


def gemm_splitk(a16, w16, K_chunk, bias=None, act=ACT_NONE, residual=None):
    """f32 [M, N] = act(a16 [M, K] @ w16 [N, K]^T + bias) + residual as a DETERMINISTIC split-K product: the K / K_chunk chunks run as one batched
    GEMM into fp32 partials [S, M, N] (S x more tiles for few-row, deep-K shapes), sc_splitk_reduce_f32 sums them in fixed order."""
    _need_cuda(a16, w16)
    assert a16.dtype == bf16 and w16.dtype == bf16 and a16.dim() == 2 and a16.is_contiguous() and w16.is_contiguous()
    M, K = a16.shape
    N = w16.shape[0]
    assert w16.shape[1] == K and K % K_chunk == 0 and K_chunk % 64 == 0 and N % 4 == 0
    S = K // K_chunk
    part = torch.empty(S, M, N, device=a16.device, dtype=torch.float32)
    gemm_batched(a16, K, K_chunk, w16, K_chunk, S, part, N, M * N, None, M, N, K_chunk, S, ldw=K)
    out = torch.empty(M, N, device=a16.device, dtype=torch.float32)
    if residual is not None:
        assert residual.dtype == torch.float32 and residual.stride(-1) == 1
    check(lib().sc_splitk_reduce_f32(ptr(part), S, M, N, ptr(bias), ptr(residual), residual.stride(-2) if residual is not None else 0, ptr(out), int(act),
                                     stream()), "sc_splitk_reduce_f32")
    return out


def l2norm(x, clamp=False):
    """x / ||x|| (no eps: kwClip.py:1436); clamp=True: x / max(||x||, 1e-8) (the operand normalisation of F.cosine_similarity)."""
    _need_cuda(x)
    assert x.dim() == 2 and x.stride(1) == 1
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(lib().sc_l2norm_fwd(ptr(x), x.stride(0), ptr(out), x.shape[0], x.shape[1], int(x.dtype == torch.float32) | (2 if clamp else 0), stream()), "sc_l2norm_fwd")
    return out


def wave_layernorm(wav, lens_i32, eps=1e-5):
    _need_cuda(wav, lens_i32)
    assert wav.dtype == torch.float32 and wav.is_contiguous() and lens_i32.dtype == torch.int32
    out = torch.empty_like(wav)
    check(lib().sc_wave_layernorm(ptr(wav), ptr(out), ptr(lens_i32), wav.shape[0], wav.shape[1], eps, stream()), "sc_wave_layernorm")
    return out


def attention(qkv, B, T, H, klens_i32=None, out=None, scale=None, causal=False, row_off_i32=None, drop=None):
    """qkv: bf16 (or IEEE half: SC_ATTN_F16) [rows, 3*H*64] packed (q|k|v); returns the same format [rows, H*64].  row_off_i32 None: uniform rows
    (rows = B*T); else packed rows, utterance b at rows row_off[b] .. (at most T each).  drop = (p, seed): dropout on the attention probabilities
    (train mode; p == 0 is the plain arithmetic).  scale / causal exist on the plain uniform entry only, IEEE half not on the uniform dropout one."""
    _need_cuda(qkv, klens_i32, row_off_i32)
    D = H * 64
    total = B * T if row_off_i32 is None else qkv.shape[0]
    assert qkv.dtype in (bf16, torch.float16) and qkv.shape == (total, 3 * D) and qkv.is_contiguous()
    f16 = qkv.dtype == torch.float16
    if (scale is not None or causal) and (row_off_i32 is not None or drop is not None):
        raise _lib.SpeechClipHipError("attention: scale / causal are served on uniform rows without dropout only")
    if f16 and drop is not None and row_off_i32 is None:
        raise _lib.SpeechClipHipError("attention: dropout on uniform rows is bf16 only")
    if out is None:
        out = torch.empty(total, D, device=qkv.device, dtype=qkv.dtype)
    assert out.dtype == qkv.dtype
    q, k, v = qkv.data_ptr(), qkv.data_ptr() + D * 2, qkv.data_ptr() + 2 * D * 2
    p_, seed = (float(drop[0]), int(drop[1]) & 0xffffffff) if drop is not None else (0.0, 0)
    if row_off_i32 is not None:
        check(lib().sc_attention_fwd_packed(q, k, v, ptr(out), ptr(klens_i32), ptr(row_off_i32), B, H, T, total, 64, 3 * D, D, 0.125, p_, seed,
                                            ATTN_F16 if f16 else 0, stream()), "sc_attention_fwd_packed")
    elif drop is not None:
        check(lib().sc_attention_fwd_dropout(q, k, v, ptr(out), ptr(klens_i32), B, H, T, 64, 3 * D, D, 0.125, 0, p_, seed, stream()), "sc_attention_fwd_dropout")
    else:
        check(lib().sc_attention_fwd(q, k, v, ptr(out), ptr(klens_i32), B, H, T, 64, 3 * D, D, 0.125 if scale is None else scale,
                                     (ATTN_CAUSAL if causal else 0) | (ATTN_F16 if f16 else 0), stream()), "sc_attention_fwd")
    return out


def attention_dropout(qkv, B, T, H, klens_i32, drop_p, seed, out=None):
    """ops.attention(..., drop=(drop_p, seed)) on uniform rows (kept for its callers)."""
    return attention(qkv, B, T, H, klens_i32, out=out, drop=(drop_p, seed))


def dropout_bf16(x, drop_p, seed, residual=None, out=None):
    """out = [residual +] dropout(x) (bf16, counter-based mask from `seed`); out=x runs in place."""
    _need_cuda(x)
    assert x.dtype == bf16 and x.is_contiguous() and (residual is None or (residual.dtype == bf16 and residual.is_contiguous() and residual.shape == x.shape))
    if out is None:
        out = torch.empty_like(x)
    check(lib().sc_dropout_bf16(ptr(x), ptr(residual), ptr(out), x.numel(), float(drop_p), int(seed) & 0xffffffff, stream()), "sc_dropout_bf16")
    return out


def dropout_add_layernorm(x, residual, gamma, beta, drop_p, seed, eps=1e-5, out=None):
    """out = LayerNorm(residual + dropout(x)) for bf16 [rows, D]: one fused pass for D = 768, else sc_dropout_bf16 (into x, in place) + layernorm."""
    _need_cuda(x, residual)
    assert x.dtype == bf16 and residual.dtype == bf16 and x.is_contiguous() and residual.is_contiguous() and x.shape == residual.shape and x.dim() == 2
    if out is None:
        out = torch.empty_like(x)
    rc = lib().sc_dropout_add_layernorm_bf16(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(out), x.shape[0], x.shape[1], eps, float(drop_p),
                                             int(seed) & 0xffffffff, stream())
    if rc == 1:
        dropout_bf16(x, drop_p, seed, residual=residual, out=x)
        return layernorm(x, gamma, beta, eps, out=out)
    check(rc, "sc_dropout_add_layernorm_bf16")
    return out


ATTN_HD_DIMS = (64, 96, 128)


def attention_hd(q, k, v, B, H, Tq, Tk, hd, q_strides, kv_strides, klens_i32=None, out=None, out_f32=False, scale=None, drop_p=0.0, seed=0):
    """Flash attention for head_dim 64 / 96 / 128 (sc_attention_hd_fwd).  q / k / v: bf16 views whose data_ptr is element (b 0, row 0, head 0);
    `q_strides` / `kv_strides` = (per-sequence, per-row) element strides.  Returns out [B, Tq, H*hd] (bf16, or f32 with out_f32); klens_i32 [B]
    valid keys per sequence (None = Tk); drop_p > 0: dropout on the probabilities (sc_attention_fwd_dropout's mask)."""
    _need_cuda(q, k, v)
    assert q.dtype == bf16 and k.dtype == bf16 and v.dtype == bf16
    D = H * hd
    if out is None:
        out = torch.empty(B, Tq, D, device=q.device, dtype=torch.float32 if out_f32 else bf16)
    assert out.dtype == (torch.float32 if out_f32 else bf16) and out.is_contiguous() and out.numel() == B * Tq * D
    check(lib().sc_attention_hd_fwd(ptr(q), ptr(k), ptr(v), ptr(out), ptr(klens_i32), B, H, Tq, Tk, hd, q_strides[0], q_strides[1],
                                    kv_strides[0], kv_strides[1], Tq * D, D, hd ** -0.5 if scale is None else scale, float(drop_p),
                                    int(seed) & 0xffffffff, ATTN_HD_OUT_F32 if out_f32 else 0, stream()), "sc_attention_hd_fwd")
    return out


def attention_hd_qkv(qkv, B, L, H, klens_i32=None, out_f32=False, drop_p=0.0, seed=0):
    """Full-row attention over packed rows qkv [B*L, 3*D] (q | k | v, D = H * head_dim) -> [B*L, D]."""
    assert qkv.dim() == 2 and qkv.is_contiguous() and qkv.shape[0] == B * L and qkv.shape[1] % (3 * H) == 0
    D = qkv.shape[1] // 3
    s = (L * 3 * D, 3 * D)
    out = attention_hd(qkv, qkv[:, D:], qkv[:, 2 * D:], B, H, L, L, D // H, s, s, klens_i32, out_f32=out_f32, drop_p=drop_p, seed=seed)
    return out.view(B * L, D)


def _attention_hd_bwd(q, k, v, O, dO, klens_i32, B, H, Tq, Tk, hd, q_strides, kv_strides, dq, dq_strides, dk, dv, dkv_strides, drop_p, seed):
    """sc_attention_hd_bwd into caller-owned dq / dk / dv views (data_ptr = element (b 0, row 0, head 0)); O / dO bf16 contiguous [B, Tq, H*hd]."""
    _need_cuda(q, k, v, O, dO, klens_i32)
    D = H * hd
    for t in (q, k, v, O, dO, dq, dk, dv):
        assert t.dtype == bf16
    assert O.is_contiguous() and dO.is_contiguous() and O.numel() == B * Tq * D and dO.numel() == B * Tq * D
    ws = torch.empty(lib().sc_attention_hd_bwd_workspace_bytes(B, H, Tq), device=q.device, dtype=torch.uint8)
    check(lib().sc_attention_hd_bwd(ptr(q), ptr(k), ptr(v), ptr(O), ptr(dO), ptr(klens_i32), B, H, Tq, Tk, hd, q_strides[0], q_strides[1], kv_strides[0],
                                    kv_strides[1], Tq * D, D, ptr(dq), dq_strides[0], dq_strides[1], ptr(dk), ptr(dv), dkv_strides[0], dkv_strides[1],
                                    hd ** -0.5, float(drop_p), int(seed) & 0xffffffff, ptr(ws), stream()), "sc_attention_hd_bwd")


def attention_hd_bwd(q, k, v, O, dO, B, H, Tq, Tk, hd, q_strides, kv_strides, klens_i32=None, drop_p=0.0, seed=0):
    """Backward of attention_hd (sc_attention_hd_bwd; Tq == Tk or Tq == 1, head_dim 64 / 96 / 128; anything else raises SpeechClipHipError).  q / k / v and
    their strides as attention_hd took them; O / dO bf16 [B, Tq, H*hd]: the forward's bf16 output and its gradient; (drop_p, seed) of that forward.
    Returns dq bf16 [B, Tq, D] and dk, dv: the two column halves of ONE bf16 [B, Tk, 2*D] buffer (dk | dv: what the k | v projection's backward consumes).
    The only temporary is the fp32 statistics workspace (2 floats per (b, h, query row))."""
    D = H * hd
    dq = torch.empty(B, Tq, D, device=q.device, dtype=bf16)
    dkv = torch.empty(B, Tk, 2 * D, device=q.device, dtype=bf16)
    dk, dv = dkv[..., :D], dkv[..., D:]
    _attention_hd_bwd(q, k, v, O, dO, klens_i32, B, H, Tq, Tk, hd, q_strides, kv_strides, dq, (Tq * D, D), dk, dv, (Tk * 2 * D, 2 * D), drop_p, seed)
    return dq, dk, dv


def attention_hd_qkv_bwd(qkv, att, datt, B, L, H, klens_i32=None, drop_p=0.0, seed=0):
    """Backward of attention_hd_qkv: qkv bf16 [B*L, 3*D] (q | k | v), att / datt bf16 [B*L, D] (the forward's output and its gradient) -> dqkv bf16 [B*L, 3*D]."""
    assert qkv.dim() == 2 and qkv.is_contiguous() and qkv.shape[0] == B * L and qkv.shape[1] % (3 * H) == 0
    D = qkv.shape[1] // 3
    assert att.shape == (B * L, D) and datt.shape == (B * L, D)
    s = (L * 3 * D, 3 * D)
    out = torch.empty(B * L, 3 * D, device=qkv.device, dtype=bf16)
    _attention_hd_bwd(qkv, qkv[:, D:], qkv[:, 2 * D:], att, datt, klens_i32, B, H, L, L, D // H, s, s, out, s, out[:, D:], out[:, 2 * D:], s, drop_p, seed)
    return out


def attention_rows(qkv, B, L, H, hd, key_padding_mask=None, scale=None):
    """Full-row MHA for any head dim: qkv bf16 [B*L, 3*H*hd] packed (q|k|v); key_padding_mask bool/uint8 [B, L] (True = padding) or None.
    Returns bf16 [B*L, H*hd] (heads concatenated, before out_proj)."""
    _need_cuda(qkv, key_padding_mask)
    D = H * hd
    assert qkv.dtype == bf16 and qkv.shape == (B * L, 3 * D) and qkv.is_contiguous()
    m = None
    if key_padding_mask is not None:
        assert key_padding_mask.shape == (B, L)
        m = key_padding_mask.to(torch.uint8).contiguous()
    out = torch.empty(B * L, D, device=qkv.device, dtype=bf16)
    check(lib().sc_attention_rows_fwd(qkv.data_ptr(), qkv.data_ptr() + D * 2, qkv.data_ptr() + 2 * D * 2, ptr(out), ptr(m), B, H, L, hd, 3 * D, D,
                                      hd ** -0.5 if scale is None else scale, stream()), "sc_attention_rows_fwd")
    return out


def attention_probs(qkv, B, L, H, hd, key_padding_mask=None, n_rows=None, scale=None):
    """Per-head attention probabilities (need_weights=True, average_attn_weights=False) of the first `n_rows` query rows (default: all):
    qkv bf16 [B*L, 3*H*hd] packed (q|k|v) -> f32 [B, H, n_rows, L]; exactly 0 at padded keys."""
    _need_cuda(qkv, key_padding_mask)
    D = H * hd
    assert qkv.dtype == bf16 and qkv.shape == (B * L, 3 * D) and qkv.is_contiguous()
    n_rows = L if n_rows is None else int(n_rows)
    m = None
    if key_padding_mask is not None:
        assert key_padding_mask.shape == (B, L)
        m = key_padding_mask.to(torch.uint8).contiguous()
    probs = torch.empty(B, H, n_rows, L, device=qkv.device, dtype=torch.float32)
    check(lib().sc_attention_probs_fwd(qkv.data_ptr(), qkv.data_ptr() + D * 2, ptr(probs), ptr(m), B, H, L, hd, n_rows, 3 * D,
                                       hd ** -0.5 if scale is None else scale, stream()), "sc_attention_probs_fwd")
    return probs


def topk_rows(x, k):
    """torch.topk(x, k, dim=-1) for f32 [..., V] on the device: (values f32 [..., k] descending, indices i64 [..., k]); ties -> lowest index."""
    _need_cuda(x)
    x2 = x.float().contiguous().view(-1, x.shape[-1])
    R, V = x2.shape
    vals = torch.empty(R, k, device=x.device, dtype=torch.float32)
    idx = torch.empty(R, k, device=x.device, dtype=torch.int32)
    check(lib().sc_topk_rows_f32(ptr(x2), V, R, V, int(k), ptr(vals), ptr(idx), stream()), "sc_topk_rows_f32")
    return vals.view(*x.shape[:-1], k), idx.long().view(*x.shape[:-1], k)


def cls_attention(cls_qkv, kv_x, lens_i32, B, T, NQ, H, hd):
    """cls_qkv bf16 [NQ, 3D]; kv_x bf16 [B*T, 2D]; returns bf16 [B, NQ, D]."""
    _need_cuda(cls_qkv, kv_x)
    D = H * hd
    assert cls_qkv.shape == (NQ, 3 * D) and kv_x.shape == (B * T, 2 * D) and cls_qkv.is_contiguous() and kv_x.is_contiguous()
    out = torch.empty(B, NQ, D, device=kv_x.device, dtype=bf16)
    check(lib().sc_cls_attention_fwd(ptr(cls_qkv), ptr(kv_x), 2 * D, ptr(lens_i32), ptr(out), B, T, NQ, H, hd, hd ** -0.5, stream()),
          "sc_cls_attention_fwd")
    return out


def cls_pool(x_rows, cls16, scores, cls_scores, lens_i32, B, T, NQ, R, D, split=0):
    """x_rows bf16 [B*T, D]; cls16 bf16 [NQ, D]; scores f32 [B*T, R]; cls_scores f32 [NQ, R] -> xbar bf16 [B, R, D], or with split = 2 / 3 the
    (hi | lo [| hi]) blocks bf16 [B, R, split*D] that keep the fp32 pooled sums to ~16 bits (operand of a depth-split*D GEMM against [W | W] /
    [W_hi | W_hi | W_lo])."""
    _need_cuda(x_rows, cls16, scores, cls_scores)
    assert x_rows.dtype == bf16 and x_rows.stride(1) == 1 and scores.dtype == torch.float32 and scores.shape == (B * T, R) and scores.is_contiguous()
    xbar = torch.empty(B, R, (split or 1) * D, device=x_rows.device, dtype=bf16)
    if split:
        check(lib().sc_cls_pool_fwd_split(ptr(x_rows), x_rows.stride(0), ptr(cls16), ptr(scores), ptr(cls_scores), ptr(lens_i32), ptr(xbar), B, T, NQ, R, D,
                                          int(split), stream()), "sc_cls_pool_fwd_split")
    else:
        check(lib().sc_cls_pool_fwd(ptr(x_rows), x_rows.stride(0), ptr(cls16), ptr(scores), ptr(cls_scores), ptr(lens_i32), ptr(xbar), B, T, NQ, R, D,
                                    stream()), "sc_cls_pool_fwd")
    return xbar


def conv0(wav, w, T0, P, gn_gamma=None, gn_beta=None, bias=None, eps=1e-5, out=None, ln_coef=None):
    """HuBERT conv layer 0.  wav f32 [B, L]; w f32 [C, 10].  GroupNorm+GELU if gn_gamma given, else raw conv + bias -- followed, when ln_coef
    (f32 [2 C + 1] = gamma | beta | eps) is given, by the LayerNorm over the channels + GELU of a "layer_norm" extractor in the same kernel.
    Returns channels-last bf16 [B, P, C] (+ (k-s) slack rows so the next conv-as-GEMM may over-read)."""
    _need_cuda(wav, w)
    B, L = wav.shape
    C = w.shape[0]
    assert wav.dtype == torch.float32 and wav.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous()
    buf = out if out is not None else torch.zeros(B * P + 8, C, device=wav.device, dtype=bf16)
    assert buf.dtype == bf16 and buf.is_contiguous() and buf.shape[0] >= B * P and buf.shape[1] == C
    wfrag = torch.empty(lib().sc_conv0_wfrag_workspace_bytes(B), device=wav.device, dtype=torch.uint8)
    if gn_gamma is not None:
        ws = torch.empty(lib().sc_conv0_stats_workspace_bytes(B), device=wav.device, dtype=torch.uint8)
        coef = torch.empty(B, C, 2, device=wav.device, dtype=torch.float32)
        with _HbmSpan("conv0_gn_stats", B * L * 4):
            check(lib().sc_conv0_gn_coef(ptr(wav), L, ptr(w), ptr(gn_gamma), ptr(gn_beta), ptr(ws), ptr(coef), B, C, T0, eps, stream()), "sc_conv0_gn_coef")
        with _HbmSpan("conv0", B * L * 4 + B * P * C * 2):
            check(lib().sc_conv0_fwd(ptr(wav), L, L, ptr(w), None, ptr(coef), ptr(buf), B, C, T0, P, 0, ptr(wfrag), stream()), "sc_conv0_fwd")
    else:
        assert ln_coef is None or (ln_coef.dtype == torch.float32 and ln_coef.numel() == 2 * C + 1 and ln_coef.is_contiguous())
        with _HbmSpan("conv0", B * L * 4 + B * P * C * 2):
            check(lib().sc_conv0_fwd(ptr(wav), L, L, ptr(w), ptr(bias), ptr(ln_coef), ptr(buf), B, C, T0, P, 1 if ln_coef is None else 2, ptr(wfrag), stream()), "sc_conv0_fwd")
    return buf


def posconv(x, valid_i32, wg, bias, gamma, beta, B, Tp, D, G, Kw, out=None, out_f32=False, eps=1e-5):
    """x bf16 [B*Tp, D]; wg bf16 [G, D/G, Kw*D/G] (folded weight-norm, K index = tap*cg + c_in)."""
    _need_cuda(x, wg)
    cg = D // G
    conv = torch.empty(B * G * Tp * cg, device=x.device, dtype=bf16)
    rc = lib().sc_posconv_conv(ptr(x), ptr(valid_i32), ptr(wg), ptr(conv), B, Tp, D, G, Kw, stream())
    if rc == 1:      # group width not covered by the windowed kernel: pack the sliding windows and use the batched GEMM
        _posconv_pack_gemm(x, valid_i32, wg, conv, B, Tp, D, G, Kw)
    else:
        check(rc, "sc_posconv_conv")
    if out is None:
        out = torch.empty(B * Tp, D, device=x.device, dtype=torch.float32 if out_f32 else bf16)
    check(lib().sc_posconv_finish(ptr(x), ptr(valid_i32), ptr(conv), ptr(bias), ptr(gamma), ptr(beta), ptr(out), B, Tp, D, G,
                                  int(out.dtype == torch.float32), eps, stream()), "sc_posconv_finish")
    return out


# ---------------------------------------------------------------------------------------------- padding-free (packed) batches
# Utterance b owns rows [row_off[b], row_off[b + 1]) of every transformer-level tensor (module/hubert.py: extract_all_layers_packed).
# The forward entries follow; the backward's packed entries (whole-encoder training on packed rows, train_front.py) sit with the front-end backward below.
def conv0_packed(wav, w, T0, row_off_i32, row_scale, rows_max, total_rows, gn_gamma=None, gn_beta=None, bias=None, eps=1e-5, out=None, ln_coef=None):
    """ops.conv0 writing utterance b at rows row_scale * row_off[b] ...; the GroupNorm statistics are those of the padded length T0."""
    _need_cuda(wav, w, row_off_i32)
    B, L = wav.shape
    C = w.shape[0]
    assert wav.dtype == torch.float32 and wav.is_contiguous() and w.dtype == torch.float32 and w.is_contiguous() and row_off_i32.dtype == torch.int32
    assert out is not None and out.dtype == bf16 and out.is_contiguous() and out.shape[0] >= row_scale * total_rows and out.shape[1] == C
    wfrag = torch.empty(lib().sc_conv0_wfrag_workspace_bytes(B), device=wav.device, dtype=torch.uint8)
    coef = None
    if gn_gamma is not None:
        ws = torch.empty(lib().sc_conv0_stats_workspace_bytes(B), device=wav.device, dtype=torch.uint8)
        coef = torch.empty(B, C, 2, device=wav.device, dtype=torch.float32)
        with _HbmSpan("conv0_gn_stats", B * L * 4):
            check(lib().sc_conv0_gn_coef(ptr(wav), L, ptr(w), ptr(gn_gamma), ptr(gn_beta), ptr(ws), ptr(coef), B, C, T0, eps, stream()), "sc_conv0_gn_coef")
    mode = 0 if gn_gamma is not None else 1
    if ln_coef is not None:      # conv + bias -> LayerNorm over the channels -> GELU in the same kernel (sc_conv0_fwd mode 2)
        assert gn_gamma is None and ln_coef.dtype == torch.float32 and ln_coef.numel() == 2 * C + 1 and ln_coef.is_contiguous()
        coef, mode = ln_coef, 2
    with _HbmSpan("conv0", row_scale * total_rows * (5 * 4 + C * 2)):
        check(lib().sc_conv0_fwd_packed(ptr(wav), L, L, ptr(w), None if gn_gamma is not None else ptr(bias), ptr(coef), ptr(out), B, C, T0,
                                        ptr(row_off_i32), row_scale, row_scale * rows_max, mode, ptr(wfrag), stream()),
              "sc_conv0_fwd_packed")
    return out


def posconv_packed(x, valid_i32, row_off_i32, wg, bias, gamma, beta, B, rows_max, total_rows, D, G, Kw, out=None, out_f32=False, eps=1e-5):
    """ops.posconv over packed rows: x bf16 [total_rows, D]."""
    _need_cuda(x, wg, row_off_i32)
    cg = D // G
    conv = torch.empty(total_rows * D, device=x.device, dtype=bf16)
    rc = lib().sc_posconv_conv_packed(ptr(x), ptr(valid_i32), ptr(row_off_i32), ptr(wg), ptr(conv), B, rows_max, D, G, Kw, stream())
    if rc == 1:
        raise _lib.SpeechClipHipError("packed batches need the windowed positional-conv kernel (D/G in 32/48/64 and Kw * D/G a multiple of 64), "
                                      f"got D/G = {cg}, Kw = {Kw}")
    check(rc, "sc_posconv_conv_packed")
    if out is None:
        out = torch.empty(total_rows, D, device=x.device, dtype=torch.float32 if out_f32 else bf16)
    check(lib().sc_posconv_finish_packed(ptr(x), ptr(valid_i32), ptr(row_off_i32), ptr(conv), ptr(bias), ptr(gamma), ptr(beta), ptr(out), B, total_rows, D, G,
                                         int(out.dtype == torch.float32), eps, stream()), "sc_posconv_finish_packed")
    return out


def attention_packed(qkv, B, rows_max, H, klens_i32, row_off_i32, out=None, drop_p=0.0, seed=0):
    """ops.attention over packed rows: qkv [total_rows, 3*H*64] (kept for its callers)."""
    return attention(qkv, B, rows_max, H, klens_i32, out=out, row_off_i32=row_off_i32, drop=(drop_p, seed))


def text_embed_packed(ids, tok, pos, row_off_i32, total_rows, out=None):
    """CLIP text tower on packed rows (sc_text_embed_packed): ids int64 [B, L], tok f32 [V, W], pos f32 [ctx, W] -> f32 [total_rows, W] with
    out[row_off[b] + t] = tok[ids[b, t]] + pos[t] for t < rows_b.  The caller has checked ids in [0, V) and rows_b <= L."""
    _need_cuda(ids, tok, pos, row_off_i32)
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1
    assert tok.dtype == torch.float32 and pos.dtype == torch.float32 and tok.is_contiguous() and pos.is_contiguous() and tok.shape[1] == pos.shape[1]
    B, L = ids.shape
    assert row_off_i32.dtype == torch.int32 and row_off_i32.numel() == B + 1
    W = tok.shape[1]
    if out is None:
        out = torch.empty(int(total_rows), W, device=tok.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (int(total_rows), W)
    check(lib().sc_text_embed_packed(ptr(ids), ids.stride(0), ptr(tok), ptr(pos), ptr(row_off_i32), ptr(out), B, L, tok.shape[0], pos.shape[0], W,
                                     int(total_rows), stream()), "sc_text_embed_packed")
    return out


def attention_text(qkv, B, rows_max, H, row_off_i32, out=None, general=False):
    """Causal attention over packed caption rows (sc_attention_fwd_text): qkv bf16 [total_rows, 3*H*64] (q | k | v), caption b at rows row_off[b] ..
    (at most rows_max each); query t sees keys 0 .. t of its own caption.  general: SC_ATTN_TEXT_GENERAL."""
    _need_cuda(qkv, row_off_i32)
    D = H * 64
    total = qkv.shape[0]
    assert qkv.dtype == bf16 and qkv.shape == (total, 3 * D) and qkv.is_contiguous()
    assert row_off_i32.dtype == torch.int32 and row_off_i32.numel() == B + 1
    if out is None:
        out = torch.empty(total, D, device=qkv.device, dtype=bf16)
    assert out.dtype == bf16 and out.shape == (total, D) and out.is_contiguous()
    q = qkv.data_ptr()
    check(lib().sc_attention_fwd_text(q, q + D * 2, q + 2 * D * 2, ptr(out), ptr(row_off_i32), B, H, int(rows_max), total, 64, 3 * D, D, 0.125,
                                      _lib.ATTN_TEXT_GENERAL if general else 0, stream()), "sc_attention_fwd_text")
    return out


def unpack_rows(src, row_off_i32, B, T_out, halo=0):
    """src [n, total_rows, D] or [total_rows, D] (packed) -> [n, B, T_out, D] / [B, T_out, D], zeros beyond each utterance's rows; the last `halo`
    rows of every utterance are not copied (the packed engine's receptive-field row)."""
    _need_cuda(src, row_off_i32)
    three = src.dim() == 3
    s3 = src if three else src.unsqueeze(0)
    n, total, D = s3.shape
    assert s3.is_contiguous() and (D * s3.element_size()) % 16 == 0
    out = torch.empty(n, B, T_out, D, device=src.device, dtype=src.dtype)
    rb = D * s3.element_size()
    check(lib().sc_unpack_rows(ptr(s3), total * rb, ptr(row_off_i32), ptr(out), B * T_out * rb, n, B, T_out, rb, int(halo), stream()), "sc_unpack_rows")
    return out if three else out[0]


def pack_rows(src, row_off_i32, total_rows, halo=0):
    """The adjoint of unpack_rows: src [n, B, T, D] or [B, T, D] (padded) -> [n, total_rows, D] / [total_rows, D]; packed row t of utterance b takes
    src[b, t] for t < min(rows_b - halo, T) and zeros otherwise."""
    _need_cuda(src, row_off_i32)
    four = src.dim() == 4
    s4 = src if four else src.unsqueeze(0)
    n, B, T, D = s4.shape
    assert s4.is_contiguous() and (D * s4.element_size()) % 16 == 0 and row_off_i32.numel() == B + 1
    out = torch.empty(n, int(total_rows), D, device=src.device, dtype=src.dtype)
    rb = D * s4.element_size()
    check(lib().sc_pack_rows(ptr(s4), B * T * rb, ptr(row_off_i32), ptr(out), int(total_rows) * rb, n, B, T, int(total_rows), rb, int(halo), stream()), "sc_pack_rows")
    return out if four else out[0]


def attention_bwd_packed(qkv, att, datt, B, rows_max, H, klens_i32, row_off_i32=None, drop=None, out=None):
    """Fused attention backward (sc_attention_bwd_packed): qkv bf16 [total_rows, 3*H*64] (q | k | v), att / datt bf16 [total_rows, H*64] (the forward's
    output and its gradient) -> dqkv bf16 [total_rows, 3*H*64].  row_off_i32 None: the uniform layout (total_rows = B * rows_max).  drop = (p, seed) of a
    forward that ran with attention dropout.  The only temporary is the fp32 statistics workspace (2 floats per row and head)."""
    _need_cuda(qkv, att, datt, klens_i32)
    D = H * 64
    total = att.shape[0]
    assert qkv.dtype == bf16 and att.dtype == bf16 and datt.dtype == bf16
    assert qkv.shape[0] >= total and qkv.shape[1] == 3 * D and att.shape == (total, D) and datt.shape == (total, D)
    assert qkv.is_contiguous() and att.is_contiguous() and datt.is_contiguous()
    if out is None:
        out = torch.empty(total, 3 * D, device=qkv.device, dtype=bf16)
    assert out.shape == (total, 3 * D) and out.is_contiguous() and out.dtype == bf16
    ws = torch.empty(lib().sc_attention_bwd_packed_workspace_bytes(total, H), device=qkv.device, dtype=torch.uint8)
    p_, seed = (float(drop[0]), int(drop[1]) & 0xffffffff) if drop is not None else (0.0, 0)
    check(lib().sc_attention_bwd_packed(qkv.data_ptr(), qkv.data_ptr() + D * 2, qkv.data_ptr() + 2 * D * 2, 3 * D, ptr(att), ptr(datt), D, ptr(klens_i32),
                                        ptr(row_off_i32), B, H, int(rows_max), total, 64, 0.125, p_, seed, out.data_ptr(), out.data_ptr() + D * 2,
                                        out.data_ptr() + 2 * D * 2, 3 * D, ptr(ws), stream()), "sc_attention_bwd_packed")
    return out


_DEV_INTS = {}


def dev_ints(values, dtype, device):
    """Small host integer lists (utterance lengths, valid-frame counts) as a device tensor, cached by value: fixed-length batches upload
    them once instead of every step, and a step that only replays cached uploads can be captured in a HIP graph (a pageable
    host-to-device copy is not capturable).  The returned tensor is shared: callers must not write to it."""
    key = (tuple(int(v) for v in values), dtype, str(device))
    t = _DEV_INTS.get(key)
    if t is None:
        if len(_DEV_INTS) > 256:
            _DEV_INTS.clear()
        t = torch.tensor(list(key[0]), dtype=dtype).to(device)
        _DEV_INTS[key] = t
    return t


def crop_pad(wav, starts, lens, Lout):
    """wav f32 [B, L] (device); starts/lens host int lists -> f32 [B, Lout]: out[b, j] = wav[b, starts[b] + j] for j < lens[b], else 0."""
    _need_cuda(wav)
    assert wav.dtype == torch.float32 and wav.dim() == 2 and wav.stride(1) == 1
    B = wav.shape[0]
    assert all(0 <= s and s + l <= wav.shape[1] and l <= Lout for s, l in zip(starts, lens))
    meta = torch.tensor([list(starts), list(lens)], dtype=torch.int32).to(wav.device)      # random crop offsets: new every step
    out = torch.empty(B, Lout, device=wav.device, dtype=torch.float32)
    check(lib().sc_crop_pad(ptr(wav), wav.stride(0), ptr(meta[0]), ptr(meta[1]), ptr(out), B, Lout, stream()), "sc_crop_pad")
    return out


def wave_prep(clips, starts=None, lens=None, Lout=None):
    """The audio hand-over on the current device (sc_wave_prep): a list of host utterances -- int16 / float32 arrays or CPU tensors [n] or [n, C] (16 kHz),
    (samples, rate) pairs, paths of 16-bit PCM .wav files -- -> f32 [B, Lout] at 16 kHz: sample conversion, mono mix, polyphase resampling, the crop window
    [starts[b], starts[b] + lens[b]) in 16 kHz samples (default: everything) and zero right-padding (Lout defaults to the longest window).  The geometry, the
    tap tables (cached per rate) and the raw samples go into ONE pinned buffer, cross PCIe in one non-blocking copy, and one library call on the current stream
    does the rest.  data/audio_transforms.py states the arithmetic."""
    return _wave_prep(clips, starts, lens, Lout)


def _wave_prep(clips, starts=None, lens=None, Lout=None, device=None, out=None, pad_bytes=0):
    """wave_prep with the knobs the tests need: device (any spelling of a GPU, default the current one), out = a caller-owned f32 [B, >= Lout] view with unit
    column stride to write into (the tests put it between sentinel guards, rows apart), pad_bytes: gaps around every utterance, filled with a pattern that
    reads as NaN in f32 and 0x7fff in int16."""
    import numpy as np
    from .data.audio_transforms import plan_wave_batch
    if not torch.cuda.is_available():
        raise _lib.SpeechClipHipError("speechclip_amd ops need a GPU: wave_prep has no CPU fallback (int16 / stereo / other-rate / path elements of a wav list "
                                      "are served by the device entry only)")
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SpeechClipHipError("speechclip_amd ops need device tensors (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    plan = plan_wave_batch(clips, starts, lens, pad_bytes=pad_bytes)
    B = len(plan.clips)
    longest = int(plan.geom[:, 8].max()) if B else 0
    Lout = longest if Lout is None else int(Lout)
    if Lout < longest:
        raise ValueError(f"wave_prep: Lout={Lout} is shorter than the longest window ({longest})")
    # one pinned buffer: offsets | geom | tables | (16-byte aligned) samples; a fresh pinned tensor per call (see image_prep)
    n_off, n_geom, n_tab = plan.offsets.nbytes, plan.geom.nbytes, plan.tables.nbytes
    head = (n_off + n_geom + n_tab + 15) // 16 * 16
    host = torch.empty(max(head + plan.packed_bytes, 16), dtype=torch.uint8, pin_memory=True)
    hb = host.numpy()
    hb[:n_off] = plan.offsets.view(np.uint8)
    hb[n_off:n_off + n_geom] = plan.geom.reshape(-1).view(np.uint8)
    hb[n_off + n_geom:n_off + n_geom + n_tab] = plan.tables.view(np.uint8)
    if pad_bytes:
        hb[head:head + plan.packed_bytes].view(np.uint16)[:] = 0x7fff
    for b, (x, _) in enumerate(plan.clips):
        o = head + int(plan.offsets[b])
        hb[o:o + x.nbytes] = x.reshape(-1).view(np.uint8)
    with torch.cuda.device(dev):
        d = host.to(dev, non_blocking=True)
        if out is None:
            out = torch.empty(B, Lout, device=dev, dtype=torch.float32)
        if not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == B and out.shape[1] >= Lout
                and (out.stride(1) == 1 or out.shape[1] <= 1) and (B <= 1 or out.stride(0) >= Lout)):
            raise ValueError(f"wave_prep: output buffer must be an f32 [{B}, >= {Lout}] tensor on {dev} with unit column stride")
        if B == 0 or Lout == 0:
            return out[:, :Lout]
        hp, dp = host.data_ptr(), d.data_ptr()
        has_tab = n_tab > 0
        with _HbmSpan("wave_prep", plan.packed_bytes + B * Lout * 4):
            check(lib().sc_wave_prep(dp + head, plan.packed_bytes, hp, dp, hp + n_off, dp + n_off, hp + n_off + n_geom if has_tab else None,
                                     dp + n_off + n_geom if has_tab else None, n_tab // 4, B, ptr(out), out.stride(0) if B > 1 else max(out.stride(0), Lout), Lout,
                                     stream()), "sc_wave_prep")
    return out[:, :Lout]


def vit_patchify(img, p, Kpad):
    _need_cuda(img)
    B, C, R, _ = img.shape
    assert C == 3 and img.dtype == torch.float32 and img.is_contiguous()
    npatch = (R // p) ** 2
    cols = torch.empty(B * npatch, Kpad, device=img.device, dtype=bf16)
    check(lib().sc_vit_patchify(ptr(img), ptr(cols), B, R, p, Kpad, stream()), "sc_vit_patchify")
    return cols


def vit_embed(patch, cls, pos, gamma, beta, B, ntok, D, eps=1e-5):
    out = torch.empty(B * ntok, D, device=patch.device, dtype=torch.float32)
    check(lib().sc_vit_embed(ptr(patch), ptr(cls), ptr(pos), ptr(gamma), ptr(beta), ptr(out), B, ntok, D, eps, stream()), "sc_vit_embed")
    return out


def infonce(feat_a, feat_b, ids=None, inv_temperature=1.0 / 0.07, margin=0.0, dcl=False, a2b=True, b2a=True):
    """Returns f32[3] device tensor: (loss, a2b term, b2a term)."""
    _need_cuda(feat_a, feat_b)
    assert feat_a.shape == feat_b.shape and feat_a.dtype == torch.float32 and feat_b.dtype == torch.float32
    feat_a, feat_b = feat_a.contiguous(), feat_b.contiguous()
    Bg, E = feat_a.shape
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.shape[0] == Bg
        ids = ids.contiguous()
    ws = torch.empty(lib().sc_infonce_workspace_bytes(Bg), device=feat_a.device, dtype=torch.uint8)
    out = torch.empty(3, device=feat_a.device, dtype=torch.float32)
    check(lib().sc_infonce_fwd(ptr(feat_a), ptr(feat_b), ptr(ids), ptr(ws), ptr(out), Bg, E, inv_temperature, margin, int(dcl), int(a2b),
                               int(b2a), stream()), "sc_infonce_fwd")
    return out


def kw_affine(x, scale, shift):
    """x f32 [B,K,D]; scale/shift f32 [K,D]."""
    _need_cuda(x)
    B, K, D = x.shape
    x = x.float().contiguous()
    out = torch.empty_like(x)
    check(lib().sc_kw_affine(ptr(x), ptr(scale.to(x.device)), ptr(shift.to(x.device)), ptr(out), B * K, K, D, stream()), "sc_kw_affine")
    return out


_COS_TABLES = {}
COS_REFINE_DELTA = 1e-3            # the MFMA path's refine window below the row maximum (cosine_scores)


def _cos_table(emb):
    """(e/|e|) of the frozen sub-word table as a three-block bf16 operand [V, 3E] = (hi | hi | lo): with the keyword side split as (hi | lo | hi),
    ONE bf16 MFMA GEMM of depth 3E returns a_hi.e_hi + a_lo.e_hi + a_hi.e_lo (~16 mantissa bits of the fp32 product).  Cached per table version."""
    import weakref
    key = emb.data_ptr()
    hit = _COS_TABLES.get(key)
    if hit is not None and hit[0] == (emb._version, param_epoch(emb), tuple(emb.shape)) and hit[2]() is emb:
        return hit[1]
    en = l2norm(emb.detach().float().contiguous(), clamp=True)
    hi = en.to(bf16)
    lo = (en - hi.float()).to(bf16)
    tab = torch.cat([hi, hi, lo], dim=1).contiguous()
    _COS_TABLES.clear()
    _COS_TABLES[key] = ((emb._version, param_epoch(emb), tuple(emb.shape)), tab, weakref.ref(emb))
    return tab


def cosine_scores(a, emb, eps=1e-8, exact=None, mask_ids=()):
    """a f32 [R,E], emb f32 [V,E] -> f32 [R,V] cosine similarities a_r . e_v / (max(|a_r|, eps) max(|e_v|, eps)).
    Small problems / `exact=True`: the fp32 SIMT kernel for the whole matrix (every entry fp32-accurate; `mask_ids` plays no part).
    Otherwise (E % 64 == 0, V % 4 == 0, R * V >= 2^22 -- the 49408-entry sub-word table -- or `exact=False`): the MFMA GEMM on three-term
    bf16 splits of the normalised operands (a_hi.e_hi + a_lo.e_hi + a_hi.e_lo: the dropped a_lo.e_lo and the bf16 roundings of the lo parts
    are each at most 2^-16 sum|a_n e_n|, 4.6e-5 in all; ~2e-5 is the most the tests provoke), followed by sc_cosine_refine_masked.  The contract of that path (tests/test_cascaded_fwd_parity_gpu.py):
      * every entry whose column is not in `mask_ids` and whose GEMM value lies within 1e-3 of the row's maximum over the columns not in
        `mask_ids` is recomputed in fp32, however many there are; every other entry keeps the GEMM's value;
      * so the arg-max over the columns not in `mask_ids` is decided by fp32 arithmetic, as on the exact path.  `mask_ids` (at most 8) are the
        ids the quantiser masks AFTERWARDS (sc_vq_fwd); a caller that masks and passes none gets the guarantee for the unmasked arg-max only;
      * the result is bitwise repeatable."""
    _need_cuda(a, emb)
    a = a.float().contiguous()
    R, E = a.shape
    V = emb.shape[0]
    if exact is None:
        exact = not (E % 64 == 0 and V % 4 == 0 and R * V >= (1 << 22))
    out = torch.empty(R, V, device=a.device, dtype=torch.float32)
    if exact:
        embf = emb.detach().float().contiguous()
        ws = torch.empty(lib().sc_cosine_workspace_bytes(R, V), device=a.device, dtype=torch.uint8)
        check(lib().sc_cosine_scores(ptr(a), ptr(embf), ptr(ws), ptr(out), R, V, E, eps, stream()), "sc_cosine_scores")
        return out
    tab = _cos_table(emb)
    a3 = split_hilo(l2norm(a, clamp=True), nblk=3)
    gemm(a3, tab, out=out, out_f32=True)
    embf = emb.detach()
    embf = embf if (embf.dtype == torch.float32 and embf.is_contiguous()) else embf.float().contiguous()
    ids, ids_p, n_mask = _mask_arg(mask_ids)                  # `ids` owns the host array until the call has returned
    check(lib().sc_cosine_refine_masked(ptr(out), ptr(a), ptr(embf), R, V, E, COS_REFINE_DELTA, eps, ids_p, n_mask, stream()),
          "sc_cosine_refine_masked")
    return out


def vq_fwd(scores, K, mask_ids=(0, 2, 3)):
    """scores f32 [R,V] -> (targets i64 [R], stats f32 [2] = (code_perplexity, prob_perplexity), ent_per_t f32 [K])."""
    import ctypes
    _need_cuda(scores)
    scores = scores.float().contiguous()
    R, V = scores.shape
    dev = scores.device
    targets = torch.empty(R, device=dev, dtype=torch.int64)
    stats = torch.empty(2, device=dev, dtype=torch.float32)
    ent = torch.empty(K, device=dev, dtype=torch.float32)
    ws = torch.empty(lib().sc_vq_workspace_bytes(R, V), device=dev, dtype=torch.uint8)
    ids = (ctypes.c_int32 * len(mask_ids))(*[int(i) for i in mask_ids])
    check(lib().sc_vq_fwd(ptr(scores), ptr(targets), ptr(stats), ptr(ent), ptr(ws), R, K, V, ctypes.cast(ids, ctypes.c_void_p), len(mask_ids),
                          stream()), "sc_vq_fwd")
    return targets, stats, ent


def gather_rows(src, idx):
    _need_cuda(src, idx)
    src = src.detach().float().contiguous()
    idx = idx.to(torch.int64).contiguous()
    out = torch.empty(idx.shape[0], src.shape[1], device=src.device, dtype=torch.float32)
    check(lib().sc_gather_rows(ptr(src), ptr(idx), ptr(out), idx.shape[0], src.shape[1], stream()), "sc_gather_rows")
    return out


# ---------------------------------------------------------------------------------------------------- trainable tail (fp32)
def _f32c(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())


# Deterministic mode ('Reproducibility'): the three order-dependent reductions of a training step -- split-K sc_sgemm, chunked
# sc_colsum and the 8 waves of sc_cls_pool_bwd -- go through their fixed-order entries (sc_*_det).  Opt in with SC_DETERMINISTIC=1 (read once,
# here), set_deterministic(True), or torch.use_deterministic_algorithms(True) (read at every call, never set).  The choice is made in sgemm /
# sgemm_batched / colsum / cls_pool_bwd below and nowhere else.  Workspaces are allocated per call from torch's caching allocator on the
# current stream, so two streams never share one.
def _env_flag(value) -> bool:
    return str(value or "").strip().lower() in ("1", "true", "on", "yes")


_DETERMINISTIC = [_env_flag(_os.environ.get("SC_DETERMINISTIC"))]
_DET_COUNTERS = {"sgemm_split": 0, "colsum_chunks": 0, "cls_pool_bwd": 0}


def set_deterministic(enabled: bool) -> None:
    _DETERMINISTIC[0] = bool(enabled)


def deterministic() -> bool:
    return _DETERMINISTIC[0] or torch.are_deterministic_algorithms_enabled()


def det_counters(reset: bool = False) -> dict:
    """Calls since the last reset that took the deterministic split-K path (more than one slice), chunk path (more than one chunk) and
    pooling-backward path."""
    out = dict(_DET_COUNTERS)
    if reset:
        for k in _DET_COUNTERS:
            _DET_COUNTERS[k] = 0
    return out


def _det_workspace(nbytes, dev):
    return torch.empty(nbytes // 4, device=dev, dtype=torch.float32)


def _sgemm_det(transa, transb, M, N, K, alpha, a, lda, stride_a, b, ldb, stride_b, beta, out, ldc, stride_c, bias, stride_bias, batch) -> bool:
    """The product through sc_sgemm_batched_det when the mode is on and the split-K rule gives more than one slice (one slice has nothing to
    order: the caller's default entry runs).  -> whether it ran."""
    L = lib()
    if not deterministic() or L.sc_sgemm_det_slices(M, N, K, batch) <= 1:
        return False
    nbytes = L.sc_sgemm_det_workspace_bytes(M, N, K, batch)
    ws = _det_workspace(nbytes, out.device)
    _DET_COUNTERS["sgemm_split"] += 1
    check(L.sc_sgemm_batched_det(int(transa), int(transb), M, N, K, alpha, ptr(a), lda, stride_a, ptr(b), ldb, stride_b, beta, ptr(out), ldc, stride_c,
                                 ptr(bias), stride_bias, batch, ptr(ws), nbytes, stream()), "sc_sgemm_batched_det")
    return True


def sgemm(a, b, transa=False, transb=False, alpha=1.0, beta=0.0, out=None, bias=None):
    """out[M,N] = alpha * op(a) @ op(b) + beta * out (+ bias[N]).  fp32, 2-D row-major tensors (last stride 1).
    transa: a stored [K,M]; transb: b stored [N,K] (nn.Linear weight layout)."""
    _need_cuda(a, b)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    M, K = (a.shape[1], a.shape[0]) if transa else a.shape
    N = b.shape[0] if transb else b.shape[1]
    assert (b.shape[1] if transb else b.shape[0]) == K, (a.shape, b.shape, transa, transb)
    if out is None:
        assert beta == 0.0
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    assert out.shape == (M, N) and out.dtype == torch.float32 and out.stride(1) == 1
    if _sgemm_det(transa, transb, M, N, K, alpha, a, a.stride(0), 0, b, b.stride(0), 0, beta, out, out.stride(0), 0, bias, 0, 1):
        return out
    check(lib().sc_sgemm(int(transa), int(transb), M, N, K, alpha, ptr(a), a.stride(0), ptr(b), b.stride(0), beta, ptr(out), out.stride(0),
                         ptr(bias), stream()), "sc_sgemm")
    return out


def sgemm_batched(M, N, K, a, lda, stride_a, b, ldb, stride_b, out, ldc, stride_c, batch, transa=False, transb=False, alpha=1.0, beta=0.0,
                  bias=None, stride_bias=0):
    """`batch` products out_i[M,N] = alpha op(a_i) op(b_i) + beta out_i (+ bias_i) with operand i at base + i*stride (elements): the
    per-head products of the attention block in one launch.  a / b / out / bias are tensors (or views) whose data_ptr is operand 0."""
    _need_cuda(a, b, out)
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and out.dtype == torch.float32
    if _sgemm_det(transa, transb, M, N, K, alpha, a, lda, stride_a, b, ldb, stride_b, beta, out, ldc, stride_c, bias, stride_bias, batch):
        return out
    check(lib().sc_sgemm_batched(int(transa), int(transb), M, N, K, alpha, ptr(a), lda, stride_a, ptr(b), ldb, stride_b, beta, ptr(out), ldc, stride_c,
                                 ptr(bias), stride_bias, batch, stream()), "sc_sgemm_batched")
    return out


def cls_pool_train_fwd(x_rows, cls_tok, scores, cls_scores, lens_i32, B, T, NQ, R, D, drop_p=0.0, seed=0):
    """-> (p f32 [B,R,NQ+T], xbar f32 [B,R,D]).  x_rows bf16 [B*T, D]; cls_tok f32 [NQ,D]; scores f32 [B*T,R]; cls_scores f32 [NQ,R]."""
    _need_cuda(x_rows)
    _f32c(cls_tok, scores, cls_scores)
    assert x_rows.dtype == bf16 and x_rows.stride(1) == 1 and scores.shape == (B * T, R)
    p = torch.empty(B, R, NQ + T, device=x_rows.device, dtype=torch.float32)
    xbar = torch.empty(B, R, D, device=x_rows.device, dtype=torch.float32)
    check(lib().sc_cls_pool_train_fwd(ptr(x_rows), x_rows.stride(0), ptr(cls_tok), ptr(scores), ptr(cls_scores), ptr(lens_i32), ptr(p), ptr(xbar),
                                      B, T, NQ, R, D, float(drop_p), int(seed) & 0xFFFFFFFF, stream()), "sc_cls_pool_train_fwd")
    return p, xbar


def cls_pool_bwd(x_rows, cls_tok, hidden, p, dzbar, u, lens_i32, B, T, NQ, R, D, normalize=False, drop_p=0.0, seed=0, nsplit=None, return_ws=False):
    """-> (du f32 [B*S,R,D], dcls_key f32 [B*S,NQ,D], dalpha f32 [B*S,n] or None): PARTIAL rows (S = nsplit key-splits per utterance); the
    caller sums over rows.  hidden: bf16 / f32 [n, B*T, D] contiguous or None."""
    _need_cuda(x_rows)
    _f32c(cls_tok, p, dzbar, u)
    dev = x_rows.device
    n = 0 if hidden is None else hidden.shape[0]
    if hidden is not None:
        assert hidden.dtype in (bf16, torch.float32) and hidden.is_contiguous() and hidden.shape[1] == B * T and hidden.shape[2] == D
    if nsplit is None:
        nsplit = max(1, min(16, 512 // max(B, 1)))           # ~2 blocks of 8 waves per CU
    ds = torch.empty(B, R, NQ + T, device=dev, dtype=torch.float32)
    pp = torch.empty_like(ds)
    du = torch.empty(B * nsplit, R, D, device=dev, dtype=torch.float32)
    dck = torch.empty(B * nsplit, NQ, D, device=dev, dtype=torch.float32)
    dalpha = torch.empty(B * nsplit, n, device=dev, dtype=torch.float32) if n else None
    det = deterministic()
    if det:
        _DET_COUNTERS["cls_pool_bwd"] += 1
    entry = lib().sc_cls_pool_bwd_det if det else lib().sc_cls_pool_bwd
    check(entry(ptr(x_rows), x_rows.stride(0), ptr(cls_tok), ptr(hidden), int(n > 0 and hidden.dtype == torch.float32), hidden.stride(0) if n else 0, n,
                int(normalize), ptr(p), ptr(dzbar), ptr(u), ptr(lens_i32), ptr(ds), ptr(pp), ptr(du), ptr(dck), ptr(dalpha), B, T, NQ, R, D,
                int(nsplit), float(drop_p), int(seed) & 0xFFFFFFFF, stream()), "sc_cls_pool_bwd_det" if det else "sc_cls_pool_bwd")
    if return_ws:          # (ds, pp): score gradients and post-dropout probabilities [B,R,NQ+T], what sc_cls_pool_dz needs
        return du, dck, dalpha, ds, pp
    return du, dck, dalpha


def layernorm_bwd(x, dy, gamma, dgamma=None, dbeta=None, eps=1e-5, dx=None, accumulate_dx=False):
    """fp32 [rows, D].  Returns dx; dgamma/dbeta are accumulated in place when given."""
    _f32c(x, dy, gamma, dgamma, dbeta)
    rows, D = x.shape
    if dx is None:
        assert not accumulate_dx
        dx = torch.empty_like(x)
    stats = torch.empty(rows, 2, device=x.device, dtype=torch.float32)
    check(lib().sc_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(stats), rows, D, eps, int(accumulate_dx),
                                 stream()), "sc_layernorm_bwd")
    return dx


def gelu_f32(z):
    _f32c(z)
    y = torch.empty_like(z)
    check(lib().sc_gelu_f32(ptr(z), ptr(y), z.numel(), 0, stream()), "sc_gelu_f32")
    return y


def gelu_bwd_(z, dh):
    """dh *= gelu'(z) in place."""
    _f32c(z, dh)
    check(lib().sc_gelu_f32(ptr(z), ptr(dh), z.numel(), 1, stream()), "sc_gelu_f32")
    return dh


def colsum(x, out=None, accumulate=False):
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, device=x.device, dtype=torch.float32)
        accumulate = False
    if deterministic() and lib().sc_colsum_det_chunks(rows, cols) > 1:
        nbytes = lib().sc_colsum_det_workspace_bytes(rows, cols)
        ws = _det_workspace(nbytes, x.device)
        _DET_COUNTERS["colsum_chunks"] += 1
        check(lib().sc_colsum_det(ptr(x), x.stride(0), rows, cols, ptr(out), int(accumulate), ptr(ws), nbytes, stream()), "sc_colsum_det")
        return out
    check(lib().sc_colsum(ptr(x), x.stride(0), rows, cols, ptr(out), int(accumulate), stream()), "sc_colsum")
    return out


def l2norm_bwd(x, dy):
    _f32c(x, dy)
    dx = torch.empty_like(x)
    check(lib().sc_l2norm_bwd(ptr(x), ptr(dy), ptr(dx), x.shape[0], x.shape[1], stream()), "sc_l2norm_bwd")
    return dx


def dropout_f32(x, drop_p, seed, out=None):
    _f32c(x)
    out = torch.empty_like(x) if out is None else out
    check(lib().sc_dropout_f32(ptr(x), ptr(out), x.numel(), float(drop_p), int(seed) & 0xFFFFFFFF, stream()), "sc_dropout_f32")
    return out


def add_rows(a, b, alpha=1.0, out=None):
    """out = alpha * a + b[r % b.shape[0]]  (fp32 2-D)."""
    _f32c(a, b)
    out = torch.empty_like(a) if out is None else out
    check(lib().sc_add_rows_f32(ptr(a), ptr(b), ptr(out), a.shape[0], a.shape[1], b.shape[0], float(alpha), stream()), "sc_add_rows_f32")
    return out


def mix_softmax_bwd(w, dalpha_b, dw):
    _f32c(w, dalpha_b, dw)
    check(lib().sc_mix_softmax_bwd(ptr(w), ptr(dalpha_b), dalpha_b.shape[0], dalpha_b.shape[1], ptr(dw), stream()), "sc_mix_softmax_bwd")
    return dw


def infonce_fwd_bwd(feat_a, feat_b, ids=None, inv_temperature=1.0 / 0.07, margin=0.0, dcl=False, a2b=True, b2a=True, want_dfeat_b=False):
    """Loss and its gradients in one go: returns (out3, dfeat_a [Bg,E], dinv scalar tensor) -- d loss/d feat_a and d loss/d inv_temperature;
    with want_dfeat_b a fourth value, dfeat_b [Bg,E] = inv_temperature * G^T feat_a from the same G = d loss / d logits."""
    _f32c(feat_a, feat_b)
    Bg, E = feat_a.shape
    dev = feat_a.device
    if ids is not None:
        ids = ids.contiguous()
    ws = torch.empty(lib().sc_infonce_workspace_bytes(Bg), device=dev, dtype=torch.uint8)
    out = torch.empty(3, device=dev, dtype=torch.float32)
    check(lib().sc_infonce_fwd(ptr(feat_a), ptr(feat_b), ptr(ids), ptr(ws), ptr(out), Bg, E, inv_temperature, margin, int(dcl), int(a2b),
                               int(b2a), stream()), "sc_infonce_fwd")
    ws2 = torch.empty(lib().sc_infonce_bwd_workspace_bytes(Bg), device=dev, dtype=torch.uint8)
    G = torch.empty(Bg, Bg, device=dev, dtype=torch.float32)
    dinv = torch.empty(1, device=dev, dtype=torch.float32)
    check(lib().sc_infonce_bwd(ptr(feat_a), ptr(feat_b), ptr(ids), ptr(ws), ptr(ws2), ptr(G), ptr(dinv), Bg, E, inv_temperature, margin, int(dcl),
                               int(a2b), int(b2a), stream()), "sc_infonce_bwd")
    da = sgemm(G, feat_b, alpha=inv_temperature)
    if want_dfeat_b:
        return out, da, dinv, sgemm(G, feat_a, transa=True, alpha=inv_temperature)
    return out, da, dinv


def grad_norm(flat_grad, max_norm=0.0):
    """-> f32[2] device tensor: (total L2 norm, clip coefficient)."""
    _f32c(flat_grad)
    ws = torch.empty(lib().sc_grad_norm_workspace_bytes(), device=flat_grad.device, dtype=torch.uint8)
    out = torch.empty(2, device=flat_grad.device, dtype=torch.float32)
    check(lib().sc_grad_norm(ptr(flat_grad), flat_grad.numel(), float(max_norm), ptr(ws), ptr(out), stream()), "sc_grad_norm")
    return out


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_coef=None):
    _f32c(p, g, m, v)
    check(lib().sc_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(clip_coef[1:] if clip_coef is not None else None), lr, betas[0], betas[1],
                             eps, weight_decay, int(step), stream()), "sc_adam_step")


def retrieval_ranks(score, own_ids, cand_ids):
    """score f32 [n, m] (device); own_ids i64 [n]; cand_ids i64 [m] -> int32 [n]: candidates ranked ahead of the row's best positive."""
    _need_cuda(score)
    assert score.dtype == torch.float32 and score.dim() == 2 and score.stride(1) == 1
    n, m = score.shape
    own = own_ids.to(score.device, torch.int64).contiguous()
    cand = cand_ids.to(score.device, torch.int64).contiguous()
    assert own.shape == (n,) and cand.shape == (m,)
    rank = torch.empty(n, device=score.device, dtype=torch.int32)
    check(lib().sc_retrieval_ranks(ptr(score), score.stride(0), ptr(own), ptr(cand), ptr(rank), n, m, stream()), "sc_retrieval_ranks")
    return rank


# ---- gallery search (search.hip, search_bf16.hip, search_items.hip) ----
def _search(entry, dtype, q, g, k, n_split, idx_base, workspace, by_item=None, select=None):
    """The entries of the fused search: the same shapes, split rule and (vals, idx) outputs; `entry` and the rows' dtype differ.  by_item = (g_item,
    q_skip, distinct) selects by item (sc_search_items*): the item codes of the gallery rows, the queries' skip codes or None, and a third output.
    select = (allow, g_group, q_group), with by_item, selects inside a subset (sc_search_select*): each of the three may be None."""
    _need_cuda(q, g)
    assert q.dtype == dtype and g.dtype == dtype and q.dim() == 2 and g.dim() == 2 and q.stride(1) == 1 and g.stride(1) == 1
    assert q.shape[1] == g.shape[1], (q.shape, g.shape)
    Q, E = q.shape
    N, k = g.shape[0], int(k)
    out = [torch.empty(Q, k, device=q.device, dtype=torch.float32), torch.empty(Q, k, device=q.device, dtype=torch.int64)]
    extra, workspace_bytes = (), lib().sc_search_workspace_bytes
    if by_item is not None:
        g_item, q_skip, distinct = by_item
        _need_cuda(g_item)
        assert g_item.dtype == torch.int32 and g_item.shape == (N,) and g_item.is_contiguous(), (g_item.dtype, g_item.shape)
        if q_skip is not None:
            _need_cuda(q_skip)
            assert q_skip.dtype == torch.int32 and q_skip.shape == (Q,) and q_skip.is_contiguous(), (q_skip.dtype, q_skip.shape)
        out.append(torch.empty(Q, k, device=q.device, dtype=torch.int32))
        extra, workspace_bytes = (ptr(g_item), ptr(q_skip), int(bool(distinct))), lib().sc_search_items_workspace_bytes
    if select is not None:
        allow, g_group, q_group = select
        if allow is not None:
            _need_cuda(allow)
            assert allow.dtype == torch.uint32 and allow.shape == ((N + 31) // 32,) and allow.is_contiguous(), (allow.dtype, allow.shape)
        if g_group is not None:
            _need_cuda(g_group)
            assert g_group.dtype == torch.int32 and g_group.shape == (N,) and g_group.is_contiguous(), (g_group.dtype, g_group.shape)
        if q_group is not None:
            _need_cuda(q_group)
            assert q_group.dtype == torch.int32 and q_group.shape == (Q,) and q_group.is_contiguous(), (q_group.dtype, q_group.shape)
        extra = (ptr(allow), ptr(g_group), ptr(q_group)) + extra
    nbytes = workspace_bytes(Q, N, k, int(n_split))
    if workspace is None and nbytes > 0:
        workspace = torch.empty(nbytes, device=q.device, dtype=torch.uint8)
    assert workspace is None or (workspace.is_cuda and workspace.numel() * workspace.element_size() >= nbytes)
    check(getattr(lib(), entry)(ptr(q), q.stride(0), ptr(g), g.stride(0), Q, N, E, k, int(n_split), int(idx_base), *extra, *(ptr(t) for t in out), ptr(workspace),
                                stream()), entry)
    return tuple(out)


def search_topk(q, g, k, n_split=0, idx_base=0, workspace=None):
    """q f32 [Q, E], g f32 [N, E] (device, last stride 1) -> (vals f32 [Q, k], idx i64 [Q, k]): for every query the k gallery rows with the largest
    fp32 fmaf-chain score, ordered by (score descending, row ascending); idx = idx_base + row.  No [Q, N] score image is formed (sc_search_topk).
    n_split = 0: the library's rule.  `workspace`: a caller's uint8 buffer of at least sc_search_workspace_bytes (tests guard it); default: allocated here."""
    return _search("sc_search_topk", torch.float32, q, g, k, n_split, idx_base, workspace)


def search_topk_bf16(q, g, k, n_split=0, idx_base=0, workspace=None):
    """search_topk on bf16 rows (search_bf16.hip): q bf16 [Q, E], g bf16 [N, E] (device, last stride 1, E % 16 == 0) -> (vals f32 [Q, k], idx i64 [Q, k]).
    The bf16 products are exact and summed in fp32 on the bf16 MFMA (sc_search_topk_bf16's contract); order, splits and workspace as search_topk."""
    return _search("sc_search_topk_bf16", bf16, q, g, k, n_split, idx_base, workspace)


def topk_merge(vals, idx, k):
    """vals f32 [Q, L], idx i64 [Q, L]: L candidates per row in any order -> the first k by (value descending, idx ascending); entries with idx < 0 or a
    NaN value take no part, missing slots are -inf / -1 (sc_topk_merge)."""
    _need_cuda(vals, idx)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.dim() == 2 and vals.shape == idx.shape
    vals, idx = vals.contiguous(), idx.contiguous()
    Q, L = vals.shape
    out_v = torch.empty(Q, int(k), device=vals.device, dtype=torch.float32)
    out_i = torch.empty(Q, int(k), device=vals.device, dtype=torch.int64)
    check(lib().sc_topk_merge(ptr(vals), ptr(idx), Q, L, int(k), ptr(out_v), ptr(out_i), stream()), "sc_topk_merge")
    return out_v, out_i


def search_items(q, g, k, g_item, q_skip=None, distinct=False, n_split=0, idx_base=0, workspace=None):
    """search_topk by item: g_item i32 [N] gives every gallery row an item code (>= 0), q_skip i32 [Q] (or None) names the item each query leaves out (< 0:
    none) -> (vals f32 [Q, k], idx i64 [Q, k], items i32 [Q, k]).  distinct=False: the first k rows whose item is not the query's skip code; distinct=True:
    the first k ITEMS, each by its best row.  Scores, order, splits and idx_base are search_topk's; missing slots hold -inf / -1 / -1 (sc_search_items).
    `workspace`: a caller's uint8 buffer of at least sc_search_items_workspace_bytes; default: allocated here."""
    return _search("sc_search_items", torch.float32, q, g, k, n_split, idx_base, workspace, (g_item, q_skip, distinct))


def search_items_bf16(q, g, k, g_item, q_skip=None, distinct=False, n_split=0, idx_base=0, workspace=None):
    """search_items on bf16 rows: search_topk_bf16's scores under the same selection (sc_search_items_bf16)."""
    return _search("sc_search_items_bf16", bf16, q, g, k, n_split, idx_base, workspace, (g_item, q_skip, distinct))


def search_select(q, g, k, g_item, allow=None, g_group=None, q_group=None, q_skip=None, distinct=False, n_split=0, idx_base=0, workspace=None):
    """search_items inside a subset of the gallery (sc_search_select): allow uint32 [ceil(N / 32)] (pack_row_mask) holds one bit per gallery row, shared by
    all queries; g_group i32 [N] (codes >= 0) and q_group i32 [Q] restrict query i to the rows with g_group[j] == q_group[i] (q_group[i] < 0: no restriction;
    both or neither).  A row takes part iff search_items lets it and its bit is set and its group matches.  Gallery tiles of 128 rows without an allowed row
    are not loaded.  With all three None this is search_items bit for bit; a query with fewer than k eligible rows gets missing slots (-inf / -1 / -1)."""
    return _search("sc_search_select", torch.float32, q, g, k, n_split, idx_base, workspace, (g_item, q_skip, distinct), (allow, g_group, q_group))


def search_select_bf16(q, g, k, g_item, allow=None, g_group=None, q_group=None, q_skip=None, distinct=False, n_split=0, idx_base=0, workspace=None):
    """search_select on bf16 rows: search_items_bf16's scores under the same selection (sc_search_select_bf16)."""
    return _search("sc_search_select_bf16", bf16, q, g, k, n_split, idx_base, workspace, (g_item, q_skip, distinct), (allow, g_group, q_group))


def pack_row_mask(mask):
    """mask bool or uint8 [N] (device) -> uint32 [ceil(N / 32)]: bit (j & 31) of word j >> 5 says whether mask[j] != 0; the unused high bits of the last word
    are 0 (sc_pack_row_mask).  What search_select takes as `allow`."""
    _need_cuda(mask)
    assert mask.dtype in (torch.bool, torch.uint8) and mask.dim() == 1, (mask.dtype, mask.shape)
    mask = mask.contiguous().view(torch.uint8)
    N = mask.shape[0]
    words = torch.empty((N + 31) // 32, device=mask.device, dtype=torch.uint32)
    check(lib().sc_pack_row_mask(ptr(mask), N, ptr(words), stream()), "sc_pack_row_mask")
    return words


def topk_merge_items(vals, idx, items, k, distinct):
    """vals f32 [Q, L], idx i64 [Q, L], items i32 [Q, L]: L candidates per row in any order -> the first k by (value descending, idx ascending), with
    distinct=True only the first of each item code; entries with idx < 0 or a NaN value take no part, missing slots are -inf / -1 / -1
    (sc_topk_merge_items)."""
    _need_cuda(vals, idx, items)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and items.dtype == torch.int32 and vals.dim() == 2 and vals.shape == idx.shape == items.shape
    vals, idx, items = vals.contiguous(), idx.contiguous(), items.contiguous()
    Q, L = vals.shape
    out_v = torch.empty(Q, int(k), device=vals.device, dtype=torch.float32)
    out_i = torch.empty(Q, int(k), device=vals.device, dtype=torch.int64)
    out_c = torch.empty(Q, int(k), device=vals.device, dtype=torch.int32)
    check(lib().sc_topk_merge_items(ptr(vals), ptr(idx), ptr(items), Q, L, int(k), int(bool(distinct)), ptr(out_v), ptr(out_i), ptr(out_c), stream()),
          "sc_topk_merge_items")
    return out_v, out_i, out_c


def search_rescore(q, g, cand_idx, short_vals, eps, k, idx_base=0):
    """The second stage of a two-stage search (search_rescore.hip): q f32 [Q, E], g f32 [N, E] (device, last stride 1), cand_idx i64 [Q, R] / short_vals f32
    [Q, R] = a bf16 search's shortlist of the rounded rows (idx_base + row or -1; scores descending), eps f32 [Q] -> (vals f32 [Q, k], idx i64 [Q, k],
    certified i32 [Q]): the first k shortlisted rows by search_topk's own fp32 score and order, and whether eps proves that no row outside the shortlist
    belongs among them (sc_search_rescore)."""
    _need_cuda(q, g, cand_idx, short_vals, eps)
    assert q.dtype == torch.float32 and g.dtype == torch.float32 and q.dim() == 2 and g.dim() == 2 and q.stride(1) == 1 and g.stride(1) == 1
    assert q.shape[1] == g.shape[1], (q.shape, g.shape)
    Q, E = q.shape
    N, k = g.shape[0], int(k)
    assert cand_idx.dtype == torch.int64 and short_vals.dtype == torch.float32 and cand_idx.dim() == 2 and cand_idx.shape == short_vals.shape
    assert cand_idx.shape[0] == Q and cand_idx.is_contiguous() and short_vals.is_contiguous(), (cand_idx.shape, short_vals.shape)
    assert eps.dtype == torch.float32 and eps.shape == (Q,) and eps.is_contiguous(), (eps.dtype, eps.shape)
    R = cand_idx.shape[1]
    vals = torch.empty(Q, k, device=q.device, dtype=torch.float32)
    idx = torch.empty(Q, k, device=q.device, dtype=torch.int64)
    certified = torch.empty(Q, device=q.device, dtype=torch.int32)
    check(lib().sc_search_rescore(ptr(q), q.stride(0), ptr(g), g.stride(0), Q, N, E, ptr(cand_idx), ptr(short_vals), R, ptr(eps), k, int(idx_base), ptr(vals),
                                  ptr(idx), ptr(certified), stream()), "sc_search_rescore")
    return vals, idx, certified


# ---- gallery search by threshold (search_range.hip) ----
RANGE_MAX_RESULTS = (1 << 30) // 12        # the hits whose 12 bytes each (f32 score + i64 index) fit in 1 GiB


def _range_operands(q, g, thresh, n_split, g_item, q_skip):
    """The checks shared by the two passes -> (entry suffix, Q, N, E, split count)."""
    _need_cuda(q, g, thresh)
    assert q.dtype in (torch.float32, bf16) and g.dtype == q.dtype and q.dim() == 2 and g.dim() == 2 and q.stride(1) == 1 and g.stride(1) == 1, (q.dtype, g.dtype)
    assert q.shape[1] == g.shape[1], (q.shape, g.shape)
    Q, E = q.shape
    N = g.shape[0]
    assert thresh.dtype == torch.float32 and thresh.shape == (Q,) and thresh.is_contiguous(), (thresh.dtype, thresh.shape)
    if q_skip is not None:
        assert g_item is not None, "q_skip needs g_item"
        _need_cuda(g_item, q_skip)
        assert g_item.dtype == torch.int32 and g_item.shape == (N,) and g_item.is_contiguous(), (g_item.dtype, g_item.shape)
        assert q_skip.dtype == torch.int32 and q_skip.shape == (Q,) and q_skip.is_contiguous(), (q_skip.dtype, q_skip.shape)
    S = int(n_split) if n_split else lib().sc_search_splits(Q, N, 1)
    return ("_bf16" if q.dtype == bf16 else ""), Q, N, E, S


def search_range_count(q, g, thresh, n_split=0, g_item=None, q_skip=None, out=None):
    """The first pass of search_range (sc_search_range_count[_bf16], by the rows' dtype) -> counts i32 [Q, S]: the hits of every query in every gallery
    range, S = n_split or sc_search_splits(Q, N, 1).  `out`: an int32 [Q, S] view with unit column stride (a band of columns of a wider table that the
    segments of an index share); nothing outside it is written.  Default: allocated here."""
    sfx, Q, N, E, S = _range_operands(q, g, thresh, n_split, g_item, q_skip)
    if out is None:
        out = torch.empty(Q, S, device=q.device, dtype=torch.int32)
    assert out.is_cuda and out.dtype == torch.int32 and out.shape == (Q, S) and (out.stride(1) == 1 or S == 1), (out.dtype, out.shape, out.stride())
    name = "sc_search_range_count" + sfx
    check(getattr(lib(), name)(ptr(q), q.stride(0), ptr(g), g.stride(0), Q, N, E, ptr(thresh), int(n_split), ptr(g_item if q_skip is not None else None),
                               ptr(q_skip), ptr(out), out.stride(0) if Q > 1 else max(out.stride(0), S), stream()), name)
    return out


def search_range_offsets(counts, max_results=None):
    """counts i32 [Q, S] (contiguous: one table for the whole gallery) -> (lims i64 [Q + 1], offs i64 [Q, S], T): the exclusive scan over (query, range) in
    row-major order -- plumbing, torch.cumsum -- and the total, whose read is the ONE host synchronisation of a search by threshold.  More than
    max_results hits (default RANGE_MAX_RESULTS, 1 GiB of results) raise ValueError here, before anything is allocated or filled."""
    assert counts.dtype == torch.int32 and counts.dim() == 2 and counts.is_contiguous()
    Q, S = counts.shape
    limit = RANGE_MAX_RESULTS if max_results is None else int(max_results)
    if Q == 0 or S == 0:
        return torch.zeros(Q + 1, device=counts.device, dtype=torch.int64), torch.zeros(Q, S, device=counts.device, dtype=torch.int64), 0
    ends = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    offs = (ends - counts.reshape(-1)).view(Q, S)
    lims = torch.cat([offs[:, 0], ends[-1:]])
    total = int(ends[-1])
    if total > limit:
        raise ValueError(f"search_range: {total} hits exceed max_results={limit}; raise the threshold, pass fewer queries or a larger max_results")
    return lims, offs, total


def search_range_fill(q, g, thresh, offs, vals, idx, n_split=0, idx_base=0, g_item=None, q_skip=None):
    """The second pass (sc_search_range_fill[_bf16]): the hits of (query i, range s) go to vals f32 [T] / idx i64 [T] from offs[i, s] on, in ascending row
    order, idx = idx_base + row.  offs: an int64 [Q, S] view with unit column stride, derived from the counts of the same operands and n_split."""
    sfx, Q, N, E, S = _range_operands(q, g, thresh, n_split, g_item, q_skip)
    _need_cuda(offs, vals, idx)
    assert offs.dtype == torch.int64 and offs.shape == (Q, S) and (offs.stride(1) == 1 or S == 1), (offs.dtype, offs.shape, offs.stride())
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.dim() == 1 and vals.shape == idx.shape and vals.is_contiguous() and idx.is_contiguous()
    if vals.numel() == 0:
        return
    name = "sc_search_range_fill" + sfx
    check(getattr(lib(), name)(ptr(q), q.stride(0), ptr(g), g.stride(0), Q, N, E, ptr(thresh), int(n_split), ptr(g_item if q_skip is not None else None),
                               ptr(q_skip), int(idx_base), ptr(offs), offs.stride(0) if Q > 1 else max(offs.stride(0), S), ptr(vals), ptr(idx), stream()), name)


def _search_range(dtype, q, g, thresh, n_split, idx_base, g_item, q_skip, max_results):
    _need_cuda(q, g)
    assert q.dtype == dtype and g.dtype == dtype, (q.dtype, g.dtype)
    counts = search_range_count(q, g, thresh, n_split, g_item, q_skip)
    lims, offs, total = search_range_offsets(counts, max_results)
    vals = torch.empty(total, device=q.device, dtype=torch.float32)
    idx = torch.empty(total, device=q.device, dtype=torch.int64)
    search_range_fill(q, g, thresh, offs, vals, idx, n_split, idx_base, g_item, q_skip)
    return lims, vals, idx


def search_range(q, g, thresh, n_split=0, idx_base=0, g_item=None, q_skip=None, max_results=None):
    """q f32 [Q, E], g f32 [N, E] (device, last stride 1), thresh f32 [Q] -> (lims i64 [Q + 1], vals f32 [T], idx i64 [T]): query i's hits -- every gallery
    row whose fp32 fmaf-chain score (search_topk's, bit for bit) is >= thresh[i] -- lie at lims[i]:lims[i + 1] in ascending row order, idx = idx_base + row.
    A NaN score or threshold hits nothing.  g_item i32 [N] / q_skip i32 [Q]: rows carrying the query's skip code (>= 0) are left out, as search_items.
    No [Q, N] score image: a count pass, torch.cumsum, one read of the total, exactly T entries allocated, a fill pass (sc_search_range_count / _fill).
    More than max_results hits (default: 1 GiB of results) raise ValueError before anything is allocated."""
    return _search_range(torch.float32, q, g, thresh, n_split, idx_base, g_item, q_skip, max_results)


def search_range_bf16(q, g, thresh, n_split=0, idx_base=0, g_item=None, q_skip=None, max_results=None):
    """search_range on bf16 rows (E % 16 == 0): search_topk_bf16's scores under the same rule (sc_search_range_count_bf16 / _fill_bf16)."""
    return _search_range(bf16, q, g, thresh, n_split, idx_base, g_item, q_skip, max_results)


# ---- cascaded tail, training (train_cascaded.hip) ----
def attn_small_bwd(qkv16, dout, B, L, H, causal=True):
    """qkv bf16 [B*L, 3*H*64] (saved by the forward), dout f32 [B*L, H*64] -> dqkv f32 [B*L, 3*H*64]."""
    _need_cuda(qkv16, dout)
    W = H * 64
    assert qkv16.dtype == bf16 and qkv16.shape == (B * L, 3 * W) and qkv16.is_contiguous()
    _f32c(dout)
    dqkv = torch.empty(B * L, 3 * W, device=dout.device, dtype=torch.float32)
    check(lib().sc_attn_small_bwd(ptr(qkv16), ptr(dout), ptr(dqkv), B, L, H, 64, int(causal), stream()), "sc_attn_small_bwd")
    return dqkv


def split_hilo(a, nblk=2):
    """a f32 [M,K] (row stride allowed) -> bf16 [M, nblk*K] = (hi | lo) or (hi | lo | hi), hi + lo = a to ~16 bits."""
    _need_cuda(a)
    assert a.dtype == torch.float32 and a.dim() == 2 and a.stride(1) == 1
    M, K = a.shape
    out = torch.empty(M, nblk * K, device=a.device, dtype=bf16)
    check(lib().sc_split_hilo_bf16(ptr(a), a.stride(0), ptr(out), M, K, nblk, stream()), "sc_split_hilo_bf16")
    return out


def quickgelu_f32(z, out_bf16=False):
    _f32c(z)
    y = torch.empty(z.shape, device=z.device, dtype=bf16 if out_bf16 else torch.float32)
    check(lib().sc_quickgelu_f32(ptr(z), ptr(y), z.numel(), 0, int(out_bf16), stream()), "sc_quickgelu_f32")
    return y


def quickgelu_bwd_(z, dh):
    """dh *= quickgelu'(z) in place."""
    _f32c(z, dh)
    check(lib().sc_quickgelu_f32(ptr(z), ptr(dh), z.numel(), 1, 0, stream()), "sc_quickgelu_f32")
    return dh


def vq_st_bwd_(cos, dprob, temp, mask_ids=(0, 2, 3)):
    """dprob f32 [R,V] becomes d loss / d cos in place; returns rowdot f32 [R] = sum_v dcos cos."""
    import ctypes
    _f32c(cos, dprob)
    R, V = cos.shape
    rowdot = torch.empty(R, device=cos.device, dtype=torch.float32)
    ids = (ctypes.c_int32 * max(1, len(mask_ids)))(*[int(i) for i in mask_ids])
    check(lib().sc_vq_st_bwd(ptr(cos), ptr(dprob), ptr(rowdot), R, V, float(temp), ctypes.cast(ids, ctypes.c_void_p), len(mask_ids), stream()),
          "sc_vq_st_bwd")
    return rowdot


# ---- vector-quantizer modes beside the shipped one: soft / gumbel (vq_modes.hip; noise contract: include/speechclip_hip.h) ----
def _mask_arg(mask_ids):
    import ctypes
    ids = (ctypes.c_int32 * max(1, len(mask_ids)))(*[int(i) for i in mask_ids])
    return ids, ctypes.cast(ids, ctypes.c_void_p), len(mask_ids)


def _seed_arg(seed):
    """seed None / 0 -> (0, off): the branch draws its seeds from [1, 2^31 - 8), so 0 is free to mean "no noise" in vq_results["gumbel_seed"]."""
    return (0, 0) if not seed else (int(seed) & 0xffffffff, 1)


def vq_gumbel_noise(R, V, seed, device="cuda"):
    """f32 [R,V] Gumbel(0,1) noise of (seed, r * V + v): what the VQ kernels regenerate on the fly."""
    out = torch.empty(R, V, device=device, dtype=torch.float32)
    check(lib().sc_vq_gumbel_noise(ptr(out), R, V, int(seed) & 0xffffffff, stream()), "sc_vq_gumbel_noise")
    return out


def vq_noisy_argmax(scores, seed=None, mask_ids=(0, 2, 3)):
    """scores f32 [R,V] -> i64 [R] arg-max of scores + noise over the unmasked columns (lowest index on ties)."""
    _f32c(scores)
    R, V = scores.shape
    targets = torch.empty(R, device=scores.device, dtype=torch.int64)
    keep, ids, n = _mask_arg(mask_ids)
    sd, on = _seed_arg(seed)
    check(lib().sc_vq_noisy_argmax(ptr(scores), ptr(targets), R, V, sd, on, ids, n, stream()), "sc_vq_noisy_argmax")
    return targets


def vq_probs(scores, temp, seed=None, mask_ids=(0, 2, 3)):
    """scores f32 [R,V] -> f32 [R,V] softmax((scores + noise) / temp) over the unmasked columns (masked: exactly 0)."""
    _f32c(scores)
    R, V = scores.shape
    out = torch.empty(R, V, device=scores.device, dtype=torch.float32)
    keep, ids, n = _mask_arg(mask_ids)
    sd, on = _seed_arg(seed)
    check(lib().sc_vq_probs(ptr(scores), ptr(out), R, V, float(temp), sd, on, ids, n, stream()), "sc_vq_probs")
    return out


_VQ_SOFT_TABLES = {}


def vq_soft_table(emb):
    """The frozen sub-word table as sc_vq_soft_embed's (hi, lo) bf16 MFMA operand, cached per table version like _cos_table."""
    import weakref
    key = emb.data_ptr()
    hit = _VQ_SOFT_TABLES.get(key)
    if hit is not None and hit[0] == (emb._version, param_epoch(emb), tuple(emb.shape)) and hit[2]() is emb:
        return hit[1]
    e = emb.detach().float().contiguous()
    V, E = e.shape
    tab = torch.empty(lib().sc_vq_soft_table_bytes(V, E), device=e.device, dtype=torch.uint8)
    check(lib().sc_vq_soft_table(ptr(e), ptr(tab), V, E, stream()), "sc_vq_soft_table")
    _VQ_SOFT_TABLES.clear()
    _VQ_SOFT_TABLES[key] = ((emb._version, param_epoch(emb), tuple(emb.shape)), tab, weakref.ref(emb))
    return tab


# route of the soft modes' product: "fused" = sc_vq_soft_embed, "probs" = sc_vq_probs + a GEMM.  Fused won 3 of 3 interleaved pairs at V = 8112 and 49408
# (profiles/vq_soft_embed_bench.txt); the tests run both.
VQ_SOFT_ROUTE = "fused"


def vq_soft_embed_probs(scores, emb, temp, seed=None, mask_ids=(0, 2, 3)):
    """The composed route: y as a dense image (sc_vq_probs), then y @ emb -- on the MFMA GEMM with y and emb^T split into bf16 (hi, lo) terms where the GEMM
    takes the shape (the three products hi.hi + lo.hi + hi.lo in one depth-3V call), on the fp32 SIMT sgemm otherwise."""
    y = vq_probs(scores, temp, seed, mask_ids)
    e = emb.detach().float().contiguous()
    V, E = e.shape
    if V % 64 == 0 and E % 4 == 0:
        et = e.t().contiguous()
        hi = et.to(bf16)
        lo = (et - hi.float()).to(bf16)
        return gemm(split_hilo(y, nblk=3), torch.cat([hi, hi, lo], dim=1).contiguous(), out_f32=True)
    return sgemm(y, e)


def vq_soft_embed(scores, emb, temp, seed=None, mask_ids=(0, 2, 3), nsplit=0, want_stats=False):
    """keywords f32 [R,E] = softmax((scores + noise) / temp) @ emb, fused (no [R,V] probability image); `nsplit` chunks of V (0 = auto).
    Shapes the fused kernel does not cover (E % 64, V < 5: it says so by returning 1) are composed from sc_vq_probs and a GEMM.
    want_stats: also (row_max, row_den) f32 [R] of the fused kernel's pre-pass (None on the composed route)."""
    _f32c(scores)
    R, V = scores.shape
    E = emb.shape[1]
    assert emb.shape[0] == V, (emb.shape, V)
    rc = 1
    if VQ_SOFT_ROUTE == "fused":
        tab = vq_soft_table(emb) if E % 64 == 0 and E >= 64 else None        # without a table the kernel answers "not covered" before it looks at it
        kw = torch.empty(R, E, device=scores.device, dtype=torch.float32)
        rmax = torch.empty(R, device=scores.device, dtype=torch.float32)
        rden = torch.empty(R, device=scores.device, dtype=torch.float32)
        ws = torch.empty(lib().sc_vq_soft_embed_workspace_bytes(R, V, E, int(nsplit)), device=scores.device, dtype=torch.uint8)
        keep, ids, n = _mask_arg(mask_ids)
        sd, on = _seed_arg(seed)
        rc = lib().sc_vq_soft_embed(ptr(scores), ptr(tab), ptr(kw), ptr(rmax), ptr(rden), ptr(ws), R, V, E, float(temp), sd, on, ids, n, int(nsplit), stream())
        if rc not in (0, 1):
            check(rc, "sc_vq_soft_embed")
    if rc == 1:
        kw, rmax, rden = vq_soft_embed_probs(scores, emb, temp, seed, mask_ids), None, None
    return (kw, rmax, rden) if want_stats else kw


def vq_mode_bwd_(cos, dprob, temp, seed=None, mask_ids=(0, 2, 3)):
    """dprob f32 [R,V] (d loss / d y, y = softmax((cos + noise) / temp)) becomes d loss / d cos in place;
    returns (rowdot_cos, rowdot_z) f32 [R] = sum_v dcos cos, sum_v dcos (cos + noise)."""
    _f32c(cos, dprob)
    R, V = cos.shape
    rd = torch.empty(R, device=cos.device, dtype=torch.float32)
    rz = torch.empty(R, device=cos.device, dtype=torch.float32)
    keep, ids, n = _mask_arg(mask_ids)
    sd, on = _seed_arg(seed)
    check(lib().sc_vq_mode_bwd(ptr(cos), ptr(dprob), ptr(rd), ptr(rz), R, V, float(temp), sd, on, ids, n, stream()), "sc_vq_mode_bwd")
    return rd, rz


def cosine_bwd_finish(a, G, rowdot, eps=1e-8):
    _f32c(a, G, rowdot)
    da = torch.empty_like(a)
    check(lib().sc_cosine_bwd_finish(ptr(a), ptr(G), ptr(rowdot), ptr(da), a.shape[0], a.shape[1], eps, stream()), "sc_cosine_bwd_finish")
    return da


def kw_bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps):
    """x f32 [B,K,E]; gamma/beta/running_* f32 [E*K] in the reference's (e, k) order -> (y, mean [K*E], rstd [K*E]); running stats updated in place."""
    _f32c(x, gamma, beta)
    B, K, E = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(K * E, device=x.device, dtype=torch.float32)
    rstd = torch.empty(K * E, device=x.device, dtype=torch.float32)
    if running_mean is not None:
        _f32c(running_mean, running_var)
    check(lib().sc_kw_bn_train_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), B, K, E,
                                   float(momentum), float(eps), stream()), "sc_kw_bn_train_fwd")
    return y, mean, rstd


def kw_bn_bwd(x, dy, gamma, mean, rstd, want_param_grads=True):
    _f32c(x, dy, gamma, mean, rstd)
    B, K, E = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(K * E, device=x.device, dtype=torch.float32) if want_param_grads else None
    db = torch.empty(K * E, device=x.device, dtype=torch.float32) if want_param_grads else None
    check(lib().sc_kw_bn_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), B, K, E, stream()), "sc_kw_bn_bwd")
    return dx, dg, db


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def image_normalize_u8(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 [B,H,W,3] (already resized / centre-cropped on the host) -> f32 [B,3,H,W] = (x/255 - mean) / std  (ToTensor + Normalize)."""
    import ctypes
    _need_cuda(u8)
    assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[-1] == 3 and u8.is_contiguous()
    B, H, W, _ = u8.shape
    out = torch.empty(B, 3, H, W, device=u8.device, dtype=torch.float32)
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    sd = (ctypes.c_float * 3)(*[float(x) for x in std])
    check(lib().sc_image_normalize_u8(ptr(u8), ptr(out), B, H, W, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), stream()),
          "sc_image_normalize_u8")
    return out


def image_prep(images, n_px, mean=CLIP_MEAN, std=CLIP_STD, return_u8=False):
    """CLIP's whole `_transform` on the current device (sc_image_prep_u8): a list of decoded uint8 host images ([h, w, 3] RGB or [h, w] L, arrays or tensors,
    every image its own size, as data.image_transforms.load_images_raw returns them) -> f32 [B, 3, n_px, n_px]; with return_u8 also the uint8
    [B, n_px, n_px, 3] crop, which equals PIL's bicubic resize + centre crop on every byte.  The plans (cached per size) and the bytes go into ONE pinned buffer,
    cross PCIe in one non-blocking copy, and one library call on the current stream does the rest; the workspace comes from torch's allocator on that stream."""
    return _image_prep(images, n_px, mean, std, return_u8)


def _image_prep(images, n_px, mean=CLIP_MEAN, std=CLIP_STD, return_u8=False, device=None, out=None, out_u8=None, workspace=None, pad_bytes=0, plans=None):
    """image_prep with the knobs the tests need: device (any spelling of a GPU, default the current one), out / out_u8 / workspace = caller-owned buffers to
    write into (contiguous, right dtype and size; the tests put them between sentinel guards), pad_bytes / plans: see plan_image_batch."""
    import ctypes
    import numpy as np
    from .data.image_transforms import plan_image_batch
    if not torch.cuda.is_available():
        raise _lib.SpeechClipHipError("speechclip_amd ops need a GPU: image_prep has no CPU fallback (the host path is data.image_transforms.load_images_u8)")
    dev = torch.device("cuda") if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.SpeechClipHipError("speechclip_amd ops need device tensors (no CPU fallback)")
    if dev.index is None:          # "cuda" -> the current device WITH its index: the tensors allocated below report an indexed device
        dev = torch.device("cuda", torch.cuda.current_device())
    n = int(n_px)
    plan = plan_image_batch(images, n, pad_bytes=pad_bytes, plans=plans)
    B = len(plan.images)
    # one pinned buffer: offsets | geom | tables | (16-byte aligned) pixels.  A fresh pinned tensor per call: torch's host allocator does not hand the block
    # out again before the copy below has finished.
    n_off, n_geom, n_tab = plan.offsets.nbytes, plan.geom.nbytes, plan.tables.nbytes
    head = (n_off + n_geom + n_tab + 15) // 16 * 16
    host = torch.empty(max(head + plan.packed_bytes, 16), dtype=torch.uint8, pin_memory=True)
    hb = host.numpy()
    hb[:n_off] = plan.offsets.reshape(-1).view(np.uint8)
    hb[n_off:n_off + n_geom] = plan.geom.reshape(-1).view(np.uint8)
    hb[n_off + n_geom:n_off + n_geom + n_tab] = plan.tables.view(np.uint8)
    if pad_bytes:
        hb[head:] = 255
    for b, im in enumerate(plan.images):
        o = head + int(plan.offsets[0, b])
        hb[o:o + im.size] = im.reshape(-1)
    with torch.cuda.device(dev):
        d = host.to(dev, non_blocking=True)
        if out is None:
            out = torch.empty(B, 3, n, n, device=dev, dtype=torch.float32)
        if out_u8 is None and return_u8:
            out_u8 = torch.empty(B, n, n, 3, device=dev, dtype=torch.uint8)
        if workspace is None:
            workspace = torch.empty(max(plan.workspace_bytes, 1), device=dev, dtype=torch.uint8)
        for t, shape, dt in ((out, (B, 3, n, n), torch.float32), (out_u8, (B, n, n, 3), torch.uint8)):
            if t is not None and not (t.is_cuda and t.device == dev and t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f"image_prep: output buffer must be a contiguous {dt} {shape} tensor on {dev}")
        if not (workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
            raise ValueError(f"image_prep: workspace must be a contiguous uint8 tensor on {dev}")
        if B == 0:
            return (out, out_u8) if return_u8 else out
        m = (ctypes.c_float * 3)(*[float(x) for x in mean])
        sd = (ctypes.c_float * 3)(*[float(x) for x in std])
        hp, dp = host.data_ptr(), d.data_ptr()
        has_tab = n_tab > 0
        with _HbmSpan("image_prep", plan.packed_bytes + 2 * plan.workspace_bytes + B * n * n * (12 + (3 if out_u8 is not None else 0))):
            check(lib().sc_image_prep_u8(dp + head, plan.packed_bytes, hp, dp, hp + n_off, dp + n_off, hp + n_off + n_geom if has_tab else None,
                                         dp + n_off + n_geom if has_tab else None, n_tab // 4, B, n, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p),
                                         ptr(workspace), workspace.numel(), ptr(out), ptr(out_u8), stream()), "sc_image_prep_u8")
    return (out, out_u8) if return_u8 else out


# ---- fine-tuning HuBERT layers (train_hubert.hip) ----
def transpose_bf16(src, ld_in, stride_in, rows, cols, batch, rows_padded=None, out=None, ld_out=None, stride_out=None):
    """batch of [rows, cols] bf16 matrices (row r of matrix z at src + z*stride_in + r*ld_in) -> out bf16 [batch, cols, rows_padded] (zero padded);
    ld_out / stride_out place matrix z at out + z*stride_out with rows of stride ld_out instead (e.g. side by side in one wide matrix)."""
    _need_cuda(src)
    rp = rows if rows_padded is None else rows_padded
    if out is None:
        out = torch.empty(batch, cols, rp, device=src.device, dtype=bf16)
    check(lib().sc_transpose_bf16(ptr(src), ld_in, stride_in, ptr(out), rp if ld_out is None else ld_out, cols * rp if stride_out is None else stride_out,
                                  rows, cols, rp, batch, stream()), "sc_transpose_bf16")
    return out


def attn_softmax_bwd(S, dP, dO_head, ld_do, O_head, ld_o, rows_per_batch, klens_i32, L, scale, drop=None):
    """S, dP f32 [Z, Lp, Lp]; dO_head / O_head: views at the head's first column, rows of stride ld_*; -> (P, dS) bf16 [Z, Lp, Lp].
    drop = (p, seed, H, h): the forward ran attention_dropout with (p, seed); this is head h of H."""
    _need_cuda(S, dP)
    Z, Lp, _ = S.shape
    P = torch.empty(Z, Lp, Lp, device=S.device, dtype=bf16)
    dS = torch.empty_like(P)
    if drop is not None and drop[0] > 0:
        check(lib().sc_attn_softmax_bwd_dropout(ptr(S), ptr(dP), Lp, Lp * Lp, ptr(dO_head), ld_do, ptr(O_head), ld_o, rows_per_batch, ptr(klens_i32), ptr(P),
                                                ptr(dS), L, Lp, Z, float(scale), float(drop[0]), int(drop[1]) & 0xffffffff, int(drop[2]), int(drop[3]),
                                                stream()), "sc_attn_softmax_bwd_dropout")
        return P, dS
    check(lib().sc_attn_softmax_bwd(ptr(S), ptr(dP), Lp, Lp * Lp, ptr(dO_head), ld_do, ptr(O_head), ld_o, rows_per_batch, ptr(klens_i32), ptr(P), ptr(dS),
                                    L, Lp, Z, float(scale), stream()), "sc_attn_softmax_bwd")
    return P, dS


def gelu_bwd_bf16(u, dh):
    _need_cuda(u, dh)
    assert u.dtype == bf16 and dh.dtype == bf16 and u.is_contiguous() and dh.is_contiguous() and u.shape == dh.shape
    du = torch.empty_like(u)
    check(lib().sc_gelu_bwd_bf16(ptr(u), ptr(dh), ptr(du), u.numel(), stream()), "sc_gelu_bwd_bf16")
    return du


def quickgelu_bwd_bf16(u, dh, out=None):
    """du bf16 = dh * quickgelu'(u) (train_vit.hip): u, dh bf16 of one shape, contiguous (any length, views at any element offset)."""
    _need_cuda(u, dh, out)
    assert u.dtype == bf16 and dh.dtype == bf16 and u.is_contiguous() and dh.is_contiguous() and u.shape == dh.shape
    du = torch.empty_like(u) if out is None else out
    assert du.dtype == bf16 and du.is_contiguous() and du.shape == u.shape
    check(lib().sc_quickgelu_bwd_bf16(ptr(u), ptr(dh), ptr(du), u.numel(), stream()), "sc_quickgelu_bwd_bf16")
    return du


def vit_embed_bwd(dx, patch, cls, pos, gamma, B, ntok, D, eps=1e-5, out=None):
    """Adjoint of vit_embed: dx f32 [B*ntok, D], the forward's patch bf16 [B*(ntok-1), D], cls f32 [D], pos f32 [ntok, D], gamma f32 [D]
    -> (dpatch bf16 [B*(ntok-1), D], dpos f32 [ntok, D], dcls = dpos[0] (a view), dgamma f32 [D], dbeta f32 [D]); out = (dpatch, dpos, dgamma, dbeta) to fill."""
    _need_cuda(patch)
    _f32c(dx, cls, pos, gamma)
    assert patch.dtype == bf16 and patch.is_contiguous() and tuple(patch.shape) == (B * (ntok - 1), D), (tuple(patch.shape), B, ntok, D)
    assert tuple(dx.shape) == (B * ntok, D) and cls.numel() == D and tuple(pos.shape) == (ntok, D) and gamma.numel() == D
    dev = patch.device
    if out is None:
        out = (torch.empty_like(patch), torch.empty(ntok, D, device=dev, dtype=torch.float32), torch.empty(D, device=dev, dtype=torch.float32),
               torch.empty(D, device=dev, dtype=torch.float32))
    dpatch, dpos, dgamma, dbeta = out
    assert dpatch.dtype == bf16 and dpatch.is_contiguous() and dpatch.shape == patch.shape
    _f32c(dpos, dgamma, dbeta)
    assert tuple(dpos.shape) == (ntok, D) and dgamma.numel() == D and dbeta.numel() == D
    ws = torch.empty(max(1, int(lib().sc_vit_embed_bwd_workspace_bytes(B, ntok, D))), device=dev, dtype=torch.uint8)
    check(lib().sc_vit_embed_bwd(ptr(dx), ptr(patch), ptr(cls), ptr(pos), ptr(gamma), ptr(dpatch), ptr(dpos), ptr(dgamma), ptr(dbeta), ptr(ws), B, ntok, D,
                                 eps, stream()), "sc_vit_embed_bwd")
    return dpatch, dpos, dpos[0], dgamma, dbeta


def layernorm_bwd_bf16(x, dy, gamma, eps=1e-5, want_param_grads=True):
    """x, dy bf16 [rows, D] -> (dx bf16, dgamma f32 [D] | None, dbeta f32 [D] | None)."""
    _need_cuda(x, dy, gamma)
    rows, D = x.shape
    assert x.dtype == bf16 and dy.dtype == bf16 and x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    npart = int(lib().sc_layernorm_bwd_bf16_partials(rows))
    part = torch.empty(npart, 2 * D, device=x.device, dtype=torch.float32)
    check(lib().sc_layernorm_bwd_bf16(ptr(x), ptr(dy), ptr(gamma), ptr(dx), ptr(part), rows, D, eps, stream()), "sc_layernorm_bwd_bf16")
    if not want_param_grads:
        return dx, None, None
    sums = colsum(part)
    return dx, sums[:D].contiguous(), sums[D:].contiguous()


def colsum_bf16(x, out=None, accumulate=False):
    _need_cuda(x)
    assert x.dtype == bf16 and x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    ws = torch.empty(int(lib().sc_colsum_bf16_workspace_bytes(rows, cols)), device=x.device, dtype=torch.uint8)
    if out is None:
        out = torch.empty(cols, device=x.device, dtype=torch.float32)
        accumulate = False
    check(lib().sc_colsum_bf16(ptr(x), x.stride(0), rows, cols, ptr(ws), ptr(out), int(accumulate), stream()), "sc_colsum_bf16")
    return out


def axpy_bf16(y, x, alpha):
    _need_cuda(y, x)
    assert y.dtype == bf16 and x.dtype == bf16 and y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel()
    check(lib().sc_axpy_bf16(ptr(y), ptr(x), float(alpha), y.numel(), stream()), "sc_axpy_bf16")
    return y


def cls_pool_dz(pp, ds, dzbar, u, lens_i32, B, T, NQ, R, D):
    """-> dz bf16 [B*T, D]: gradient of the mixed frames from sc_cls_pool_bwd's workspaces."""
    _f32c(pp, ds, dzbar, u)
    dz = torch.empty(B * T, D, device=pp.device, dtype=bf16)
    check(lib().sc_cls_pool_dz(ptr(pp), ptr(ds), ptr(dzbar), ptr(u), ptr(lens_i32), ptr(dz), B, T, NQ, R, D, D, stream()), "sc_cls_pool_dz")
    return dz


# ---------------------------------------------------------------------------------------------- front-end backward (train_front.py)
def posconv_conv(x, valid_i32, wg, B, Tp, D, G, Kw):
    """The grouped positional conv alone: x bf16 [B*Tp, D] (frames >= valid[b] read as zero), wg bf16 [G, D/G, Kw*D/G] -> bf16 [B, G, Tp, D/G]."""
    _need_cuda(x, wg)
    cg = D // G
    conv = torch.empty(B * G * Tp * cg, device=x.device, dtype=bf16)
    rc = lib().sc_posconv_conv(ptr(x), ptr(valid_i32), ptr(wg), ptr(conv), B, Tp, D, G, Kw, stream())
    if rc == 1:
        _posconv_pack_gemm(x, valid_i32, wg, conv, B, Tp, D, G, Kw)
    else:
        check(rc, "sc_posconv_conv")
    return conv


def posconv_pack(x, valid_i32, B, Tp, D, G, Kw):
    """Sliding-window layout of the masked input: bf16 [B, G, Tp + Kw, D/G] (+64 slack elements), Kw/2 zero rows in front."""
    cg = D // G
    xg = torch.empty(B * G * (Tp + Kw) * cg + 64, device=x.device, dtype=bf16)
    xg[B * G * (Tp + Kw) * cg:].zero_()
    check(lib().sc_posconv_pack(ptr(x), ptr(valid_i32), ptr(xg), B, Tp, D, G, Kw, stream()), "sc_posconv_pack")
    return xg


def _posconv_pack_gemm(x, valid_i32, wg, conv, B, Tp, D, G, Kw):
    """The route of the group widths the windowed kernel does not take: pack the sliding windows (sc_posconv_pack), then conv[b][g][t][:] = wg[g] . (the Kw * cg elements of
    slab (b, g) from row t on), one batched GEMM over overlapping rows.  The GEMM reads 16-byte rows and takes K in multiples of 64, so a group width that is no multiple
    of 8 (D/G = 68) is widened with zero channels and a window length that is no multiple of 64 with zero weight columns: what a row reads past its window are the next
    rows' elements (finite, times zero) or the zeroed slack behind xg."""
    pad = torch.nn.functional.pad
    cg = D // G
    cgp = (cg + 7) // 8 * 8
    w = wg.reshape(G, cg, Kw, cg)
    if cgp != cg:
        x = pad(x.reshape(B * Tp, G, cg), (0, cgp - cg)).reshape(B * Tp, G * cgp)
        w = pad(w, (0, cgp - cg))
    K = Kw * cgp
    Kp = (K + 63) // 64 * 64
    w = w.reshape(G, cg, K)
    if Kp != K:
        w = pad(w, (0, Kp - K))
    xg = posconv_pack(x, valid_i32, B, Tp, G * cgp, G, Kw)
    gemm_batched(xg, cgp, (Tp + Kw) * cgp, w.contiguous(), cg * Kp, G, conv, cg, Tp * cg, None, Tp, cg, Kp, B * G)


# The per-utterance kernels serve both layouts: uniform rows (B utterances of Tp rows each) are the packed layout with row_off[b] = b * Tp.  row_off_i32 (B + 1
# device ints, utterance b owns rows [row_off[b], row_off[b + 1]) of every transformer-level tensor) selects the *_packed entry; the row count is the tensor's own.
def _rows_of(t, B, Tp, D, row_off_i32):
    """Row count of the bf16 [rows, D] tensor t: B * Tp on uniform rows, row_off[B] (= what t holds) on packed rows."""
    assert t.dtype == bf16 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == D
    assert t.shape[0] == B * Tp if row_off_i32 is None else (row_off_i32.is_cuda and row_off_i32.dtype == torch.int32 and row_off_i32.numel() == B + 1)
    return t.shape[0]


def posconv_finish_train(x, valid_i32, conv, bias, B, Tp, D, G, row_off_i32=None):
    """-> (u, s) bf16 [rows, D]: u = conv + bias regrouped from the slabs (utterance b = [G][rows_b][D/G] at element row_off[b] * D), s = mask(x) + gelu(u)."""
    rows = _rows_of(x, B, Tp, D, row_off_i32)
    assert conv.numel() >= rows * D and bias.numel() == D
    u = torch.empty(rows, D, device=x.device, dtype=bf16)
    s = torch.empty_like(u)
    if row_off_i32 is None:
        check(lib().sc_posconv_finish_train(ptr(x), ptr(valid_i32), ptr(conv), ptr(bias), ptr(u), ptr(s), B, Tp, D, G, stream()), "sc_posconv_finish_train")
    else:
        check(lib().sc_posconv_finish_train_packed(ptr(x), ptr(valid_i32), ptr(row_off_i32), ptr(conv), ptr(bias), ptr(u), ptr(s), B, rows, D, G, stream()),
              "sc_posconv_finish_train_packed")
    return u, s


def posconv_dgrad_finish(convT, ds, valid_i32, B, Tp, D, G, row_off_i32=None):
    """dx bf16 [rows, D] = mask(ds + convT regrouped, time reversed inside each utterance's own rows)."""
    rows = _rows_of(ds, B, Tp, D, row_off_i32)
    assert convT.numel() >= rows * D
    dx = torch.empty(rows, D, device=ds.device, dtype=bf16)
    if row_off_i32 is None:
        check(lib().sc_posconv_dgrad_finish(ptr(convT), ptr(ds), ptr(valid_i32), ptr(dx), B, Tp, D, G, stream()), "sc_posconv_dgrad_finish")
    else:
        check(lib().sc_posconv_dgrad_finish_packed(ptr(convT), ptr(ds), ptr(valid_i32), ptr(row_off_i32), ptr(dx), B, rows, D, G, stream()),
              "sc_posconv_dgrad_finish_packed")
    return dx


def reverse_rows_bf16(x, B, T, D, row_off_i32=None):
    """out[row_off[b] + rows_b - 1 - t] = x[row_off[b] + t]: time reversal inside every utterance's own rows (uniform: out[b, T - 1 - t] = x[b, t])."""
    rows = _rows_of(x, B, T, D, row_off_i32)
    out = torch.empty_like(x)
    if row_off_i32 is None:
        check(lib().sc_reverse_rows_bf16(ptr(x), ptr(out), B, T, D, stream()), "sc_reverse_rows_bf16")
    else:
        check(lib().sc_reverse_rows_packed_bf16(ptr(x), ptr(row_off_i32), ptr(out), B, rows, D, stream()), "sc_reverse_rows_packed_bf16")
    return out


def _conv0_grad_rows(wav, dy, C, P, row_off_i32, row_scale):
    """Checks shared by conv0_bwd / conv0_wgrad.  dy bf16 [rows (+ slack), C]: utterance b's frames at rows b * P .. (uniform, B * P rows) or
    row_scale * row_off[b] .. (packed, P = row_scale * total_rows rows in all) -> (B, L, partials buffer f32 [B, C * 12])."""
    _need_cuda(wav, dy)
    B, L = wav.shape
    assert wav.dtype == torch.float32 and wav.is_contiguous() and dy.dtype == bf16 and dy.is_contiguous() and dy.dim() == 2 and dy.shape[1] == C
    assert dy.shape[0] >= B * P if row_off_i32 is None else (dy.shape[0] >= P and row_off_i32.is_cuda and row_off_i32.dtype == torch.int32 and row_off_i32.numel() == B + 1)
    return B, L, torch.empty(B, C * 12, device=wav.device, dtype=torch.float32)


def conv0_bwd(wav, w, gamma, beta, dy, T0, P, eps=1e-5, row_off_i32=None, row_scale=None):
    """wav f32 [B, L]; w f32 [C, 10]; dy as _conv0_grad_rows -> (dw f32 [C, 10], dgamma f32 [C], dbeta f32 [C], per-utterance partials f32 [B, C, 12])."""
    C = w.shape[0]
    B, L, part = _conv0_grad_rows(wav, dy, C, P, row_off_i32, row_scale)
    assert w.dtype == torch.float32 and w.is_contiguous()
    if row_off_i32 is None:
        check(lib().sc_conv0_bwd(ptr(wav), L, ptr(w), ptr(gamma), ptr(beta), ptr(dy), ptr(part), B, C, T0, P, eps, stream()), "sc_conv0_bwd")
    else:
        check(lib().sc_conv0_bwd_packed(ptr(wav), L, ptr(w), ptr(gamma), ptr(beta), ptr(dy), ptr(part), B, C, T0, ptr(row_off_i32), row_scale, eps, stream()),
              "sc_conv0_bwd_packed")
    tot = colsum(part).view(C, 12)
    return tot[:, :10].contiguous(), tot[:, 10].contiguous(), tot[:, 11].contiguous(), part.view(B, C, 12)


def conv0_wgrad(wav, du, C, T0, P, row_off_i32=None, row_scale=None):
    """wav f32 [B, L]; du (as _conv0_grad_rows) = gradient of conv layer 0's (pre-norm) output -> (dw f32 [C, 10], dbias f32 [C], partials f32 [B, C, 12])."""
    B, L, part = _conv0_grad_rows(wav, du, C, P, row_off_i32, row_scale)
    if row_off_i32 is None:
        check(lib().sc_conv0_wgrad(ptr(wav), L, ptr(du), ptr(part), B, C, T0, P, stream()), "sc_conv0_wgrad")
    else:
        check(lib().sc_conv0_wgrad_packed(ptr(wav), L, ptr(du), ptr(part), B, C, T0, ptr(row_off_i32), row_scale, stream()), "sc_conv0_wgrad_packed")
    tot = colsum(part).view(C, 12)
    return tot[:, :10].contiguous(), tot[:, 10].contiguous(), part.view(B, C, 12)


# The packed forms under their earlier names (argument order of the C entries): forwards into the merged wrappers above, nothing else.
posconv_finish_train_packed = lambda x, valid, off, conv, bias, B, total, D, G: posconv_finish_train(x, valid, conv, bias, B, 0, D, G, off)      # noqa: E731
posconv_dgrad_finish_packed = lambda convT, ds, valid, off, B, total, D, G: posconv_dgrad_finish(convT, ds, valid, B, 0, D, G, off)                 # noqa: E731
reverse_rows_packed_bf16 = lambda x, off, B, total, D: reverse_rows_bf16(x, B, 0, D, off)                                                             # noqa: E731
conv0_bwd_packed = lambda wav, w, gamma, beta, dy, T0, off, scale, total, eps=1e-5: conv0_bwd(wav, w, gamma, beta, dy, T0, scale * total, eps, off, scale)      # noqa: E731
conv0_wgrad_packed = lambda wav, du, C, T0, off, scale, total: conv0_wgrad(wav, du, C, T0, scale * total, off, scale)                                  # noqa: E731


# ---- packed rows only (padding-free whole-encoder training)
def posconv_conv_packed(x, lim_i32, row_off_i32, wg, B, rows_max, total_rows, D, G, Kw):
    """posconv_conv over packed rows: x bf16 [total_rows, D] (rows t >= lim[b] of utterance b read as zero) -> conv slabs, utterance b = [G][rows_b][D/G] at
    element row_off[b] * D."""
    _need_cuda(x, wg, row_off_i32)
    assert x.dtype == bf16 and x.is_contiguous() and x.shape == (total_rows, D)
    conv = torch.empty(total_rows * D, device=x.device, dtype=bf16)
    rc = lib().sc_posconv_conv_packed(ptr(x), ptr(lim_i32), ptr(row_off_i32), ptr(wg), ptr(conv), B, rows_max, D, G, Kw, stream())
    if rc == 1:
        raise _lib.SpeechClipHipError("packed batches need the windowed positional-conv kernel (D/G in 32/48/64 and Kw * D/G a multiple of 64), "
                                      f"got D/G = {D // G}, Kw = {Kw}")
    check(rc, "sc_posconv_conv_packed")
    return conv


def posconv_pack_gapped(x, lim_i32, row_off_i32, B, total_rows, D, G, gap, lead, slab_rows):
    """-> bf16 [G, slab_rows, D/G] (+64 slack elements): utterance b's rows t < min(lim[b], rows_b) at slab row lead + row_off[b] + b * gap + t, zeros elsewhere."""
    assert x.dtype == bf16 and x.is_contiguous() and x.shape == (total_rows, D) and slab_rows >= lead + total_rows + B * gap
    out = torch.empty(slab_rows * D + 64, device=x.device, dtype=bf16)
    out[slab_rows * D:].zero_()
    check(lib().sc_posconv_pack_gapped(ptr(x), ptr(lim_i32), ptr(row_off_i32), ptr(out), B, total_rows, D, G, gap, lead, slab_rows, stream()),
          "sc_posconv_pack_gapped")
    return out


def gemm_batched2(a, lda, stride_a, stride_a2, w, ldw, stride_w, stride_w2, out, ldc, stride_c, stride_c2, M, N, K, outer, inner):
    """outer x inner products out_z[M,N] = a_z[M,K] w_z[N,K]^T, z = (zo, zi): operand at base + zo*stride + zi*stride2 (elements); out dtype f32 => fp32."""
    _need_cuda(a, w, out)
    flags = GEMM_OUT_F32 if out.dtype == torch.float32 else 0
    check(lib().sc_gemm_bf16_batched2(ptr(a), lda, stride_a, stride_a2, ptr(w), ldw, stride_w, stride_w2, ptr(out), ldc, stride_c, stride_c2, M, N, K,
                                      outer, inner, flags, stream()), "sc_gemm_bf16_batched2")
    return out


def attn_softmax_bwd_heads(S, dP, dO, O, rows_per_batch, klens_i32, L, scale, B, H, drop=None):
    """All heads at once: S, dP f32 [B*H, Lp, Lp]; dO / O bf16 [rows, H*64]; -> (P, dS) bf16 [B*H, Lp, Lp].  drop = (p, seed) of the forward."""
    _need_cuda(S, dP)
    Z, Lp, _ = S.shape
    assert Z == B * H and dO.stride(1) == 1 and O.stride(1) == 1
    P = torch.empty(Z, Lp, Lp, device=S.device, dtype=bf16)
    dS = torch.empty_like(P)
    p_, seed = (float(drop[0]), int(drop[1]) & 0xffffffff) if drop is not None else (0.0, 0)
    check(lib().sc_attn_softmax_bwd_heads(ptr(S), ptr(dP), Lp, Lp * Lp, ptr(dO), dO.stride(0), ptr(O), O.stride(0), rows_per_batch, ptr(klens_i32), ptr(P),
                                          ptr(dS), L, Lp, B, H, float(scale), p_, seed, stream()), "sc_attn_softmax_bwd_heads")
    return P, dS


def attn_bwd_probs(qkv, datt, att, klens_i32, B, T, H, drop=None):
    """P (dropped if the forward dropped) and dS bf16 [B*H, Lp, Lp] straight from the packed rows: qkv bf16 [>= B*T, 3*H*64], datt / att bf16 [B*T, H*64]."""
    _need_cuda(qkv, datt, att)
    d = H * 64
    Lp = -(-T // 64) * 64
    P = torch.empty(B * H, Lp, Lp, device=qkv.device, dtype=bf16)
    dS = torch.empty_like(P)
    p_, seed = (float(drop[0]), int(drop[1]) & 0xffffffff) if drop is not None else (0.0, 0)
    check(lib().sc_attn_bwd_probs(qkv.data_ptr(), qkv.data_ptr() + d * 2, qkv.data_ptr() + 2 * d * 2, 3 * d, ptr(datt), ptr(att), d, ptr(klens_i32), ptr(P),
                                  ptr(dS), B, H, T, Lp, 0.125, p_, seed, stream()), "sc_attn_bwd_probs")
    return P, dS

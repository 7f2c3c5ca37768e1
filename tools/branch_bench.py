"""Timing of the multi-layer parallel branch (one process, one JSON line per item):
  attention  sc_attention_fwd (head_dim 64) vs sc_attention_hd_fwd (64 / 96 / 128) at B = 256, L = 500: TF/s over 4*B*L^2*d
  branch     forward_cls of TransformerEncoder(n_layers = 1) and (n_layers = 2) at B = 256, T = 499, d = 768 (8 heads), and the difference
  hubert     one HuBERT-base encoder layer (hubert.py's eval post-LN sequence: 12 heads of 64, FFN 3072, bf16 rows) at the same B, T, and the
             ratio (extra branch layer) / (HuBERT-base layer)
  --train    the attention backward instead: sc_attention_hd_bwd (statistics + dK / dV sweep + dQ sweep, one call) at head_dim 64 / 96 / 128, B = 256,
             L = 500, full and ragged lengths, TF/s over 10*B*L^2*d (S and dP twice, dV, dK, dQ); at head_dim 64 beside sc_attention_bwd_packed on
             the uniform layout; the Tq = 1 form (the CLS query of a branch's last layer); and forward + backward of the whole stack's autograd
             node (forward_cls_train, n_layers = 2, B = 256, T = 499, d = 768, 8 heads) in both orders, eval and train mode.  The first line
             records the library's hash and the shader clock read after the timed runs' warm-up.  The entry is three kernels in one call: their
             separate times come from running `--train --trace` under a kernel trace (profiles/branch_stack_train_bench.txt has both).
Usage: python tools/branch_bench.py [--iters N] [--train]"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _library_and_clock():
    from speechclip_amd import _lib
    path = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "libspeechclip_hip.so")
    rec = dict(item="setup", library_sha256=hashlib.sha256(open(path, "rb").read()).hexdigest()[:16], device=torch.cuda.get_device_name(0))
    x = torch.randn(4096, 4096, device="cuda")
    for _ in range(50):          # read the clock under load, not the idle one
        x = torch.tanh(x)
    try:
        o = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level:\s*\d+:?\s*\(?(\d+)Mhz", o)
        rec["sclk_MHz"] = int(m.group(1)) if m else None
    except (OSError, subprocess.TimeoutExpired):
        rec["sclk_MHz"] = None
    torch.cuda.synchronize()
    return rec


def train_items(a, ops):
    B, L = 256, 500
    bf = torch.bfloat16
    print(json.dumps(_library_and_clock()), flush=True)
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(200, L + 1, (B,), generator=g).to(torch.int32).cuda()
    full = torch.full((B,), L, dtype=torch.int32).cuda()
    for d, hd in ((768, 64), (768, 96), (1024, 128)):
        H = d // hd
        qkv = torch.randn(B * L, 3 * d, generator=g).to(bf).cuda()
        dO = torch.randn(B * L, d, generator=g).to(bf).cuda()
        if a.trace:      # one shape per kernel instantiation, so a kernel trace's per-kernel statistics are per-shape times
            for p in (0.0, 0.1):
                att = ops.attention_hd_qkv(qkv, B, L, H, full, drop_p=p, seed=3)
                ms = _time(lambda: ops.attention_hd_qkv_bwd(qkv, att, dO, B, L, H, full, drop_p=p, seed=3), a.iters)
                print(json.dumps(dict(item="attention_bwd", kernel="sc_attention_hd_bwd", head_dim=hd, d=d, lens="full", drop_p=p, ms=round(ms, 4))), flush=True)
            continue
        for tag, kl in (("full", full), ("ragged", lens)):
            att = ops.attention_hd_qkv(qkv, B, L, H, kl)
            valid = float((kl.double() ** 2).sum().item()) if tag == "ragged" else float(B) * L * L      # (query, key) pairs that take part
            flops = 10.0 * valid * d
            ms = _time(lambda: ops.attention_hd_qkv_bwd(qkv, att, dO, B, L, H, kl), a.iters)
            rec = dict(item="attention_bwd", kernel="sc_attention_hd_bwd", head_dim=hd, d=d, lens=tag, ms=round(ms, 4), tflops=round(flops / ms / 1e9, 1))
            if hd == 64:
                ms64 = _time(lambda: ops.attention_bwd_packed(qkv, att, dO, B, L, H, kl, None), a.iters)
                print(json.dumps(dict(rec, kernel="sc_attention_bwd_packed", ms=round(ms64, 4), tflops=round(flops / ms64 / 1e9, 1))), flush=True)
            print(json.dumps(rec), flush=True)
        if hd != 64:       # the last layer's form: one CLS query per utterance, k | v rows of [B*L, 2d]
            q1 = torch.randn(B, d, generator=g).to(bf).cuda()
            kv = qkv[:, d:].contiguous()
            d1 = torch.randn(B, 1, d, generator=g).to(bf).cuda()
            qs, ks = (d, d), (L * 2 * d, 2 * d)
            o1 = ops.attention_hd(q1, kv, kv[:, d:], B, H, 1, L, hd, qs, ks, lens)
            ms = _time(lambda: ops.attention_hd_bwd(q1, kv, kv[:, d:], o1, d1, B, H, 1, L, hd, qs, ks, lens), a.iters)
            print(json.dumps(dict(item="attention_bwd_cls_query", kernel="sc_attention_hd_bwd", head_dim=hd, d=d, Tq=1, lens="ragged", ms=round(ms, 4))), flush=True)
        del qkv, dO, att
    if a.trace:
        return
    # the whole stack as one autograd node: forward + backward with gradients to every parameter, the CLS token and the frames
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    T, d = L - 1, 768
    x = torch.randn(B, T, d, generator=g).to(bf).cuda().requires_grad_(True)
    G = torch.randn(B, d, generator=g).cuda()
    al = (lens - 1).long()
    for norm_first in (False, True):
        torch.manual_seed(0)
        m = TransformerEncoder(n_layers=2, d_model=d, nhead=8, dim_feedforward=4 * d, norm_first=norm_first).cuda()
        cls = torch.nn.Parameter(torch.randn(1, 1, d).cuda())

        def step():
            m.zero_grad(set_to_none=True)
            x.grad = cls.grad = None
            (m.forward_cls_train(cls, x, al, seed=7) * G).sum().backward()
        for mode in ("eval", "train"):
            m.train(mode == "train")
            ms = _time(step, max(3, a.iters // 4))
            print(json.dumps(dict(item="branch_stack_fwd_bwd", n_layers=2, norm_first=norm_first, mode=mode, B=B, T=T, d=d, ms=round(ms, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="time the attention backward (sc_attention_hd_bwd) and the stack's training node instead of the forward items")
    ap.add_argument("--trace", action="store_true", help="with --train: only the full-length attention backward per head dim, without and with dropout (for a kernel trace)")
    a = ap.parse_args()
    from speechclip_amd import ops
    if a.train:
        return train_items(a, ops)
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    B, L = 256, 500
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(200, L + 1, (B,), generator=g).to(torch.int32).cuda()
    full = torch.full((B,), L, dtype=torch.int32).cuda()
    for d, hd in ((768, 64), (768, 96), (1024, 128)):
        H = d // hd
        qkv = torch.randn(B * L, 3 * d, generator=g).to(torch.bfloat16).cuda()
        for tag, kl in (("full", full), ("ragged", lens)):
            flops = 4.0 * float(kl.sum().item()) * L * d if tag == "ragged" else 4.0 * B * L * L * d
            ms = _time(lambda: ops.attention_hd_qkv(qkv, B, L, H, kl), a.iters)
            rec = dict(item="attention", kernel="sc_attention_hd_fwd", head_dim=hd, d=d, lens=tag, ms=round(ms, 4), tflops=round(flops / ms / 1e9, 1))
            if hd == 64:
                ms64 = _time(lambda: ops.attention(qkv, B, L, H, kl), a.iters)
                print(json.dumps(dict(rec, kernel="sc_attention_fwd", ms=round(ms64, 4), tflops=round(flops / ms64 / 1e9, 1))), flush=True)
            print(json.dumps(rec), flush=True)
    T, d = L - 1, 768
    x = torch.randn(B, T, d, generator=g).to(torch.bfloat16).cuda()
    al = (lens - 1).long()
    res = {}
    for n in (1, 2):
        torch.manual_seed(0)
        m = TransformerEncoder(n_layers=n, d_model=d, nhead=8, dim_feedforward=4 * d).eval().cuda()
        cls = torch.randn(1, 1, d).cuda()
        with torch.no_grad():
            res[n] = _time(lambda: m.forward_cls(cls, x, al), a.iters)
        print(json.dumps(dict(item="branch_forward", n_layers=n, B=B, T=T, d=d, ms=round(res[n], 4))), flush=True)
    extra = res[2] - res[1]
    print(json.dumps(dict(item="branch_forward_extra_layer", ms=round(extra, 4))), flush=True)
    # one HuBERT-base encoder layer as HubertModel.extract_all_layers runs it (eval, post-LN, padded rows): the yardstick of the extra layer
    from speechclip_amd.ops import ACT_GELU
    bf, M, H = torch.bfloat16, B * T, 12
    w = lambda n, k: (torch.randn(n, k, generator=g) * k ** -0.5).to(bf).cuda()    # noqa: E731
    z = lambda n: torch.zeros(n, device="cuda")                                     # noqa: E731
    wqkv, wo, w1, w2 = w(3 * d, d), w(d, d), w(4 * d, d), w(d, 4 * d)
    ln = (torch.ones(d, device="cuda"), z(d))
    bqkv, bo, b1, b2 = z(3 * d), z(d), z(4 * d), z(d)
    h = (0.5 * torch.randn(M, d, generator=g)).to(bf).cuda()
    qkv, att, tmp, tmp2, ffn, h_out = (torch.empty(M, n, dtype=bf, device="cuda") for n in (3 * d, d, d, d, 4 * d, d))
    hl = (lens - 1).contiguous()

    def hubert_layer():
        ops.gemm(h, wqkv, bqkv, out=qkv)
        ops.attention(qkv, B, T, H, hl, out=att)
        ops.gemm(att, wo, bo, residual=h, out=tmp)
        ops.layernorm(tmp, *ln, out=tmp2)
        ops.gemm(tmp2, w1, b1, ACT_GELU, out=ffn)
        ops.gemm(ffn, w2, b2, residual=tmp2, out=tmp)
        ops.layernorm(tmp, *ln, out=h_out)
    ms_h = _time(hubert_layer, a.iters)
    print(json.dumps(dict(item="hubert_base_layer", B=B, T=T, ms=round(ms_h, 4))), flush=True)
    print(json.dumps(dict(item="extra_layer_vs_hubert_layer", ratio=round(extra / ms_h, 3), target=1.25)), flush=True)


if __name__ == "__main__":
    main()

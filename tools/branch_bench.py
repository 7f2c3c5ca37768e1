"""Timing of the multi-layer parallel branch (one process, one JSON line per item):
  attention  sc_attention_fwd (head_dim 64) vs sc_attention_hd_fwd (64 / 96 / 128) at B = 256, L = 500: TF/s over 4*B*L^2*d
  branch     forward_cls of TransformerEncoder(n_layers = 1) and (n_layers = 2) at B = 256, T = 499, d = 768 (8 heads), and the difference
  hubert     one HuBERT-base encoder layer (hubert.py's eval post-LN sequence: 12 heads of 64, FFN 3072, bf16 rows) at the same B, T, and the
             ratio (extra branch layer) / (HuBERT-base layer)
Usage: python tools/branch_bench.py [--iters N]"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from speechclip_amd import ops
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

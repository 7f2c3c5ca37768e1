"""Attention backward alone on one GPU: the fused kernel (sc_attention_bwd_packed) beside the image-based chain of train_hubert.attention_bwd
(probabilities kernel + two image transposes + three head transposes + three batched GEMMs), B = 256, H = 12, L = 499.  Prints one JSON line per item:
ms per call (CUDA events, median of `--iters` after warm-up) and the peak memory the call adds above its inputs.
Lengths: full, and the `bench.py --varlen` set.
    python tools/attn_bwd_bench.py [--iters 10] [--B 256]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechclip_amd import ops  # noqa: E402
from speechclip_amd.train_hubert import attention_bwd, attention_bwd_packed  # noqa: E402

BF = torch.bfloat16


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--B", type=int, default=256)
    a = ap.parse_args()
    B, H, T = a.B, 12, 499
    d, Lp = H * 64, 512
    g = torch.Generator().manual_seed(0)
    # the length set of `bench.py --varlen` (make_batch: seed 7122, L_i ~ U{32000 .. 160000} samples) in frames of the conv stack: (L - 400) // 320 + 1
    from bench import make_batch
    ragged = [min(T, (n - 400) // 320 + 1) for n in make_batch(B, 160000, 0, "cpu", True)[1]]
    for name, lens in (("full", [T] * B), ("bench_varlen", ragged)):
        kl = torch.tensor(lens, dtype=torch.int32).cuda()
        # padded layout (both kernels)
        qkv = torch.zeros(B * T + (Lp - T), 3 * d, dtype=BF, device="cuda")
        qkv[:B * T] = torch.randn(B * T, 3 * d, generator=g).to(BF).cuda()
        dO = torch.randn(B * T, d, generator=g).to(BF).cuda()
        att = ops.attention(qkv[:B * T], B, T, H, kl)
        ms, mb = timed(lambda: attention_bwd(qkv, att, dO, B, T, H, kl), a.iters)
        print(json.dumps({"item": "attention_bwd", "kernel": "image chain (sc_attn_bwd_probs + transposes + 3 batched GEMMs)", "layout": "padded", "lens": name,
                          "rows": B * T, "ms": round(ms, 3), "peak_MiB": round(mb, 1)}), flush=True)
        ms, mb = timed(lambda: attention_bwd_packed(qkv[:B * T], att, dO, B, T, H, kl, None), a.iters)
        print(json.dumps({"item": "attention_bwd", "kernel": "sc_attention_bwd_packed", "layout": "padded (row_off = NULL)", "lens": name, "rows": B * T,
                          "ms": round(ms, 3), "peak_MiB": round(mb, 1)}), flush=True)
        if name != "full":      # packed rows: utterance b owns lens[b] + 1 rows
            rows = [n + 1 if n < T else n for n in lens]
            off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
            tot = int(off[-1])
            offd = torch.from_numpy(off).cuda()
            qp = torch.randn(tot, 3 * d, generator=g).to(BF).cuda()
            dOp = torch.randn(tot, d, generator=g).to(BF).cuda()
            attp = ops.attention_packed(qp, B, T, H, kl, offd)
            ms, mb = timed(lambda: attention_bwd_packed(qp, attp, dOp, B, T, H, kl, offd), a.iters)
            print(json.dumps({"item": "attention_bwd", "kernel": "sc_attention_bwd_packed", "layout": "packed", "lens": name, "rows": tot, "ms": round(ms, 3),
                              "peak_MiB": round(mb, 1)}), flush=True)
        del qkv, dO, att
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

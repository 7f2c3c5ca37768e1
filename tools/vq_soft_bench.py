#!/usr/bin/env python
"""A/B of the soft quantizer modes' product keywords = softmax((x + g) / T) @ emb at the cascaded model's sizes (R = B*K = 2048 keyword rows, E = 512,
V = 8112 reduced / 49408 full sub-word table, T = 0.1, Gumbel noise on):

  fused     sc_vq_soft_embed at auto nsplit (pre-pass + MFMA kernel + finish; no [R, V] probability image)
  composed  what the kernels from before the fused one offer: the probabilities materialised (noise added and soft-maxed by torch here, as a caller of those
            kernels would have to), then sc_split_hilo_bf16 + the bf16 MFMA GEMM against [emb^T | emb^T] (train_tail._mfma_f32; V padded to the GEMM's
            multiple of 32 with zero columns)

Interleaved pairs in one process, warmed, device-event times of `--iters` back-to-back calls; per pair: ms, the implied TF/s of the three-term product
(3 * 2 R V E), and the bytes each route has to move (from the shapes).  The routing rule (EXPERIMENTS.md): the fused kernel stays the default only if it is at
least as fast in 3 of 3 pairs at both V.  Usage: python tools/vq_soft_bench.py [--pairs 3] [--iters 20] > profiles/vq_soft_embed_bench.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--vocab", type=int, nargs="*", default=[8112, 49408])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vq_soft_bench: needs the GPU (a CPU run measures nothing)")
    from speechclip_amd import ops
    from speechclip_amd._lib import lib
    from speechclip_amd.train_tail import _dup_k
    R, E, T, seed = args.rows, args.width, 0.1, 20261
    print(f"# device {torch.cuda.get_device_name(0)}; R={R} E={E} T={T} noise on; {args.pairs} interleaved pairs x {args.iters} calls each")
    verdict = []
    for V in args.vocab:
        g = torch.Generator().manual_seed(V)
        x = (torch.randn(R, V, generator=g) * 0.3).clamp_(-1, 1).cuda()
        emb = (torch.randn(V, E, generator=g) * 0.02).cuda()
        Vp = (V + 31) // 32 * 32
        embT2 = _dup_k(torch.nn.functional.pad(emb, (0, 0, 0, Vp - V)).t().contiguous().to(torch.bfloat16))           # [E, 2 Vp]
        noise = ops.vq_gumbel_noise(R, V, seed)
        mask = torch.zeros(V, dtype=torch.bool, device="cuda")
        mask[[0, 2, 3]] = True

        def composed():
            y = torch.softmax(((x + noise) / T).masked_fill(mask, float("-inf")), -1)
            if Vp != V:
                y = torch.nn.functional.pad(y, (0, Vp - V))
            return ops.gemm(ops.split_hilo(y), embT2, out_f32=True)

        def fused():
            return ops.vq_soft_embed(x, emb, T, seed)

        ref = torch.softmax(((x.double() + noise.double()) / T).masked_fill(mask, float("-inf")), -1) @ emb.double()
        for name, fn in (("fused", fused), ("composed", composed)):
            out = fn()
            print(f"# V={V} {name}: |out - fp64| / |fp64| = {((out.double() - ref).norm() / ref.norm()).item():.2e}")
        for _ in range(3):
            fused(), composed()
        flops = 3 * 2.0 * R * V * E
        by_f = R * V * 4 * 3 + 2 * Vp * E * 2 * ((R + 127) // 128) + R * E * 4          # scores read three times (two pre-pass sweeps + main), the (hi, lo) table per row tile
        by_c = R * V * 4 * 2 + R * V * 4 * 4 + R * Vp * (4 + 4) + (R * 2 * Vp * 2 + E * 2 * Vp * 2) + R * E * 4   # add, scale/mask, softmax r/w; split r/w; GEMM operands
        wins = 0
        for p in range(args.pairs):
            tf, tc = timed(fused, args.iters), timed(composed, args.iters)
            wins += tf <= tc
            print(f"V={V} pair {p}: fused {tf:.3f} ms ({flops / tf / 1e9:.1f} TF/s three-term, >= {by_f / 1e6:.0f} MB) | "
                  f"composed {tc:.3f} ms ({flops / tc / 1e9 * 2 / 3:.1f} TF/s two-term, >= {by_c / 1e6:.0f} MB) | fused/composed {tf / tc:.2f}")
        verdict.append(wins == args.pairs)
        auto = lib().sc_vq_soft_embed_workspace_bytes(R, V, E, 0) // (R * E * 4) or 1
        sweep = "  ".join(f"{n}: {timed(lambda n=n: ops.vq_soft_embed(x, emb, T, seed, nsplit=n), args.iters):.3f}" for n in (1, 2, 4, 8, 16, 32))
        print(f"V={V}: fused by nsplit (ms; auto = {auto}, partial products {auto * R * E * 4 / 1e6:.0f} MB written and read back)  {sweep}")
        print(f"V={V}: fused at least as fast in {wins} of {args.pairs} pairs")
    print("ROUTE:", "fused (default kept)" if all(verdict) else "probs + GEMM (fused loses: see EXPERIMENTS.md)")


if __name__ == "__main__":
    main()

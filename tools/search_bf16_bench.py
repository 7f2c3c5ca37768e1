#!/usr/bin/env python
"""Gallery search: bf16 row storage against the fp32 entry of the same library.

Workload (the grid of tools/search_bench.py): unit-norm random rows (seed 7122), E = 512, K = 10, galleries of N = 5 000 / 123 287 / 1 000 000 rows,
Q = 1 / 256 / 1 000 queries.  The bf16 arm searches the same rows rounded to bf16 (round to nearest even), as EmbeddingIndex(storage="bf16") stores them.

Arms, timed after warm-up in three interleaved passes (device events around `iters` back-to-back calls, the order alternating from pass to pass):
  fp32  ops.search_topk       (sc_search_topk: fp32 rows, v_mfma_f32_32x32x2_f32)
  bf16  ops.search_topk_bf16  (sc_search_topk_bf16: bf16 rows, v_mfma_f32_32x32x16_bf16)

Every (N, Q) pair runs in a child process of its own under a time limit; the first child that fails ends the run.  Reported per pair: ms per pass and the
medians, each arm's gallery bytes per second (N E element-size bytes per call: what one pass over the gallery reads) and TF/s (2 Q N E flop), in how many
passes bf16 was faster, and how many of the fp32 top-10 positions are in the bf16 top-10 (mean over the queries).  No ratio is asked of this file: bf16
storage is opt-in, and the table states what was measured, whichever way it fell.

Usage: python tools/search_bf16_bench.py [--passes 3] [--out profiles/search_bf16_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from search_bench import CHILD_LIMIT_S, E, GALLERIES, K, QUERIES, timed, unit_rows  # noqa: E402  (the fp32 tool beside this file: the same grid, rows and clock)


def one(N, Q, passes):
    import torch
    from speechclip_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7122)
    g, q = unit_rows(N, gen), unit_rows(Q, gen)
    g16, q16 = g.to(torch.bfloat16), q.to(torch.bfloat16)

    def fp32():
        return ops.search_topk(q, g, K)

    def bf16():
        return ops.search_topk_bf16(q16, g16, K)

    (_, fi), (_, bi) = fp32(), bf16()
    kept = (fi[:, :, None] == bi[:, None, :]).any(2).sum(1).float().mean().item()
    iters = 20 if Q * N <= 10 ** 8 else 3
    for _ in range(2):
        fp32(), bf16()
    arms, times = (fp32, bf16), ([], [])
    for r in range(passes):
        for i in range(2):
            a = (i + r) % 2
            times[a].append(timed(arms[a], iters))
        print(f"N {N:>7} Q {Q:>4} pass {r}: fp32 {times[0][-1]:9.3f} ms | bf16 {times[1][-1]:9.3f} ms | fp32 / bf16 {times[0][-1] / times[1][-1]:6.2f}", flush=True)
    mf, mb = statistics.median(times[0]), statistics.median(times[1])
    wins = sum(b < f for f, b in zip(*times))
    flop = 2.0 * Q * N * E
    print(f"N {N:>7} Q {Q:>4} median: fp32 {mf:9.3f} ms | bf16 {mb:9.3f} ms | fp32 / bf16 {mf / mb:6.2f} | gallery bytes: fp32 {4.0 * N * E / mf / 1e6:7.1f} GB/s, "
          f"bf16 {2.0 * N * E / mb / 1e6:7.1f} GB/s | fp32 {flop / mf / 1e9:6.2f} TF/s, bf16 {flop / mb / 1e9:7.2f} TF/s | splits {ops.lib().sc_search_splits(Q, N, K)}, "
          f"{iters} calls per pass | bf16 faster in {wins} of {passes} passes | fp32 top-{K} positions in the bf16 top-{K}: {kept:.2f} of {K}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bf16_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "Q"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_bf16_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], args.one[1], args.passes)
    lines = [f"# unit-norm random rows (seed 7122), E = {E}, K = {K}; {args.passes} interleaved passes, device-event time per call in ms",
             "# fp32 = ops.search_topk on fp32 rows; bf16 = ops.search_topk_bf16 on the same rows rounded to bf16; one child process per (N, Q)"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for N in GALLERIES:
        for Q in QUERIES:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", str(N), str(Q), "--passes", str(args.passes)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            out = [ln for ln in p.stdout.splitlines() if ln.startswith("N ")]
            print("\n".join(out), flush=True)
            lines += out
            if p.returncode != 0:                  # a fault, an abort or the time limit: nothing more is started on the GPU
                print(p.stdout[-2000:], flush=True)
                lines.append(f"N {N} Q {Q}: child ended with status {p.returncode}; run stopped")
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
                sys.exit(1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

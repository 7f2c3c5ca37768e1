#!/usr/bin/env python
"""Gallery search: the two-stage search (bf16 shortlist, fp32 re-score, certificate, fp32 fallback) against the fp32 and the bf16 search of the same index.

Workload: E = 512, K = 10, galleries of N = 123 287 / 1 000 000 rows in ONE segment, Q = 1 / 256 / 1 000 queries, seed 7122, on two kinds of rows:
  random    unit-norm random rows and queries (the grid of tools/search_bench.py)
  captions  five rows per item, row = unit(item + 0.3 noise) with unit item and unit noise (the five-captions shape); a query is one more such row of a
            random item

Arms, all through EmbeddingIndex.search (so every arm pays the same host side: the ids of the result are read back), timed after warm-up in three
interleaved passes (device events around `iters` back-to-back calls, the order rotating from pass to pass):
  fp32       index.search(q, K) on fp32 rows                       (sc_search_topk)
  bf16       the same rows rounded to bf16, index16.search(q, K)   (sc_search_topk_bf16: NOT the fp32 result)
  rerank R   index.search(q, K, rerank=R), R = 32 / 64 / 128       (sc_search_topk_bf16 with K = R, sc_search_rescore, sc_search_topk for the uncertified)

Every (rows, N, Q) cell runs in a child process of its own under a time limit; the first child that fails ends the run.  Reported per cell: the medians in
ms, each rerank arm's certified share of the queries, and that every rerank arm returned the fp32 arm's scores and positions bit for bit.  No ratio is asked
of this file: rerank is opt-in, and the table states what was measured, whichever way it fell.

Usage: python tools/search_rerank_bench.py [--passes 3] [--out profiles/search_rerank_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from search_bench import E, K, timed, unit_rows  # noqa: E402  (the fp32 tool beside this file: the same rows and clock)

GALLERIES, QUERIES, RERANKS, KINDS = (123287, 1000000), (1, 256, 1000), (32, 64, 128), ("random", "captions")
CHILD_LIMIT_S = 200


def rows_of(kind, N, Q, gen):
    import torch
    from speechclip_amd import ops
    if kind == "random":
        return unit_rows(N, gen), unit_rows(Q, gen)
    items = (N + 4) // 5
    centre = unit_rows(items, gen)
    g = ops.l2norm(centre.repeat_interleave(5, 0)[:N] + 0.3 * unit_rows(N, gen))
    pick = torch.randint(items, (Q,), device="cuda", generator=gen)
    return g, ops.l2norm(centre[pick] + 0.3 * unit_rows(Q, gen))


def one(kind, N, Q, passes):
    import torch
    from speechclip_amd.module import EmbeddingIndex
    gen = torch.Generator(device="cuda").manual_seed(7122)
    g, q = rows_of(kind, N, Q, gen)
    index = EmbeddingIndex(E, shadow=True).add(g)
    index16 = EmbeddingIndex(E, storage="bf16")                # the bf16 arm searches the shadow rows themselves: exactly what astype("bf16") holds
    index16.segments, index16._n = list(index.shadow_segments), len(index)
    del g
    arms = [("fp32", lambda: index.search(q, K)), ("bf16", lambda: index16.search(q, K))]
    arms += [(f"rerank {R}", (lambda R: lambda: index.search(q, K, rerank=R))(R)) for R in RERANKS]
    want = index.search(q, K)
    share, exact = {}, True
    for R in RERANKS:
        s, p, _, c = index.search(q, K, rerank=R, return_certified=True)
        share[R] = c.float().mean().item()
        exact = exact and torch.equal(s.view(torch.int32), want[0].view(torch.int32)) and torch.equal(p, want[1])
    kept = (want[1][:, :, None] == index16.search(q, K)[1][:, None, :]).any(2).sum(1).float().mean().item()
    iters = 20 if Q * N <= 10 ** 8 else 3
    for _, fn in arms:
        fn(), fn()
    times = [[] for _ in arms]
    for r in range(passes):
        for i in range(len(arms)):
            a = (i + r) % len(arms)
            times[a].append(timed(arms[a][1], iters))
    med = [statistics.median(t) for t in times]
    cells = " | ".join(f"{name} {m:8.3f} ms" for (name, _), m in zip(arms, med))
    shares = ", ".join(f"R={R}: {share[R]:.3f}" for R in RERANKS)
    ratio = ", ".join(f"R={R}: {med[0] / med[2 + n]:.2f}" for n, R in enumerate(RERANKS))
    print(f"{kind:>8} N {N:>7} Q {Q:>4} median of {passes}: {cells} | fp32 / rerank {ratio} | fp32 / bf16 {med[0] / med[1]:.2f} | certified share {shares} | "
          f"rerank == fp32 bit for bit: {exact} | fp32 top-{K} positions in the bf16 top-{K}: {kept:.2f} | {iters} calls per pass", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_rerank_bench.txt"))
    ap.add_argument("--one", nargs=3, metavar=("KIND", "N", "Q"), help="(internal) time one cell in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_rerank_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], int(args.one[1]), int(args.one[2]), args.passes)
    lines = [f"# E = {E}, K = {K}, one segment, seed 7122; medians of {args.passes} interleaved passes, device-event time per EmbeddingIndex.search call in ms",
             "# fp32 = index.search; bf16 = the same rows rounded to bf16; rerank R = index.search(..., rerank=R); one child process per cell"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for kind in KINDS:
        for N in GALLERIES:
            for Q in QUERIES:
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", kind, str(N), str(Q), "--passes",
                                    str(args.passes)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                out = [ln for ln in p.stdout.splitlines() if ln.lstrip().startswith(kind)]
                print("\n".join(out), flush=True)
                lines += out
                if p.returncode != 0:              # a fault, an abort or the time limit: nothing more is started on the GPU
                    print(p.stdout[-2000:], flush=True)
                    lines.append(f"{kind} N {N} Q {Q}: child ended with status {p.returncode}; run stopped")
                    with open(args.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
                    sys.exit(1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

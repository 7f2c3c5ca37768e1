#!/usr/bin/env python
"""Gallery search: the fused similarity + top-K entry against the dense path it replaces.

Workload: unit-norm random rows (seed 7122), E = 512, K = 10, galleries of N = 5 000 / 123 287 / 1 000 000 rows, Q = 1 / 256 / 1 000 queries.

Arms, timed after warm-up in three interleaved passes (device events around `iters` back-to-back calls, the order alternating from pass to pass):
  fused  ops.search_topk (sc_search_topk: fp32-input MFMA scores kept in accumulators, per-row candidate lists in LDS, no [Q, N] image)
  dense  ops.sgemm(q, g, transb=True) + ops.topk_rows, in query chunks that keep the score image at or below 1 GiB: the only path before the fused entry

Every (N, Q) pair runs in a child process of its own under a time limit; the first child that fails ends the run.  Reported per pair: ms per pass and the
medians, the fused arm's TF/s (2 Q N E flop) against the 157 TF/s fp32 matrix peak, for Q = 1 the gallery traffic in GB/s (4 N E bytes), and whether the
two arms return the same positions.  Rule this file settles: the fused arm is faster than the dense arm in 3 of 3 passes at N = 123 287 and N = 10^6 for
Q = 256 (no margin beyond the sign is asked for).

Usage: python tools/search_bench.py [--passes 3] [--out profiles/search_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E, K = 512, 10
GALLERIES, QUERIES = (5000, 123287, 1000000), (1, 256, 1000)
CHILD_LIMIT_S = 150


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def unit_rows(n, gen):
    import torch
    from speechclip_amd import ops
    out = torch.empty(n, E, device="cuda")
    for at in range(0, n, 65536):
        rows = min(65536, n - at)
        out[at:at + rows] = ops.l2norm(torch.randn(rows, E, device="cuda", generator=gen))
    return out


def one(N, Q, passes):
    import torch
    from speechclip_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7122)
    g, q = unit_rows(N, gen), unit_rows(Q, gen)
    chunk = max(1, min(Q, (1 << 30) // (4 * N)))

    def fused():
        return ops.search_topk(q, g, K)

    def dense():
        parts = [ops.topk_rows(ops.sgemm(q[at:at + chunk], g, transb=True), K) for at in range(0, Q, chunk)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    (fv, fi), (dv, di) = fused(), dense()
    same = f"positions equal on {(fi == di).all(1).float().mean().item() * 100:.1f} % of the queries, values bitwise equal: {bool(torch.equal(fv, dv))}"
    iters = 20 if Q * N <= 10 ** 8 else 3
    for _ in range(2):
        fused(), dense()
    arms, times = (fused, dense), ([], [])
    for r in range(passes):
        for i in range(2):
            a = (i + r) % 2
            times[a].append(timed(arms[a], iters))
        print(f"N {N:>7} Q {Q:>4} pass {r}: fused {times[0][-1]:9.3f} ms | dense {times[1][-1]:9.3f} ms | dense / fused {times[1][-1] / times[0][-1]:6.2f}", flush=True)
    mf, md = statistics.median(times[0]), statistics.median(times[1])
    wins = sum(f < d for f, d in zip(*times))
    extra = f" | gallery read at {4.0 * N * E / mf / 1e6:7.1f} GB/s" if Q == 1 else ""
    print(f"N {N:>7} Q {Q:>4} median: fused {mf:9.3f} ms | dense {md:9.3f} ms | dense / fused {md / mf:6.2f} | fused {2.0 * Q * N * E / mf / 1e9:6.2f} TF/s = "
          f"{2.0 * Q * N * E / mf / 1e9 / 157.0 * 100:4.1f} % of 157{extra} | splits {ops.lib().sc_search_splits(Q, N, K)}, dense chunk {chunk} queries, "
          f"{iters} calls per pass | fused faster in {wins} of {passes} passes | {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "Q"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], args.one[1], args.passes)
    lines = [f"# unit-norm random rows (seed 7122), E = {E}, K = {K}; {args.passes} interleaved passes, device-event time per call in ms",
             "# fused = ops.search_topk; dense = ops.sgemm + ops.topk_rows in query chunks with a score image <= 1 GiB; one child process per (N, Q)"]
    print("\n".join(lines), flush=True)
    verdict = {}
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
            if Q == 256 and N > 5000:
                verdict[N] = f"faster in {args.passes} of {args.passes}" in out[-1]
    ok = all(verdict.values()) and len(verdict) == 2
    lines.append(f"verdict: fused faster than dense in every pass at Q = 256 for N = 123 287 and N = 1 000 000: {ok}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

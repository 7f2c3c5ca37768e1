#!/usr/bin/env python
"""Gallery search by threshold: what the two-pass entry costs, against the dense path it replaces and against one top-K scan.

Workload: unit-norm random rows (seed 7122), E = 512, galleries of N = 5 000 / 123 287 / 1 000 000 rows, Q = 1 / 256 / 1 000 queries.  Every query has a
threshold of its own: its 10th-largest and its 100th-largest score, as ops.search_topk returns them (so a query has 10 or 100 hits on fp32 rows, and about
as many on the rows rounded to bf16).

Arms, timed after warm-up in three interleaved passes (device events around `iters` back-to-back calls, the order rotating from pass to pass):
  range@10, range@100   ops.search_range (count pass, cumsum, one read of the total, fill pass) at the two thresholds
  bf16@10, bf16@100     ops.search_range_bf16 on the same rows rounded to bf16, same thresholds
  dense@10              ops.sgemm(q, g, transb=True), comparison with the thresholds, nonzero and a gather of the scores -- wherever the [Q, N] fp32 score
                        image fits in 1 GiB; the only path before this entry
  topk                  ops.search_topk at K = 10: the floor of ONE scan of the gallery.  The two-pass design should cost about two: the ratio is recorded,
                        nothing is asserted on it.

Every (N, Q) pair runs in a child process of its own under a time limit; the first child that fails ends the run.  Nothing in the product is chosen on the
strength of these numbers: search_range is a call of its own, and no existing path routes to it.

Usage: python tools/search_range_bench.py [--passes 3] [--out profiles/search_range_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E, K = 512, 10
GALLERIES, QUERIES = (5000, 123287, 1000000), (1, 256, 1000)
DENSE_LIMIT = 1 << 30
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
    gb, qb = g.to(torch.bfloat16), q.to(torch.bfloat16)
    top = ops.search_topk(q, g, 100)[0]
    t10, t100 = top[:, 9].contiguous(), top[:, 99].contiguous()
    has_dense = 4 * Q * N <= DENSE_LIMIT

    def dense():
        s = ops.sgemm(q, g, transb=True)
        at = (s >= t10[:, None]).nonzero()
        return at, s[at[:, 0], at[:, 1]]

    arms = [("range@10", lambda: ops.search_range(q, g, t10)), ("range@100", lambda: ops.search_range(q, g, t100)),
            ("bf16@10", lambda: ops.search_range_bf16(qb, gb, t10)), ("bf16@100", lambda: ops.search_range_bf16(qb, gb, t100)),
            ("topk", lambda: ops.search_topk(q, g, K))]
    if has_dense:
        arms.append(("dense@10", dense))
    lims, vals, idx = ops.search_range(q, g, t10)
    hits = {"range@10": int(lims[-1]), "range@100": int(ops.search_range(q, g, t100)[0][-1]), "bf16@10": int(ops.search_range_bf16(qb, gb, t10)[0][-1]),
            "bf16@100": int(ops.search_range_bf16(qb, gb, t100)[0][-1])}
    same = "n/a"
    if has_dense:
        at, dv = dense()                                                          # row-major nonzero: ascending query, then ascending row -- the entry's order
        same = str(bool(torch.equal(at[:, 1], idx) and torch.equal(torch.bincount(at[:, 0], minlength=Q).cumsum(0), lims[1:])))
    iters = 20 if Q * N <= 10 ** 8 else 3
    for _ in range(2):
        for _, fn in arms:
            fn()
    times = {name: [] for name, _ in arms}
    for r in range(passes):
        for i in range(len(arms)):
            name, fn = arms[(i + r) % len(arms)]
            times[name].append(timed(fn, iters))
        print(f"N {N:>7} Q {Q:>4} pass {r}: " + " | ".join(f"{name} {times[name][-1]:9.3f} ms" for name, _ in arms), flush=True)
    med = {name: statistics.median(v) for name, v in times.items()}
    dense_txt = f"dense@10 {med['dense@10']:9.3f} ms | dense / range@10 {med['dense@10'] / med['range@10']:6.2f}" if has_dense else "dense@10       n/a (score image above 1 GiB)"
    print(f"N {N:>7} Q {Q:>4} median: " + " | ".join(f"{name} {med[name]:9.3f} ms" for name in ("range@10", "range@100", "bf16@10", "bf16@100", "topk")) +
          f" | {dense_txt} | range@10 / topk {med['range@10'] / med['topk']:5.2f} | bf16@10 / range@10 {med['bf16@10'] / med['range@10']:5.2f} | hits "
          f"{hits['range@10']} / {hits['range@100']} / {hits['bf16@10']} / {hits['bf16@100']} | splits {ops.lib().sc_search_splits(Q, N, 1)}, {iters} calls per pass | "
          f"same hits as dense: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_range_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "Q"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_range_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], args.one[1], args.passes)
    lines = [f"# unit-norm random rows (seed 7122), E = {E}; thresholds per query at its 10th / 100th largest score (ops.search_topk); {args.passes} interleaved "
             "passes, device-event time per call in ms",
             "# range = ops.search_range, bf16 = ops.search_range_bf16 (count pass + cumsum + one read of the total + fill pass); dense = ops.sgemm + comparison + "
             f"nonzero + gather where the score image is <= 1 GiB; topk = ops.search_topk at K = {K} (one scan); one child process per (N, Q)"]
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

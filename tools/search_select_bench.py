#!/usr/bin/env python
"""Gallery search inside a subset: what the row mask costs when nothing can be skipped, what tile skipping buys when the subset is contiguous, and how both
compare with what a user could do before -- gather the allowed rows into a new tensor and search that.  Same library, same box, same run.

Workload: E = 512, K = 10, unit-norm galleries of N = 123 287 / 1 000 000 rows (one item code per row), Q = 1 / 256 unit-norm queries, seed 7122; both
storages, the bf16 arms on the same rows rounded to bf16.

Arms per storage, timed after warm-up in three interleaved passes (device events around `iters` back-to-back calls, the starting arm rotating from pass to
pass):
  items        ops.search_items[_bf16] on the whole gallery                                   (the scan every other arm is compared with)
  ones         ops.search_select[_bf16], all rows allowed                                     (the predicate's overhead: same result as `items`)
  block 10 %   ops.search_select[_bf16], one contiguous block of N / 10 rows allowed          (what tile skipping buys)
  block 1 %    the same with N / 100 rows
  view 10 % / 1 %      ops.search_items[_bf16] on the slice g[start : start + n] with idx_base = start: what a contiguous block costs without any mask, no copy
  random 10 %  ops.search_select[_bf16], N / 10 rows allowed, uniformly random: every tile is live  (the predicate's cost when nothing can be skipped)
  random 1 %   the same with N / 100 rows
  gather+ 10 % / 1 %   index_select of the random rows into a new tensor, then ops.search_items[_bf16] on it  (the comparator, gather included)
  gather  10 % / 1 %   ops.search_items[_bf16] on the rows gathered beforehand                 (the comparator for a subset reused across many calls)
The block starts at row 0.37 N, aligned to nothing.  Before anything is timed, `ones` is checked against `items`, every block arm against its view and every
random arm against the gathered search, bit for bit (fp32) or by the rows returned being allowed (bf16).

Every (N, Q) pair runs in a child process of its own under a time limit, on at most 16 CPU threads; the first child that fails ends the run.  Reported per
pair and storage: ms per pass, the medians, and each arm's ratio to `items`.  There is no threshold.

Usage: python tools/search_select_bench.py [--passes 3] [--out profiles/search_select_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from search_bench import CHILD_LIMIT_S, E, K, timed, unit_rows  # noqa: E402  (the fp32 tool beside this file: the same rows and clock)

GALLERIES = (123287, 1000000)
QUERIES = (1, 256)
FRACTIONS = ((10, "10 %"), (100, "1 %"))


def one(N, Q, passes):
    import torch
    from speechclip_amd import ops
    torch.set_num_threads(min(16, torch.get_num_threads()))
    gen = torch.Generator(device="cuda").manual_seed(7122)
    g, q = unit_rows(N, gen), unit_rows(Q, gen)
    items = torch.arange(N, device="cuda", dtype=torch.int32)
    ones = ops.pack_row_mask(torch.ones(N, dtype=torch.bool, device="cuda"))
    subsets = {}
    for div, label in FRACTIONS:
        n = N // div
        block = torch.zeros(N, dtype=torch.bool, device="cuda")
        start = int(0.37 * N)
        block[start:start + n] = True
        rows = torch.randperm(N, device="cuda", generator=gen)[:n].sort().values
        rnd = torch.zeros(N, dtype=torch.bool, device="cuda")
        rnd[rows] = True
        subsets[label] = dict(block=ops.pack_row_mask(block), start=start, n=n, random=ops.pack_row_mask(rnd), rows=rows, codes=items[rows].contiguous())
    arms = []
    for st in ("fp32", "bf16"):
        qq, gg = (q, g) if st == "fp32" else (q.to(torch.bfloat16), g.to(torch.bfloat16))
        by_item, select = (ops.search_items, ops.search_select) if st == "fp32" else (ops.search_items_bf16, ops.search_select_bf16)
        whole = lambda qq=qq, gg=gg, f=by_item: f(qq, gg, K, items)
        all_ones = lambda qq=qq, gg=gg, f=select: f(qq, gg, K, items, allow=ones)
        assert all(torch.equal(x, y) for x, y in zip(whole(), all_ones())), st
        arms += [(st, "items", whole), (st, "ones", all_ones)]
        for label, s in subsets.items():
            gathered = gg.index_select(0, s["rows"])
            lo, hi = s["start"], s["start"] + s["n"]
            block = lambda qq=qq, gg=gg, f=select, s=s: f(qq, gg, K, items, allow=s["block"])
            view = lambda qq=qq, gg=gg, f=by_item, lo=lo, hi=hi: f(qq, gg[lo:hi], K, items[lo:hi], idx_base=lo)
            rnd = lambda qq=qq, gg=gg, f=select, s=s: f(qq, gg, K, items, allow=s["random"])
            gather_in = lambda qq=qq, gg=gg, f=by_item, s=s: f(qq, gg.index_select(0, s["rows"]), K, s["codes"])
            gather_out = lambda qq=qq, gathered=gathered, f=by_item, s=s: f(qq, gathered, K, s["codes"])
            # what is timed is what was asked for: the block against the view, the random rows against the gathered search
            got_b, want_b, got_r, want_r = block(), view(), rnd(), gather_out()
            assert (got_b[1] >= lo).all() and (got_b[1] < hi).all() and torch.isin(got_r[1], s["rows"]).all(), (st, label)
            if st == "fp32":
                assert torch.equal(got_b[0], want_b[0]) and torch.equal(got_b[1], want_b[1]), (st, label, "block")
                assert torch.equal(got_r[0], want_r[0]) and torch.equal(got_r[1], s["rows"][want_r[1]]), (st, label, "random")
            arms += [(st, f"block {label}", block), (st, f"view {label}", view), (st, f"random {label}", rnd), (st, f"gather+ {label}", gather_in),
                     (st, f"gather {label}", gather_out)]
    iters = 20 if Q * N <= 10 ** 8 else 5
    for _ in range(2):
        for _, _, fn in arms:
            fn()
    times = [[] for _ in arms]
    for r in range(passes):
        for i in range(len(arms)):
            a = (i + r) % len(arms)
            times[a].append(timed(arms[a][2], iters))
        print(f"N {N:>7} Q {Q:>4} pass {r}: " + " | ".join(f"{st} {name} {t[-1]:7.3f}" for (st, name, _), t in zip(arms, times)) + " ms", flush=True)
    med = [statistics.median(t) for t in times]
    spread = [max(t) - min(t) for t in times]
    per = len(arms) // 2
    for s, st in enumerate(("fp32", "bf16")):
        m, base = med[per * s:per * s + per], med[per * s]
        print(f"N {N:>7} Q {Q:>4} median {st}: " + " | ".join(f"{name} {t:7.3f} ms ({t / base:5.2f} x)" for (_, name, _), t in zip(arms[per * s:], m))
              + f" | largest pass-to-pass spread of an arm {max(spread[per * s:per * s + per]):.3f} ms, splits {ops.lib().sc_search_splits(Q, N, K)}, {iters} calls per pass",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_select_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "Q"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_select_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], args.one[1], args.passes)
    lines = [f"# E = {E}, K = {K}, unit-norm rows and queries (seed 7122), one item code per row; {args.passes} interleaved passes, device-event time per call in ms;",
             "# (r x) = the arm's median over the median of `items` = ops.search_items[_bf16] on the whole gallery.  ones / block / random = ops.search_select[_bf16] with",
             "# all rows, one contiguous block, or uniformly random rows allowed; view = ops.search_items[_bf16] on the block's slice of g (no mask, no copy);",
             "# gather+ / gather = index_select of the random rows + ops.search_items[_bf16] on them, with / without the gather in the timed region; one child",
             "# process per (N, Q)"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))))
    for N in GALLERIES:
        for Q in QUERIES:
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", str(N), str(Q), "--passes", str(args.passes)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
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

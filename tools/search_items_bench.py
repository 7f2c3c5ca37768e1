#!/usr/bin/env python
"""Gallery search by item: what the id-aware selection costs over the plain entry of the same library, same box, same run.

Workload: E = 512, K = 10, galleries of N = 123 287 / 1 000 000 rows with FIVE ROWS PER ITEM (row = unit-norm item centre + 0.5 unit-norm noise,
normalised: the five rows of an item are neighbours, so a query near an item meets all five -- the case `distinct` is for), Q = 1 / 256 / 1 000 queries,
each near one item (centre + noise) which is also its skip code: the hard-negative query of INTEGRATION.md.  Seed 7122; both storages, the bf16 arms on
the same rows rounded to bf16.

Arms per storage, timed after warm-up in three interleaved passes (device events around `iters` back-to-back calls, the starting arm rotating from pass to
pass):
  plain     ops.search_topk[_bf16]                                   (sc_search_topk[_bf16])
  items0    ops.search_items[_bf16], distinct=False, q_skip=None     (the same result through the id-aware kernel: identity 1 of the header)
  items1    ops.search_items[_bf16], distinct=True, q_skip=own item  (K nearest other items)

Every (N, Q) pair runs in a child process of its own under a time limit; the first child that fails ends the run.  Reported per pair and storage: ms per
pass, the medians and the two ratios to the plain arm.  There is no threshold: the plain Python path still calls the plain entries, and the table states
what the id-aware selection costs, whichever way it fell.

Usage: python tools/search_items_bench.py [--passes 3] [--out profiles/search_items_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from search_bench import CHILD_LIMIT_S, E, K, timed, unit_rows  # noqa: E402  (the fp32 tool beside this file: the same rows and clock)

GALLERIES = (123287, 1000000)
QUERIES = (1, 256, 1000)
PER_ITEM = 5


def near(centres, gen):
    """Unit-norm rows around the given unit-norm centres, in chunks (a 10^6-row gallery is 2 GB)."""
    import torch
    from speechclip_amd import ops
    out = torch.empty_like(centres)
    for at in range(0, centres.shape[0], 65536):
        c = centres[at:at + 65536]
        out[at:at + 65536] = ops.l2norm(c + 0.5 * ops.l2norm(torch.randn(c.shape, device="cuda", generator=gen)))
    return out


def one(N, Q, passes):
    import torch
    from speechclip_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7122)
    n_items = -(-N // PER_ITEM)
    centres = unit_rows(n_items, gen)
    items = (torch.arange(N, device="cuda") // PER_ITEM).to(torch.int32)
    g = near(centres[items.long()], gen)
    own = torch.randint(0, n_items, (Q,), device="cuda", generator=gen)
    q = near(centres[own], gen)
    skip = own.to(torch.int32)
    del centres
    rows = {"fp32": (q, g), "bf16": (q.to(torch.bfloat16), g.to(torch.bfloat16))}
    entries = {"fp32": (ops.search_topk, ops.search_items), "bf16": (ops.search_topk_bf16, ops.search_items_bf16)}
    arms = []
    for st in ("fp32", "bf16"):
        (qq, gg), (plain, by_item) = rows[st], entries[st]
        arms += [(st, "plain", lambda qq=qq, gg=gg, plain=plain: plain(qq, gg, K)),
                 (st, "items0", lambda qq=qq, gg=gg, by_item=by_item: by_item(qq, gg, K, items)),
                 (st, "items1", lambda qq=qq, gg=gg, by_item=by_item: by_item(qq, gg, K, items, q_skip=skip, distinct=True))]
    # what is timed is what was asked for: identity 1, and a distinct result without the own item
    for st in ("fp32", "bf16"):
        p, a, b = (fn() for s, _, fn in arms if s == st)
        assert torch.equal(p[0], a[0]) and torch.equal(p[1], a[1])
        assert not (b[2] == skip[:, None]).any() and (b[2].sort(1).values.diff(dim=1) != 0).all() and (b[1] >= 0).all()
    own_rows = (p[1] // PER_ITEM == own[:, None]).sum(1).float().mean().item()
    iters = 20 if Q * N <= 10 ** 8 else 3
    for _ in range(2):
        for _, _, fn in arms:
            fn()
    times = [[] for _ in arms]
    for r in range(passes):
        for i in range(len(arms)):
            a = (i + r) % len(arms)
            times[a].append(timed(arms[a][2], iters))
        print(f"N {N:>7} Q {Q:>4} pass {r}: " + " | ".join(f"{st} {name} {t[-1]:8.3f}" for (st, name, _), t in zip(arms, times)) + " ms", flush=True)
    med = [statistics.median(t) for t in times]
    for s, st in enumerate(("fp32", "bf16")):
        p, a, b = med[3 * s:3 * s + 3]
        print(f"N {N:>7} Q {Q:>4} median {st}: plain {p:8.3f} ms | items, distinct=0, no skip {a:8.3f} ms ({a / p:5.2f} x plain) | items, distinct=1, skip {b:8.3f} ms "
              f"({b / p:5.2f} x plain) | splits {ops.lib().sc_search_splits(Q, N, K)}, {iters} calls per pass"
              + (f" | rows of the query's own item in the plain top-{K}: {own_rows:.2f}" if s else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_items_bench.txt"))
    ap.add_argument("--one", type=int, nargs=2, metavar=("N", "Q"), help="(internal) time one pair in this process")
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            sys.exit("search_items_bench: needs the GPU (a CPU run measures nothing)")
        return one(args.one[0], args.one[1], args.passes)
    lines = [f"# E = {E}, K = {K}, {PER_ITEM} rows per item (item centre + 0.5 noise, unit norm), queries near one item each (seed 7122); {args.passes} interleaved passes,",
             "# device-event time per call in ms.  plain = ops.search_topk[_bf16]; items = ops.search_items[_bf16] (distinct=0 without a skip returns the plain result;",
             "# distinct=1 with the query's own item as its skip code: the K nearest other items); one child process per (N, Q)"]
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

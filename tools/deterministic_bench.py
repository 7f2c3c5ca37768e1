#!/usr/bin/env python
"""Times the three order-dependent reductions of the training tail in their default (atomic) and deterministic (fixed-order) forms at the shapes of the P-base
step (B = 256 pairs, T = 499 frames, D = 768, 8 heads, 13 hidden states), through the C ABI.

    python tools/deterministic_bench.py [--out profiles/deterministic_kernels_bench.txt] [--iters 40] [--B 256] [--T 499]

Per shape the two forms alternate call by call on one stream; every call is bracketed by HIP events; the table gives the median and the 10th / 90th percentile
of the per-call times after a warm-up.  Workspaces are allocated once outside the timed region (the step allocates them from torch's caching allocator)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, iters, warmup=5):
    """fns: {name: callable}; alternates them; -> {name: [ms]}"""
    out = {k: [] for k in fns}
    for i in range(warmup + iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                out[k].append(e0.elapsed_time(e1))
    return out


def row(tag, t):
    def q(v, f):
        v = sorted(v)
        return v[min(len(v) - 1, int(f * len(v)))]
    a, d = t["default"], t["det"]
    ma, md = statistics.median(a), statistics.median(d)
    return (f"{tag:58s} default {ma * 1e3:8.1f} us [{q(a, .1) * 1e3:7.1f} .. {q(a, .9) * 1e3:7.1f}]   deterministic {md * 1e3:8.1f} us "
            f"[{q(d, .1) * 1e3:7.1f} .. {q(d, .9) * 1e3:7.1f}]   ratio {md / ma:5.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deterministic_kernels_bench.txt"))
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--T", type=int, default=499)
    a = ap.parse_args()
    from speechclip_amd import ops
    from speechclip_amd._lib import check, lib, ptr, stream
    L, dev = lib(), torch.device("cuda")
    B, T, D, H, NQ, n = a.B, a.T, 768, 8, 1, 13
    R = NQ * H
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)          # noqa: E731
    lines = [f"deterministic_bench: B={B} T={T} D={D} heads={H} hidden states={n}; {a.iters} alternating calls per form after 5 warm-up calls; "
             f"device {torch.cuda.get_device_name(0)}", ""]

    # ---- split-K sgemm: the branch's feed-forward products with K = 4 D = 3072 (linear2 forward: transb; the gradient through linear1: beta = 1)
    for tag, tb, beta, bias in (("sgemm linear2 fwd   [B,4D] x [D,4D]^T + bias", True, 0.0, True), ("sgemm d linear1    [B,4D] x [4D,D], beta=1", False, 1.0, False)):
        M, N, K = B, D, 4 * D
        A, Bm = rnd(M, K), (rnd(N, K) if tb else rnd(K, N))
        C, bv = rnd(M, N), (rnd(N) if bias else None)
        slices = L.sc_sgemm_det_slices(M, N, K, 1)
        nb = L.sc_sgemm_det_workspace_bytes(M, N, K, 1)
        ws = torch.empty(nb // 4, device=dev)
        f0 = lambda: check(L.sc_sgemm(0, int(tb), M, N, K, 1.0, ptr(A), K, ptr(Bm), Bm.stride(0), beta, ptr(C), N, ptr(bv), stream()), "sc_sgemm")          # noqa: E731
        f1 = lambda: check(L.sc_sgemm_det(0, int(tb), M, N, K, 1.0, ptr(A), K, ptr(Bm), Bm.stride(0), beta, ptr(C), N, ptr(bv), ptr(ws), nb, stream()), "sc_sgemm_det")          # noqa: E731
        if beta:
            C.mul_(0)          # beta = 1 accumulates call after call: start from 0 and keep the operands small
            A.mul_(1e-3)
        lines.append(row(f"{tag} ({slices} slices)", timed({"default": f0, "det": f1}, a.iters)))

    # ---- chunked colsum: the head's partial rows [B * nsplit, R * D] and a bias gradient [B, D]
    nsplit = max(1, min(16, 512 // B))
    for tag, rows, cols in ((f"colsum du partial rows [{B * nsplit}, {R * D}]", B * nsplit, R * D), (f"colsum bias gradient   [{B}, {D}]", B, D)):
        x, out = rnd(rows, cols), torch.empty(cols, device=dev)
        chunks = L.sc_colsum_det_chunks(rows, cols)
        nb = L.sc_colsum_det_workspace_bytes(rows, cols)
        ws = torch.empty(nb // 4, device=dev)
        f0 = lambda: check(L.sc_colsum(ptr(x), cols, rows, cols, ptr(out), 0, stream()), "sc_colsum")          # noqa: E731
        f1 = lambda: check(L.sc_colsum_det(ptr(x), cols, rows, cols, ptr(out), 0, ptr(ws), nb, stream()), "sc_colsum_det")          # noqa: E731
        lines.append(row(f"{tag} ({chunks} chunks)", timed({"default": f0, "det": f1}, a.iters)))

    # ---- pooling backward: both passes (the scores pass is shared by the two forms)
    x_rows = rnd(B * T, D).to(torch.bfloat16)
    hid = torch.empty(n, B * T, D, device=dev, dtype=torch.bfloat16)
    for i in range(n):
        hid[i] = rnd(B * T, D).to(torch.bfloat16)
    cls, u, dzbar = rnd(NQ, D), rnd(R, D) * D ** -0.5, rnd(B, R, D)
    lens = torch.randint(T // 2, T + 1, (B,), device=dev, generator=g).to(torch.int32)
    scores, cls_scores = (x_rows.float() @ u.t()).contiguous(), (cls @ u.t()).contiguous()
    p, _ = ops.cls_pool_train_fwd(x_rows, cls, scores, cls_scores, lens, B, T, NQ, R, D, 0.1, 1)
    ds, pp = torch.empty(B, R, NQ + T, device=dev), torch.empty(B, R, NQ + T, device=dev)
    du, dck, da = torch.empty(B * nsplit, R, D, device=dev), torch.empty(B * nsplit, NQ, D, device=dev), torch.empty(B * nsplit, n, device=dev)

    def pool(entry, name):
        return lambda: check(entry(ptr(x_rows), D, ptr(cls), ptr(hid), 0, hid.stride(0), n, 0, ptr(p), ptr(dzbar), ptr(u), ptr(lens), ptr(ds), ptr(pp), ptr(du), ptr(dck),
                                   ptr(da), B, T, NQ, R, D, nsplit, 0.1, 1, stream()), name)
    lines.append(row(f"cls_pool_bwd (nsplit {nsplit}, {n} bf16 hidden states)", timed({"default": pool(L.sc_cls_pool_bwd, "sc_cls_pool_bwd"),
                                                                                    "det": pool(L.sc_cls_pool_bwd_det, "sc_cls_pool_bwd_det")}, a.iters)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""CPU only: the self-check of tests/gemm_ref.py, the fp64 statements, rounding model and derived bounds behind tests/test_gemm_parity_gpu.py.

The case list is the REDUCED one: every case of the 128-row kernels whose output has at most 1.2 M elements, and one shrunk case per path and epilogue of the 256-row
kernels (gemm_ref.shrunk_cases: the same fields feed the reference, the rounding model and the bound).  For every case:
    real    (a) the reference's rms is at least 10x the mean bound;
            (b) a torch fp32 emulation of the path (the epilogue's rounding points; two summation orders: one addition per k, and 32-deep dot products with the
                walk rotated) stays within HALF the fp32 part of the bound -- (err - store) / (bound - store) <= 0.5 at every element, the bound without its
                store terms being its fp32 part; the printed column is that ratio itself -- and within the whole bound, and -- act = 0, at least 4096 outputs -- satisfies both 6 / sqrt(n) statistics of gemm_ref.stats;
    exact   (c) the emulation reproduces the expected bits under both orders, and for a 16-bit output with a residual the `once` and `twice` models differ on at
                least one element (a case that cannot tell them apart proves nothing about the rounding points);
    both    (d) every mutant of gemm_ref.MUTANTS that applies leaves the bound (real) or breaks bit-equality (exact); over the list, every mutant is caught on
                some case.  The mutant table keeps the two kinds apart: the largest err / bound over the REAL cases, and the largest number of differing elements
                over the EXACT cases, each with its case; `once_for_twice` (one rounding where two are modelled) stays inside the two store terms of a
                real case's bound by construction, so only exact cases catch it, and the table shows that; the reverse leaves the bound of a real case where
                the residual cancels the pre-residual value (the extra store's error is judged against a small result).

    python tools/gemm_bounds.py          # every reduced case, then the mutant table, then the failures (none expected)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gemm_ref as G   # noqa: E402

REDUCED_MAX_OUTPUTS = 1_200_000


def reduced_cases():
    small = [c for c in G.all_cases() if c.path in G.ROWS128 and G.nprod(c) * c.M * c.N <= REDUCED_MAX_OUTPUTS]
    return small + G.shrunk_cases()


def check_case(c, rep, mutants=True):
    inp = G.inputs(c)
    r = G.ref(c, inp)
    fig = 0.0
    if c.kind == "real":
        bd, store = G.bound(c, inp, r)
        out = r["out"]
        if not bool(torch.isfinite(out).all() and torch.isfinite(bd).all() and (bd > 0).all()):
            rep["failures"].append((c.id, "reference or bound not finite and positive"))
            return
        rms, mb = float((out * out).mean().sqrt()), float(bd.mean())
        if rms < 10 * mb:
            rep["failures"].append((c.id, f"rms {rms:.3g} below 10x the mean bound {mb:.3g}"))
        for order in G.ORDERS:
            em = G.emulate(c, inp, order)
            err = (em - out).abs()
            ratio = G.worst((err - store).clamp_min(0), bd - store)[0]
            whole = G.worst(err, bd)[0]
            fig = max(fig, ratio)
            if not ratio <= 0.5:
                rep["failures"].append((c.id, f"{order}: fp32 emulation above half the fp32 part of the bound: (err - store) / (bound - store)", ratio))
            if not whole <= 1.0:
                rep["failures"].append((c.id, f"{order}: fp32 emulation outside the bound", whole))
            if G.wants_stats(c):
                n, s1, s2, lim = G.stats(em, out, bd)
                rep["stats"][(c.id, order)] = (n, s1, s2, lim)
                if not (s1 <= lim and s2 <= lim):
                    rep["failures"].append((c.id, f"{order}: the emulation breaks a 6 / sqrt(n) statistic", (n, s1, s2, lim)))
    else:
        want = G.expected_bits(c, r)
        for order in G.ORDERS:
            em = G.emulate(c, inp, order).to(G.F32).to(G.out_dt(c))
            if not torch.equal(em, want):
                rep["failures"].append((c.id, f"{order}: the emulation does not reproduce the expected bits", int((em != want).sum())))
        if c.out == 16 and c.res:
            other = "once_for_twice" if G.rounding_points(c) == "twice" else "twice_for_once"
            if torch.equal(G.expected_bits(c, G.ref(c, inp, other)), want):
                rep["failures"].append((c.id, "`once` and `twice` give the same bits: the case cannot tell them apart"))
    rep["table"][c.id] = fig
    if not mutants:
        return
    for m in G.MUTANTS:
        mr = G.ref(c, inp, m)
        if mr is None:
            continue
        if c.kind == "real":          # err / bound over the elements where the wrong kernel's output is finite
            ok = torch.isfinite(mr["got"])
            margin = G.worst((mr["got"] - r["out"]).abs()[ok], bd[ok])[0] if bool(ok.any()) else 0.0
        else:                         # the number of elements whose bits differ
            margin = float((G.expected_bits(c, mr) != want).sum())
        rep["applied"][m] = rep["applied"].get(m, 0) + 1
        best = rep["margins"].setdefault(m, {"real": (0.0, None), "exact": (0.0, None)})
        if margin > best[c.kind][0]:
            best[c.kind] = (margin, c.id)


def run(cases=None, quiet=False, mutants=True):
    """-> dict(table: case id -> worst (err - store) / (bound - store) of the emulation (limit 0.5), failures, stats, applied,
    margins: mutant -> {"real": (largest err / bound, case id), "exact": (largest number of differing elements, case id)})"""
    cases = reduced_cases() if cases is None else list(cases)
    assert len({c.id for c in cases}) == len(cases), "duplicate case ids"
    rep = dict(table={}, failures=[], margins={}, stats={}, applied={})
    for c in cases:
        check_case(c, rep, mutants)
        if not quiet:
            print(f"{c.id:48s} {c.path:14s} {c.kind:6s} {G.rounding_points(c):6s} emulation (err - store) / (bound - store) {rep['table'][c.id]:8.4f}  (limit 0.5)")
    if mutants:
        for m in G.MUTANTS:
            best = rep["margins"].get(m, {"real": (0.0, None), "exact": (0.0, None)})
            (rm, rc), (em, ec) = best["real"], best["exact"]
            if not quiet:
                print(f"mutant {m:22s} applied to {rep['applied'].get(m, 0):4d} cases; real: largest err / bound {rm:10.4g} on {rc};  exact: most differing elements {em:8.0f} on {ec}")
            if not (rm > 1 or em > 0):
                rep["failures"].append((m, "mutant is caught on no case", best))
    if not quiet:
        print(f"{len(rep['table'])} cases, {len(rep['failures'])} failures")
        for f in rep["failures"]:
            print("FAIL", f)
    return rep


if __name__ == "__main__":
    sys.exit(1 if run()["failures"] else 0)

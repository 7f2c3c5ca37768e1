#!/usr/bin/env python3
"""CPU only: the self-check of tests/attention_bwd_ref.py, the fp64 statements and derived bounds behind tests/test_attention_bwd_parity_gpu.py.

For every case:  (a) the references and bounds are finite, each operand's rms over the elements that take part is at least 10x its mean bound, and the last valid key
                     holds 5 % .. 95 % of the probability on the plain heads (conditions on the INPUTS);
                 (b) an fp32 emulation of the kernels at their rounding points, in two summation orders (tile by tile as the kernels walk, and reversed), stays within
                     HALF the fp32 part of every element's bound -- the figure printed is (|err| - bf16 part) / (fp32 part) -- within the whole bound, and within
                     the slope threshold; so does the fp64 model with the bf16 roundings alone;
                 (c) every mutant leaves the per-element bound on elements where its own output is finite, or, for the two sub-ulp mutants, the slope threshold;
                     the table says which check catches it and by what margin (worst err / bound, or |slope - 1| / threshold, over the cases it can show in).

    python tools/attention_bwd_bounds.py            # every case, then the mutant table, then the failures (none expected); exit status 1 on any
    python tools/attention_bwd_bounds.py --reduced  # the list of tests/test_attention_bwd_bounds_cpu.py"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import attention_bwd_ref as A   # noqa: E402


def check_case(c, failures, margins, quiet=False, mutants=True):
    R = A.case_reference(c)
    row = {}
    for op in A.OPS:
        ref, b32, bbf = (A.part_rows(c, op, x[op]) for x in (R.ref, R.b32, R.bbf))
        r, b = A.cat(ref), A.cat(b32) + A.cat(bbf)
        if not bool(torch.isfinite(r).all() and torch.isfinite(b).all()):
            failures.append((c.id, op, "reference or bound not finite"))
        rms, mb = float((r * r).mean().sqrt()), float(b.mean())
        row[op + " rms/bound"] = rms / mb
        one_key = op != "dv" and all(c.kl(b_) <= 1 for b_ in range(c.B))          # dq = dk = 0 analytically: nothing to be well-posed about
        if not rms >= 10 * mb and not one_key:
            failures.append((c.id, op, f"rms {rms:.3g} below 10x the mean bound {mb:.3g}"))
    try:
        A.single_key_check(c, R)
    except AssertionError as e:
        failures.append((c.id, "single kept key", str(e)))
    mass = A.sentinel_mass(c, R)
    if mass and not (0.05 <= min(mass) and max(mass) <= 0.95):
        failures.append((c.id, "sentinel", f"last valid key holds {min(mass):.3f} .. {max(mass):.3f} of the probability"))
    for mode in ("model", "f32", "f32rev"):
        got = A.case_model(c, mode)
        for op in A.OPS:
            g, r, b32, bbf = A.cat(got[op]), A.cat(R.ref[op]), A.cat(R.b32[op]), A.cat(R.bbf[op])
            whole = A.worst((g - r).abs(), b32 + bbf)[0]
            part = A.worst(((g - r).abs() - bbf).clamp_min(0), b32)[0]
            row[f"{op} {mode}"] = (whole, part)
            if not whole <= 1.0:
                failures.append((c.id, op, f"{mode}: err / bound {whole:.3f}"))
            if mode != "model" and not part <= 0.5:
                failures.append((c.id, op, f"{mode}: fp32 part of the error at {part:.3f} of the fp32 part of the bound"))
            if A.participating(c, op) >= A.SLOPE_MIN:
                d, thr = A.slope_check(got[op], R.ref[op], R.b32[op], R.vsum[op])
                row[f"{op} {mode} slope"] = d / thr
                if not d <= thr:
                    failures.append((c.id, op, f"{mode}: |slope - 1| {d:.3e} above the threshold {thr:.3e}"))
        if mode != "model":
            for name, g, r, e in (("lse", got["lse"], R.lse, R.e_lse), ("delta", got["delta"], R.delta, R.e_delta)):
                w = A.worst((A.cat(g) - A.cat(r)).abs(), A.cat(e))[0]
                row[f"{name} {mode}"] = w
                if not w <= 0.5:
                    failures.append((c.id, name, f"{mode}: statistics error at {w:.3f} of its bound"))
    if not quiet:
        print(f"{c.id:24s} " + " ".join(f"{op}: rms/bound {row[op + ' rms/bound']:6.1f} model {row[op + ' model'][0]:.2f} f32 {max(row[op + ' f32'][1], row[op + ' f32rev'][1]):.3f}"
                                         + (f" slope {max(row[f'{op} {m} slope'] for m in ('model', 'f32', 'f32rev')):.2f}" if f"{op} model slope" in row else "") for op in A.OPS)
              + f" | lse {max(row['lse f32'], row['lse f32rev']):.3f} delta {max(row['delta f32'], row['delta f32rev']):.3f}")
    if c.group == "image":
        for given in (False, True):
            Rg, md = A.case_reference(c, given=given), A.image_model(c)
            for n in ("P", "dS"):
                r, bd = A.cat([im[n][0] for im in Rg.img]), A.cat([im[n][1] + im[n][2] for im in Rg.img])
                w = A.worst((A.cat([m[n] for m in md]) - r).abs(), bd)[0]
                if not w <= 1.0:
                    failures.append((c.id, n + " image", f"model at {w:.3f} of the bound (given={given})"))
                for mut in A.IMAGE_MUTANTS if not given and mutants else ():
                    wm = A.worst((A.cat([m[n] for m in A.image_model(c, mut)]) - r).abs(), bd)[0]
                    m_ = margins.setdefault(mut, [0.0, 0.0, 0])
                    m_[0], m_[2] = max(m_[0], wm), m_[2] + (n == "P")
    if not mutants:
        return
    for mut in A.MUTANTS + A.SLOPE_MUTANTS:
        if mut in A.NEEDS and not A.NEEDS[mut](c):
            continue
        got = A.case_model(c, "model", mut)
        best, sbest = 0.0, 0.0
        only = A.single_kept(c) if mut == "delta_stored_in_hd" else range(c.B)          # measured where it acts, the units with one kept key (p = 0.25: V = +-3 there gives O = +-4, exact in bf16, and nothing to see)
        for op in A.OPS:
            g, r, b = (A.cat([x[b_] for b_ in only]) for x in (got[op], R.ref[op], [x + y for x, y in zip(R.b32[op], R.bbf[op])]))
            fin = torch.isfinite(g)
            best = max(best, A.worst((g - r).abs()[fin], b[fin])[0])
            if A.participating(c, op) >= A.SLOPE_MIN:
                d, thr = A.slope_check(got[op], R.ref[op], R.b32[op], R.vsum[op])
                sbest = max(sbest, d / thr)
        m = margins.setdefault(mut, [0.0, 0.0, 0])
        m[0], m[1], m[2] = max(m[0], best), max(m[1], sbest), m[2] + 1


def run(ids, quiet=False):
    failures, margins = [], {}
    t0 = time.time()
    for cid in ids:
        check_case(A.case(cid), failures, margins, quiet)
    print(f"\n{len(ids)} cases in {time.time() - t0:.1f} s\n\n{'mutant':24s} {'cases':>5s} {'err/bound':>12s} {'slope/thr':>10s}  caught by")
    for mut in A.MUTANTS + A.SLOPE_MUTANTS + A.IMAGE_MUTANTS:
        if mut not in margins:
            failures.append(("-", mut, "no case of the list can show this mutant"))
            continue
        e, s, n = margins[mut]
        by = " and ".join(n_ for n_, on in (("per-element bound", e > 1.0), ("slope check", s > 1.0)) if on) or "NOTHING"
        print(f"{mut:24s} {n:5d} {e:12.3g} {s:10.3g}  {by}")
        if mut in A.SLOPE_MUTANTS:
            if not s > 1.0:
                failures.append(("-", mut, f"inside the slope threshold everywhere ({s:.3f})"))
        elif not e > 1.0:
            failures.append(("-", mut, f"inside the per-element bound everywhere ({e:.3f})"))
    print(f"\n{len(failures)} failures")
    for f in failures:
        print("FAILED", *f)
    return failures, margins


if __name__ == "__main__":
    reduced = "--reduced" in sys.argv[1:]
    counts = {g: len(A.ids_of(g)) for g in A.N_CASES}
    assert counts == A.N_CASES, counts
    fails, _ = run(list(A.REDUCED) if reduced else [c.id for c in A.all_cases() if c.id != "packed-H12"] + ["packed-H12"])
    sys.exit(1 if fails else 0)

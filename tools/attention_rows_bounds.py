#!/usr/bin/env python3
"""CPU only: the self-check of tests/attention_rows_ref.py, the fp64 statement and derived bound behind tests/test_attention_rows_parity_gpu.py.

For every case of the list it prints
  * the fp32 emulation's worst err / bound over both summation orders, the stored bf16 value against the whole bound and the fp32 value in front of the store against the fp32
    part of the bound alone (both must stay <= 1: the derived bound holds for a correct implementation); census cases
    must be exact in the emulation AND equal bf16(sum v / n_live);
  * that the chunk-by-chunk fp64 recurrence restates the plain softmax (to 1e-12): the two state mutants are variants of that recurrence;
and, over the sentinel family, the share of the rows each mutant CHANGES that leave the bound (at least 0.9 for every mutant: `acc_not_rescaled` is judged on the rising
staircase cases, `sum_reset_at_skipped_chunk` changes only batch entries in which a masked chunk follows a live one).
It also prints the MODEL values of the comparison with sc_attention_hd_fwd (the per-row metric of tests/test_attention_fwd_parity_gpu.py for a model of a correct flash
kernel -- probabilities and output rounded to bf16 -- on attention_rows_ref.HD_CASES) and of the module-level comparisons (attention_rows_ref.mod_model: the fp64 chain
with the attention output and the 16-bit GEMM outputs rounded to bf16 as well, on attention_rows_ref.MOD_CASES), and checks that no reference row of either has max|ref| < 1e-2.

    python tools/attention_rows_bounds.py            # every case
    python tools/attention_rows_bounds.py --emit     # the HD_MODEL and MOD_MODEL dicts of the GPU test, to paste"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import attention_rows_ref as A   # noqa: E402

MIN_SHARE = 0.9
CHANGED = 1e-9


def emulation_ratio(c, inp, r, bd):
    """the fp32 emulation over both orders: err / bound after the store, err / (bound - store) in front of it; -> (the two ratios, the stored emulations)"""
    w, wp, ems = 0.0, 0.0, []
    for order in A.ORDERS:
        em = A.emulate(c, inp, order)["out"]
        ems.append(em)
        w = max(w, A.worst((em - r).abs(), bd.bound)[0])                                           # the stored value against the whole bound
        if c.family != "census":
            pre = A.emulate(c, inp, order, store=False)["out"]
            wp = max(wp, A.worst((pre - r).abs(), bd.bound - bd.store)[0] / bd.limit)            # the fp32 value in front of the store against the fp32 part alone
    return w, wp, ems


def mutant_rows(c, inp, r, bd, m):
    """-> (rows the mutant changes, rows among them with an element outside the bound); a row is one (b, i, h)"""
    if m == "acc_not_rescaled" and c.profile != "rise":
        return 0, 0
    mr = A.ref(c, inp, m)["out"]
    diff = (mr - r).abs()
    changed = (diff > CHANGED * (1 + r.abs())).any(-1)
    out = (diff > bd.bound).any(-1)
    return int(changed.sum()), int((changed & out).sum())


def hd_model(x):
    """the MODEL of tests/test_attention_fwd_parity_gpu.py on one comparison case: -> (worst per-row metric of the modelled flash kernel, smallest max|ref| of a row)"""
    import test_attention_fwd_parity_gpu as T
    c = A.cross_case(x)
    inp = A.inputs(c)
    lens = A.prefix_lengths(inp["pad"])
    r = A.ref(c, inp)["out"]
    worst, rmin = 0.0, float("inf")
    for b in range(c.B):
        q, k, v = (inp[n][b].to(torch.float32).to(torch.bfloat16) for n in "qkv")
        model = T.attn_ref(q, k, v, lens[b], inp["scale"], p_fmt=torch.bfloat16, out_fmt=torch.bfloat16)
        plain = T.attn_ref(q, k, v, lens[b], inp["scale"])
        assert float((plain - r[b]).abs().max()) <= 1e-5, x.id                    # the two fp64 statements agree (exp of scale against exp2 of the fp32 constant c: 1e-7 relative on a score)
        worst = max(worst, float(T.row_metric(model, r[b]).max()))
        rmin = min(rmin, float(r[b].abs().amax(-1).min()))
    return worst, rmin


def run(ids=None, quiet=False, mutants=True):
    """-> (table: case id -> emulation ratio, failures, shares: mutant -> (changed rows, rejected rows), models: comparison / module case id -> MODEL)"""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    known = {c.id: c for c in A.cases()}
    table, failures, shares, hd = {}, [], {m: [0, 0] for m in A.MUTANTS}, {}
    for cid in (list(known) if ids is None else ids):
        c = known[cid]
        inp = A.inputs(c)
        r, bd = A.ref(c, inp)["out"], A.bound(c, inp)["out"]
        if not (r.shape == bd.bound.shape == (c.B, c.L, c.H, c.hd) and bool(torch.isfinite(r).all() and torch.isfinite(bd.bound).all() and (bd.bound >= bd.store).all())):
            failures.append((cid, "reference or bound not finite, of the wrong shape, or the store term above the bound"))
        on = A.ref(c, inp, online=True)["out"]
        if float((on - r).abs().max()) > 1e-12 * (1 + float(r.abs().max())):
            failures.append((cid, "the chunked fp64 recurrence does not restate the plain softmax", float((on - r).abs().max())))
        w, wp, ems = emulation_ratio(c, inp, r, bd)
        table[cid] = max(w, wp)
        note = ""
        if c.family == "census":
            want = A.census_expected(c, inp)
            exact = all(bool((em == want).all()) for em in ems) and bool((A.rnd(r, A.BF) == want).all())
            note = "  census: emulation " + ("bitwise" if exact else "NOT bitwise")
            if not exact:
                failures.append((cid, "census: the emulation is not bf16(sum v / n_live) bit for bit"))
        if not max(w, wp) <= 1.0:
            failures.append((cid, "fp32 emulation outside the derived bound", w))
        if not quiet:
            print(f"{cid:48s} fp32-emulation worst err / bound: stored {w:8.4f}  fp32 part {wp:8.4f}{note}")
        if mutants and c.family == "sentinel":
            for m in A.MUTANTS:
                ch, rej = mutant_rows(c, inp, r, bd, m)
                shares[m][0] += ch
                shares[m][1] += rej
    if mutants and ids is None:
        for m, (ch, rej) in shares.items():
            share = rej / ch if ch else 0.0
            if not quiet:
                print(f"mutant {m:28s} changes {ch:6d} rows, {rej:6d} leave the bound: share {share:6.3f}")
            if not (ch > 0 and share >= MIN_SHARE):
                failures.append((m, "mutant rejected on less than 90 % of the rows it changes", share))
    if ids is None:
        for x in A.HD_CASES:
            hd[x.id], rmin = hd_model(x)
            if not quiet:
                print(f"{x.id:48s} MODEL {hd[x.id]:.3e}   smallest max|ref| of a row {rmin:.3e}")
            if rmin < 1e-2:
                failures.append((x.id, "a reference row has max|ref| < 1e-2", rmin))
        for m in A.MOD_CASES:
            hd[m.id], rmin = A.mod_model(m)
            if not quiet:
                print(f"{m.id:48s} MODEL {hd[m.id]:.3e}   smallest max|ref| of a row {rmin:.3e}")
            if rmin < 1e-2:
                failures.append((m.id, "a reference row has max|ref| < 1e-2", rmin))
    if not quiet:
        print(f"{len(table)} cases, worst emulation ratio {max(table.values()):.4f}, {len(failures)} failures")
        for f in failures:
            print("FAIL", f)
    return table, failures, shares, hd


if __name__ == "__main__":
    if "--emit" in sys.argv:
        hd = {x.id: hd_model(x)[0] for x in A.HD_CASES}
        print("HD_MODEL = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in hd.items()) + "}")
        print("MOD_MODEL = {" + ", ".join(f'"{m.id}": {A.mod_model(m)[0]:.2e}' for m in A.MOD_CASES) + "}")
        sys.exit(0)
    sys.exit(1 if run()[1] else 0)

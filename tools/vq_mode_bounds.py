#!/usr/bin/env python3
"""CPU only: the self-check of tests/vq_modes_parity_ref.py, the fp64 statements and derived bounds behind tests/test_vq_modes_parity_gpu.py (csrc/vq_modes.hip).

For every case:  (a) the reference and the bound are finite and no output's rms over the whole tensor is below 10x its own mean bound (a condition on the INPUTS);
                 (b) a torch fp32 emulation of the kernel's arithmetic, in two summation orders, stays within HALF the fp32 part of the bound at every element (the
                     bound without its store term; the whole bound for an output of exact operations alone -- the convention of tools/tail_kernel_bounds.py).  The
                     noise is the float64 contract rounded to fp32; the product is emulated with the bf16 (hi, lo) pairs of P and of the table;
                 (c) every mutant statement of the group leaves the bound of some output on some case; the table names the case with the largest margin;
                 (d) the exact statements are well-posed: the fragment-ordered table restated on the host holds every element of the padded table once and
                     hi + lo gives the entry back to 2^-17; the fp32 emulation of the product on the one-hot / two-hot inputs IS the stated row, or half the sum of
                     the two rows, bit for bit in both orders;
                 (e) the REDUCED list (what tests/test_vq_mode_bounds_cpu.py runs) reaches every group and every mutant.

    python tools/vq_mode_bounds.py            # every case, then the mutant table, then the failures (none expected)
    python tools/vq_mode_bounds.py --reduced
    python tools/vq_mode_bounds.py --emit     # per case and output: rms |ref|, mean and largest bound (how wide each bound is), reduced list"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vq_modes_parity_ref as P   # noqa: E402

REDUCED_SOFT_R, REDUCED_SOFT_E, REDUCED_SOFT_V = (65, 200), (64, 128, 320), 333
REDUCED_HOT = ("onehot-65x333x64", "onehot-200x333x320", "twohot-129x333x128", "twohot-200x333x768")


def reduced_ids():
    ids = [c.id for c in P.noise_cases()] + [c.id for c in P.arg_cases()]
    ids += [c.id for c in P.prob_cases() if c.V in (5, 257) or (c.R == 7 and c.nmask == 3)]
    ids += [c.id for c in P.soft_cases() if c.R in REDUCED_SOFT_R and c.E in REDUCED_SOFT_E and c.V == REDUCED_SOFT_V]
    ids += [c.id for c in P.bwd_cases() if c.V < 1000]
    return ids


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins, self.sizes = quiet, {}, [], {}, {}

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))


def check_case(rep, G, c, mutants=True):
    inp = G.inputs(c)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(ref) == set(bd), (c.id, sorted(ref), sorted(bd))
    for name, r in ref.items():
        b = bd[name].bound
        if r.shape != b.shape:
            rep.fail(c.id, f"{name}: the bound's shape {tuple(b.shape)} is not the output's {tuple(r.shape)}")
        if not bool(torch.isfinite(r).all() and torch.isfinite(b).all() and (b >= 0).all()):
            rep.fail(c.id, f"{name}: reference or bound not finite")
            continue
        rms, mb = float((r * r).mean().sqrt()), float(b.mean())
        rep.sizes[(c.id, name)] = (rms, mb, float(b.max()))
        if rms < 10 * mb and name not in getattr(c, "zero", ()):          # (zero: outputs whose statement IS zero up to the bound -- bwd_cases says why)
            rep.fail(c.id, f"{name}: rms {rms:.3g} below 10x its mean bound {mb:.3g}")
    worst_e = 0.0
    for order in P.ORDERS:
        em = G.emulate(c, inp, order)
        for name, r in ref.items():
            b = bd[name]
            ratio = P.worst(((em[name].reshape(r.shape) - r).abs() - b.store).clamp_min(0), b.bound - b.store)[0] * 0.5 / b.limit
            worst_e = max(worst_e, ratio)
    rep.table[c.id] = worst_e
    if not rep.quiet:
        print(f"{c.id:56s} fp32-emulation worst (err - store) / (bound - store) {worst_e:8.4f}")
    if not worst_e <= 0.5:
        rep.fail(c.id, "fp32 emulation above half the fp32 part of the bound", worst_e)
    if mutants:
        for m in G.mutants:
            mref = G.ref(c, inp, m)
            if mref is None:
                continue
            margin = 0.0
            for name, r in ref.items():
                ok = torch.isfinite(mref[name])
                if bool(ok.any()):
                    margin = max(margin, P.worst((mref[name] - r).abs()[ok], bd[name].bound[ok])[0])
            key = (G.name, m)
            if margin > rep.margins.get(key, (0.0, None))[0]:
                rep.margins[key] = (margin, c.id)


def check_exact(rep):
    """(d) of the header"""
    for V in P.TABLE_V:
        for E in P.TABLE_E:
            emb = P.table_emb(V, E)
            bits = P.table_bits(emb)
            n = P.table_elems(V, E)
            if bits.numel() != n:
                rep.fail(f"table-{V}x{E}", "element count", bits.numel())
                continue
            hi, lo = bits[:n // 2].view(P.BF).to(P.F64), bits[n // 2:].view(P.BF).to(P.F64)
            pad = torch.zeros(P.nsteps(V) * 32, E, dtype=P.F64)
            pad[:V] = emb.to(P.F64)
            # as multisets: the fragment order is a permutation of the padded table
            if not bool(((hi + lo).sort().values - pad.reshape(-1).sort().values).abs().max() <= 2.0 ** -17 * 1.001 * float(pad.abs().max())):
                rep.fail(f"table-{V}x{E}", "hi + lo does not give the table back")
    hot = {c.id: c for c in P.hot_cases()}
    for cid in REDUCED_HOT:
        c = hot[cid]
        inp = P.hot_inputs(c)
        ref = P.hot_ref(c, inp)
        sc = P.SoftCase(c.id, c.R, P.HOT_V, c.E, c.temp, False, ())
        for order in P.ORDERS:
            em = P.soft_emulate(sc, dict(x=inp["x"], emb=inp["emb"], g=None), order)
            if not torch.equal(em["kw"], ref["kw"]):
                rep.fail(cid, f"the fp32 emulation ({order}) of the product is not the stated row bit for bit")
        if not torch.equal(ref["kw"].to(P.F32).to(P.F64), ref["kw"]):
            rep.fail(cid, "the stated rows are not fp32 values")


def run(ids=None, quiet=False, mutants=True):
    """-> (table: case id -> worst fp32-emulation figure, failures, margins: (group, mutant) -> (largest err / bound, case id)).  ids None: every case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    known = {c.id: (G, c) for G in P.GROUPS.values() for c in G.cases()}
    assert len(known) == sum(len(G.cases()) for G in P.GROUPS.values()), "duplicate case ids"
    rep = Report(quiet)
    ids = list(known) if ids is None else list(ids)
    for i in ids:
        if i not in known:
            rep.fail(i, "no such case")
            continue
        check_case(rep, *known[i], mutants=mutants)
    check_exact(rep)
    if mutants:
        groups = {known[i][0].name for i in ids if i in known}
        for G in P.GROUPS.values():
            if G.name not in groups:
                continue
            for m in G.mutants:
                margin, cid = rep.margins.get((G.name, m), (0.0, None))
                if not quiet:
                    print(f"mutant {G.name:8s} {m:30s} largest err/bound {margin:10.3g}  on {cid}")
                if not margin > 1:
                    rep.fail(G.name, f"mutant {m} stays inside the bound of every case run", margin)
    red = reduced_ids()
    if {known[i][0].name for i in red if i in known} != set(P.GROUPS):
        rep.fail("REDUCED", "groups not covered", sorted(set(P.GROUPS) - {known[i][0].name for i in red if i in known}))
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    run.sizes = rep.sizes
    return rep.table, rep.failures, rep.margins


if __name__ == "__main__":
    if "--emit" in sys.argv:
        table, failures, _ = run(reduced_ids(), quiet=True)
        print(f"{'case':56s} {'output':10s} {'rms |ref|':>11s} {'mean bound':>11s} {'max bound':>11s} {'emulation':>9s}")
        for (cid, name), (rms, mb, xb) in run.sizes.items():
            print(f"{cid:56s} {name:10s} {rms:11.3e} {mb:11.3e} {xb:11.3e} {table[cid]:9.4f}")
        for f in failures:
            print("FAIL", f)
    else:
        _, failures, _ = run(reduced_ids() if "--reduced" in sys.argv else None)
    sys.exit(1 if failures else 0)

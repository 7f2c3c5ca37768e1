#!/usr/bin/env python3
"""CPU only: the self-check of tests/tail_kernels_ref.py, the fp64 statements and derived bounds behind tests/test_tail_kernels_parity_gpu.py.

For every case:  (a) the reference and the bound are finite and no output's rms over the whole tensor is below 10x its own mean bound (a condition on the INPUTS);
                 (b) a torch fp32 emulation of the kernel's arithmetic, in two summation orders, stays within HALF the fp32 part of the bound at every element.  The
                     fp32 part is the bound without its store term (one attained rounding of the output, which the emulation performs too); the figure printed is
                     (|err| - store) / (bound - store), divided by 2 for an output whose bound declares limit 1.0 (IEEE operations only: the emulation is the kernel's
                     own arithmetic, so it is held to the whole bound -- the convention of the split-K finish in tools/row_kernel_bounds.py);
                 (c) every mutant statement of the group leaves the bound of some output on some case on elements where the wrong kernel's own output
                     is finite (a non-finite output is caught by that alone and proves nothing about the bound); the table names the case with the largest such margin and
                     counts the cases on which the wrong output is not finite;
                 (d) the REDUCED list (what tests/test_tail_kernel_bounds_cpu.py runs) reaches every group and every mutant.

    python tools/tail_kernel_bounds.py            # every case, then the mutant table, then the failures (none expected)
    python tools/tail_kernel_bounds.py --reduced"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tail_kernels_ref as T   # noqa: E402

REDUCED_IDS = (
    "adam-n257-t1-wd1e-06-clip", "adam-n257-t2-wd0.01-clip", "adam-n257-t10-wd0-noclip", "adam-n257-t1000-wd0.01-noclip", "adam-n257-t100000-wd1e-06-clip",
    "adam-n1-t2-wd0-clip",
    "gradnorm-n1-max4", "gradnorm-n255-max0", "gradnorm-n257-max1e+09", "gradnorm-n262145-max4", "gradnorm-n1-small-max0.0001",
    "colsum-1x1-ld1-acc", "colsum-255x65-ld65-set", "colsum-256x65-ld72-set", "colsum-256x65-ld72-acc", "colsum-257x64-ld64-set", "colsum-1000x130-ld130-acc",
    "gelu_fwd-n257", "gelu_bwd-n257", "qgelu_fwd-n257", "qgelu_fwd_bf16-n257", "qgelu_bwd-n257", "gelu_fwd-n1", "qgelu_bwd-n1",
    "lnbwd-D4-set-params-rows5", "lnbwd-D4-acc-noparams-rows3", "lnbwd-D260-acc-params-rows33", "lnbwd-D260-set-noparams-rows1", "lnbwd-D772-set-params-rows4",
    "lnbwd-D1024-set-params-rows33",
    "kwbn-B2-K1-E5-run", "kwbn-B6-K8-E16-run", "kwbn-B6-K8-E16-norun", "kwbn-B3-K3-E257-run", "kwbn-B256-K8-E64-run",
    "vqst-1x5-T0.1-mask3", "vqst-1x5-T1-mask8", "vqst-7x255-T0.1-mask0", "vqst-7x256-T1-mask3", "vqst-7x257-T0.1-mask8",
)
REDUCED_WHOLE_GROUPS = ("l2bwd", "addrows", "mixbwd", "cosfin", "hilo", "attnbwd")      # tiny: every case
SGEMM_REDUCED_WORK = 2_000_000                                                # sgemm: every case with M N K batch at most this; infonce: Bg <= 130


def reduced_ids():
    ids = list(REDUCED_IDS)
    for g in REDUCED_WHOLE_GROUPS:
        ids += [c.id for c in T.GROUPS[g].cases()]
    ids += [c.id for c in T.GROUPS["sgemm"].cases() if c.M * c.N * c.K * c.batch <= SGEMM_REDUCED_WORK]
    ids += [c.id for c in T.GROUPS["infonce"].cases() if c.Bg <= 130]
    return ids


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins, self.nonfinite = quiet, {}, [], {}, {}

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))


def check_case(rep, G, c, mutants=True):
    inp = G.inputs(c)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(ref) == set(bd), (c.id, sorted(ref), sorted(bd))
    if G.name == "infonce" and not c.inv_t * float((inp["a"] @ inp["b"].t()).max()) < 80:          # no maximum is subtracted: fp32 exp must stay finite
        rep.fail(c.id, "inv_t * max cos is not below 80")
    for name, r in ref.items():
        b = bd[name].bound
        if r.shape != b.shape:
            rep.fail(c.id, f"{name}: the bound's shape {tuple(b.shape)} is not the output's {tuple(r.shape)}")
        if not bool(torch.isfinite(r).all() and torch.isfinite(b).all() and (b >= 0).all()):
            rep.fail(c.id, f"{name}: reference or bound not finite")
            continue
        rms, mb = float((r * r).mean().sqrt()), float(b.mean())
        if rms < 10 * mb and not getattr(c, "zero", False):          # (zero: a case whose statement IS zero up to the bound -- all ids equal in the loss)
            rep.fail(c.id, f"{name}: rms {rms:.3g} below 10x its mean bound {mb:.3g}")
    worst_e = 0.0
    for order in T.ORDERS:
        em = G.emulate(c, inp, order)
        for name, r in ref.items():
            b = bd[name]
            ratio = T.worst(((em[name].reshape(r.shape) - r).abs() - b.store).clamp_min(0), b.bound - b.store)[0] * 0.5 / b.limit
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
            # a wrong kernel whose output is not finite is caught by that alone; its margin is taken over the elements that ARE finite, so that the table shows
            # whether it also leaves the bound where nothing overflowed
            finite = all(bool(torch.isfinite(v).all()) for v in mref.values())
            margin = 0.0
            for name, r in ref.items():
                ok = torch.isfinite(mref[name])
                if bool(ok.any()):
                    margin = max(margin, T.worst((mref[name] - r).abs()[ok], bd[name].bound[ok])[0])
            key = (G.name, m)
            if not finite:
                rep.nonfinite[key] = rep.nonfinite.get(key, 0) + 1
            if margin > rep.margins.get(key, (0.0, None))[0]:
                rep.margins[key] = (margin, c.id)


def run(ids=None, quiet=False, mutants=True):
    """-> (table: case id -> worst fp32-emulation figure, failures, margins: (group, mutant) -> (largest FINITE err / bound, case id)).  ids None: every case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    known = {c.id: (G, c) for G in T.GROUPS.values() for c in G.cases()}
    assert len(known) == sum(len(G.cases()) for G in T.GROUPS.values()), "duplicate case ids"
    rep = Report(quiet)
    ids = list(known) if ids is None else list(ids)
    for i in ids:
        if i not in known:
            rep.fail(i, "no such case")
            continue
        check_case(rep, *known[i], mutants=mutants)
    if mutants:
        groups = {known[i][0].name for i in ids if i in known}
        for G in T.GROUPS.values():
            if G.name not in groups:
                continue
            for m in G.mutants:
                margin, cid = rep.margins.get((G.name, m), (0.0, None))
                if not quiet:
                    print(f"mutant {G.name:10s} {m:28s} largest err/bound over finite elements {margin:10.3g}  on {cid}  (+ {rep.nonfinite.get((G.name, m), 0)} cases not finite)")
                if not margin > 1:
                    rep.fail(G.name, f"mutant {m} stays inside the bound of every case run", margin)
    red = reduced_ids()
    if {known[i][0].name for i in red if i in known} != set(T.GROUPS):
        rep.fail("REDUCED", "groups not covered", sorted(set(T.GROUPS) - {known[i][0].name for i in red if i in known}))
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    return rep.table, rep.failures, rep.margins


if __name__ == "__main__":
    _, failures, _ = run(reduced_ids() if "--reduced" in sys.argv else None)
    sys.exit(1 if failures else 0)

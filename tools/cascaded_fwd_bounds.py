#!/usr/bin/env python3
"""CPU only: the self-check of tests/cascaded_fwd_ref.py, the fp64 statements and derived bounds behind tests/test_cascaded_fwd_parity_gpu.py.

Three duties:
  (a) WELL-POSED: every reference and bound is finite where the statement is (the -inf / NaN the top-K statement itself returns aside), and the conditions the statements
      rest on hold on the inputs alone: the candidate sets of the refine cases are the ones the cases are named for and no input sits near the threshold, a masked column leads
      where the case says so, the chain cases' fp64 arg-max over the unmasked ids is decisive by more than twice the refine bound (cascaded_fwd_ref.WELLPOSED).
  (b) TIGHT: for every case and both summation orders, a torch fp32 emulation of the kernel's arithmetic stays within `limit` (0.5; 1.0 for an output that is one rounding or an
      integer) of the fp32 part of the bound at every element.
  (c) SHARP: every mutant statement of every group leaves the bound of some output on some case of the list run, on elements where the wrong kernel's own output is finite.
      A mutant that no case rejects is a FAILURE of this tool.
It also MEASURES what the refine buys on the chain cases: the three-term bf16 split evaluated in fp64 (cascaded_fwd_ref.ch_three_term) against the refine bound on the entries
that are surely refined -- the margin a kernel that skips the refine would show on the real unrefined values.  The figure is printed, not asserted (the module's
REFINE_MARGIN_NOTE says why).

    python tools/cascaded_fwd_bounds.py            # every case
    python tools/cascaded_fwd_bounds.py --reduced  # what tests/test_cascaded_fwd_bounds_cpu.py runs"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cascaded_fwd_ref as C   # noqa: E402

NOT_REDUCED = ("vq/V49408-R8-K8", "chain/auto-R4096-V1028-E64-mask023-lead", "probs/hd1024-L65-rows1-ragged", "refine/V1031-E512-all")


def reduced_ids():
    return [c.id for G in C.GROUPS.values() for c in G.cases() if c.id not in NOT_REDUCED]


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins, self.nonfinite, self.group_worst, self.three_term = quiet, {}, [], {}, {}, {}, {}

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))


def _statement_finite(t):
    return bool((torch.isfinite(t) | (t == -C.INF)).all())


def check_case(rep, G, c):
    inp = G.inputs(c)
    if G.name in C.WELLPOSED:
        try:
            C.WELLPOSED[G.name](c, inp)
        except AssertionError as e:
            rep.fail(c.id, "not well-posed", e.args)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(ref) == set(bd), (c.id, sorted(ref), sorted(bd))
    for name, r in ref.items():
        b = bd[name]
        if r.shape != b.bound.shape:
            rep.fail(c.id, f"{name}: the bound's shape {tuple(b.bound.shape)} is not the output's {tuple(r.shape)}")
        elif not (_statement_finite(r) and bool(torch.isfinite(b.bound).all() and (b.bound >= b.store).all() and (b.store >= 0).all())):
            rep.fail(c.id, f"{name}: reference or bound not finite, or the store term above the bound")
    worst_e = 0.0
    for order in C.ORDERS:
        em = G.emulate(c, inp, order)
        for name, r in ref.items():
            b = bd[name]
            err = torch.where(em[name].reshape(r.shape) == r, torch.zeros_like(r), (em[name].reshape(r.shape) - r).abs())       # -inf == -inf: no error
            worst_e = max(worst_e, C.worst((err - b.store).clamp_min(0), b.bound - b.store)[0] / b.limit)
    rep.table[c.id] = worst_e
    if G.name not in rep.group_worst or worst_e > rep.group_worst[G.name][0]:
        rep.group_worst[G.name] = (worst_e, c.id)
    if not rep.quiet:
        print(f"{c.id:56s} fp32-emulation worst (err - store) / (bound - store) / limit {worst_e:8.4f}")
    if not worst_e <= 1.0:
        rep.fail(c.id, "fp32 emulation above its limit of the fp32 part of the bound", worst_e)
    for m in G.mutants:
        mref = G.ref(c, inp, m)
        if mref is None:
            continue
        key = (G.name, m)
        margin = 0.0
        for name, r in ref.items():
            same = mref[name] == r
            ok = torch.isfinite(mref[name]) & torch.isfinite(r) & ~same
            if not bool((torch.isfinite(mref[name]) | same).all()):
                rep.nonfinite[key] = rep.nonfinite.get(key, 0) + 1
            if bool(ok.any()):
                margin = max(margin, C.worst((mref[name] - r).abs()[ok], bd[name].bound[ok])[0])
        if margin > rep.margins.get(key, (0.0, None))[0]:
            rep.margins[key] = (margin, c.id)
    if G.name == "chain":
        sure = C.ch_sure(c, inp)
        b32 = C.cos_bound(inp["a"], inp["e"], C.rf_nd(c.E), C.rf_nd(c.E) + 1)
        err = (C.ch_three_term(c, inp) - ref["out"]).abs()
        rep.three_term[c.id] = (C.worst(err[sure], b32[sure])[0], float(err[sure].max()), float((err / C.ch_b3(c, inp)).max()))
        if not rep.quiet:
            print(f"{c.id:56s} three-term split: |err| / refine bound over the sure candidates {rep.three_term[c.id][0]:8.3f} (largest |err| {rep.three_term[c.id][1]:.3g}); "
                  f"|err| / three-term bound over every entry {rep.three_term[c.id][2]:8.4f}")
        if not rep.three_term[c.id][2] <= 0.5:
            rep.fail(c.id, "the emulated three-term split is above half its bound", rep.three_term[c.id][2])


def run(ids=None, quiet=False):
    """-> (table: case id -> worst fp32-emulation figure, failures, margins: (group, mutant) -> (largest FINITE err / bound, the case that rejects it),
    three_term: chain case id -> (err / refine bound on sure candidates, largest err, err / three-term bound)).  ids None: every case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    known = {c.id: (G, c) for G in C.GROUPS.values() for c in G.cases()}
    assert len(known) == sum(len(G.cases()) for G in C.GROUPS.values()), "duplicate case ids"
    rep = Report(quiet)
    ids = list(known) if ids is None else list(ids)
    for i in ids:
        if i not in known:
            rep.fail(i, "no such case")
            continue
        check_case(rep, *known[i])
    groups = {known[i][0].name for i in ids if i in known}
    for G in C.GROUPS.values():
        if G.name not in groups:
            continue
        w, cid = rep.group_worst[G.name]
        if not quiet:
            print(f"group {G.name:10s} worst fp32-emulation / limit {w:8.4f}  on {cid}")
        for m in G.mutants:
            margin, cid = rep.margins.get((G.name, m), (0.0, None))
            if not quiet:
                print(f"mutant {G.name:10s} {m:28s} rejected by {cid}: err/bound {margin:10.3g} over finite elements (+ {rep.nonfinite.get((G.name, m), 0)} outputs not finite)")
            if not margin > 1:
                rep.fail(G.name, f"mutant {m} stays inside the bound of every case run", margin)
    red = reduced_ids()
    if {known[i][0].name for i in red if i in known} != set(C.GROUPS) or any(i not in known for i in red):
        rep.fail("REDUCED", "groups not covered, or an unknown id")
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    return rep.table, rep.failures, rep.margins, rep.three_term


if __name__ == "__main__":
    failures = run(reduced_ids() if "--reduced" in sys.argv else None)[1]
    sys.exit(1 if failures else 0)

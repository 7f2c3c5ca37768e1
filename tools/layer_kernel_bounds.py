#!/usr/bin/env python3
"""CPU only: the self-check of tests/layer_kernels_ref.py, the fp64 statements and derived bounds behind tests/test_layer_kernels_parity_gpu.py.

Two duties:
  (a) TIGHT: for every case and both summation orders, a torch fp32 emulation of the kernel's arithmetic stays within `limit` of the fp32 part of the bound at every
      element.  The fp32 part is the bound without its store term (one attained rounding of the output, which the emulation performs too); the figure printed is
      (|err| - store) / (bound - store) / limit and must not exceed 1 (limit: 0.5, or 1.0 for an output made of IEEE operations alone).
  (b) SHARP: every mutant statement of every group leaves the bound of some output on some case of the list run, on elements where the wrong kernel's own output
      is finite.  The table names the case with the largest margin.  A mutant that no case rejects is a FAILURE of this tool, not a skipped line.
Beside them, the slope check (layer_kernels_ref.slope_check) is held to the same two duties on the bf16 outputs it serves: the emulation stays inside its allowance,
and the mutants a bf16 store can hide from a per-element bound at some width (var_Dm1 at D = 1024, alpha_bf16) leave it.

    python tools/layer_kernel_bounds.py            # every case, then per group the worst emulation figure, the mutant table, the failures (none expected)
    python tools/layer_kernel_bounds.py --reduced  # what tests/test_layer_kernel_bounds_cpu.py runs"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import layer_kernels_ref as L   # noqa: E402

REDUCED_CB_ROWS, REDUCED_CB_COLS = (1, 3, 5, 64, 65, 64 * 8 + 1, 64 * 9 + 7), (7, 257)
SLOPE_MUTANTS = {"ln_bwd": ("var_Dm1",), "axpy": ("alpha_bf16",)}


def reduced_ids():
    ids = [c.id for c in L.lnb_cases() if c.rows <= 5 or (c.D == 64 and c.rows == 4097)]
    ids += [c.id for c in L.gb_cases()]
    ids += [c.id for c in L.cb_cases() if c.rows in REDUCED_CB_ROWS and c.cols in REDUCED_CB_COLS]
    ids += [c.id for G in ("axpy", "cls_pool_dz", "wgrad") for c in L.GROUPS[G].cases()]
    return ids


def slope_of(G, c, inp, out):
    """-> (ratio, smallest allowance) of the slope check the GPU test runs on this case's bf16 output, or None where it runs none"""
    if G.name == "ln_bwd" and c.rows >= 4:
        return L.slope_check(out["dx"], L.lnb_ref(c, inp)["dx"], L.lnb_pre(c, inp)["dx"])[::2]
    if G.name == "gelu_bwd" and c.kind == "slope":
        return L.slope_check(out["du"], L.gb_ref(c, inp)["du"], L.gb_pre(c, inp))[::2]
    if G.name == "axpy" and c.n >= 510:
        b = L.ax_bound(c, inp)["y"]
        return L.slope_check(out["y"], L.ax_ref(c, inp)["y"], b.bound - b.store)[::2]
    return None


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins, self.nonfinite, self.group_worst, self.slope = quiet, {}, [], {}, {}, {}, {}

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))


def check_case(rep, G, c):
    inp = G.inputs(c)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(ref) == set(bd), (c.id, sorted(ref), sorted(bd))
    for name, r in ref.items():
        b = bd[name]
        if r.shape != b.bound.shape:
            rep.fail(c.id, f"{name}: the bound's shape {tuple(b.bound.shape)} is not the output's {tuple(r.shape)}")
        if not bool(torch.isfinite(r).all() and torch.isfinite(b.bound).all() and (b.bound >= b.store).all() and (b.store >= 0).all()):
            rep.fail(c.id, f"{name}: reference or bound not finite, or the store term above the bound")
    worst_e = 0.0
    for order in L.ORDERS:
        em = G.emulate(c, inp, order)
        for name, r in ref.items():
            b = bd[name]
            worst_e = max(worst_e, L.worst(((em[name].reshape(r.shape) - r).abs() - b.store).clamp_min(0), b.bound - b.store)[0] / b.limit)
        s = slope_of(G, c, inp, em)
        if s is not None and not s[0] <= 1:
            rep.fail(c.id, f"the fp32 emulation ({order}) leaves the slope allowance", s[0])
    rep.table[c.id] = worst_e
    if G.name not in rep.group_worst or worst_e > rep.group_worst[G.name][0]:
        rep.group_worst[G.name] = (worst_e, c.id)
    if not rep.quiet:
        print(f"{c.id:72s} fp32-emulation worst (err - store) / (bound - store) / limit {worst_e:8.4f}")
    if not worst_e <= 1.0:
        rep.fail(c.id, "fp32 emulation above its limit of the fp32 part of the bound", worst_e)
    for m in G.mutants:
        mref = G.ref(c, inp, m)
        if mref is None:
            continue
        key = (G.name, m)
        margin = 0.0
        for name, r in ref.items():
            ok = torch.isfinite(mref[name])
            if not bool(ok.all()):
                rep.nonfinite[key] = rep.nonfinite.get(key, 0) + 1
            if bool(ok.any()):
                margin = max(margin, L.worst((mref[name] - r).abs()[ok], bd[name].bound[ok])[0])
        if margin > rep.margins.get(key, (0.0, None))[0]:
            rep.margins[key] = (margin, c.id)
        if m in SLOPE_MUTANTS.get(G.name, ()):                       # the wrong kernel's output as a bf16 store would leave it
            out = {k: L.bfr(v.to(L.F32)) for k, v in mref.items()}
            s = slope_of(G, c, inp, out)
            if s is not None and s[0] > rep.slope.get(key, (0.0, None))[0]:
                rep.slope[key] = (s[0], c.id)


def run(ids=None, quiet=False):
    """-> (table: case id -> worst fp32-emulation figure, failures, margins: (group, mutant) -> (largest FINITE err / bound, the case that rejects it),
    slope: (group, mutant) -> (largest slope difference / allowance, case)).  ids None: every case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    known = {c.id: (G, c) for G in L.GROUPS.values() for c in G.cases()}
    assert len(known) == sum(len(G.cases()) for G in L.GROUPS.values()), "duplicate case ids"
    rep = Report(quiet)
    ids = list(known) if ids is None else list(ids)
    for i in ids:
        if i not in known:
            rep.fail(i, "no such case")
            continue
        check_case(rep, *known[i])
    groups = {known[i][0].name for i in ids if i in known}
    for G in L.GROUPS.values():
        if G.name not in groups:
            continue
        w, cid = rep.group_worst[G.name]
        if not quiet:
            print(f"group {G.name:12s} worst fp32-emulation / limit {w:8.4f}  on {cid}")
        for m in G.mutants:
            margin, cid = rep.margins.get((G.name, m), (0.0, None))
            if not quiet:
                print(f"mutant {G.name:12s} {m:28s} rejected by {cid}: err/bound {margin:10.3g} over finite elements (+ {rep.nonfinite.get((G.name, m), 0)} outputs not finite)")
            if not margin > 1:
                rep.fail(G.name, f"mutant {m} stays inside the bound of every case run", margin)
        for m in SLOPE_MUTANTS.get(G.name, ()):
            s, cid = rep.slope.get((G.name, m), (0.0, None))
            if not quiet:
                print(f"slope  {G.name:12s} {m:28s} rejected by {cid}: slope difference / allowance {s:10.3g}")
            if not s > 1:
                rep.fail(G.name, f"mutant {m} stays inside the slope allowance of every case run", s)
    red = reduced_ids()
    if {known[i][0].name for i in red if i in known} != set(L.GROUPS) or any(i not in known for i in red):
        rep.fail("REDUCED", "groups not covered, or an unknown id")
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    return rep.table, rep.failures, rep.margins, rep.slope


if __name__ == "__main__":
    failures = run(reduced_ids() if "--reduced" in sys.argv else None)[1]
    sys.exit(1 if failures else 0)

"""CPU only: the MODEL errors behind the bounds of tests/test_text_tower_gpu.py (sc_attention_fwd_text), the well-posedness of its references, and the
sensitivity of its bounds to the bugs a causal attention over packed captions can have.  Same model, metric and bound as tools/attention_bounds.py (imported: its
self-check on the reduced case list runs first, so the convention this file leans on is the one that file establishes); no kernel runs here.

For every case of the test (builders and the fp64 statement imported from the test module):
  * MODEL = per-row max|err| / max|ref| of the CPU model of a correct kernel (probabilities rounded to bf16 before P.V, the row sum over the unrounded ones, one
    bf16 rounding of the output), maximum over all rows.  The test's bound is 4 x that + 1e-3.
  * the reference is well-posed: finite, no row with max|ref| < 1e-2 (the 1e-3 floor never carries a row).
  * MUTANT references fall outside the bound:
      diag-1      causal mask one key short (key i dropped; row 0 keeps its key)              at least 90 % of the rows i >= 1
      diag+1      causal mask one key long (key i + 1 admitted)                               at least 90 % of the rows that have a key i + 1
      neighbour   the next caption's first key admitted (a key index past the caption's last row reads the neighbour's row 0)   at least 90 % of all rows
      scale^2     the scale applied twice                                                     at least 90 % of the rows i >= 1

    python tools/text_tower_bounds.py            the table; exits non-zero if a check fails or a constant of the test is not reproduced
    python tools/text_tower_bounds.py --emit     the MODEL dict of the test, to paste
    python tools/text_tower_bounds.py --no-self-check    skip tools/attention_bounds.py's own run"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import attention_bounds as A          # noqa: E402
import test_text_tower_gpu as T       # noqa: E402


def worst(mod, ref):
    return max(T.row_metric(m, r).max().item() for m, r in zip(mod, ref))


def outside(mut, ref, bound, rows_of):
    """(rows outside the bound, rows judged) over all captions and heads; rows_of(T_b) -> bool [T_b] selects the judged rows"""
    k = n = 0
    for m, r in zip(mut, ref):
        sel = rows_of(r.shape[0])
        ex = T.row_metric(m, r)[sel] > bound
        k, n = k + int(ex.sum()), n + ex.numel()
    return k, n


def check_case(cid, rep, mutants=True):
    ins, ref = T.case_inputs(cid), T.case_reference(cid)
    model = worst([T.causal_ref(q, k, v, model=True) for q, k, v in ins], ref)
    bound = T.bound_of(model)
    rmin = min(r.abs().amax(-1).min().item() for r in ref)
    rep.need(all(torch.isfinite(r).all() for r in ref), f"{cid}: non-finite reference")
    rep.need(rmin >= 1e-2, f"{cid}: a reference row has max|ref| = {rmin:.2e} < 1e-2")
    const = T.MODEL.get(cid)
    rep.need(const is not None and abs(const - model) <= 0.02 * model, f"{cid}: MODEL constant in the test {const} is not the value computed here {model:.3e}")
    notes = []
    if mutants:
        B = len(ins)
        nxt = [(ins[(b + 1) % B][1][0], ins[(b + 1) % B][2][0]) for b in range(B)]          # the next caption's first key / value row [H, 64]
        table = (
            ("diag-1", [torch.cat([r[:1], T.causal_ref(q, k, v, diag=-1)[1:]]) for (q, k, v), r in zip(ins, ref)], lambda n: torch.arange(n) >= 1),
            ("diag+1", [T.causal_ref(q, k, v, diag=1) for q, k, v in ins], lambda n: torch.arange(n) < n - 1),
            ("neighbour", [T.causal_ref(q, k, v, extra=nxt[b]) for b, (q, k, v) in enumerate(ins)], lambda n: torch.ones(n, dtype=torch.bool)),
            ("scale^2", [T.causal_ref(q, k, v, scale=T.SCALE * T.SCALE) for q, k, v in ins], lambda n: torch.arange(n) >= 1),
        )
        for name, mut, rows_of in table:
            k, n = outside(mut, ref, bound, rows_of)
            rep.need(n > 0 and k >= 0.9 * n, f"{cid}: mutant '{name}' stays inside the bound on {n - k} of {n} judged (row, head) pairs")
            notes.append(f"{name} {k}/{n}")
    rep.line(f"{cid:10s} model {model:.3e} bound {bound:.3e} min max|ref| {rmin:.2e} | " + "; ".join(notes))
    return model


def run(ids=None, quiet=False, mutants=True):
    rep = A.Report(quiet)
    models = {cid: check_case(cid, rep, mutants) for cid in T.CASES if ids is None or cid in ids}
    return models, rep.fail


def main():
    if "--emit" in sys.argv:
        models, _ = run(quiet=True, mutants=False)
        print("MODEL = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in models.items()) + "}")
        return 0
    fail = []
    if "--no-self-check" not in sys.argv:
        torch.manual_seed(0)
        _, fail = A.run(A.REDUCED, quiet=True)
        print("tools/attention_bounds.py self-check (reduced cases): " + ("passed" if not fail else f"FAILED {fail}"))
    models, mine = run()
    fail = list(fail) + mine
    print("FAILED: %d checks" % len(fail) if fail else "all checks passed")
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())

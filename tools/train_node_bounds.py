"""CPU only: the MODEL errors behind the bounds of tests/test_train_nodes_parity_gpu.py, the well-posedness of its references, and the sensitivity of its bounds to
the wiring errors a training node can have.  The twin of tools/train_mode_bounds.py for the host drivers (layer node, layer mix, branch stack, image tower); no
kernel runs here.

For every case of the test (same builders and the same judged-tensor lists, imported from the test module; references: tests/train_mode_ref.py, train_nodes_ref.py):
  * MODEL = the test's metric for the CPU model of a correct implementation (model=True) against the fp64 reference.  The test's bound is 4 x that + 1e-3.  The
    constants pasted into the test must be reproduced to 2 %; a constant outside 1e-3 .. 2e-2 (the node-* constants of the train-mode test are 3e-3 .. 1.3e-2)
    is reported, except below the range for the tensors of an fp32 stretch (the branch's CLS tail, the tower's head, the column sum of the top gradient).
  * well-posed: finite; no judged row and no judged tensor with max|ref| < 1e-2 (the 1e-3 floor never carries one), no all-zero row; the k slice of every
    q | k | v bias gradient, left out of the metrics as analytically zero, has max|ref| < 1e-9, and the MODEL's slice keeps the zero rule of the test with room
    for another draw of the rounding noise (check_case).  Nothing else is left out.
  * the fp64 image-tower node equals vit_train_ref.oracle_visual_grads to 1e-10 (relative to the largest entry of each tensor).
  * every MUTANT -- the reference with one wrong wiring -- falls outside the bound on at least one judged tensor of at least one case it applies to:
      no direct gradient      hidden[li - 1]'s own gradient not added to the stream gradient
      flags shifted           the frozen / trained flags moved by one layer
      mask on residual        post-LN: the dropout mask also on the residual path
      no join (mid) / (h)     pre-LN: a residual join of the backward dropped
      LN bwd from t1/t2       the LayerNorm backward fed its own output instead of the saved stream copy
      other act derivative    erf-GELU's derivative in a QuickGELU body and vice versa
      k/v swapped             the k and v slices of the q | k | v gradients exchanged
      keys < len              branch stack: key length len instead of len + 1
      CLS without dq Wq / dy  the CLS row of the last branch layer without dq W_q / without the residual gradient
      dn1w without dg1        pre-LN branch: the all-row LayerNorm gradient not added into dn1w
      site seed reused        a dropout site of the last branch layer on the previous site's seed
      mix LN bwd skipped      layer mix with normalize: the LayerNorm backward left out
      class row on row 1      image tower: the class-row gradient seeded on row 1
      dcls without class row  class_embedding's gradient without the class row's share

    python tools/train_node_bounds.py             the tables (a few seconds; tests/test_train_node_bounds_cpu.py runs all of it); exits non-zero if a check fails or a constant of the test is not reproduced
    python tools/train_node_bounds.py --emit      the MODEL dict of the test, to paste"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_train_nodes_parity_gpu as T   # noqa: E402
import train_mode_ref as R                # noqa: E402

MIN_REF = 1e-2          # tools/train_mode_bounds.py's threshold: below it the 1e-3 floor of bound_of would carry the row or tensor
MODEL_RANGE = (1e-3, 2e-2)


class Report:
    def __init__(self, quiet=False):
        self.fail, self.quiet = [], quiet
        self.mutants = {}          # mutant -> [(case, tensors outside, tensors judged)]

    def line(self, s):
        if not self.quiet:
            print(s)

    def need(self, ok, what):
        if not ok:
            self.fail.append(what)
            self.line("   FAILED: " + what)


def metric(kind, got, ref):
    return R.row_metric(got, ref) if kind == "rows" else torch.tensor([R.tensor_metric(got, ref)])


ZERO_MARGIN = 1.15, 1.5          # see check_case


def check_case(cid, rep, ref, mod, mutants, fp32_only=lambda name: False, single_query=lambda name: False):
    """ref / mod: judged tensors (name -> (kind, tensor)) of the reference and of the model; mutants: name -> judged tensors; fp32_only(name): the tensor comes out
    of an fp32 stretch (its model error may lie below MODEL_RANGE).  -> {MODEL key: value}
    The zero rule (|k slice| < 1e-2 |q slice|) is well-posed where the MODEL keeps it with room for another draw of the same rounding noise: the slice is the norm
    of a sum of N independent rounding terms, one per (utterance, head, query), whose relative spread is about 1 / sqrt(2 N); two spreads are 1.15 for the
    N >= 100 queries of every full layer and 1.5 for the B H = 8 single queries of the last branch layer (single_query(name))."""
    models, left_out, n_rows = {}, [], 0
    rmin, zero_worst = float("inf"), 0.0
    rep.need(list(ref) == list(mod), f"{cid}: the model judges other tensors than the reference")
    for name, (kind, r) in ref.items():
        key = f"{cid}/{name}"
        if kind == "zero":
            left_out.append(name)
            rep.need(r[0].abs().max().item() < 1e-9, f"{key}: named analytically zero, max|ref| = {r[0].abs().max().item():.2e}")
            kn, qn = (t.norm().item() for t in mod[name][1])
            zero_worst = max(zero_worst, kn / qn)
            rep.need(ZERO_MARGIN[single_query(name)] * kn < 1e-2 * qn, f"{key}: the model's k slice is {kn / qn:.2e} of the q slice: the zero rule is ill-posed on these inputs")
            continue
        rep.need(bool(torch.isfinite(r).all()), f"{key}: non-finite reference")
        amax = r.abs().amax(-1).flatten() if kind == "rows" else r.abs().max().reshape(1)
        n_rows += amax.numel() if kind == "rows" else 0
        lo = amax.min().item()
        rmin = min(rmin, lo)
        rep.need(lo >= MIN_REF, f"{key}: max|ref| = {lo:.2e} < {MIN_REF} ({int((amax < MIN_REF).sum())} of {amax.numel()})")
        m = metric(kind, mod[name][1], r).max().item()
        models[key] = m
        const = T.MODEL.get(key)
        rep.need(const is not None and abs(const - m) <= 0.02 * m + 1e-12, f"{key}: MODEL constant in the test {const} is not the value computed here {m:.3e}")
        rep.need(m <= MODEL_RANGE[1] and (m >= MODEL_RANGE[0] or fp32_only(name)), f"{key}: model error {m:.2e} outside {MODEL_RANGE}: a rounding node is misplaced")
    vals = list(models.values())
    rep.line(f"{cid:28s} model {min(vals):.2e} .. {max(vals):.2e}  bound {R.bound_of(min(vals)):.2e} .. {R.bound_of(max(vals)):.2e}  min max|ref| {rmin:.2e}  "
             f"rows left out 0/{n_rows}  tensors judged {len(models)}  k-bias slices by the zero rule: {len(left_out)} (model |k| / |q| up to {zero_worst:.1e})")
    for mname, mu in mutants.items():
        outside = []
        if list(mu) != list(ref):
            outside.append("other tensors: " + ",".join(sorted(set(mu) ^ set(ref)))[:60])
        for name, (kind, r) in ref.items():
            if name not in mu:
                continue
            if kind == "zero":
                k, q = mu[name][1]
                if not k.norm().item() < 1e-2 * q.norm().item():
                    outside.append(name)
                continue
            ex = metric(kind, mu[name][1], r) > R.bound_of(models[f"{cid}/{name}"])
            if ex.any():
                outside.append(f"{name} {int(ex.sum())}/{ex.numel()}" if kind == "rows" else name)
        rep.mutants.setdefault(mname, []).append((cid, len(outside), len(ref)))
        rep.line(f"    mutant {mname:24s} outside on {len(outside)}/{len(ref)}: " + ", ".join(outside[:6]) + (" ..." if len(outside) > 6 else ""))
    return models


# ================================================================================================ the families
def run_node(cid, rep, mutants):
    c = T.node_case(cid)
    tens = lambda **kw: T.node_tensors(c, T.node_reference(cid, **kw))      # noqa: E731
    mu = {}
    if mutants:
        mu["no direct gradient"] = tens(wiring=("no_direct",))
        if not all(c.train):
            mu["flags shifted"] = tens(train=c.train[1:] + c.train[:1])
        if c.drop and not c.pre_ln:
            mu["mask on residual"] = tens(wiring=("residual_masked",))
        if c.pre_ln:
            mu["no join (mid)"] = tens(wiring=("no_join_mid",))
            mu["no join (h)"] = tens(wiring=("no_join_h",))
            mu["LN bwd from t1/t2"] = tens(wiring=("ln_from_out",))
            mu["other act derivative"] = tens(wiring=("act_bwd_swapped",))
        if any(c.train):
            mu["k/v swapped"] = tens(swap_kv=True)
    top = f"L{c.n - 1}." + ("fc2_b" if c.pre_ln else "ln2_b")          # the column sum of the top layer's own gradient: no rounding on its path
    return check_case(cid, rep, tens(), tens(model=True), mu, fp32_only=lambda name: name == top)


def run_wsum(cid, rep, mutants):
    tens = lambda **kw: T.wsum_tensors(T.wsum_reference(cid, **kw))      # noqa: E731
    mu = {}
    if mutants and cid == "wsum-normalize":
        mu["mix LN bwd skipped"] = tens(wiring=("skip_ln_bwd",))
    return check_case(cid, rep, tens(), tens(model=True), mu)


def run_branch(cid, rep, mutants):
    c = T.branch_case(cid)
    tens = lambda **kw: T.branch_tensors(c, T.branch_reference(cid, **kw))      # noqa: E731
    mu = {}
    if mutants:
        mu["keys < len"] = tens(wiring=("klen_len",))
        mu["CLS without dq Wq"] = tens(wiring=("no_dq",))
        mu["CLS without dy"] = tens(wiring=("no_dy",))
        mu["k/v swapped"] = tens(swap_kv=c.n - 1)
        if c.pre_ln:
            mu["dn1w without dg1"] = tens(wiring=("no_dg1",))
            if c.n > 1:
                mu["no join (mid)"] = tens(wiring=("no_join_mid",))
                mu["LN bwd from t1/t2"] = tens(wiring=("ln_from_out",))
        if c.p > 0:
            mu["site seed reused"] = tens(reuse_last=3)
    return check_case(cid, rep, tens(), tens(model=True), mu,
                      fp32_only=lambda name: name in ("out", "nf_w", "nf_b") or (name.startswith(f"L{c.n - 1}.") and ".in_" not in name),      # the fp32 CLS tail
                      single_query=lambda name: name.startswith(f"L{c.n - 1}."))


def tower_vs_oracle(cid):
    """max over the 32 gradients and the feature of |node - oracle| / max|oracle|"""
    import vit_train_ref as V
    _, ref, image, w, _ = T.tower_setup(cid)
    feat, grads = V.oracle_visual_grads(ref, image, w)
    res = T.tower_reference(cid)
    worst = ((res["feat"] - feat).abs().max() / feat.abs().max()).item()
    assert sorted(grads) == sorted(res["grads"]) and len(grads) == 32
    for k, g in grads.items():
        worst = max(worst, ((res["grads"][k] - g).abs().max() / g.abs().max()).item())
    return worst


def run_tower(cid, rep, mutants):
    tens = lambda **kw: T.tower_tensors(T.tower_reference(cid, **kw))      # noqa: E731
    worst = tower_vs_oracle(cid)
    rep.need(worst < 1e-10, f"{cid}: the fp64 node differs from oracle_visual_grads by {worst:.2e}")
    rep.line(f"{cid:28s} fp64 node against oracle_visual_grads: {worst:.2e}")
    mu = {}
    if mutants:
        mu["class row on row 1"] = tens(wiring=("seed_row1",))
        mu["dcls without class row"] = tens(wiring=("dcls_cut",))
        mu["no join (mid)"] = tens(wiring=("no_join_mid",))
        mu["no join (h)"] = tens(wiring=("no_join_h",))
        mu["LN bwd from t1/t2"] = tens(wiring=("ln_from_out",))
        mu["other act derivative"] = tens(wiring=("act_bwd_swapped",))
        mu["k/v swapped"] = tens(swap_kv=True)
    return check_case(cid, rep, tens(), tens(model=True), mu, fp32_only=lambda name: name in ("feat", "proj", "ln_post.weight", "ln_post.bias"))


def all_cases():
    return ([(c.id, run_node) for c in T.NODE_CASES] + [(c, run_wsum) for c in T.WSUM_CASES] + [(c.id, run_branch) for c in T.BRANCH_CASES] +
            [(c, run_tower) for c in T.TOWER_CASES])


ALL_MUTANTS = ("no direct gradient", "flags shifted", "mask on residual", "no join (mid)", "no join (h)", "LN bwd from t1/t2", "other act derivative", "k/v swapped",
               "keys < len", "CLS without dq Wq", "CLS without dy", "dn1w without dg1", "site seed reused", "mix LN bwd skipped", "class row on row 1",
               "dcls without class row")


def run(ids=None, quiet=False, mutants=True):
    """-> ({case: {MODEL key: value}}, failures, {mutant: [(case, tensors outside, tensors judged)]})"""
    rep = Report(quiet)
    models = {}
    for cid, fn in all_cases():
        if ids is None or cid in ids:
            models[cid] = fn(cid, rep, mutants)
    if mutants:
        rep.line("\nmutant                     cases outside / cases applied   (tensors outside / judged per case)")
        for mname in ALL_MUTANTS:
            rows = rep.mutants.get(mname, [])
            hit = sum(1 for _, o, _ in rows if o > 0)
            rep.need(hit > 0, f"mutant '{mname}' stays inside the bound on every judged tensor of every case")
            rep.line(f"{mname:26s} {hit}/{len(rows)}   " + "  ".join(f"{cid} {o}/{n}" for cid, o, n in rows))
        rep.need(set(rep.mutants) <= set(ALL_MUTANTS), "a mutant is missing from ALL_MUTANTS")
    return models, rep.fail, rep.mutants


def main():
    torch.manual_seed(0)
    if "--emit" in sys.argv:
        models, _, _ = run(quiet=True, mutants=False)
        print("MODEL = {")
        for cid, ms in models.items():
            line = "    "
            for k, v in ms.items():
                item = f'"{k}": {v:.2e}, '
                if len(line) + len(item) > 164:
                    print(line.rstrip())
                    line = "    "
                line += item
            print(line.rstrip())
        print("}")
        return 0
    models, fail, _ = run()
    print(f"{len(models)} cases, {sum(len(m) for m in models.values())} judged tensors")
    print("FAILED: %d checks" % len(fail) if fail else "all checks passed")
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())

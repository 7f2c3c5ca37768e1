"""CPU only: the MODEL errors behind the bounds of tests/test_train_mode_parity_gpu.py, the well-posedness of its references, and the sensitivity of its bounds to
the bugs a train-mode path can have.  The twin of tools/attention_bounds.py and tools/packed_frontend_bounds.py; no kernel runs here.

For every case of the test (same builders, imported from the test module; the references and the model are tests/train_mode_ref.py):
  * MODEL = the test's metric for the CPU model of a correct implementation (model=True) against the fp64 reference: per row max|err| / max|ref|, worst judged row,
    for the row tensors (p, pp, xbar, dz; hidden states and dh_in; h0 and dx6; the frozen encoder's hidden states), max|err| / max|ref| over the tensor for every
    parameter-shaped gradient.  The test's bound is 4 x that + 1e-3.  The constants pasted into the test must be reproduced to 2 %.
  * the reference alone must be well-posed: finite; no judged row with 0 < max|ref| < 1e-2 (the 1e-3 floor never carries a row) and no all-zero row outside the
    pooling head under dropout (an utterance whose every key was dropped pools exactly zero: the kernel must give exact zeros there); no judged parameter gradient
    with max|ref| < 1e-2 -- k_b, analytically zero, is left out BY NAME as tests/test_dropout_gpu.py does; every mask site has a dropped and a kept element in every
    judged row (attention: the row's keys over all heads).  Rows with fewer than 16 mask elements (utterances of 0 / 1 / 2 frames) cannot be asked for both: they are
    counted as "short" and still judged against the bound.  The share of rows and tensors these rules leave out is printed; it must be 0 for the row tensors
    and exactly the k_b tensors for the gradients.
  * every MUTANT reference -- the reference computed with a wrong mask or wiring -- must fall outside the bound of its case on at least one judged tensor:
      layer node       dropout1 / dropout3 seeds swapped; the mask also on the residual path; 1 / (1 - p) left out at dropout1 of layer 0; the activation mask in the
                       forward but not in the backward; layer 1 on layer 0's four seeds; three seeds per layer instead of four; packed rows: b * Tmax instead of
                       row_off[b], the utterance's own length as pair stride
      frozen encoder   four seeds per layer when the activation rate is 0; features / hidden-0 seeds swapped; dropout1 / dropout3 swapped; mask on the residual
      front stretch    features / hidden-0 seeds swapped; the backward's mask on dxp taken from the other site; 1 / (1 - p) left out on the features
      pooling head     mask stride NQ + len[b] instead of NQ + T; mask index without the r term; ds from the dropped probabilities; d alpha without the ds . u term

    python tools/train_mode_bounds.py             the table; exits non-zero if a check fails or a constant of the test is not reproduced
    python tools/train_mode_bounds.py --reduced   the subset tests/test_train_mode_bounds_cpu.py runs
    python tools/train_mode_bounds.py --emit      the MODEL dict of the test, to paste"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_train_mode_parity_gpu as T   # noqa: E402
import train_mode_ref as R               # noqa: E402

SHORT = 16          # mask elements below which a row cannot be asked to hold a dropped and a kept element


class Report:
    def __init__(self, quiet=False):
        self.fail, self.quiet = [], quiet

    def line(self, s):
        if not self.quiet:
            print(s)

    def need(self, ok, what):
        if not ok:
            self.fail.append(what)
            self.line("   FAILED: " + what)


# ================================================================================================ judged tensors per family: name -> ("rows" | "tensor", fp64 tensor)
def pool_tensors(c, res):
    cat = lambda t: torch.cat([t[b, :n] for b, n in enumerate(c.lens)])      # noqa: E731
    out = dict(p=("rows", res["p"].reshape(-1, res["p"].shape[-1])), pp=("rows", res["pp"].reshape(-1, res["pp"].shape[-1])),
               xbar=("rows", res["xbar"].reshape(-1, c.D)), du=("tensor", res["du"]), dck=("tensor", res["dck"]), dz=("rows", cat(res["dz"])))
    if c.n:
        out["dalpha"] = ("tensor", res["dalpha"])
    return out


def node_tensors(c, res):
    out = {f"hidden{li}": ("rows", T.node_rows(c, res["hidden"][li])) for li in range(T.NODE_LAYERS)}
    out["dh_in"] = ("rows", T.node_rows(c, res["dh_in"]))
    for li in range(T.NODE_LAYERS):
        if res["grads"][li] is not None:
            for name, g in zip(R.LAYER_NAMES, res["grads"][li]):
                out[f"L{li}.{name}"] = ("tensor", g)
    return out


def front_tensors(res):
    out = dict(h0=("rows", torch.cat(res["h0"])), dx6=("rows", torch.cat(res["dx6"])))
    out.update({k: ("tensor", v) for k, v in res["grads"].items()})
    return out


def frozen_tensors(res):
    return {f"h{i}": ("rows", torch.cat([res[b][i] for b in range(len(res))])) for i in range(len(res[0]))}


ZERO_BY_NAME = ("k_b",)          # analytically zero (softmax rows are shift invariant)


def metric(kind, got, ref):
    return R.row_metric(got, ref) if kind == "rows" else torch.tensor([R.tensor_metric(got, ref)])


def site_rows_ok(keep, rep, what):
    """keep: 0 / 1 (or rescaled) mask, one row per judged row.  -> (short rows, rows)"""
    if keep is None:
        return 0, 0
    k = keep.reshape(keep.shape[0], -1) != 0
    if k.shape[1] < SHORT:
        return k.shape[0], k.shape[0]
    bad = int((k.all(-1) | (~k).all(-1)).sum())
    rep.need(bad == 0, f"{what}: {bad} of {k.shape[0]} rows have no dropped or no kept element")
    return 0, k.shape[0]


# ================================================================================================ one case
def check_case(cid, rep, ref, mod, tensors, mutants, zero_rows_ok=False, sites=()):
    """ref / mod: results of the family's reference(model=False / True); tensors: result -> judged tensors; mutants: name -> result.  -> {MODEL key: value}"""
    rt, mt = tensors(ref), tensors(mod)
    models, left_out, n_rows, n_zero = {}, [], 0, 0
    rmin = float("inf")
    for name, (kind, r) in rt.items():
        key = f"{cid}/{name}"
        rep.need(bool(torch.isfinite(r).all()), f"{key}: non-finite reference")
        if name.split(".")[-1] in ZERO_BY_NAME:
            left_out.append(name)
            rep.need(r.abs().max().item() < 1e-9, f"{key}: named analytically zero, max|ref| = {r.abs().max().item():.2e}")
            continue
        amax = r.abs().amax(-1).flatten() if kind == "rows" else r.abs().max().reshape(1)
        zero = int((amax == 0).sum())
        if kind == "rows":
            n_rows += amax.numel()
            n_zero += zero
            rep.need(zero == 0 or zero_rows_ok, f"{key}: {zero} all-zero reference rows")
        else:
            rep.need(zero == 0, f"{key}: the reference gradient is zero")
        if (amax > 0).any():
            lo = amax[amax > 0].min().item()
            rmin = min(rmin, lo)
            rep.need(lo >= 1e-2, f"{key}: max|ref| = {lo:.2e} < 1e-2")
        m = metric(kind, mt[name][1], r).max().item()
        models[key] = m
        const = T.MODEL.get(key)
        rep.need(const is not None and abs(const - m) <= 0.02 * m + 1e-12, f"{key}: MODEL constant in the test {const} is not the value computed here {m:.3e}")
    short = rows_seen = 0
    for what, keep in sites:
        s, n = site_rows_ok(keep, rep, f"{cid}: mask site {what}")
        short, rows_seen = short + s, rows_seen + n
    vals = list(models.values())
    rep.line(f"{cid:26s} model {min(vals):.2e} .. {max(vals):.2e}  bound {R.bound_of(min(vals)):.2e} .. {R.bound_of(max(vals)):.2e}  min max|ref| {rmin:.2e}  "
             f"rows left out 0/{n_rows} (exactly zero under dropout: {n_zero}; short mask rows: {short}/{rows_seen})  gradients left out by name: {left_out or 'none'}")
    for mname, res in mutants.items():
        mu = tensors(res)
        outside = []
        for name, (kind, r) in rt.items():
            key = f"{cid}/{name}"
            if key not in models:
                continue
            ex = metric(kind, mu[name][1], r) > R.bound_of(models[key])
            if ex.any():
                outside.append(f"{name} {int(ex.sum())}/{ex.numel()}" if kind == "rows" else name)
        rep.need(len(outside) > 0, f"{cid}: mutant '{mname}' stays inside the bound on every judged tensor")
        rep.line(f"    mutant {mname:22s} outside on {len(outside)}/{len(models)}: " + ", ".join(outside[:8]) + (" ..." if len(outside) > 8 else ""))
    return models


# ================================================================================================ the families
def pool_cases():
    return [f"{c.id}/p{p}" for c in T.POOL_CASES for p in T.POOL_P]


def run_pool(cid, rep, mutants):
    name, p = cid.split("/p")
    p = float(p)
    c = T.pool_case(name)
    mu = {}
    if mutants:
        if p > 0:
            mu["stride NQ+len"] = T.pool_reference(name, p, keep=T.pool_keep(c, p, lens=c.lens, NQ=c.NQ))
            mu["no r term"] = T.pool_reference(name, p, keep=T.pool_keep(c, p, share_rows=True))
            mu["ds from dropped"] = T.pool_reference(name, p, from_dropped=True)
        if c.n:
            mu["dalpha without ds.u"] = T.pool_reference(name, p, dalpha_without_ds=True)
    keep = T.pool_keep(c, p)
    sites = [] if keep is None else [(f"b{b}", keep[b, :, :c.NQ + n]) for b, n in enumerate(c.lens)]
    return check_case(cid, rep, T.pool_reference(name, p), T.pool_reference(name, p, model=True), lambda r: pool_tensors(c, r), mu, zero_rows_ok=p > 0, sites=sites)


def run_node(cid, rep, mutants):
    c = T.node_case(cid)
    masks = T.node_masks(c)
    mu = {}
    if mutants:
        mk = lambda **kw: T.node_reference(cid, masks=T.node_masks(c, **kw))      # noqa: E731
        mu["swap s1/s3"] = mk(plan=lambda li, s: (s[4 * li], s[4 * li + 3], s[4 * li + 2], s[4 * li + 1]))
        mu["mask on residual"] = T.node_reference(cid, wiring=("residual_masked",))
        mu["no rescale at L0 d1"] = mk(rescale_off=(0, "d1"))
        ones = [[dict(m, d2=torch.ones_like(m["d2"])) for m in per] for per in masks]
        mu["act mask fwd only"] = T.node_reference(cid, bwd_masks=ones)
        mu["L1 on L0's seeds"] = mk(plan=lambda li, s: tuple(s[0:4]))
        mu["3 seeds per layer"] = mk(plan=lambda li, s: tuple(s[3 * li:3 * li + 4]))
        if c.packed:
            mu["b*Tmax for row_off"] = mk(attn_kw=lambda b: dict(packed_base=b * max(c.rows)))
            mu["own length stride"] = mk(attn_kw=lambda b: dict(packed_stride=(c.rows[b] + 1) // 2))
    sites = []
    for li in range(T.NODE_LAYERS):
        for b, n in enumerate(c.lens):
            m = masks[li][b]
            sites += [(f"L{li} b{b} {k}", m[k][:n]) for k in ("d1", "d2", "d3")]
            sites.append((f"L{li} b{b} attn", m["attn"][:, :n, :n].transpose(0, 1)))
    return check_case(cid, rep, T.node_reference(cid), T.node_reference(cid, model=True), lambda r: node_tensors(c, r), mu, sites=sites)


def run_front(cid, rep, mutants):
    layout = cid.split("-")[1]
    enc, _, geo, _ = T.front_setup()
    x6 = T.front_x6_model()
    B, d = len(x6), enc.cfg.encoder_embed_dim
    mu = {}
    masks = [T.front_masks(layout, b, geo["valid"][b]) for b in range(B)]
    if mutants:
        mu["swap the two seeds"] = T.front_reference(layout, x6, masks=[T.front_masks(layout, b, geo["valid"][b], swap=True) for b in range(B)])
        other = [dict(features=R.elem_mask(T.FRONT_DROP["seed"] ^ R.FRONT_HIDDEN_XOR, R.first_row(geo["layout"][layout], b), geo["valid"][b], d, T.FRONT_DROP["features"]))
                 for b in range(B)]
        mu["dxp mask of other site"] = T.front_reference(layout, x6, bwd_masks=other)
        nores = [dict(m, features=m["features"] * (1 - T.FRONT_DROP["features"])) for m in masks]
        mu["no rescale on features"] = T.front_reference(layout, x6, masks=nores)
    sites = [(f"b{b} {k}", masks[b][k]) for b in range(B) for k in ("features", "hidden")]
    return check_case(cid, rep, T.front_reference(layout, x6), T.front_reference(layout, x6, model=True), front_tensors, mu, sites=sites)


def frozen_cases():
    return [f"{c.id}-{lay}" for c in T.FROZEN_CASES for lay in T.FRONT_LAYOUTS]


def run_frozen(cid, rep, mutants):
    name, layout = cid.rsplit("-", 1)
    enc = T.frozen_setup(name)[0]
    rates, nl = enc.dropout_rates(), enc.cfg.encoder_layers
    mu = {}
    if mutants:
        seed = T.frozen_seed()
        if rates["activation"] == 0:
            mu["4 seeds per layer"] = T.frozen_reference(name, layout, plan=R.frozen_seed_plan(seed, nl, rates, four_always=True))
        sf, sh, ls = R.frozen_seed_plan(seed, nl, rates)
        mu["swap features/hidden"] = T.frozen_reference(name, layout, plan=(sh, sf, ls))
        mu["swap s1/s3"] = T.frozen_reference(name, layout, swap13=True)
        mu["mask on residual"] = T.frozen_reference(name, layout, wiring=("residual_masked",))
    return check_case(cid, rep, T.frozen_reference(name, layout), T.frozen_reference(name, layout, model=True), frozen_tensors, mu)


def all_cases():
    return ([(c, run_pool) for c in pool_cases()] + [(c.id, run_node) for c in T.NODE_CASES] + [(f"front-{lay}", run_front) for lay in T.FRONT_LAYOUTS] +
            [(c, run_frozen) for c in frozen_cases()])


REDUCED = ("pool-768/p0.25", "pool-cascaded/p0.25", "pool-large/p0.0", "pool-192/p0.25", "node-packed", "node-frozen0", "front-packed", "frozen-768-padded",
           "frozen-tiny3-packed", "frozen-act-packed")


def run(ids=None, quiet=False, mutants=True):
    rep = Report(quiet)
    models = {}
    for cid, fn in all_cases():
        if ids is None or cid in ids:
            models[cid] = fn(cid, rep, mutants)
    return models, rep.fail


def main():
    torch.manual_seed(0)
    if "--emit" in sys.argv:
        models, _ = run(quiet=True, mutants=False)
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
    models, fail = run(REDUCED if "--reduced" in sys.argv else None)
    print(f"{len(models)} cases, {sum(len(m) for m in models.values())} judged tensors")
    print("FAILED: %d checks" % len(fail) if fail else "all checks passed")
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())

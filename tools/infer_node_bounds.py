"""CPU only: the MODEL errors behind the bounds of tests/test_infer_nodes_parity_gpu.py, the well-posedness of its references, and the sensitivity of its bounds to
the wiring errors an eval-mode driver can have.  The twin of tools/train_node_bounds.py for the inference half; no kernel runs here.

For every case of the test (same builders and judged-tensor lists, imported from the test module; references: tests/infer_nodes_ref.py):
  * MODEL = the test's metric for the CPU model of a correct implementation (model = the case's operand format) against the fp64 reference.  The test's bound is
    4 x that + 1e-3.  The constants pasted into the test must be reproduced to 2 %.
  * well-posed: finite; no judged row and no judged tensor with max|ref| < 1e-2 (the 1e-3 floor never carries one); every utterance contributes exactly its
    valid frames (HubertModel.valid_frames), nothing else is left out.
  * the fp64 references equal the oracle classes in double to 1e-10: HubertModelRef (oracle.hubert_ref.hubert_forward) on the valid frames, ClipRef.encode_image,
    torch.nn.TransformerEncoder on the CLS row and every valid row, ClipRef.encode_text.
  * the half-range case: the largest value the CPU model hands to a half store lies in [2^15, 6e4], nothing exceeds 65504.
  * every MUTANT -- the reference with one wrong wiring -- falls outside the bound on at least one judged row or tensor of at least one case it applies to; a
    mutant that hits whole rows leaves the bound on at least 90 % of the rows it changes in at least one case:
      LN affines swapped          ln1 and ln2 of every layer exchange weight and bias
      residual behind the LN      pre-LN: both residuals taken from the LayerNorm's output instead of the stream
      2nd residual from h         post-LN: fc2's residual read from the layer's input where tmp2 (LayerNorm 1's output) is meant
      encoder LN flipped          the encoder LayerNorm missing on state 0 of a post-LN model, present on a pre-LN one
      wave LN over padded len     cfg.normalize statistics over the batch's padded length instead of the utterance's own
      GroupNorm over own len      statistics over the utterance's own frames instead of those of the padded length
      halo row as key             the row behind an utterance's valid frames admitted as a key
      key mask one short          one valid key less
      dropped slot kept           a dropped layer still runs and keeps its slot
      bf16 where f16 claimed      the bf16 CPU model under the bound of the f16 case
      mix weights shifted         softmax(w) moved by one state
      mix softmax count           the softmax over one weight more than there are states
      LN on the mix               normalize_features on the mixed output instead of per state
      ln_post on row 1            the image tower's head fed row 1 instead of the class row
      ln_pre missing              the image tower without ln_pre
      branch final norm missing   the branch without model.norm
      CLS key masked at length 1  key 0 masked for the utterance of one frame (post-LN branches)
      EOT row off by one          the text feature taken from the row in front of the EOT row
      causal mask admits key i+1  the text tower's query i also sees key i + 1
      position by packed row      the positional embedding indexed by the packed row instead of the position

    python tools/infer_node_bounds.py             the tables (tests/test_infer_node_bounds_cpu.py runs all of it); exits non-zero if a check fails
    python tools/infer_node_bounds.py --emit      the MODEL dict of the test, to paste"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import infer_nodes_ref as I                 # noqa: E402
import test_infer_nodes_parity_gpu as T     # noqa: E402
import train_mode_ref as R                  # noqa: E402

MIN_REF = 1e-2          # below it the 1e-3 floor of bound_of would carry the row or tensor
CHANGED = 1e-9          # a row a mutant "changes": its metric against the unmutated reference is above this
ROWS_OUTSIDE = 0.9


class Report:
    def __init__(self, quiet=False):
        self.fail, self.quiet = [], quiet
        self.mutants = {}          # mutant -> [(case, rows or tensors outside, changed)]

    def line(self, s):
        if not self.quiet:
            print(s)

    def need(self, ok, what):
        if not ok:
            self.fail.append(what)
            self.line("   FAILED: " + what)


def metric(kind, got, ref):
    return R.row_metric(got, ref) if kind == "rows" else torch.tensor([R.tensor_metric(got, ref)])


def check_case(cid, rep, ref, mod, mutants, bound_case=None):
    """ref / mod: judged tensors (name -> (kind, tensor)); mutants: name -> judged tensors.  -> {MODEL key: value}"""
    models, n_rows, rmin = {}, 0, float("inf")
    rep.need(list(ref) == list(mod), f"{cid}: the model judges other tensors than the reference")
    for name, (kind, r) in ref.items():
        key = f"{cid}/{name}"
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
    vals = list(models.values())
    rep.line(f"{cid:28s} model {min(vals):.2e} .. {max(vals):.2e}  bound {R.bound_of(min(vals)):.2e} .. {R.bound_of(max(vals)):.2e}  min max|ref| {rmin:.2e}  "
             f"rows judged {n_rows}  tensors judged {len(models)}")
    for mname, mu in mutants.items():
        outside = changed = 0
        rep.need(list(mu) == list(ref), f"{cid}: mutant {mname} judges other tensors")
        rows_kind = False
        for name, (kind, r) in ref.items():
            m = metric(kind, mu[name][1], r)
            rows_kind |= kind == "rows"
            changed += int((m > CHANGED).sum())
            outside += int((m > R.bound_of(models[f"{(bound_case or cid)}/{name}"] if bound_case is None else T.MODEL[f"{bound_case}/{name}"])).sum())
        rep.mutants.setdefault(mname, []).append((cid, outside, changed, rows_kind))
        rep.line(f"    mutant {mname:26s} outside on {outside} of {changed} changed {'rows' if rows_kind else 'tensors'}")
    return models


# ================================================================================================ the families
def _valid_rows_only(cid, rep, res):
    valid = T.enc_setup(cid)[3]
    rep.need(all(h.shape[0] == v for hs, v in zip(res, valid) for h in hs), f"{cid}: a judged state does not hold exactly the valid frames")


def run_encoder(cid, rep, mutants):
    c = T.enc_case(cid)
    tens = lambda **kw: T.enc_tensors(T.enc_reference(cid, **kw))      # noqa: E731
    res = T.enc_reference(cid)
    _valid_rows_only(cid, rep, res)
    rep.need(len(res[0]) == T.n_states(c, dict(c.over).get("encoder_layers", 2)), f"{cid}: number of states")
    mu = {}
    if mutants and cid not in T.REPORT_ONLY:
        mu["LN affines swapped"] = tens(wiring=("ln_swapped",))
        mu["encoder LN flipped"] = tens(wiring=("enc_ln_flipped",))
        mu["halo row as key"] = tens(wiring=("halo_key",))
        mu["key mask one short"] = tens(wiring=("key_mask_short",))
        if c.pre_ln:
            mu["residual behind the LN"] = tens(wiring=("res_after_ln",))
            mu["wave LN over padded len"] = tens(wiring=("wave_ln_padded",))
        else:
            mu["2nd residual from h"] = tens(wiring=("res2_from_h",))
            mu["GroupNorm over own len"] = tens(wiring=("gn_own_len",))
        if c.drop:
            mu["dropped slot kept"] = tens(wiring=("keep_dropped",))
    ref, mod = T.enc_model_tensors(cid)
    if mu and c.pre_ln:          # the wiring mutants are judged on the states from the wave; the layers-alone tensors (own*) they leave as they are
        own = {k: v for k, v in ref.items() if k.startswith("own")}
        mu = {k: dict(v, **own) for k, v in mu.items()}
        if c.fmt == "f16":       # the bf16 CPU model where the half format is claimed: must leave the bound of the layers-alone tensors
            mu["bf16 where f16 claimed"] = dict({k: v for k, v in ref.items() if not k.startswith("own")},
                                                **{k: v for k, v in T.enc_model_tensors(cid, model="bf16")[1].items() if k.startswith("own")})
    return check_case(cid, rep, ref, mod, mu)


def run_mix(cid, rep, mutants):
    mu = {}
    if mutants:
        mu["mix weights shifted"] = T.mix_reference(cid, wiring=("w_shifted",))
        mu["mix softmax count"] = T.mix_reference(cid, wiring=("softmax_more",))
        if cid == "wrap-norm":
            mu["LN on the mix"] = T.mix_reference(cid, wiring=("ln_on_mix",))
    return check_case(cid, rep, T.mix_reference(cid), T.mix_reference(cid, model=True), mu)


def run_method(cid, rep, mutants):
    return check_case(cid, rep, T.method_reference(cid), T.method_reference(cid, model=True), {})


def run_tower(cid, rep, mutants):
    mu = {}
    if mutants:
        mu["ln_post on row 1"] = T.tower_eval_reference(cid, wiring=("post_row1",))
        mu["ln_pre missing"] = T.tower_eval_reference(cid, wiring=("no_ln_pre",))
    return check_case(cid, rep, T.tower_eval_reference(cid), T.tower_eval_reference(cid, model=True), mu)


def run_branch(cid, rep, mutants):
    c = T.branch_case(cid)
    mu = {}
    if mutants:
        mu["branch final norm missing"] = T.branch_reference(cid, wiring=("no_final_norm",))
        if not c.pre_ln:
            mu["CLS key masked at length 1"] = T.branch_reference(cid, wiring=("cls_key_masked",))
    return check_case(cid, rep, T.branch_reference(cid), T.branch_reference(cid, model=True), mu)


def branch_vs_torch(cid):
    """max over the CLS rows and every valid row of |branch_eval - torch.nn.TransformerEncoder in double| / max|torch row|"""
    from torch import nn
    c, d = T.branch_case(cid), T.branch_inputs(cid)
    layer = nn.TransformerEncoderLayer(c.D, c.H, c.ffn, 0.0, "gelu", 1e-5, batch_first=True, norm_first=c.pre_ln)
    ref = nn.TransformerEncoder(layer, c.n, nn.LayerNorm(c.D, eps=1e-5), enable_nested_tensor=False).double().eval()
    names = "self_attn.in_proj_weight self_attn.in_proj_bias self_attn.out_proj.weight self_attn.out_proj.bias norm1.weight norm1.bias linear1.weight linear1.bias " \
            "linear2.weight linear2.bias norm2.weight norm2.bias".split()
    sd = {f"layers.{li}.{n}": d["params"][12 * li + j].double() for li in range(c.n) for j, n in enumerate(names)}
    sd.update({"norm.weight": d["params"][-2].double(), "norm.bias": d["params"][-1].double()})
    ref.load_state_dict(sd)
    B, L = len(T.BRANCH_LEN), T.BRANCH_T + 1
    src = torch.cat([d["cls"].double().expand(B, 1, c.D), d["frames"].double()], 1)
    mask = torch.arange(L)[None, :] >= (torch.tensor(T.BRANCH_LEN)[:, None] + 1)
    with torch.no_grad():
        want = ref(src, src_key_padding_mask=mask)
    mine = T.branch_reference(cid)
    rows = torch.cat([want[b, :l + 1] for b, l in enumerate(T.BRANCH_LEN)])
    return max(R.row_metric(mine["full"][1], rows).max().item(), R.row_metric(mine["cls"][1], want[:, 0]).max().item())


def run_text(cid, rep, mutants):
    mu = {}
    if mutants:
        mu["EOT row off by one"] = T.text_reference(cid, wiring=("eot_off",))
        mu["causal mask admits key i+1"] = T.text_reference(cid, wiring=("causal_plus1",))
        mu["position by packed row"] = T.text_reference(cid, wiring=("pos_by_packed_row",))
    return check_case(cid, rep, T.text_reference(cid), T.text_reference(cid, model=True), mu)


def text_vs_oracle(cid):
    from oracle.clip_ref import ClipRef
    m, ids, cref = T.text_setup(cid)
    ref = ClipRef(cref).double().eval()
    ref.load_state_dict({k: v.double() for k, v in m.model.state_dict().items()})
    with torch.no_grad():
        want = ref.encode_text(ids)
    return R.row_metric(T.text_reference(cid)["feat"][1], want).max().item()


def all_cases():
    return ([(c.id, run_encoder) for c in T.ENC_CASES] + [(c, run_mix) for c in T.WRAP_MIX] + [(c, run_method) for c in T.WRAP_METHODS] +
            [(c, run_tower) for c in T.TOWER_CASES] + [(c.id, run_branch) for c in T.BRANCH_CASES] + [(c, run_text) for c in T.TEXT_CASES])


ALL_MUTANTS = ("LN affines swapped", "residual behind the LN", "2nd residual from h", "encoder LN flipped", "wave LN over padded len", "GroupNorm over own len",
               "halo row as key", "key mask one short", "dropped slot kept", "bf16 where f16 claimed", "mix weights shifted", "mix softmax count", "LN on the mix",
               "ln_post on row 1", "ln_pre missing", "branch final norm missing", "CLS key masked at length 1",
               "EOT row off by one", "causal mask admits key i+1", "position by packed row")


# ================================================================================================ the oracle classes, the half range
ORACLE_ENC = ("enc-post-tiny3", "enc-post-768", "enc-pre-tiny-f16", "enc-pre-1024-f16")


def encoder_vs_oracle(cid):
    """max over states and utterances of |reference - HubertModelRef in double| / max|oracle state|, on the valid frames"""
    import dataclasses
    from oracle.hubert_ref import HubertModelRef, HubertRefConfig, hubert_forward, preprocess_input
    enc, wav, _, valid, _ = T.enc_setup(cid)
    fields = {f.name for f in dataclasses.fields(HubertRefConfig)}
    ref = HubertModelRef(HubertRefConfig(**{k: v for k, v in dataclasses.asdict(enc.cfg).items() if k in fields})).double().eval()
    ref.load_state_dict({k: v.double() for k, v in enc.state_dict().items()})
    padded, mask = preprocess_input([wav[b, :l].double() for b, l in enumerate(T.ENC_LENS)], enc.cfg.normalize)
    # the oracle takes its softmax in fp32 (`w.float()`, as fairseq does) whatever the module's dtype: with Tensor.float as the identity for this one call the
    # whole oracle runs in double, and 1e-10 is an honest threshold
    from unittest import mock
    with mock.patch.object(torch.Tensor, "float", lambda self: self):
        want = hubert_forward(ref, padded, mask)["layer_results"]
    mine = T.enc_reference(cid)
    worst = 0.0
    for b, v in enumerate(valid):
        assert len(mine[b]) == len(want)
        for i, w in enumerate(want):
            worst = max(worst, ((mine[b][i] - w[b, :v]).abs().max() / w[b, :v].abs().max()).item())
    return worst


def tower_vs_oracle(cid):
    import test_train_nodes_parity_gpu as TN
    _, ref, image, _, _ = TN.tower_setup(cid)
    with torch.no_grad():
        want = ref.encode_image(image.double())
    return ((T.tower_eval_reference(cid)["feat"][1] - want).abs().max() / want.abs().max()).item()


def half_range_report(cid="half-f16"):
    """-> (the largest magnitude the CPU model hands to a 16-bit store of the layers, the same without the boost)"""
    probe = {}
    T.enc_reference(cid, model=True, probe=probe)
    return probe["max"]


def run(ids=None, quiet=False, mutants=True):
    """-> ({case: {MODEL key: value}}, failures, {mutant: [(case, outside, changed, rows?)]})"""
    rep = Report(quiet)
    models = {}
    for cid, fn in all_cases():
        if ids is None or cid in ids:
            models[cid] = fn(cid, rep, mutants)
    if ids is None:
        for cid in ORACLE_ENC:
            w = encoder_vs_oracle(cid)
            rep.need(w < 1e-10, f"{cid}: the fp64 reference differs from HubertModelRef by {w:.2e}")
            rep.line(f"{cid:28s} fp64 reference against HubertModelRef in double: {w:.2e}")
        for cid in T.TOWER_CASES:
            w = tower_vs_oracle(cid)
            rep.need(w < 1e-10, f"{cid}: the fp64 tower differs from ClipRef.encode_image by {w:.2e}")
            rep.line(f"{cid:28s} fp64 tower against ClipRef.encode_image in double: {w:.2e}")
        for c in T.BRANCH_CASES:
            w = branch_vs_torch(c.id)
            rep.need(w < 1e-10, f"{c.id}: the fp64 branch differs from torch.nn.TransformerEncoder by {w:.2e}")
            rep.line(f"{c.id:28s} fp64 branch against torch.nn.TransformerEncoder in double: {w:.2e}")
        for cid in T.TEXT_CASES:
            w = text_vs_oracle(cid)
            rep.need(w < 1e-10, f"{cid}: the fp64 text tower differs from ClipRef.encode_text by {w:.2e}")
            rep.line(f"{cid:28s} fp64 text tower against ClipRef.encode_text in double: {w:.2e}")
        top = half_range_report()
        rep.need(2.0 ** 15 <= top <= 6e4 and top <= I.HALF_MAX, f"half-f16: the largest half-stored value of the CPU model is {top:.1f}, outside [2^15, 6e4]")
        rep.line(f"{'half-f16':28s} largest half-stored value of the CPU model: {top:.1f} (half max {I.HALF_MAX:.0f})")
    if mutants:
        rep.line("\nmutant                       cases outside / applied   (outside / changed per case)")
        for mname in ALL_MUTANTS:
            rows = rep.mutants.get(mname, [])
            hit = sum(1 for _, o, _, _ in rows if o > 0)
            rep.need(hit > 0 or (ids is not None and not rows), f"mutant '{mname}' stays inside the bound on every judged row and tensor of every case")
            # (the format mutant is rounding noise on every row, not a wiring that moves whole rows: it has to leave the bound, the 90 % rule is for wirings)
            whole = [(o, ch) for _, o, ch, rk in rows if rk and ch > 0 and mname != "bf16 where f16 claimed"]
            if whole:
                rep.need(max(o / ch for o, ch in whole) >= ROWS_OUTSIDE, f"mutant '{mname}' leaves the bound on fewer than 90 % of the rows it changes in every case: {whole}")
            rep.line(f"{mname:28s} {hit}/{len(rows)}   " + "  ".join(f"{cid} {o}/{ch}" for cid, o, ch, _ in rows))
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

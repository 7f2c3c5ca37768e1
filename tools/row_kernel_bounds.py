#!/usr/bin/env python3
"""CPU only: the self-check of tests/row_kernels_ref.py, the fp64 statements and derived bounds behind tests/test_row_kernels_parity_gpu.py.

For every case:  (a) the reference is finite and no output row has an rms below 10x its own mean bound (a condition on the INPUTS);
                 (b) a torch fp32 emulation of the kernel's arithmetic (two-pass statistics; summation orders "seq" and "pair64") stays within HALF the bound at every
                     element -- the factor 2 is the margin for the GPU's own summation order and its hardware transcendentals.  The half is taken of the fp32
                     terms: the store term (one bf16 / half / fp32 rounding, which the emulation performs too and which is attained) stays whole, so the figure
                     printed is (|err| - store term) / (bound - store term);
                 (c) every mutant reference leaves the bound (or, for the sub-ulp LayerNorm mutants, the slope / offset allowance) somewhere in the group it targets;
                 (d) the REDUCED list (what tests/test_row_kernel_bounds_cpu.py runs) covers every dispatch path and every mutant.

    python tools/row_kernel_bounds.py            # every case: the table of fp32-emulation ratios and mutant margins, then the failures (none expected)
    python tools/row_kernel_bounds.py --reduced"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import row_kernels_ref as R   # noqa: E402

F64, F32, BF, H16 = R.F64, R.F32, R.BF, R.H16

LN_MUTANTS = ("var_Dm1", "eps_outside", "mean_Dm4", "neighbour_stats", "affine_shift4", "gelu_first")
SUB_ULP = ("var_Dm1", "mean_Dm4")
MUTANTS = {"dropln": ("mask_no_row", "no_keep_scale"), "mix": ("last_dropped", "stride_short", "softmax_nm1", "norm_Dm4"),
           "hn": ("Tp_for_T", "per_layer", "mean_sq", "eps_inside"), "wave": ("len_plus1", "len_minus1", "single_pass_f32", "unbiased"),
           "splitk": ("bias_res_swapped", "ldr_ignored"), "pool": ("keys_plus1", "keys_minus1", "no_cls", "cls_scores_transposed", "wave_tail_dropped", "lo_zero"),
           "clsattn": ("keys_plus1", "keys_minus1", "no_cls", "wave_tail_dropped")}

# what the CPU test runs: every dispatch path, every kernel template argument, every mutant
REDUCED = ("ln768", "ln512", "ln512_gelu", "ln1024f", "ln1024f_half", "ln768f", "gen_bf_bf-768-gelu", "gen_bf_bf-1020-aff-ldo", "gen_bf_f32-512-out_f32", "gen_bf_f32-260-aff-gelu-ldi",
           "gen_f32_bf-768-ld_out", "gen_f32_bf-256-aff-gelu-ldi", "gen_f32_f32-260-aff-ldi", "gen_f32_f32-252-aff-gelu-ldi", "gen_f32_half-260-aff-ldo", "gen_f32_half-8-aff-gelu-ldi",
           "dropln768-p0.1", "mix-n13-D260-bf16-norm-spread30", "mix-n2-D768-f32-norm-random", "mix-n25-D260-f32-equal", "l2-D260-bf16-slice", "l2-D4-f32", "hn-D260-bf16-method1",
           "hn-D64-f32-method2", "hn-D64-f32-method1", "wave-ld8", "wave-ld5001", "splitk-S2-3x260-gelu-resldwide", "splitk-S7-3x260-bias-gelu-resld0", "splitk-S2-3x260-bias-gelu-resldN", "splitk-S7-3x260-resldN",
           "pool-NQ2-R8-D260-T70", "pool-NQ8-R8-D128-T70", "clsattn-NQ2-H4-hd260-T70", "clsattn-NQ1-H4-hd16-T70")


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins = quiet, {}, [], {}

    def case(self, cid, emul, note="", limit=0.5):
        self.table[cid] = emul
        if not self.quiet:
            print(f"{cid:48s} fp32-emulation worst err/bound {emul:8.4f} {note}")
        if not emul <= limit:
            self.failures.append((cid, f"fp32 emulation above {limit} of the bound", emul))

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))

    def mutant(self, group, name, ratio):
        key = (group, name)
        self.margins[key] = max(self.margins.get(key, 0.0), ratio)


def well_posed(rep, cid, ref, bound):
    if not bool(torch.isfinite(ref).all() and torch.isfinite(bound).all()):
        rep.fail(cid, "reference or bound not finite")
        return
    r2 = ref.reshape(-1, ref.shape[-1])
    rms, mb = (r2 * r2).mean(-1).sqrt(), bound.reshape(-1, ref.shape[-1]).mean(-1)
    bad = rms < 10 * mb
    if bool(bad.any()):
        i = int(bad.float().argmax())
        rep.fail(cid, f"row {i}: rms {float(rms[i]):.3g} below 10x its mean bound {float(mb[i]):.3g}")


def ratio(a, b, bound, store=None):
    """worst |a - b| / bound; with `store` (the bound's store term): worst (|a - b| - store) / (bound - store), what (b) holds to 0.5"""
    if store is None:
        return R.worst((a - b).abs(), bound)[0]
    return R.worst(((a - b).abs() - store).clamp_min(0), bound - store)[0]


# ------------------------------------------------------------------------------------------------ LayerNorm
def check_ln(rep, c, reduced, mutants):
    if R.ln_dispatch(c) != c.path:
        rep.fail(c.id, f"the dispatcher sends this case to {R.ln_dispatch(c)}, not {c.path}")
    poly2 = c.path == "ln512_gelu"
    worst_e, slope_note = 0.0, ""
    for rows in ((1, max(c.rows)) if reduced else c.rows):
        x, gamma, beta = R.ln_inputs(c, rows)
        ref, _ = R.ln_ref(x, gamma, beta, c.gelu)
        bound = R.ln_bound(x, gamma, beta, c.gelu, c.out_dt, poly2)
        well_posed(rep, f"{c.id}[rows={rows}]", ref, bound)
        store = (R.GELU_POLY2_ABS + R.GELU_POLY2_REL * ref.abs()) if poly2 else R.store_bound(ref, c.out_dt)
        sub = c.out_dt != F32 and not c.gelu and rows >= 32
        for order in R.ORDERS:
            em = R.ln_emulate(x, gamma, beta, c.gelu, c.out_dt, order)
            worst_e = max(worst_e, ratio(em, ref, bound, store))
            if sub:
                so = R.ln_scale_offset(em, x, gamma, beta, c.out_dt)
                slope_note = f"slope {so['slope_diff'] / so['slope_allow']:.3f} offset {so['offset_ratio']:.3f}"
                if so["slope_diff"] > so["slope_allow"] or so["offset_ratio"] > 1:
                    rep.fail(c.id, f"fp32 emulation ({order}) outside the slope / offset allowance", so)
        if not mutants:
            continue
        for m in LN_MUTANTS:
            if (m == "gelu_first" and not (c.gelu and c.affine)) or (m == "neighbour_stats" and rows < 2) or (m == "affine_shift4" and not c.affine):
                continue
            mref, _ = R.ln_ref(x, gamma, beta, c.gelu, mutant=m)
            got = mref.to(F32).to(c.out_dt).to(F64)
            mr = ratio(got, ref, bound)
            if sub:
                so = R.ln_scale_offset(got, x, gamma, beta, c.out_dt)
                mr = max(mr, so["slope_diff"] / so["slope_allow"], so["offset_ratio"])
            rep.mutant(c.path, m, mr)
    rep.case(c.id, worst_e, slope_note)


def check_dln(rep, c, reduced, mutants):
    worst_e = 0.0
    for rows in ((max(c.rows),) if reduced else c.rows):
        x, res, gamma, beta = R.dln_inputs(c, rows)
        v, dv = R.dln_sum(x, res, c.p, R.DLN_SEED)
        ref, _ = R.ln_ref(v, gamma, beta, False)
        bound = R.ln_bound(v, gamma, beta, False, BF, dx=dv)
        well_posed(rep, c.id, ref, bound)
        keep = (v - res) != 0 if c.p > 0 else torch.ones_like(v, dtype=torch.bool)
        ks = torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(c.p, dtype=F32))
        v32 = res.to(F32) + torch.where(keep, x.to(F32) * ks, torch.zeros(1, dtype=F32))
        for order in R.ORDERS:
            worst_e = max(worst_e, ratio(R.ln_emulate(v32, gamma, beta, False, BF, order), ref, bound, R.store_bound(ref, BF)))
        if mutants and c.p > 0 and rows > 1:
            for m in MUTANTS["dropln"]:
                mv, _ = R.dln_sum(x, res, c.p, R.DLN_SEED, m)
                rep.mutant("dropln", m, ratio(R.ln_ref(mv, gamma, beta, False)[0].to(F32).to(BF).to(F64), ref, bound))
    rep.case(c.id, worst_e)


def check_ws(rep, c, reduced, mutants):
    worst_e = 0.0
    for rows in ((max(c.rows),) if reduced else c.rows):
        h, w = R.ws_inputs(c, rows)
        ref, pre = R.ws_ref(h, w, c.normalize)
        bound = pre + R.store_bound(ref, BF)
        well_posed(rep, c.id, ref, bound)
        for order in R.ORDERS:
            worst_e = max(worst_e, ratio(R.ws_emulate(h, w, c.normalize, order), ref, bound, R.store_bound(ref, BF)))
        if mutants and c.n > 1:
            for m in MUTANTS["mix"]:
                if (m == "norm_Dm4" and not c.normalize) or (m == "stride_short" and rows < 2) or (m == "last_dropped" and c.wkind == "one_dead" and c.n // 2 == c.n - 1):
                    continue
                rep.mutant("mix", m, ratio(R.ws_ref(h, w, c.normalize, mutant=m)[0].to(F32).to(BF).to(F64), ref, bound))
    rep.case(c.id, worst_e)


def check_l2(rep, c, reduced, mutants):
    x = R.l2_inputs(c)
    ref = R.l2_ref(x)
    bound = R.l2_bound(x, ref)
    well_posed(rep, c.id, ref, bound)
    rep.case(c.id, max(ratio(R.l2_emulate(x, o), ref, bound) for o in R.ORDERS))
    z = torch.zeros(2, c.D, dtype=F64)
    if not torch.equal(R.l2_ref(z, 1e-8), z):
        rep.fail(c.id, "the clamped statement of an all-zero row is not zero")


def check_hn(rep, c, reduced, mutants):
    x = R.hn_inputs(c)
    ref = R.hn_ref(x, R.HN_T, c.method)
    bound = R.hn_bound(x, ref, R.HN_T, c.method, c.f32)
    well_posed(rep, c.id, ref, bound)
    rep.case(c.id, max(ratio(R.hn_emulate(x, R.HN_T, c.method, c.f32, o), ref, bound, R.store_bound(ref, F32 if c.f32 else BF)) for o in R.ORDERS))
    # the fp64 statement against the oracle's restatement of normalize_hiddenstates (which sees the T frames of the padded batch only)
    from oracle.speechclip_ref import normalize_hidden_states
    want = normalize_hidden_states([x[i, :, :R.HN_T] for i in range(R.HN_N)], c.method)
    for i in range(R.HN_N):
        if not torch.allclose(ref[i, :, :R.HN_T], want[i], rtol=1e-12, atol=0):
            rep.fail(c.id, "the fp64 statement differs from oracle.normalize_hidden_states")
    if mutants:
        for m in MUTANTS["hn"]:
            if (m == "eps_inside") != (c.method == "method1"):
                continue
            rep.mutant("hn", m, ratio(R.hn_ref(x, R.HN_T, c.method, m).to(F32).to(F32 if c.f32 else BF).to(F64), ref, bound))


def check_wave(rep, ld, reduced, mutants):
    cid = f"wave-ld{ld}"
    x, lens = R.wv_inputs(ld)
    ref, bound, store = R.wv_ref(x, lens)
    if float(ref.abs().max()) > 100:
        rep.fail(cid, "a sample past the length reached the reference")
    for b, n in enumerate(lens):          # (len <= 1: the statement is exactly zero; judged, but no rms to speak of)
        if n >= 2:
            well_posed(rep, f"{cid}[b={b}]", ref[b:b + 1, :n], bound[b:b + 1, :n])
    rep.case(cid, max(ratio(R.wv_emulate(x, lens, o), ref, bound, store) for o in R.ORDERS))
    if mutants:
        for m in MUTANTS["wave"]:
            rep.mutant("wave", m, ratio(R.wv_ref(x, lens, mutant=m)[0].to(F32).to(F64), ref, bound))


def check_sk(rep, c, reduced, mutants):
    part, bias, res, ldr = R.sk_inputs(c)
    rmn = R.sk_res_view(res, c)
    ref, bound = R.sk_ref(part, bias, rmn, c.gelu)
    well_posed(rep, c.id, ref, bound)
    if c.gelu:
        u = R.sk_exact_f32(part, bias, None)
        em = torch.nn.functional.gelu(u)
        em = (em + rmn.to(F32)) if rmn is not None else em
    else:
        em = R.sk_exact_f32(part, bias, rmn)
    if c.gelu:
        rep.case(c.id, ratio(em.to(F64), ref, bound, R.U * ref.abs()))
    else:       # IEEE adds in the kernel's own fixed order: this IS the kernel's result (the GPU test asks for its bits), so there is no order or transcendental to leave room for
        rep.case(c.id, ratio(em.to(F64), ref, bound) / 2, "(exact-order fp32 adds: half of err/bound shown, i.e. held to 1)")
    if mutants and c.gelu:
        if bias is not None and res is not None:
            rep.mutant("splitk", "bias_res_swapped", ratio(R.sk_ref(part, bias, rmn, True, "bias_res_swapped")[0], ref, bound))
        if c.res in ("ldwide", "ld0"):
            rep.mutant("splitk", "ldr_ignored", ratio(R.sk_ref(part, bias, R.sk_res_view(res, c, "ldr_ignored"), True)[0], ref, bound))


def check_pool(rep, c, reduced, mutants):
    x, cls, s, cs = R.pool_inputs(c)
    ref, pre = R.pool_ref(c, x, cls, s, cs)
    for b, n in enumerate(c.lens):
        if n > 0:
            a = torch.cat([cs, s[b, :n]], 0)
            if not bool((a.argmax(0) == c.NQ + n - 1).any()):
                rep.fail(c.id, f"utterance {b}: the last valid key holds no row maximum")
    worst_e = 0.0
    for split in (False, True):
        bound = R.pool_bound(ref, pre, split)
        well_posed(rep, c.id, ref, bound)
        for order in R.ORDERS:
            acc = R.pool_emulate(c, x, cls, s, cs, order)
            hi = acc.to(BF)
            got = (hi.to(F64) + (acc - hi.to(F32)).to(BF).to(F64)) if split else hi.to(F64)
            worst_e = max(worst_e, ratio(got, ref, bound, bound - pre))
    rep.case(c.id, worst_e)
    if mutants:
        b16, bsp = R.pool_bound(ref, pre, False), R.pool_bound(ref, pre, True)
        for m in MUTANTS["pool"]:
            if m == "lo_zero":
                rep.mutant("pool", m, ratio(ref.to(F32).to(BF).to(F64), ref, bsp))
                continue
            if m == "cls_scores_transposed" and (c.NQ == 1 or c.R == 1):
                continue
            rep.mutant("pool", m, ratio(R.pool_ref(c, x, cls, s, cs, m)[0].to(F32).to(BF).to(F64), ref, b16))


def check_attn(rep, c, reduced, mutants):
    cq, kv = R.attn_inputs(c)
    ref, pre = R.attn_ref(c, cq, kv)
    bound = pre + R.store_bound(ref, BF)
    well_posed(rep, c.id, ref, bound)
    D, hd = c.H * c.hd, c.hd
    for b, n in enumerate(c.lens):
        if n > 0:
            k = torch.cat([cq[:, D:2 * D], kv[b, :n, :D]], 0).view(-1, c.H, hd)
            a = torch.einsum("hd,khd->hk", cq[0, :D].view(c.H, hd), k)
            if not bool((a.argmax(-1) == c.NQ + n - 1).any()):
                rep.fail(c.id, f"utterance {b}: the last valid key holds no row maximum")
    rep.case(c.id, max(ratio(R.attn_emulate(c, cq, kv, o), ref, bound, R.store_bound(ref, BF)) for o in R.ORDERS))
    if mutants:
        for m in MUTANTS["clsattn"]:
            rep.mutant("clsattn", m, ratio(R.attn_ref(c, cq, kv, m)[0].to(F32).to(BF).to(F64), ref, bound))


def all_checks():
    """[(case id, group, callable(rep, reduced, mutants))]"""
    out = []
    out += [(c.id, "ln", (lambda rep, rd, mu, c=c: check_ln(rep, c, rd, mu))) for c in R.ln_cases()]
    out += [(c.id, "dropln", (lambda rep, rd, mu, c=c: check_dln(rep, c, rd, mu))) for c in R.dln_cases()]
    out += [(c.id, "mix", (lambda rep, rd, mu, c=c: check_ws(rep, c, rd, mu))) for c in R.ws_cases()]
    out += [(c.id, "l2", (lambda rep, rd, mu, c=c: check_l2(rep, c, rd, mu))) for c in R.l2_cases()]
    out += [(c.id, "hn", (lambda rep, rd, mu, c=c: check_hn(rep, c, rd, mu))) for c in R.hn_cases()]
    out += [(f"wave-ld{ld}", "wave", (lambda rep, rd, mu, ld=ld: check_wave(rep, ld, rd, mu))) for ld in R.WV_LDS]
    out += [(c.id, "splitk", (lambda rep, rd, mu, c=c: check_sk(rep, c, rd, mu))) for c in R.sk_cases()]
    out += [(c.id, "pool", (lambda rep, rd, mu, c=c: check_pool(rep, c, rd, mu))) for c in R.pool_cases()]
    out += [(c.id, "clsattn", (lambda rep, rd, mu, c=c: check_attn(rep, c, rd, mu))) for c in R.attn_cases()]
    return out


def expected_mutants(ids):
    """every (group, mutant) a run over `ids` must have pushed outside its bound"""
    want = set()
    ln = {c.id: c for c in R.ln_cases()}
    groups = {cid: g for cid, g, _ in all_checks()}
    for cid in ids:
        g = groups[cid]
        if g == "ln":
            c = ln[cid]
            for m in LN_MUTANTS:
                if m in SUB_ULP and c.path == "ln512_gelu":
                    continue          # no GELU-free case on this template argument: the statistics code is the one "ln512" judges
                if m == "gelu_first" and not any(k.gelu and k.affine and k.path == c.path and k.id in ids for k in ln.values()):
                    continue
                if m in SUB_ULP and not any(k.path == c.path and not k.gelu and k.id in ids for k in ln.values()):
                    continue
                want.add((c.path, m))
        elif g in MUTANTS:
            want |= {(g, m) for m in MUTANTS[g]}
    return want


def run(ids=None, quiet=False, mutants=True, reduced=None):
    """-> (table: case id -> worst fp32-emulation err / bound, failures).  ids None: every case with every row count; else those cases (reduced row counts)."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    checks = all_checks()
    known = [cid for cid, _, _ in checks]
    assert len(set(known)) == len(known), "duplicate case ids"
    reduced = (ids is not None) if reduced is None else reduced
    ids = known if ids is None else list(ids)
    missing = [i for i in ids if i not in known]
    rep = Report(quiet)
    for i in missing:
        rep.fail(i, "no such case")
    for cid, _, fn in checks:
        if cid in ids:
            fn(rep, reduced, mutants)
    if mutants:
        for key in sorted(expected_mutants([i for i in ids if i in known])):
            m = rep.margins.get(key, 0.0)
            if not quiet:
                print(f"mutant {key[0]:14s} {key[1]:24s} worst err/bound {m:10.3g}")
            if not m > 1:
                rep.fail(key[0], f"mutant {key[1]} stays inside the bound of every case of its group", m)
    # (d) the reduced list reaches every dispatch path of sc_layernorm and every group
    ln = {c.id: c for c in R.ln_cases()}
    paths = {ln[i].path for i in REDUCED if i in ln}
    if paths != set(R.LN_PATHS):
        rep.fail("REDUCED", "dispatch paths not covered", sorted(set(R.LN_PATHS) - paths))
    groups = {g for cid, g, _ in checks if cid in REDUCED}
    if groups != {g for _, g, _ in checks}:
        rep.fail("REDUCED", "groups not covered", sorted({g for _, g, _ in checks} - groups))
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    return rep.table, rep.failures


if __name__ == "__main__":
    _, failures = run(REDUCED if "--reduced" in sys.argv else None)
    sys.exit(1 if failures else 0)

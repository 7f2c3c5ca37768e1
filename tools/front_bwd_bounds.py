#!/usr/bin/env python3
"""CPU only: the self-check of tests/front_bwd_ref.py, the fp64 statements and derived bounds behind tests/test_front_bwd_parity_gpu.py.

For every case:  (a) the statement is well-posed and IS the operation: conv layer 0's contract equals fp64 autograd of conv1d -> group_norm -> gelu (dy zero on the frames
                     without a gradient), the transposed positional conv and its weight gradient equal fp64 autograd of the grouped conv1d(padding = Kw // 2)[..., :rows], the
                     literal gapped / padded split-K chain equals the direct statement, conv_layer_backward's statement equals fp64 autograd of the strided view; in the
                     exact-integer cases every term is a multiple of one quantum and no sum reaches 2^24 quanta (conv_layer_backward: 256);
                 (b) THE CAP of conv layer 0's bound holds on the reference alone: per case the median of bound / |ref| <= 0.05 and at most 1 % of elements with bound > |ref|, for
                     each of dw, dgamma, dbeta (cases T0 <= 2 and the long case are outside it: front_bwd_ref's header says why);
                 (c) a torch fp32 emulation of a CORRECT kernel (the kernel's split over the waves, first frame to last and last to first) stays within HALF the fp32 part of
                     the bound -- (|err| - U |ref|) / (bound - U |ref|) -- and reproduces the exact cases bit for bit;
                 (d) every mutant leaves its bound or changes a bit on a case of its group; one that no case rejects is reported by name;
                 (e) the REDUCED list (what tests/test_front_bwd_bounds_cpu.py runs) covers every group and every mutant.

    python tools/front_bwd_bounds.py            # every case, then the failures (none expected)
    python tools/front_bwd_bounds.py --reduced"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import front_bwd_ref as B   # noqa: E402
import row_kernels_ref as R   # noqa: E402

F64, F32, BF, U = R.F64, R.F32, R.BF, R.U
ORDERS = ("wave4", "wave4rev")
MUTANTS = B.MUTANTS

REDUCED = ("c0b-C64-T1", "c0b-C64-T2", "c0b-C64-T3", "c0b-C64-T7", "c0b-C64-T64", "c0b-C128-T5", "c0b-pk-C128-T7-scale4", "c0b-pk-trap-T1217", "c0w-c0b-C64-T64", "c0w-c0b-pk-C128-T7-scale4",
           "rows-D24-G2-uniform-B2-Tp5-V4", "rows-D64-G2-packed-B9", "rows-D192-G4-packed-B8", "adj-cg32-Kw2-uniform-Tp70", "adj-cg64-Kw3-packed", "adj-cg64-Kw16-uniform-Tp8",
           "pw-cg8-Kw4-uniform-B4-Tp70", "pw-cg8-Kw4-uniform-B2-Tp5", "pw-cg8-Kw4-packed-B3-Rg1024", "pw-cg32-Kw16-packed-B3-Rg511", "pw-real-cg32-Kw16-uniform-B4-Tp70",
           "cl-k3s2-C64-dim128-rows5", "cl-k2s2-C128-dim64-rows64", "cl-real-k3s2-C64-dim128-rows65")


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins, self.notes = quiet, {}, [], {}, {}

    def case(self, cid, emul, note="", limit=0.5):
        self.table[cid] = emul
        self.notes[cid] = note
        if not self.quiet:
            print(f"{cid:44s} emulation worst err/bound {emul:8.4f} {note}")
        if not emul <= limit:
            self.failures.append((cid, f"emulation above {limit} of the bound", emul))

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))

    def mutant(self, group, name, ratio, cid):
        key = (group, name)
        if ratio > self.margins.get(key, (0.0, None))[0]:
            self.margins[key] = (ratio, cid)


def ratio(a, b, bound, store=None):
    if store is None:
        return R.worst((a - b).abs(), bound)[0]
    store = torch.minimum(store, bound)
    return R.worst(((a - b).abs() - store).clamp_min(0), bound - store)[0]


def differs(a, b):
    return 0.0 if (a is None or torch.equal(a, b)) else float("inf")


# ------------------------------------------------------------------------------------------------ conv layer 0
def c0b_autograd(c, inp):
    """fp64 autograd of conv1d -> group_norm -> gelu per utterance, dy zero where the layout holds no frame"""
    x, w, gamma, beta, dy = inp["x"], inp["w"], inp["gamma"], inp["beta"], inp["dy"]
    out = []
    for b, tl in enumerate(B.c0b_tlim(c)):
        wd, gd, bd = (t.clone().requires_grad_(True) for t in (w.view(c.C, 1, 10), gamma, beta))
        u = F.conv1d(x[b, :B.conv0_L(c.T0)][None, None], wd, stride=5)
        if c.T0 > 1:
            y = F.gelu(F.group_norm(u, c.C, gd, bd, B.EPS))
        else:       # F.group_norm refuses one value per channel: the same normalisation spelled out
            y = F.gelu((u - u.mean(-1, keepdim=True)) / (u.var(-1, unbiased=False, keepdim=True) + B.EPS).sqrt() * gd.view(1, -1, 1) + bd.view(1, -1, 1))
        g = torch.zeros(c.T0, c.C, dtype=F64)
        g[:tl] = dy[b, :tl]
        y.backward(g.t()[None])
        out.append(torch.cat([wd.grad.view(c.C, 10), gd.grad[:, None], bd.grad[:, None]], 1))
    return torch.stack(out)


def check_c0b(rep, c, mutants):
    inp = B.c0b_inputs(c)
    ref, bound = B.c0b_ref(c, inp)
    if not (bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all())):
        rep.fail(c.id, "reference or bound not finite")
    ag = c0b_autograd(c, inp)
    scale = ag.abs().amax((0, 1), keepdim=True).clamp_min(1e-300)
    if float(((ag - ref).abs() / scale).max()) > 1e-9:
        rep.fail(c.id, "the statement differs from fp64 autograd of conv1d -> group_norm -> gelu", float(((ag - ref).abs() / scale).max()))
    note = ""
    if c.cap:
        cap, bad = B.c0b_cap(ref, bound)
        note = " ".join(f"{k} median {v[0]:.1e} over {v[1]:.3f}" for k, v in cap.items())
        if bad:
            rep.fail(c.id, "the cap does not hold on the reference", bad)
    if "dc" in c.kinds:
        b = c.kinds.index("dc")
        fr = B.frames(inp["x"], c.T0)
        u = torch.einsum("tj,cj->ct", fr[b], inp["w"])
        dcr = u.mean(-1) ** 2 / u.var(-1, unbiased=False).clamp_min(1e-300) if c.T0 > 1 else torch.zeros(1)
        note += f" dc {inp['dc']:g} sd, channels with mean^2/var >= 100: {int((dcr >= 100).sum())}"
        if 4 <= c.T0 <= 64 and not int((dcr >= 100).sum()) >= 1:
            rep.fail(c.id, "no channel of the DC utterance has mean^2 / var >= 100", float(dcr.max()))
    worst = max(ratio(B.c0b_emulate(c, inp, o), ref, bound, U * ref.abs()) for o in ORDERS)
    rep.case(c.id, worst, note)
    if mutants:
        for m in MUTANTS["c0b"]:
            if (m == "var_T0m1" and c.T0 == 1) or (m == "m_over_grad_frames" and c.rows is None) or (m == "one_sweep_f32" and "dc" not in c.kinds):
                continue
            if m == "mean_terms_skipped" and all(t == c.T0 for t in B.c0b_tlim(c)):
                continue
            rep.mutant("c0b", m, ratio(B.c0b_ref(c, inp, mutant=m)[0].to(F32).to(F64), ref, bound), c.id)


def check_c0w(rep, c, mutants):
    cid = "c0w-" + c.id
    x, du, cond = B.c0w_inputs(c)
    q = cond["quantum"]
    if not (cond["worst"] < 2 ** 24 and bool((x / q == (x / q).round()).all()) and bool((du == du.round()).all())):
        rep.fail(cid, "a sum may reach 2^24 quanta, or a term is no multiple of the quantum", cond)
    want = B.c0w_ref(c, x, du)
    live = (torch.arange(c.T0).view(1, c.T0, 1) < torch.tensor(B.c0b_tlim(c)).view(-1, 1, 1)).to(F32)
    terms = (du.to(F32) * live).transpose(1, 2).unsqueeze(2) * B.frames(x, c.T0).to(F32).permute(0, 2, 1).unsqueeze(1)            # [B, C, 10, T0]
    ok = all(torch.equal(B.wave_sum(terms.contiguous(), rev).to(F64), want[..., :10]) for rev in (False, True)) and bool((want[..., 11] == 0).all())
    rep.case(cid, 0.0 if ok else float("inf"), "(bitwise)")


# ------------------------------------------------------------------------------------------------ row kernels
def check_rows(rep, c, mutants):
    inp = B.row_inputs(c)
    u, s, bound = B.finish_train_ref(c, inp)
    V, total = B.row_vec(c.D, c.G), sum(c.rows)
    if (total * c.D // V) % 256 == 0:
        rep.fail(c.id, "rows D / V is a multiple of 256: no partly filled block")
    # emulation: fp32 throughout with the erf GELU in fp32
    u32 = (B.slab_rows(c, inp["slab"]).to(F32) + inp["bias"].to(F32)).to(BF)
    s_em = ((inp["x"] * B.live_rows(c)).to(F32) + F.gelu(u32.to(F32))).to(BF).to(F64)
    ok = torch.equal(u32.to(F64), u)
    rep.case(c.id, max(ratio(s_em, s, bound, R.BF_STORE * s.abs()), 0.0 if ok else float("inf")))
    dx = B.dgrad_finish_ref(c, inp)
    off = B.row_off(c.rows)
    for b, v in enumerate(c.valid):
        if not bool((dx[off[b] + min(v, c.rows[b]):off[b + 1]] == 0).all()):
            rep.fail(c.id, "dgrad_finish's statement is not zero from valid on")
    if mutants:
        rep.mutant("rows", "mask_t_le_valid", max(ratio(B.bits(B.finish_train_ref(c, inp, "mask_t_le_valid")[1]), s, bound), differs(B.dgrad_finish_ref(c, inp, "mask_t_le_valid"), dx)), c.id)
        rep.mutant("rows", "slab_row_t", differs(B.dgrad_finish_ref(c, inp, "slab_row_t"), dx), c.id)
        rep.mutant("rows", "reverse_rows_b_minus_t", differs(B.reverse_ref(c, inp["x"], "reverse_rows_b_minus_t"), B.reverse_ref(c, inp["x"])), c.id)


# ------------------------------------------------------------------------------------------------ the positional conv: adjoint chain and weight gradient
def _grouped_conv_grads(x, du, w, rows, valid, G, Kw):
    """fp64 autograd of conv1d(mask(x), w, padding = Kw // 2, groups = G)[..., :rows_b] per utterance -> (dx [total, D], dW [D, cg, Kw])"""
    off, dxs = B.row_off(rows), []
    wd = w.clone().requires_grad_(True)
    for b, r in enumerate(rows):
        xm = x[off[b]:off[b + 1]].clone().requires_grad_(True)
        mask = (torch.arange(r) < min(valid[b], r)).to(F64).view(r, 1)
        y = F.conv1d((xm * mask).t()[None], wd, padding=Kw // 2, groups=G)[0, :, :r]
        y.backward(du[off[b]:off[b + 1]].t())
        dxs.append(xm.grad)
    return torch.cat(dxs, 0), wd.grad


def check_adj(rep, c, mutants):
    inp = B.adj_inputs(c)
    want, worst = B.adj_ref(c, inp)
    if not worst < 2 ** 24:
        rep.fail(c.id, "a partial sum may reach 2^24", worst)
    if sum(c.rows) <= 300:      # the statement is the input gradient of torch's own grouped conv (no mask on its input: every row of du counts)
        dx, _ = _grouped_conv_grads(torch.zeros_like(inp["du"]), inp["du"], inp["wfold"], c.rows, c.rows, c.G, c.Kw)
        off = B.row_off(c.rows)
        mine = torch.cat([B.convT64(inp["du"][off[b]:off[b + 1]], inp["wfold"], c.G, c.Kw)[0] for b in range(len(c.rows))], 0)
        if not torch.equal(dx, mine):
            rep.fail(c.id, "the transposed conv differs from autograd of conv1d(padding = Kw // 2)[..., :rows]", float((dx - mine).abs().max()))
    rep.case(c.id, 0.0, "(bitwise)")
    if mutants:
        for m in MUTANTS["adj"]:
            rep.mutant("adj", m, differs(B.adj_ref(c, inp, m)[0], want), c.id)


def check_pw(rep, c, mutants):
    inp = B.pw_inputs(c)
    want = B.pw_ref(c, inp)
    sp = B.pw_split(c)
    chain = B.pw_chain(c, inp)
    if c.real:
        bound = B.pw_bound(c, inp)
        if float(((chain - want).abs() / bound.clamp_min(1e-300)).max()) > 1e-6:
            rep.fail(c.id, "the literal chain differs from the direct statement")
        # emulation: the product rounded to fp32 once per split chunk (or per block of 64 rows), the chunks added in turn
        M, S = sp["M"], sp["S"]
        worst = 0.0
        for step in (64, sp["chunk"]):
            acc = torch.zeros_like(want).to(F32)
            for lo in range(0, M, step):
                acc = acc + _pw_rows(c, inp, lo, min(M, lo + step)).to(F32)
            worst = max(worst, ratio(acc.to(F64), want, bound, U * want.abs()))
        rep.case(c.id, worst, f"S {S} M {M}")
    else:
        mag = float(B.pw_ref(c, inp, absolute=True).max())
        if not (mag < 2 ** 24 and torch.equal(chain, want)):
            rep.fail(c.id, "a sum may reach 2^24, or the literal chain differs from the direct statement", mag)
        if sum(c.rows) <= 300:
            _, dW = _grouped_conv_grads(inp["x"], inp["du"], torch.zeros(c.G * c.cg, c.cg, c.Kw, dtype=F64), c.rows, c.valid, c.G, c.Kw)
            if not torch.equal(dW, want):
                rep.fail(c.id, "the statement differs from autograd of the grouped conv1d")
        rep.case(c.id, 0.0, f"(bitwise) S {sp['S']} M {sp['M']} Rg {sp['Rg']}")
    if mutants and not c.real:
        for m in MUTANTS["pw"]:
            rep.mutant("pw", m, differs(B.pw_chain(c, inp, m), want), c.id)


def _pw_rows(c, inp, lo, hi):
    """the literal chain restricted to K rows [lo, hi)"""
    import copy
    full = B.pw_chain(c, inp)
    if lo == 0 and hi >= B.pw_split(c)["M"]:
        return full
    # rows outside [lo, hi) removed from the gradient operand: linear in du, so chain(du restricted) is the chunk's partial
    sp = B.pw_split(c)
    keep = torch.zeros(sp["M"], dtype=torch.bool)
    keep[lo:hi] = True
    inp2 = copy.copy(inp)
    du = inp["du"].clone()
    off = B.row_off(c.rows)
    for b, r in enumerate(c.rows):
        p0 = (off[b] + b * c.Kw) if c.packed else b * sp["Tq"]
        du[off[b]:off[b + 1]] *= keep[p0:p0 + r].to(F64).view(r, 1)
    inp2["du"] = du
    return B.pw_chain(c, inp2)


# ------------------------------------------------------------------------------------------------ conv_layer_backward
def check_cl(rep, c, mutants):
    inp = B.cl_inputs(c)
    ref = B.cl_ref(c, inp)
    Mi = c.B * c.rows_out
    xd, wd = inp["xin"].clone().requires_grad_(True), inp["w"].clone().requires_grad_(True)
    view = torch.as_strided(xd, (Mi, c.k * c.C), (c.s * c.C, 1))
    (view @ wd.permute(0, 2, 1).reshape(c.dim, c.k * c.C).t()).backward(inp["du"])
    if not (torch.allclose(xd.grad, ref["dX"], rtol=1e-12, atol=1e-12) and torch.allclose(wd.grad, ref["dW"], rtol=1e-12, atol=1e-12)):
        rep.fail(c.id, "the statement differs from fp64 autograd of the strided view")
    if not bool((ref["dX"][c.s * Mi + (1 if c.k > c.s else 0):] == 0).all()):
        rep.fail(c.id, "slack rows the view does not reach are not zero in the statement")
    if c.real:
        dX, bound, dW, bW, store = B.cl_real_bound(c, inp)
        # emulation: every tap's product rounded to fp32 once, stored as bf16, the overlapping tap added in fp32 to the stored value and stored again
        em = torch.zeros_like(dX)
        for j in range(c.k):
            rows = slice(j, j + c.s * Mi, c.s)
            y = ref["taps"][j].to(F32)
            em[rows] = (y + (em[rows][:Mi].to(F32) if j >= c.s else 0)).to(BF).to(F64)
        rep.case(c.id, ratio(em, dX, bound, store), "paths " + " ".join(B.cl_gemm_case(c, j).path + ":" + B.Gm.rounding_points(B.cl_gemm_case(c, j)) for j in range(c.k)))
        return
    if not (ref["worst"] <= 256 and float(ref["dW"].abs().max()) < 2 ** 24):
        rep.fail(c.id, "an intermediate exceeds 256", ref["worst"])
    rep.case(c.id, 0.0, f"(bitwise) worst |intermediate| {ref['worst']:.0f}")
    if mutants:
        for m in MUTANTS["cl"]:
            if c.k > c.s:
                rep.mutant("cl", m, differs(B.cl_ref(c, inp, m)["dX"], ref["dX"]), c.id)


def all_checks():
    out = []
    out += [(c.id, "c0b", (lambda rep, mu, c=c: check_c0b(rep, c, mu))) for c in B.c0b_cases()]
    out += [("c0w-" + c.id, "c0w", (lambda rep, mu, c=c: check_c0w(rep, c, mu))) for c in B.c0w_cases()]
    out += [(c.id, "rows", (lambda rep, mu, c=c: check_rows(rep, c, mu))) for c in B.row_cases()]
    out += [(c.id, "adj", (lambda rep, mu, c=c: check_adj(rep, c, mu))) for c in B.adj_cases()]
    out += [(c.id, "pw", (lambda rep, mu, c=c: check_pw(rep, c, mu))) for c in B.pw_cases()]
    out += [(c.id, "cl", (lambda rep, mu, c=c: check_cl(rep, c, mu))) for c in B.cl_cases()]
    return out


def run(cases=None, quiet=False, mutants=True):
    """-> (table: case id -> worst emulation err / bound (0 / inf for a bitwise case), failures).  cases None: every case."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    checks = all_checks()
    known = [cid for cid, _, _ in checks]
    assert len(set(known)) == len(known), "duplicate case ids"
    ids = known if cases is None else list(cases)
    rep = Report(quiet)
    for i in ids:
        if i not in known:
            rep.fail(i, "no such case")
    groups = set()
    for cid, g, fn in checks:
        if cid in ids:
            groups.add(g)
            fn(rep, mutants)
    if mutants:
        for key in sorted((g, m) for g in groups if g in MUTANTS for m in MUTANTS[g]):
            m, where = rep.margins.get(key, (0.0, None))
            if not quiet:
                print(f"mutant {key[0]:6s} {key[1]:24s} worst err/bound {m:10.3g} on {where}")
            if not m > 1:
                rep.fail(key[0], f"mutant {key[1]} stays inside the bound (or keeps the bits) of every case of its group", m)
    red = {g for cid, g, _ in checks if cid in REDUCED}
    if red != {g for _, g, _ in checks}:
        rep.fail("REDUCED", "groups not covered", sorted({g for _, g, _ in checks} - red))
    if not quiet:
        print(f"{len(rep.table)} cases, {len(rep.failures)} failures")
        for f in rep.failures:
            print("FAIL", f)
    return rep.table, rep.failures


if __name__ == "__main__":
    _, failures = run(REDUCED if "--reduced" in sys.argv else None)
    sys.exit(1 if failures else 0)

#!/usr/bin/env python3
"""CPU only: the self-check of tests/front_kernels_ref.py, the fp64 statements and derived bounds behind tests/test_front_kernels_parity_gpu.py.

For every case:  (a) the statement is well-posed: reference and bound finite; in the exact-integer cases every term is a multiple of one quantum and no partial sum
                     reaches 2^24 quanta, the hi + lo splits are exact and the lo part the case is about is not zero; the derived relative bound on the GroupNorm scale
                     stays below GN_REL_CAP; the positional-conv statement equals torch's conv1d(padding = Kw // 2)[..., :Tp];
                 (b) a torch fp32 / bf16 emulation of a CORRECT kernel's arithmetic (summation orders "seq" and "pair64") reproduces the exact cases bit for bit and stays
                     within HALF the non-store part of the bound in the bounded ones: the figure printed is (|err| - store term) / (bound - store term), the store term
                     being the one rounding (or the packed-half GELU constant) that the emulation performs too;
                 (c) every mutant leaves its bound or fails its bitwise comparison in the group it targets;
                 (d) the REDUCED list (what tests/test_front_kernel_bounds_cpu.py runs) covers every group and every mutant.

    python tools/front_kernel_bounds.py            # every case, then the failures (none expected)
    python tools/front_kernel_bounds.py --reduced"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import front_kernels_ref as K   # noqa: E402
import row_kernels_ref as R   # noqa: E402

F64, F32, BF, U = R.F64, R.F32, R.BF, R.U

MUTANTS = {"gn": ("var_T0m1", "eps_outside", "next_channel", "unpadded_len"), "c0": ("shift_dropped", "next_channel", "frame_T0_live", "ln_512"),
           "c0x": ("x_lo_dropped", "w_lo_dropped"), "pcx": ("product_dropped", "tap_shift", "valid_plus1", "valid_minus1", "neighbour_group", "chunk_no_halo"),
           "e2e": ("product_dropped", "tap_shift", "valid_minus1", "neighbour_group", "bias_after_gelu", "residual_unmasked"),
           "finish": ("bias_after_gelu", "residual_unmasked"), "patchify": ("gyx_swapped",), "embed": ("cls_pos1",)}

REDUCED = ("gn-T1-C16", "gn-T17-C264-ld", "gn-T4097-C16", "c0-mfma-m0-C64-T49-P64", "c0-mfma-m1-C128-T64-P128", "c0-mfma-m2-C192-T49-P64", "c0-mfma-m2-C64-T570-P576",
           "c0-valu-m0-C72-T100-P128", "c0-valu-m1-C8-T49-P64", "c0x-mfma-xlo-C128-T49-P64-bias", "c0x-mfma-wlo-C128-T49-P64", "c0x-valu-xlo-C72-T49-P70", "c0x-valu-wlo-C72-T49-P70-bias",
           "pcx-cg32-Kw2-Tp70-v1_99", "pcx-cg48-Kw4-Tp582-v255_256", "pcx-cg64-Kw3-Tp812-v511_512", "pcx-cg32-Kw16-Tp582-v257_582", "posconv-64-4-16-Tp30", "posconv-272-4-6-Tp33",
           "finish-D80-G4-ln-bf16", "finish-D192-G4-f32", "finish-D1020-G51-ln-f32", "finish-D1024-G16-bf16", "patchify", "pack", "embed-D260-ntok5", "embed-D1024-ntok10",
           "normalize", "crop")


class Report:
    def __init__(self, quiet):
        self.quiet, self.table, self.failures, self.margins = quiet, {}, [], {}

    def case(self, cid, emul, note="", limit=0.5):
        self.table[cid] = emul
        if not self.quiet:
            print(f"{cid:48s} emulation worst err/bound {emul:8.4f} {note}")
        if not emul <= limit:
            self.failures.append((cid, f"emulation above {limit} of the bound", emul))

    def fail(self, cid, what, value=None):
        self.failures.append((cid, what, value))

    def mutant(self, group, name, ratio):
        key = (group, name)
        self.margins[key] = max(self.margins.get(key, 0.0), ratio)


def finite(rep, cid, *ts):
    if not all(bool(torch.isfinite(t).all()) for t in ts):
        rep.fail(cid, "reference or bound not finite")


def ratio(a, b, bound, store=None):
    if store is None:
        return R.worst((a - b).abs(), bound)[0]
    return R.worst(((a - b).abs() - store).clamp_min(0), bound - store)[0]


def differs(a, b):
    """a mutant's margin in a bitwise comparison: inf when the bits differ"""
    return 0.0 if torch.equal(a, b) else float("inf")


# ------------------------------------------------------------------------------------------------ conv0 coefficients
def check_gn(rep, c, mutants):
    x, w, gamma, beta, offs = K.gn_inputs(c)
    ref = K.gn_ref(x, w, gamma, beta, c.T0)
    finite(rep, c.id, ref["scale"], ref["shift"], ref["b_scale"], ref["b_shift"])
    if not float(ref["rel"].max()) < K.GN_REL_CAP:
        rep.fail(c.id, "the derived relative bound on scale is above the cap", float(ref["rel"].max()))
    if not (bool((ref["var"][4] == 0).all()) and torch.allclose(ref["scale"][4], gamma / K.EPS ** 0.5, rtol=1e-14)):
        rep.fail(c.id, "the silent utterance's statement is not gamma / sqrt(eps)")
    worst = 0.0
    for order in R.ORDERS:
        sc, sh = K.gn_emulate(x, w, gamma, beta, c.T0, order)
        worst = max(worst, ratio(sc, ref["scale"], ref["b_scale"], U * ref["scale"].abs()), ratio(sh, ref["shift"], ref["b_shift"], U * ref["shift"].abs()))
    rep.case(c.id, worst, f"offsets {offs[1]:g} / {offs[2]:g} sd, worst bound on scale {float(ref['rel'].max()):.2e}")
    if mutants:
        for m in MUTANTS["gn"]:
            if m == "var_T0m1" and c.T0 == 1:
                continue
            mr = K.gn_ref(x, w, gamma, beta, c.T0, mutant=m)
            rep.mutant("gn", m, max(ratio(rnd32(mr["scale"]), ref["scale"], ref["b_scale"]), ratio(rnd32(mr["shift"]), ref["shift"], ref["b_shift"])))


def rnd32(t):
    return t.to(F32).to(F64)


# ------------------------------------------------------------------------------------------------ conv0 forward
def c0_store(c, ref):
    if c.mode == 1 or c.form == "valu":
        return R.BF_STORE * ref.abs()
    return R.GELU_POLY2_ABS + R.GELU_POLY2_REL * ref.abs()


def check_c0(rep, c, mutants):
    x, w, p = K.c0_inputs(c)
    ref, bound = K.c0_ref(c, x, w, p)
    finite(rep, c.id, ref, bound)
    if c.P > c.T0 and not (bool((ref[:, c.T0:] == 0).all()) and bool((bound[:, c.T0:] == 0).all())):
        rep.fail(c.id, "frames [T0, P) are not stated as exactly zero")
    if c.mode == 0 and not torch.allclose(ref[2, :c.T0], R.gelu64(p["shift"][2]).expand(c.T0, -1), rtol=1e-12, atol=1e-300):
        rep.fail(c.id, "the silent utterance's forward is not gelu(shift)")
    rep.case(c.id, max(ratio(K.c0_emulate(c, x, w, p, o), ref, bound, c0_store(c, ref)) for o in R.ORDERS))
    if mutants:
        for m in MUTANTS["c0"]:
            if m == "ln_512" and not (c.mode == 2 and c.C < 512):
                continue
            if (m == "next_channel" and c.mode != 0) or (m == "frame_T0_live" and c.P == c.T0) or (m == "shift_dropped" and c.mode != 0 and p["bias"] is None):
                continue
            rep.mutant("c0", m, ratio(K.bits(K.c0_ref(c, x, w, p, mutant=m)[0]), ref, bound))


def check_c0x(rep, c, mutants):
    x, w, bias, cond = K.c0x_inputs(c)
    q = cond["quantum"]
    fr = K.frames(x, c.T0)
    prods = fr.unsqueeze(2) * w.view(1, 1, c.C, K.CK)
    if not (cond["worst"] < 2 ** 24 and bool((prods / q == (prods / q).round()).all()) and (bias is None or bool((bias / q == (bias / q).round()).all()))):
        rep.fail(c.id, "a partial sum may reach 2^24 quanta, or a term is no multiple of the quantum", cond)
    xh, xl = K._split_bf(x.to(F32))
    wh, wl = K._split_bf(w.to(F32))
    if not (torch.equal((xh + xl).to(F64), x) and torch.equal((wh + wl).to(F64), w) and bool(((xl != 0).any() and not (wl != 0).any()) if c.kind == "xlo" else ((wl != 0).any() and not (xl != 0).any()))):
        rep.fail(c.id, "hi + lo is not exact, or the wrong lo part is zero")
    if bias is not None:
        bh, bl = K._split_bf(bias.to(F32))
        if not torch.equal((bh + bl).to(F64), bias):
            rep.fail(c.id, "the bias does not split exactly")
    want = K.c0x_ref(c, x, w, bias)
    cc = K.C0Case(c.id, c.form, 1, c.C, c.T0, c.P, 0, 0, c.bias)
    ok = all(torch.equal(K.c0_emulate(cc, x, w, dict(bias=bias), o), want) for o in R.ORDERS)
    rep.case(c.id, 0.0 if ok else float("inf"), "(bitwise)")
    if mutants and c.form == "mfma":
        for m, drop in (("x_lo_dropped", "x_lo"), ("w_lo_dropped", "w_lo")):
            if (drop == "x_lo") == (c.kind == "xlo"):
                rep.mutant("c0x", m, differs(K.c0_emulate(cc, x, w, dict(bias=bias), "seq", drop=drop), want))


# ------------------------------------------------------------------------------------------------ positional conv
def check_pcx(rep, c, mutants):
    D = c.G * c.cg
    x, wg = K.pcx_inputs(c)
    out, mag = K.pc_conv64(x, c.valid, wg, c.B, c.Tp, D, c.G, c.Kw)
    if not float(mag.max()) < 2 ** 24:
        rep.fail(c.id, "a partial sum may reach 2^24", float(mag.max()))
    path = K.pc_path(c)
    if c.Tp * c.Kw <= 4096:      # the statement is torch's own conv1d
        xm = x.view(c.B, c.Tp, D).clone()
        for b, n in enumerate(c.valid):
            xm[b, min(n, c.Tp):] = 0
        wt = wg.view(c.G, c.cg, c.Kw, c.cg).permute(0, 1, 3, 2).reshape(D, c.cg, c.Kw)
        t = F.conv1d(xm.transpose(1, 2), wt, padding=c.Kw // 2, groups=c.G)[..., :c.Tp]
        if not torch.equal(t.view(c.B, c.G, c.cg, c.Tp).transpose(2, 3), out):
            rep.fail(c.id, "the statement differs from conv1d(padding = Kw // 2)[..., :Tp]")
    want = K.bits(out)
    em = K.pc_conv64(x.to(F32), c.valid, wg.to(F32), c.B, c.Tp, D, c.G, c.Kw)[0]        # fp32 throughout; integers below 2^24: any order gives these bits
    rep.case(c.id, 0.0 if torch.equal(em.to(BF).to(F64), want) else float("inf"), f"(bitwise) NJ {path['NJ']} NW {path['NW']} nk {path['nk']} chunks {path['chunks']}" if c.cg in (32, 48, 64) else "(bitwise) pack + GEMM route")
    if mutants:
        for m in MUTANTS["pcx"]:
            if (m == "chunk_no_halo" and (path["chunks"] == 1 or c.Kw < 2)) or (m == "tap_shift" and c.Kw < 1):
                continue
            if m in ("valid_plus1", "valid_minus1") and all(n == 0 or n >= c.Tp for n in c.valid):
                continue
            rep.mutant("pcx", m, differs(K.bits(K.pc_conv64(x, c.valid, wg, c.B, c.Tp, D, c.G, c.Kw, m, chunk=64 * path["NW"])[0]), want))


def check_pf(rep, c, mutants):
    B, Tp = K.PF_B, K.PF_TP
    dt = F32 if c.f32 else BF
    x, cv, bias, gamma, beta = K.pf_inputs(c.id, B, Tp, c.D, c.G, c.affine)
    ref, bound = K.pf_ref(x, K.PF_VALID, cv, bias, gamma, beta, B, Tp, c.D, c.G, dt)
    finite(rep, c.id, ref, bound)
    store = R.store_bound(ref, dt)
    rep.case(c.id, max(ratio(K.pf_emulate(x, K.PF_VALID, cv, bias, gamma, beta, B, Tp, c.D, c.G, dt, o), ref, bound, store) for o in R.ORDERS))
    if mutants:
        for m in MUTANTS["finish"]:
            rep.mutant("finish", m, ratio(K.pf_ref(x, K.PF_VALID, cv, bias, gamma, beta, B, Tp, c.D, c.G, dt, mutant=m)[0].to(dt).to(F64), ref, bound))


def check_e2e(rep, c, mutants):
    x, wg, bias, gamma, beta = K.e2e_inputs(c)
    ref, bound = K.e2e_ref(c, x, wg, bias, gamma, beta)
    finite(rep, c.id, ref, bound)
    cg = c.D // c.G
    worst = 0.0
    for order in R.ORDERS:      # the slab as an fp32 sum of the products in `order`, stored as bf16
        cv64, _ = K.pc_conv64(x, c.valid, wg, 2, c.Tp, c.D, c.G, c.Kw)
        xm = x.view(2, c.Tp, c.D).clone()
        for b, n in enumerate(c.valid):
            xm[b, min(n, c.Tp):] = 0
        win = F.pad(xm.view(2, c.Tp, c.G, cg).permute(0, 2, 1, 3), (0, 0, c.Kw // 2, c.Kw)).unfold(2, c.Kw, 1)[:, :, :c.Tp].to(F32)      # [B, G, Tp, cg, Kw]
        terms = win.permute(0, 1, 2, 4, 3).reshape(2, c.G, c.Tp, 1, c.Kw * cg) * wg.to(F32).view(1, c.G, 1, cg, c.Kw * cg)
        slab = R.fsum(terms.contiguous(), order).to(BF).to(F64)
        worst = max(worst, ratio(K.pf_emulate(x, c.valid, slab, bias, gamma, beta, 2, c.Tp, c.D, c.G, BF, order), ref, bound, R.store_bound(ref, BF)))
    rep.case(c.id, worst)
    if mutants:
        for m in MUTANTS["e2e"]:
            if m == "valid_minus1" and all(n == 0 for n in c.valid):
                continue
            rep.mutant("e2e", m, ratio(K.bits(K.e2e_ref(c, x, wg, bias, gamma, beta, mutant=m)[0]), ref, bound))


# ------------------------------------------------------------------------------------------------ the copies, the ViT stem, the image
def check_patchify(rep, mutants):
    ok = True
    for p, Rr, Kpad in K.PT_CASES:
        img = K.pt_inputs(p, Rr)
        ok &= torch.equal(rnd32(img), img) and img.unique().numel() == img.numel() and bool((K.bits(img) != img).any())
        want = K.pt_ref(img, p, Kpad)
        g = Rr // p      # the statement is the stride = patch convolution's im2col
        unf = F.unfold(img, p, stride=p).transpose(1, 2).reshape(2 * g * g, 3 * p * p)
        ok &= torch.equal(K.bits(unf), want[:, :3 * p * p]) and bool((want[:, 3 * p * p:] == 0).all())
        if mutants:
            rep.mutant("patchify", "gyx_swapped", differs(K.pt_ref(img, p, Kpad, "gyx_swapped"), want))
    rep.case("patchify", 0.0 if ok else float("inf"), "(bitwise)")


def check_pack(rep, mutants):
    ok = True
    for D, G, Kw, Tp, valid in K.PACK_CASES:
        x = R.rnd(torch.randn(2 * Tp, D, generator=R.gen("pack", D), dtype=F64), BF)
        xg = K.pack_ref(x, valid, 2, Tp, D, G, Kw)
        ok &= xg.shape == (2, G, Tp + Kw, D // G) and bool((xg[:, :, :Kw // 2] == 0).all()) and bool((xg[:, :, Kw // 2 + Tp:] == 0).all())
        for b, n in enumerate(valid):
            n = min(n, Tp)
            ok &= torch.equal(xg[b, :, Kw // 2:Kw // 2 + n].permute(1, 0, 2).reshape(n, D), x.view(2, Tp, D)[b, :n]) and bool((xg[b, :, Kw // 2 + n:] == 0).all())
    rep.case("pack", 0.0 if ok else float("inf"), "(bitwise)")


def check_embed(rep, D, ntok, mutants):
    cid = f"embed-D{D}-ntok{ntok}"
    patch, cls, pos, gamma, beta = K.ve_inputs(D, ntok)
    ref, bound = K.ve_ref(patch, cls, pos, gamma, beta, ntok)
    finite(rep, cid, ref, bound)
    rep.case(cid, max(ratio(K.ve_emulate(patch, cls, pos, gamma, beta, ntok, o), ref, bound, U * ref.abs()) for o in R.ORDERS))
    if mutants:
        rep.mutant("embed", "cls_pos1", ratio(rnd32(K.ve_ref(patch, cls, pos, gamma, beta, ntok, mutant="cls_pos1")[0]), ref, bound))


def check_normalize(rep, mutants):
    u8 = K.in_inputs()
    if not all(u8[b, :, :, ch].unique().numel() == 256 for b in range(2) for ch in range(3)):
        rep.fail("normalize", "not every byte value in every channel of every image")
    worst = 0.0
    for mean, std in K.IN_STATS:
        ref, bound = K.in_ref(u8, mean, std)
        finite(rep, "normalize", ref, bound)
        worst = max(worst, ratio(K.in_emulate(u8, mean, std), ref, bound))
    rep.case("normalize", worst)


def check_crop(rep, mutants):
    c = K.CROP
    ok = c["ld"] > c["Lout"] and c["Lout"] % 256 != 0 and 0 in c["lens"] and any(s + n == c["ld"] for s, n in zip(c["starts"], c["lens"])) \
        and all(s + n <= c["ld"] and n <= c["Lout"] for s, n in zip(c["starts"], c["lens"]))
    rep.case("crop", 0.0 if ok else float("inf"), "(bitwise)")


def all_checks():
    """[(case id, group, callable(rep, mutants))]"""
    out = []
    out += [(c.id, "gn", (lambda rep, mu, c=c: check_gn(rep, c, mu))) for c in K.gn_cases()]
    out += [(c.id, "c0", (lambda rep, mu, c=c: check_c0(rep, c, mu))) for c in K.c0_cases()]
    out += [(c.id, "c0x", (lambda rep, mu, c=c: check_c0x(rep, c, mu))) for c in K.c0x_cases()]
    out += [(c.id, "pcx", (lambda rep, mu, c=c: check_pcx(rep, c, mu))) for c in K.pcx_cases()]
    out += [(c.id, "pcx", (lambda rep, mu, c=c: check_pcx(rep, c, False))) for c in K.pcx_pack_cases()]
    out += [(c.id, "e2e", (lambda rep, mu, c=c: check_e2e(rep, c, mu))) for c in K.E2E]
    out += [(c.id, "finish", (lambda rep, mu, c=c: check_pf(rep, c, mu))) for c in K.pf_cases()]
    out += [("patchify", "patchify", check_patchify), ("pack", "pack", check_pack), ("normalize", "normalize", check_normalize), ("crop", "crop", check_crop)]
    out += [(f"embed-D{D}-ntok{n}", "embed", (lambda rep, mu, D=D, n=n: check_embed(rep, D, n, mu))) for D in K.VE_D for n in K.VE_NTOK]
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
            m = rep.margins.get(key, 0.0)
            if not quiet:
                print(f"mutant {key[0]:10s} {key[1]:20s} worst err/bound {m:10.3g}")
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

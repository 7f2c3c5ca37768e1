"""CPU: the self-check of tools/tail_kernel_bounds.py on its reduced case list -- the fp64 statements of tests/tail_kernels_ref.py are well-posed (finite, no output
whose rms is below 10x its mean bound), a torch fp32 emulation of each kernel's arithmetic (two summation orders) stays within half the fp32 part of its bound, and every
mutant of every group leaves the bound on a case the tool names.  Then: the case lists hold every shape and path the kernels branch on, and the three host-side
dispatchers (sc_sgemm's split-K rule, sc_colsum's chunk rule, sc_grad_norm's block rule), restated in the reference module, select the path each case is named for.
Keeps the bounds and the mutants honest when someone edits the inputs."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("tail_kernel_bounds", os.path.join(ROOT, "tools", "tail_kernel_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tail_kernel_bounds_self_check_reduced_cases():
    import tail_kernels_ref as T
    tool = _tool()
    ids = tool.reduced_ids()
    table, failures, margins = tool.run(ids, quiet=True)
    assert sorted(table) == sorted(ids)
    assert not failures, failures
    assert all(0 <= v <= 0.5 for v in table.values()), table
    for G in T.GROUPS.values():
        for m in G.mutants:
            margin, cid = margins[(G.name, m)]
            assert margin > 1 and cid in ids, (G.name, m, margin, cid)


def test_case_lists_hold_the_required_shapes_and_paths():
    import tail_kernels_ref as T
    # sc_sgemm / sc_sgemm_batched
    gm = T.gemm_cases()
    assert {(c.ta, c.tb) for c in gm} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c.M for c in gm} >= set(T.GEMM_MN) and {c.N for c in gm} >= set(T.GEMM_MN)
    for t in {(c.ta, c.tb) for c in gm}:
        assert {c.K for c in gm if (c.ta, c.tb) == t} >= set(T.GEMM_K), t
    assert {c.batch for c in gm} == {1, 3} and {c.layout for c in gm} == set(T.GEMM_LAYOUTS) and any(c.ldc_pad for c in gm)
    split = lambda c: T.gemm_split(c.M, c.N, c.K, c.batch)      # noqa: E731
    for c in gm:
        assert (split(c)[0] > 1) == (c.K >= 2048), c.id                      # every case has fewer than 128 tiles: the K threshold alone decides
        assert (T.gemm_ld(c, 7) % 4 != 0) == (c.layout == "ldodd") and (T.gemm_ld(c, 8) % 4 != 0) == (c.layout == "ldodd")
    assert split(gm[0]._replace(M=130, N=130, K=2047, batch=1)) == (1, 2048) and T.gemm_split(1024, 1024, 4096, 1)[0] == 1     # below the K threshold; 256 tiles
    k2050 = [c for c in gm if c.K == 2050]
    assert all(split(c) == (8, 272) and c.K - 7 * 272 == 146 for c in k2050)                                                   # the last slice: 146, not a multiple of 4
    assert any(c.batch == 3 and c.bias for c in k2050)
    for abi in T.GEMM_AB:
        for sp in (False, True):
            assert any((c.alpha, c.beta, c.bias) == abi and (split(c)[0] > 1) == sp for c in gm), (abi, sp)
    assert any(c.batch == 3 and split(c)[0] > 1 and c.layout == "off1" for c in gm)
    # sc_colsum
    cs = T.cs_cases()
    assert {(c.rows, c.cols, c.ld) for c in cs} == set(T.CS_SHAPES) and {c.acc for c in cs} == {0, 1}
    chunks = {s: T.cs_chunks(s[0], s[1])[0] for s in T.CS_SHAPES}
    assert chunks[(1, 1, 1)] == 1 and chunks[(255, 65, 65)] == 1 and chunks[(256, 65, 72)] == 4 and chunks[(257, 64, 64)] == 5
    assert chunks[(1000, 130, 130)] == 16 and chunks[(256, 32704, 32704)] == 2 and chunks[(256, 32768, 32768)] == 1               # either side of cb < 512
    # sc_grad_norm
    gn = T.gn_cases()
    assert {c.n for c in gn} == set(T.GN_N) and {c.max_norm for c in gn if not c.small} == set(T.GN_MAX)
    assert [T.gn_blocks(n) for n in (1, 255, 256, 262143, 262144, 262145, 1000003)] == [(1, "single"), (1, "single"), (2, "single"), (1024, "single"),
                                                                                      (1024, "stride"), (1024, "stride"), (1024, "stride")]
    # sc_adam_step
    ad = T.adam_cases()
    assert {(c.n, c.step, c.wd, c.clip) for c in ad} == {(n, t, w, k) for n in T.ADAM_N for t in T.ADAM_STEPS for w in T.ADAM_WD for k in (False, True)}
    # sc_layernorm_bwd
    lb = T.lb_cases()
    assert {c.D for c in lb} == set(T.LB_D) and all(c.rows == T.LB_ROWS for c in lb)
    assert {(c.acc, c.params) for c in lb} == {(a, b) for a in (False, True) for b in (False, True)}
    for D in T.LB_D:
        assert {c.acc for c in lb if c.D == D} == {False, True} and {c.params for c in lb if c.D == D} == {False, True}
    # activations and the small row kernels
    act = T.act_cases()
    assert {c.kind for c in act} == set(T.ACT_KINDS) and {c.n for c in act} >= set(T.ACT_N)
    z = T.act_grid()
    assert float(z.min()) == -12 and float(z.max()) == 12 and bool((z == 0).sum() >= 3) and bool(((z == 0) & torch.signbit(z)).any())
    ties = z[z > 10.5]
    assert bool(((ties.float().view(torch.int32) & 0xffff) == 0x8000).any())                                                # exactly half way between two bf16 numbers
    for name, dims in (("l2bwd", T.SM_D), ("cosfin", T.SM_D), ("addrows", T.SM_D), ("hilo", T.SM_D)):
        cases = T.GROUPS[name].cases()
        assert {c.D for c in cases} == set(dims) and {c.rows for c in cases} == set(T.SM_ROWS), name
    assert {c.opt for c in T.add_cases()} == {False, True}
    hl = T.hilo_cases()
    assert {c.opt[0] for c in hl} == {2, 3} and {nb for c in hl for nb in [c.opt[0]] if c.opt[1] > c.D} == {2, 3}
    mx = T.mix_cases()
    assert {(c.D, c.rows) for c in mx} == {(n, B) for n in T.MIX_N for B in T.MIX_B}
    w = T.mix_inputs(mx[-1])["w"]
    assert float(w.max() - w.min()) == 20.0
    # the cascaded tail
    assert {(c.B, c.K, c.E) for c in T.kb_cases()} == set(T.KB_SHAPES) and {c.running for c in T.kb_cases()} == {True, False}
    vq = T.vq_cases()
    assert {(c.R, c.V, c.temp, c.nmask) for c in vq} == {(R, V, t, m) for (R, V) in T.VQ_SHAPES for t in T.VQ_TEMPS for m in T.VQ_NMASK}
    assert all(c.nmask == 0 or {0, c.V - 1} <= set(T.vq_mask_ids(c)) for c in vq)
    at = T.at_cases()
    assert {(c.B, c.L, c.H, c.causal, c.scale) for c in at} == {(B, L, H, ca, s) for (B, L, H) in T.AT_SHAPES for ca in (True, False) for s in T.AT_SCALES}
    c = [k for k in at if k.L == 7 and k.causal][0]
    inp = T.at_inputs(c)
    m = T._at_manual(c, inp)
    assert torch.allclose(T._at_pack(c, m["dq"], m["dk"], m["dv"]), T.at_autograd(c, inp), rtol=1e-11, atol=1e-300)          # the mutants' hand-written backward IS the autograd statement
    # the loss
    nce = T.nce_cases()
    assert {(c.Bg, c.E) for c in nce} == {(b, e) for b in T.NCE_BG for e in T.NCE_E} | {(2048, 64)}
    assert {round(c.inv_t, 6) for c in nce} == {round(v, 6) for v in T.NCE_INVT} and {c.ids for c in nce} == set(T.NCE_KINDS)
    assert {c.margin for c in nce} == {0.0, 0.2} and {c.dcl for c in nce} == {False, True} and {(c.a2b, c.b2a) for c in nce} == set(T.NCE_DIRS)
    main = [c for c in nce if 2 < c.Bg < 2048]                                                                                # (the rotation, clear of the forced dcl of tiny batches)
    for E in T.NCE_E:                                                                                                          # no option moves with another
        assert len({(round(c.inv_t, 6), c.margin) for c in main if c.E == E}) == 4, E
    for kind in T.NCE_KINDS:
        assert {c.margin for c in main if c.ids == kind} == {0.0, 0.2} and len({round(c.inv_t, 6) for c in main if c.ids == kind}) == 2, kind
        if kind != "allsame":
            assert {c.dcl for c in main if c.ids == kind} == {False, True}, kind
    for E in T.NCE_E:
        assert {c.ids for c in nce if c.E == E} == set(T.NCE_KINDS) and {c.dcl for c in main if c.E == E and c.ids != "allsame"} == {False, True}, E
    assert any(c.ids == "dup" and c.dcl and 65 < c.Bg < 2048 for c in nce) and any(c.ids == "none" and c.dcl and c.Bg > 2 for c in nce)
    assert {(c.margin, c.dcl) for c in main} == {(m, d) for m in (0.0, 0.2) for d in (False, True)} and {(c.a2b, c.b2a) for c in main if c.E in (4, 20)} == set(T.NCE_DIRS)
    assert all(not c.dcl and c.zero for c in nce if c.ids == "allsame") and any(c.ids == "dup" and c.Bg > 65 for c in nce)
    for c in nce:
        if c.ids == "dup" and c.Bg > 65:
            ids = T.nce_ids(c)
            assert int(ids[63]) == int(ids[64]) == int(ids[65]) and int(ids.min()) >= 2 ** 32
        if c.ids == "unique":
            ids = T.nce_ids(c)
            assert len(set(ids.tolist())) == c.Bg and (c.Bg < 2 or len(set((ids & 0xffffffff).tolist())) < c.Bg)


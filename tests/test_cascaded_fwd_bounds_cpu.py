"""CPU: the self-check of tools/cascaded_fwd_bounds.py on its reduced case list -- every statement of tests/cascaded_fwd_ref.py is well-posed (candidate sets, leads and
decisive arg-maxima hold on the inputs alone), a torch fp32 emulation of each kernel's arithmetic (two summation orders) stays within its limit of the fp32 part of every
bound, and every mutant of every group leaves the bound on a case the tool names.  Then: the case lists hold every shape and path the issue of record names, and the two
host dispatch rules restated in the reference module -- vq_nsplit and the `exact` rule of ops.cosine_scores -- select the path each case is named for (compared with the
real library and the real sources).  The argument rules that need no GPU are in tests/test_cascaded_fwd_host.py."""
import importlib.util
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("cascaded_fwd_bounds", os.path.join(ROOT, "tools", "cascaded_fwd_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cascaded_fwd_bounds_self_check_reduced_cases():
    import cascaded_fwd_ref as C
    tool = _tool()
    ids = tool.reduced_ids()
    table, failures, margins, three = tool.run(ids, quiet=True)
    assert sorted(table) == sorted(ids)
    assert not failures, failures
    assert all(0 <= v <= 1.0 for v in table.values()), table
    for G in C.GROUPS.values():
        for m in G.mutants:
            margin, cid = margins[(G.name, m)]
            assert margin > 1 and cid in ids, (G.name, m, margin, cid)
    assert set(three) == {c.id for c in C.ch_cases() if c.id in ids}


def test_the_parent_refine_kernel_is_rejected_for_the_stated_reasons():
    """the kernel before the mask / cap fixes IS two of the mutants: its maximum ran over the masked columns too (every -lead case: no unmasked entry refined) and it kept at
    most 128 candidates (every case with more: the rest unrefined).  Each must leave the bound exactly on those cases and on no other."""
    import cascaded_fwd_ref as C
    for c in C.rf_cases():
        if c.R == 0 or c.id == "refine/V1031-E512-all":
            continue
        inp = C.rf_inputs(c)
        ref, b = C.rf_ref(c, inp)["out"], C.rf_bound(c, inp)["out"].bound
        um = C.unmasked(c.V, c.mask)
        ncand = int(um.sum()) if c.ncand is None else c.ncand
        for mutant, hit in (("max_over_masked", c.lead), ("first_128_by_index", ncand > C.MAXCAND)):
            wrong = C.rf_ref(c, inp, mutant)["out"]
            r = C.worst((wrong - ref).abs()[:, um], b[:, um])[0]
            assert (r > 1) == hit, (c.id, mutant, r)


def test_a_mutant_no_case_rejects_is_a_failure_of_the_tool(monkeypatch):
    import cascaded_fwd_ref as C
    tool = _tool()
    G = C.GROUPS["kwaffine"]
    monkeypatch.setitem(C.GROUPS, "kwaffine", G._replace(mutants=G.mutants + ("harmless",), ref=lambda c, inp, mutant=None: C.ka_ref(c, inp, None if mutant == "harmless" else mutant)))
    failures = tool.run([c.id for c in C.ka_cases()], quiet=True)[1]
    assert any("harmless" in f[1] for f in failures), failures


def test_case_lists_hold_the_required_shapes_and_paths():
    import cascaded_fwd_ref as C
    ka = C.ka_cases()
    assert {c.rows * c.D for c in ka} >= {1, 255, 256, 257} and {c.K for c in ka} == {1, 8} and any(c.rows % c.K for c in ka if c.K == 8)
    cs = C.cs_cases()
    for kind in ("real", "int"):
        assert {c.E for c in cs if c.kind == kind} == set(C.CS_E), kind
    assert {c.R for c in cs} == set(C.CS_SIZES) and {c.V for c in cs} == set(C.CS_SIZES)
    for c in cs:
        if c.kind == "real" and min(c.R, c.V) >= 5:
            inp = C.cs_inputs(c)
            for x in (inp["a"], inp["e"]):
                n = (x * x).sum(-1).sqrt()
                assert float(n[0]) == 0 and 0 < float(n[1]) < C.EPS and float(n[2:].max() / n[2:].min()) > 2.0 ** 38, c.id
    rf = C.rf_cases()
    assert {c.V for c in rf} == {5, 256, 257, 1031} and {c.E for c in rf} == {4, 64, 260, 512}
    assert {c.ncand for c in rf} >= {1, 2, 127, 128, 129, 300, None} and any(c.delta == 0 for c in rf) and any(c.R == 0 for c in rf)
    assert any(c.lead and c.ncand and c.ncand > C.MAXCAND for c in rf) and any(c.lead and c.mask == (0, 2, 3) for c in rf)
    ch = C.ch_cases()
    assert all(c.E % 64 == 0 and c.V % 4 == 0 for c in ch) and sum(c.V > 1031 for c in ch) == 0
    auto = [c for c in ch if c.exact is None]
    assert len(auto) == 1 and not C.exact_rule(auto[0].R, auto[0].V, auto[0].E) and C.exact_rule(auto[0].R - 16, auto[0].V, auto[0].E) and auto[0].E == 64
    assert all(C.exact_rule(c.R, c.V, c.E) for c in ch if c.exact is False)            # the small cases reach the MFMA path only because they ask for it
    vq = C.vq_cases()
    assert {c.V for c in vq} == {1, 7, 255, 256, 257, 1031, 49408} and {c.R for c in vq} >= {1, 63, 64, 65, 1024} and {c.K for c in vq} == {1, 8, 257}
    assert {len(c.mask) for c in vq} == {0, 3, 8} and [c.R for c in vq if c.V > 1031] == [8]
    assert any(0 in c.mask and c.V - 1 in c.mask for c in vq) and any(max(c.mask, default=0) >= c.V for c in vq)
    assert {C.vq_nsplit(c.R) for c in vq} == {1, 8, 32} and any(c.R % C.vq_nsplit(c.R) for c in vq if C.vq_nsplit(c.R) > 1)
    assert {c.E for c in C.gt_cases()} == {1, 255, 256, 257, 4} and any(c.R == 0 for c in C.gt_cases())
    rk = C.rk_cases()
    assert {c.m for c in rk} == {1, 63, 64, 65, 300} and {c.n for c in rk} == {1, 3, 4, 5} and any(c.ld > c.m for c in rk)
    tk = C.tk_cases()
    assert {c.V for c in tk} == {1, 255, 256, 257, 1031} and {1, 10} <= {c.K for c in tk} and any(c.K == c.V and c.V > 256 for c in tk) and any(c.ld > c.V for c in tk)
    pb = C.pb_cases()
    assert {c.hd for c in pb} == {8, 96, 1024} and {c.L for c in pb} == {1, 63, 64, 65, 130} and {0, 1, 5} <= {c.n_rows for c in pb} and any(c.n_rows == c.L > 1 for c in pb)
    assert {c.pad for c in pb} == {"none", "ragged", "full"} and any(c.ld_extra for c in pb) and any(c.peaked for c in pb)
    assert sum(c.V > 1031 for G in ("refine", "cosine", "topk", "chain", "vq") for c in C.GROUPS[G].cases()) == 1


def test_inputs_carry_the_edges_the_cases_are_named_for():
    import torch
    import cascaded_fwd_ref as C
    c = [k for k in C.vq_cases() if k.id == "vq/V255-R64-K8"][0]
    x, um = C.vq_inputs(c)["x"], C.unmasked(c.V, c.mask)
    assert bool((x[0::4][:, ~um].min(1).values > x[0::4][:, um].max(1).values).all())                 # a masked column holds the maximum
    mx = x[1::4][:, um].max(1, keepdim=True).values
    assert bool(((x[1::4][:, um] == mx).sum(1) == 2).all()) and bool((x[1::4][:, 0] == mx[:, 0]).all())     # an exact tie, and a masked column at the same value before it
    assert bool((x[2::4][:, um].max(1).values == 30).all()) and bool(torch.isinf(x[:, um]).any(0).sum() == 1)
    for c in C.rk_cases():
        inp = C.rk_inputs(c)
        if c.n >= 3:
            pos = inp["cand"][None, :] == inp["own"][:, None]
            assert not bool(pos[1].any()) and bool(((inp["cand"] & 0xffffffff) == (inp["own"][1] & 0xffffffff)).any()), c.id
            if c.m >= 63:
                assert int(pos.sum(1).max()) > 1, c.id
                r = C.rk_ref(c, inp)["rank"]
                assert any(C.rk_ref(c, inp, m)["rank"].ne(r).any() for m in C.RK_MUTANTS), c.id


def test_dispatch_rules_restated_match_the_sources():
    import cascaded_fwd_ref as C
    from speechclip_amd import ops
    from speechclip_amd.module.speechclip_c_modules.vector_quantizers import SimpleVectorQuantizer
    src = inspect.getsource(ops.cosine_scores)
    assert "exact = not (E % 64 == 0 and V % 4 == 0 and R * V >= (1 << 22))" in src and C.AUTO_THRESHOLD == 1 << 22
    assert abs(ops.COS_REFINE_DELTA - C.DELTA) < 1e-9
    kw = open(os.path.join(ROOT, "speechclip_amd", "model", "kwClip.py")).read()           # the two calls that feed the quantizer name its masked ids; the analysis calls are exact
    feeds = [m.start() for m in re.finditer(r"ops\.cosine_scores\(", kw)]
    assert len(feeds) == 4 and sum("mask_ids=(0, 2, 3)" in kw[i:i + 200] for i in feeds) == 2 and sum("exact=True" in kw[i:i + 200] for i in feeds) == 2
    assert all("vector_quantizer(x=cos" in kw[i:i + 400] for i in feeds if "mask_ids" in kw[i:i + 200])
    assert inspect.signature(SimpleVectorQuantizer.forward).parameters["prob_msk"].default == [0, 2, 3]
    hip = open(os.path.join(ROOT, "speechclip_amd", "csrc", "cascaded.hip")).read()
    assert "static int vq_nsplit(int R) { return R >= 1024 ? 32 : (R >= 64 ? 8 : 1); }" in hip
    assert re.search(r"constexpr int MAXCAND = (\d+);", hip).group(1) == str(C.MAXCAND)
    from speechclip_amd import _lib
    L = _lib.lib()
    for R_, V in ((1, 1), (63, 7), (64, 255), (65, 256), (1024, 7), (8, 49408)):
        assert L.sc_vq_workspace_bytes(R_, V) == 4 * C.vq_workspace_floats(R_, V), (R_, V)
        assert L.sc_cosine_workspace_bytes(R_, V) == 4 * (R_ + V)

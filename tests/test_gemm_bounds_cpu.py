"""CPU: the self-check of tools/gemm_bounds.py on its reduced case list -- the fp64 statements of tests/gemm_ref.py are well-posed, an fp32 emulation of every path
(two summation orders, the epilogue's rounding points) stays within half the fp32 part of its bound, inside the whole bound and inside both 6 / sqrt(n) statistics,
reproduces the bits of every exact case, `once` and `twice` part ways wherever a case claims to tell them apart, and every mutant is caught.  Then: the host's
dispatcher, restated in the reference module, sends every case of every list to the kernel (and the epilogue, tile order, band, K walk) its list names, and the lists
hold every shape the kernels branch on.  Keeps the bounds, the model and the mutants honest when someone edits the inputs or the dispatcher."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gemm_bounds", os.path.join(ROOT, "tools", "gemm_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gemm_bounds_self_check_reduced_cases():
    import gemm_ref as G
    tool = _tool()
    cases = tool.reduced_cases()
    rep = tool.run(cases, quiet=True)
    assert sorted(rep["table"]) == sorted(c.id for c in cases)
    assert not rep["failures"], rep["failures"]
    ids = {c.id for c in cases}
    assert all(0 <= v <= 0.5 for v in rep["table"].values())                                       # (err - store) / (bound - store) itself, not half of it
    for m in G.MUTANTS:
        (rm, rc), (em, ec) = rep["margins"][m]["real"], rep["margins"][m]["exact"]
        print(f"mutant {m:22s} applied to {rep['applied'][m]:4d} cases; real: err / bound {rm:.4g} on {rc}; exact: {em:.0f} differing elements on {ec}")
        assert (rm > 1 and rc in ids) or (em > 0 and ec in ids), (m, rep["margins"][m])
        if m == "once_for_twice":                          # inside the two store terms of a real case's bound by construction: the exact cases are what catches it
            assert em > 0 and not rm > 1, (m, rep["margins"][m])
        else:                                               # every other mutant leaves the bound of a real case AND breaks the bits of an exact one
            assert rm > 1 and (em > 0 or m in ("act_after_res",)), (m, rep["margins"][m])
    assert {p for c in cases for p in [c.path]} == set(G.PATHS)                                     # every path has its case
    assert {G.rounding_points(c) for c in cases if c.path in ("g256", "g8p_pers") and c.res and c.out == 16} == {"once", "twice"}
    assert any(s for (cid, _), s in rep["stats"].items()) and all(s1 <= lim and s2 <= lim for (_, s1, s2, lim) in rep["stats"].values())


def test_every_case_lands_on_the_path_its_list_names():
    import gemm_ref as G
    cases = G.all_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        d = G.dispatch(c)
        assert d["path"] == c.path, (c.id, d)
        assert d["last_path"] == (3 if c.path.startswith("g8p") else 0), (c.id, d)
        assert c.mode == {"g256": 0}.get(c.path, c.mode) and c.mode in (-1, 0, 16, 26), c.id
        if c.kind == "exact":
            assert c.act == 0 and not (c.out == 16 and c.res and c.K < 128), c.id
    for name, f in G.CASE_LISTS.items():
        want = {"bf128x64": {"bf128x64"}, "bf128x128": {"bf128x128"}, "f16": {"h128x64", "h128x128"}, "g256": {"g256"}, "g256_batch": {"g256_batch"},
                "batched128": {"bf128_batched"}, "g8p": {"g8p_pers"}}[name]
        assert {c.path for c in f()} == want, name
    # the refusals of sc_gemm8p_try and the thresholds of the dispatcher, on shapes next to the lists'
    base = G._c("t", "g8p_pers", 16, "real", 512, 512, 128)
    assert G.gemm8p_try(base, 16) == ("g8p_pers", "static", 0)
    for bad in (base._replace(N=520), base._replace(M=255), base._replace(K=64), base._replace(ldc=516), base._replace(res=True, ldr=516), base._replace(lda=132),
                base._replace(ldw=132), base._replace(N=8448), base._replace(N=8448, M=257), base._replace(N=8448, out=32), base._replace(N=8448, f16=True)):
        assert G.gemm8p_try(bad, 16) is None, bad
    assert G.gemm8p_try(base._replace(ldc=516, out=32), 16) is not None                            # fp32 rows need 16 bytes = 4 elements only
    assert G.gemm8p_try(base._replace(K=384, M=2048), 16)[1] == "dyn" and G.gemm8p_try(base._replace(K=384, M=2048), 26)[1] == "static"
    assert G.gemm8p_try(base._replace(K=320, M=2048), 16)[1] == "static" and G.gemm8p_try(base._replace(K=384, M=768), 16)[1] == "static"   # nk = 5; 6 blocks
    assert G.gemm8p_try(base._replace(N=4096), -1)[2] == 4 and G.gemm8p_try(base._replace(N=4096), 16)[2] == 0 and G.gemm8p_try(base._replace(N=3840), -1)[2] == 0
    dflt = base._replace(mode=-1, M=2125, N=4096)
    assert G.dispatch(dflt)["path"] == "g8p_pers" and G.dispatch(dflt._replace(M=1793))["path"] == "g8p_pers"  # 144 tiles; 8 x 16 = 128 tiles
    assert G.dispatch(dflt._replace(M=1792))["path"] == "g256"                                                  # 112 tiles: below 128, at least 100
    g = G._c("t", "g256", 0, "real", 2560, 2560, 128)
    assert G.dispatch(g)["path"] == "g256" and G.dispatch(g._replace(M=2304))["path"] == "bf128x128" and G.dispatch(g._replace(M=2305))["path"] == "g256"
    assert G.dispatch(g._replace(N=252, M=100000))["path"] == "bf128x128" and G.dispatch(g._replace(M=255, N=100000))["path"] == "bf128x128"
    assert G.dispatch(g._replace(lda=128, K=192))["kpair"] == 1 and G.dispatch(g._replace(lda=256, K=384))["kpair"] == 2 and G.dispatch(g._replace(lda=64, K=192))["kpair"] == 0
    b = G._c("t", "g256_batch", -1, "real", 300, 260, 64, api="batched", S=25, bias=False)
    assert G.dispatch(b)["path"] == "g256_batch" and G.dispatch(b._replace(S=24))["path"] == "bf128_batched" and G.dispatch(b._replace(bias=True))["path"] == "bf128_batched"
    assert G.dispatch(b._replace(act=1))["path"] == "bf128_batched" and G.dispatch(b._replace(M=255, S=100))["path"] == "bf128_batched"
    for bad, what in ((g._replace(K=96), "K"), (g._replace(N=2562), "N"), (g._replace(M=0), "M"), (g._replace(lda=132), "ld"),
                      (G._c("t", "bf128_batched", -1, "real", 70, 64, 64, api="batched2", S=256, inner=256, bias=False), "outer*inner")):
        assert G.arg_error(bad) == what, bad


def test_case_lists_hold_the_required_shapes():
    import gemm_ref as G
    L = {k: f() for k, f in G.CASE_LISTS.items()}
    kinds = lambda cs: {c.kind for c in cs}      # noqa: E731
    # the 128-row kernels: every N with every M, every K with every N and every M, both kinds on every (M, N)
    for name, Ns, Ms in (("bf128x64", G.N64, G.M128), ("bf128x128", G.N128, G.M128 + (257,))):
        cs = L[name]
        for N in Ns:
            for M in Ms:
                assert kinds(c for c in cs if (c.M, c.N) == (M, N)) == {"exact", "real"}, (name, M, N)
            assert {c.K for c in cs if c.N == N} >= set(G.K64), (name, N)
        for M in Ms:
            assert {c.K for c in cs if c.M == M} >= set(G.K64), (name, M)
        assert {(c.out, c.res) for c in cs} == {(o, r) for o in (16, 32) for r in (False, True)} and {c.act for c in cs} == {0, 1, 2}
        assert any(c.ldw > c.K for c in cs) and any(c.kind == "exact" and c.out == 16 and c.res for c in cs)
    assert any(c.also == "below100" and c.M >= 2304 and c.N >= 256 for c in L["bf128x128"]) and any(c.lda < c.K for c in L["bf128x128"])
    assert any(c.N == c.K and c.kind == "exact" for c in L["bf128x64"])
    f16 = L["f16"]
    assert all(c.f16 for c in f16) and {c.N for c in f16} >= set(G.N64) | set(G.N128) and {c.M for c in f16} >= {1, 129, 257}
    assert {c.act for c in f16} == {0, 1, 2} and {(c.out, c.res) for c in f16} == {(o, r) for o in (16, 32) for r in (False, True)} and any(c.ldw > c.K for c in f16)
    # gemm256_kernel
    g = L["g256"]
    assert all(-(-c.M // 256) * -(-c.N // 256) >= 100 for c in g)
    for M in (2560, 2561, 2815):
        assert {c.N for c in g if c.M == M} >= {2560, 2312, 2308}, M
    assert {c.K for c in g} >= {64, 128, 192, 448} and kinds(g) == {"exact", "real"}
    assert {G.epilogue256(c) for c in g} == {"vector", "f32", "scalar"}
    assert {G.epilogue256(c) for c in g if c.N == 2308 and c.out == 16} == {"scalar"} and any(G.epilogue256(c) == "scalar" and c.N % 8 == 0 for c in g)      # N % 8 == 4; ldc % 8 == 4
    assert any(G.fast_epilogue_runs(c) and c.kind == k for c in g for k in ("exact",)) and any(G.fast_epilogue_runs(c) and c.kind == "real" for c in g)
    assert any(c.K == 64 and G.epilogue256(c) == "vector" for c in g)                                  # nk = 1: the fast epilogue is refused
    assert any(G.dispatch(c)["band"] == 4 for c in g) and {G.dispatch(c)["kpair"] for c in g} == {0, 1, 2}
    assert any(c.lda == 64 and c.K == 192 for c in g) and any(c.lda > c.K for c in g) and any(c.ldw > c.K for c in g)
    assert any(c.ldc == c.N + 8 for c in g) and any(c.ldc == c.N + 4 for c in g) and any(c.res and c.ldr != c.ldc for c in g)
    assert {G.rounding_points(c) for c in g if c.kind == "exact" and c.out == 16 and c.res} == {"once", "twice"}
    assert any(c.res and -(-c.M // 256) * -(-c.N // 256) > G.N_CU for c in g)                           # a residual epilogue with a next tile behind it
    assert {c.act for c in g} == {0, 1, 2}
    bt = L["g256_batch"]
    assert all((c.S, c.M, c.N) == (25, 300, 260) for c in bt) and {c.K for c in bt} == {64, 192} and {c.w_mod for c in bt} == {1, 25} and {c.out for c in bt} == {16, 32}
    assert all(G.layout(c)["strideC"] > c.M * c.ldc for c in bt) and kinds(bt) == {"exact", "real"}
    sm = L["batched128"]
    b1 = [c for c in sm if c.api == "batched"]
    assert {c.S for c in b1} == {1, 3} and {c.w_mod for c in b1} == {1, 2} and all(c.bias for c in b1) and {c.N for c in b1} == {64, 132}
    b2 = [c for c in sm if c.api == "batched2"]
    assert {c.inner for c in b2} == {1, 4} and all((c.M, c.N) == (70, 64) for c in b2) and all(c.ldc > c.inner * c.N and c.lda == c.inner * c.K for c in b2)
    # gemm8p
    p = [c for c in L["g8p"] if c.path == "g8p_pers"]
    grid = [c for c in p if c.mode == 16 and c.M < 1000 and not c.also]
    for M in (256, 257, 511, 589):
        assert {c.N for c in grid if c.M == M} == {256, 512, 1280}, M
    assert {c.K for c in p} >= {128, 192, 320, 384, 448}
    assert {(c.act, c.res, c.out, c.f16) for c in p} == {(a, r, o, h) for a in (0, 1, 2) for r in (False, True) for o in (16, 32) for h in (False, True)}   # 24 keys
    blocks = lambda c: min(-(-c.M // 256) * (c.N // 256), G.N_CU)      # noqa: E731
    assert any(blocks(c) < 8 for c in p) and any(blocks(c) >= 8 for c in p) and any(-(-c.M // 256) * (c.N // 256) > G.N_CU for c in p)
    assert {G.dispatch(c)["order"] for c in p} == {"dyn", "static"} and any(c.K == 320 and G.dispatch(c)["order"] == "static" for c in p)
    sw = [c for c in p if c.also == "switch"]
    assert {c.mode for c in sw} == {16, 26} and all((c.M, c.N) == (256 * 33 + 77, 2048) for c in sw) and {G.dispatch(c)["order"] for c in sw} == {"dyn", "static"}
    assert any(c.mode == -1 and G.dispatch(c)["band"] == 4 and (c.M, c.N) == (2125, 4096) for c in p)
    assert any(c.lda < c.K for c in p) and any(c.lda > c.K for c in p) and any(c.ldc == c.N + 8 for c in p) and any(c.ldw > c.K for c in p)
    assert any(c.kind == "exact" and c.out == 16 and c.res and G.rounding_points(c) == "twice" for c in p)
    # N > 8192 under mode 16: sc_gemm8p_try declines and the 33 tiles run on gemm_bf16_kernel<128, 128>
    t = [c for c in L["bf128x128"] if c.also == "declined8p"]
    assert {c.kind for c in t} == {"exact", "real"} and len(t) == 2 and all((c.M, c.N, c.K) == (256, 8448, 128) and c.mode == 16 for c in t)
    assert all(G.gemm8p_try(c, c.mode) is None and G.dispatch(c)["path"] == "bf128x128" and G.dispatch(c)["last_path"] == 0 for c in t)
    # every test stays short: no reference above the tile-switch shape's; and no case with more than 2e7 outputs, where the sign-weighted statistic's own
    # expectation under exact rounding (gemm_ref's docstring) would come close to 6 / sqrt(n)
    assert max(G.nprod(c) * c.M * c.N for c in G.all_cases()) <= 20_000_000
    assert max(G.nprod(c) * c.M * c.N * c.K for c in G.all_cases()) <= 8525 * 2048 * 384

"""CPU: the self-check of tools/layer_kernel_bounds.py on its reduced case list -- a torch fp32 emulation of each kernel's arithmetic (two summation orders) stays within
its limit of the fp32 part of every bound of tests/layer_kernels_ref.py, every mutant of every group leaves the bound on a case the tool names, and the slope check
sees the two mutants a bf16 store can hide.  Then: the case lists hold every shape and path the issue of record names, and the host-side rules restated in the
reference module -- sc_layernorm_bwd_bf16_partials, sc_colsum_bf16's chunk rule, wgrad's S / chunk / Mp -- select the path each case is named for; the two C helpers
are compared with the real library when it is loaded, and wgrad itself (run on stand-in ops, no GPU) with the restatement written from its description."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("layer_kernel_bounds", os.path.join(ROOT, "tools", "layer_kernel_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layer_kernel_bounds_self_check_reduced_cases():
    import layer_kernels_ref as R
    tool = _tool()
    ids = tool.reduced_ids()
    table, failures, margins, slope = tool.run(ids, quiet=True)
    assert sorted(table) == sorted(ids)
    assert not failures, failures
    assert all(0 <= v <= 1.0 for v in table.values()), table
    for G in R.GROUPS.values():
        for m in G.mutants:
            margin, cid = margins[(G.name, m)]
            assert margin > 1 and cid in ids, (G.name, m, margin, cid)
    for g, ms in tool.SLOPE_MUTANTS.items():
        for m in ms:
            assert slope[(g, m)][0] > 1, (g, m, slope[(g, m)])


def test_a_mutant_no_case_rejects_is_a_failure_of_the_tool(monkeypatch):
    import layer_kernels_ref as R
    tool = _tool()
    G = R.GROUPS["axpy"]
    monkeypatch.setitem(R.GROUPS, "axpy", G._replace(mutants=G.mutants + ("harmless",), ref=lambda c, inp, mutant=None: R.ax_ref(c, inp, None if mutant == "harmless" else mutant)))
    failures = tool.run([c.id for c in R.ax_cases()], quiet=True)[1]
    assert any("harmless" in f[1] for f in failures), failures


def test_slope_check_sees_what_the_store_hides():
    """var over D - 1 at D = 256 moves dx by 1 / 512 of itself -- half the bf16 store's half-ulp: per element it passes on most of a row, the row's slope does not.
    At D = 1024 the shift (1 / 2048) is below the slope's own derived allowance (the D-term sums of s1 and s2 are budgeted D U); there the fp32 partial rows, which
    no store hides, reject it per element."""
    import layer_kernels_ref as R
    c = [k for k in R.lnb_cases() if k.D == 256 and k.rows == 5][0]
    inp = R.lnb_inputs(c)
    ref, wrong, pre = R.lnb_ref(c, inp)["dx"], R.lnb_ref(c, inp, "var_Dm1")["dx"], R.lnb_pre(c, inp)["dx"]
    ratio, row, allow = R.slope_check(R.bfr(wrong.to(R.F32)), ref, pre)
    assert ratio > 1 and allow < 0.25 / (2 * c.D), (ratio, row, allow)
    assert R.slope_check(R.bfr(ref.to(R.F32)), ref, pre)[0] == 0.0
    for order in R.ORDERS:
        assert R.slope_check(R.lnb_emulate(c, inp, order)["dx"], ref, pre)[0] <= 1.0
    c = [k for k in R.lnb_cases() if k.D == 1024 and k.rows == 5][0]
    inp = R.lnb_inputs(c)
    assert R.worst((R.lnb_ref(c, inp, "var_Dm1")["part"] - R.lnb_ref(c, inp)["part"]).abs(), R.lnb_bound(c, inp)["part"].bound)[0] > 1


def test_case_lists_hold_the_required_shapes_and_paths():
    import layer_kernels_ref as R
    # sc_layernorm_bwd_bf16
    lb = R.lnb_cases()
    assert {c.D for c in lb if c.kern == "scalar"} == {64, 192, 960} and {c.D for c in lb if c.kern == "vec"} == {256, 768, 1024}
    assert all((c.D % 256 == 0) == (c.kern == "vec") and c.rpb == (32 if c.rows >= 4096 else 4) and c.id == f"ln_bwd/{c.kern}/rpb{c.rpb}/D{c.D}/rows{c.rows}" for c in lb)
    for D in (64, 192, 960, 256, 768, 1024):
        assert {c.rows for c in lb if c.D == D} >= {1, 3, 4, 5}
    for kern in ("scalar", "vec"):
        big = [c for c in lb if c.kern == kern and c.rows > 5]
        assert len({c.D for c in big}) == 2 and all({c.rows for c in big if c.D == D} == {4095, 4096, 4097, 4129} for D in {c.D for c in big})
    assert [R.lnb_partials(r) for r in (1, 4, 5, 4095, 4096, 4097, 4129)] == [(1, 4), (1, 4), (2, 4), (1024, 4), (128, 32), (129, 32), (130, 32)]
    assert 4097 % 32 == 1 and 4129 % 32 == 1 and 4095 % 4 == 3 and 5 % 4 == 1                                  # last chunks of one row, and one that is not full
    inp = R.lnb_inputs([c for c in lb if c.D == 768 and c.rows == 4097][0])
    x = inp["x"]
    small = x.std(-1) < 0.02
    assert bool(small.any()) and bool(((x.mean(-1).abs() > 40) & (x.std(-1) < 2)).any()) and bool((inp["gamma"] == 0).sum() == 1)
    # sc_gelu_bwd_bf16
    gb = R.gb_cases()
    assert {c.n for c in gb if c.kind == "tail"} == {0, 2, 6, 8, 10, 2050, 2052, 2054} and [c.n for c in gb if c.kind == "allbits"] == [65280]
    u = R.gb_all_finite_bits()
    assert u.numel() == 65280 and bool(torch.isfinite(u).all()) and u.to(R.F32).to(R.BF).view(torch.int16).unique().numel() == 65280
    assert [R.gb_path(n) for n in (0, 2, 8, 10, 2054)] == ["empty", "tail2", "vec8", "vec8+tail2", "vec8+tail6"]
    # sc_colsum_bf16
    cb = R.cb_cases()
    assert {c.rows for c in cb} == {1, 3, 4, 5, 63, 64, 65, 512, 513, 583, 65535, 65536, 65665} and {c.cols for c in cb} == {1, 7, 256, 257, 2304}
    for rows in {c.rows for c in cb}:
        mine = [c for c in cb if c.rows == rows]
        assert {c.acc for c in mine} == {0, 1} and {c.ld - c.cols for c in mine} == {0, 24}, rows
    assert all(c.rows <= 65 for c in cb if c.cols == 2304)
    assert [R.cb_chunks(r) for r in (1, 64, 65, 512, 513, 583, 65535, 65536, 65665)] == [(1, 64), (1, 64), (2, 64), (8, 64), (9, 64), (10, 64), (1024, 64), (512, 128),
                                                                                       (514, 128)]
    assert R.cb_path(512) == "rpb64/st2loop" and R.cb_path(513) == "rpb64/st2loop+tail" and R.cb_path(65) == "rpb64/st2tail" and R.cb_path(65536) == "rpb128/st2loop"
    assert bool((R.cb_inputs(cb[0])["x"][:, :cb[0].cols].mean(0).abs() > 0.2).all())
    # sc_axpy_bf16, sc_cls_pool_dz
    assert {(c.n, c.alpha) for c in R.ax_cases()} == {(n, a) for n in (2, 510, 512, 514, 4098) for a in (1.0, 0.37, -2.5, 0.0)}
    pz = R.pz_cases()
    assert {(c.B, c.T, c.NQ, c.R, c.D) for c in pz} == {(3, 5, 1, 8, 768), (2, 9, 2, 4, 80), (1, 1, 1, 1, 64), (2, 7, 1, 8, 260)}
    assert {c.ld_dz - c.D for c in pz} == {0, 8} and any(0 in c.lens and c.T in c.lens and any(0 < n < c.T for n in c.lens) for c in pz)
    # sc_transpose_bf16
    tg = R.tr_grid_cases()
    assert {(c.R, c.C) for c in tg} == {(r, k) for r in R.TR_RC for k in R.TR_RC} and {c.batch for c in tg} == {1, 3}
    for r in R.TR_RC:
        a, b, d = R.tr_pads(r)
        assert a == r and b % 64 == 0 and b >= r and d % 4 == 0 and d % 64 != 0 and d >= r
    tv = R.tr_vector_cases()
    assert sum(R.tr_vec(c) for c in tv) == 3 and {c.id.split("/")[2] for c in tv if not R.tr_vec(c)} >= {"cols%4", "rows_padded%4", "ld_in%4", "ld_out%4", "stride_in%4",
                                                                                                        "stride_out%4", "in-base+4B", "out-base+4B"}
    assert {R.tr_vec(c) for c in tv if c.ld_in < c.C} == {True, False} and any(c.ld_out > c.Rp and c.stride_out == c.Rp for c in tv)
    assert any(R.tr_vec(c) for c in tg) and any(not R.tr_vec(c) for c in tg)


def _wgrad_restated_plainly(M, N, K):
    """a second restatement, from train_hubert.wgrad's docstring and comment alone: tiles of 256 when N and K both reach 256, else of 128; at most 32 splits, at most
    512 // tiles, one per 2048 rows from 4096 rows on and none below, never fewer than one; chunk the smallest multiple of 64 with chunk S >= M"""
    t = 256 if min(N, K) >= 256 else 128
    tiles = ((N + t - 1) // t) * ((K + t - 1) // t)
    S = max(1, min(32, 512 // tiles, (M // 2048) if M >= 4096 else 1))
    chunk = ((M + 64 * S - 1) // (64 * S)) * 64
    return S, chunk, chunk * S, t


def test_wgrad_split_rule_restated_and_as_run():
    import layer_kernels_ref as R
    expect = {(48, 128, 128): (1, 64, 64), (4095, 128, 128): (1, 4096, 4096), (4096, 128, 128): (2, 2048, 4096), (4097, 256, 256): (2, 2112, 4224),
              (6149, 128, 128): (3, 2112, 6336), (65536, 64, 64): (32, 2048, 65536), (8197, 16640, 64): (3, 2752, 8256), (8192, 1024, 1024): (4, 2048, 8192),
              (65536, 1280, 1024): (25, 2624, 65600), (4096, 8192, 8192): (1, 4096, 4096), (100000, 128, 128): (32, 3136, 100352)}
    for shape, want in expect.items():
        assert R.wg_split(*shape)[:3] == want == _wgrad_restated_plainly(*shape)[:3], (shape, R.wg_split(*shape))
    assert R.wg_clause(8197, 16640, 64) == "tiles" and R.wg_clause(48, 128, 128) == "below4096" and R.wg_clause(6149, 256, 256) == "rows"
    assert R.wg_clause(100000, 128, 128) == "cap32" and R.wg_clause(4096, 8192, 8192) == "floor1"
    # wgrad itself on stand-in ops: what it asks of the transposes and the batched product is the restated S / chunk / Mp
    from speechclip_amd import train_hubert
    seen = {}

    class Ops:
        @staticmethod
        def transpose_bf16(src, ld_in, stride_in, rows, cols, batch, rows_padded=None, **kw):
            seen.setdefault("Mp", set()).add(rows_padded)
            return torch.zeros(batch, cols, 1)

        @staticmethod
        def gemm_batched(a, lda, stride_a, w, stride_w, w_mod, out, ldc, stride_c, bias, M, N, K, batch, ldw=None):
            seen.update(S=batch, chunk=K, lda=lda, stride_a=stride_a, stride_w=stride_w, ldw=ldw, w_mod=w_mod)

        @staticmethod
        def colsum(x):
            seen["colsum_rows"] = x.shape[0]
            return x[0]
    real = train_hubert.ops
    train_hubert.ops = Ops
    try:
        for (M, N, K) in list(expect)[:7]:
            seen.clear()
            out = train_hubert.wgrad(torch.zeros(M, N), torch.zeros(M, K))
            S, chunk, Mp, _ = R.wg_split(M, N, K)
            assert seen["Mp"] == {Mp} and (seen["S"], seen["chunk"], seen["lda"], seen["ldw"], seen["stride_a"], seen["stride_w"], seen["w_mod"]) == (S, chunk, Mp, Mp, chunk,
                                                                                                                                               chunk, S), (M, N, K, seen)
            assert tuple(out.shape) == (N, K) and (seen.get("colsum_rows") == S if S > 1 else "colsum_rows" not in seen)
    finally:
        train_hubert.ops = real


def test_c_helpers_match_the_restated_rules():
    import layer_kernels_ref as R
    from speechclip_amd import _lib
    L = _lib.lib()                       # raises if the .so is missing: no fallback
    for rows in (0, 1, 3, 4, 5, 31, 32, 33, 4095, 4096, 4097, 4129, 70000, 2 ** 33 + 5):
        assert int(L.sc_layernorm_bwd_bf16_partials(rows)) == (R.lnb_partials(rows)[0] if rows else 0), rows
    for rows in (1, 63, 64, 65, 512, 513, 65535, 65536, 65665, 2 ** 33 + 5):
        for cols in (1, 7, 257, 2304):
            assert int(L.sc_colsum_bf16_workspace_bytes(rows, cols)) == R.cb_workspace_bytes(rows, cols), (rows, cols)

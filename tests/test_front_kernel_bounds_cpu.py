"""CPU: the self-check of tools/front_kernel_bounds.py on its reduced case list -- the fp64 statements of tests/front_kernels_ref.py are well-posed (finite; no partial sum
of an exact-integer case reaches 2^24 quanta and its hi + lo splits are exact; the derived bound on the GroupNorm scale stays below its cap; the positional-conv statement
is torch's conv1d(padding = Kw // 2)[..., :Tp]), a torch fp32 / bf16 emulation of each kernel's arithmetic (two summation orders) reproduces the exact cases bit for bit and
stays within half the non-store part of every bound, and every mutant (variance over T0 - 1, eps outside the root, the coefficients of channel c + 1, statistics of the
unpadded length, the shift dropped, x_lo . w_hi dropped, w_lo dropped, LayerNorm over 512 channels, frame T0 written live, one (tap, channel) product dropped, a tap shift of
one, valid off by one either way, the neighbouring group's channels, a chunk without the previous chunk's rows, bias after the GELU, residual not masked, gy / gx swapped,
the class row given position 1) leaves its bound or fails its bitwise comparison.  The case lists must hold the shapes at which each kernel branch exists."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("front_kernel_bounds", os.path.join(ROOT, "tools", "front_kernel_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_front_kernel_bounds_self_check_reduced_cases():
    tool = _tool()
    table, failures = tool.run(tool.REDUCED, quiet=True)
    assert sorted(table) == sorted(tool.REDUCED)
    assert not failures, failures
    assert all(0 <= v <= 0.5 for v in table.values()), table


def test_case_lists_hold_the_required_shapes_and_paths():
    import front_kernels_ref as K
    tool = _tool()
    # the launch rule, restated: Tp -> (NW, chunks)
    assert [(K.pc_nw(Tp), -(-Tp // (64 * K.pc_nw(Tp)))) for Tp in (70, 500, 582, 812)] == [(4, 1), (8, 1), (4, 3), (8, 2)]
    pcx = K.pcx_cases()
    paths = [K.pc_path(c) for c in pcx]
    assert {p["chunks"] for p in paths} == {1, 2, 3}
    assert {(p["NJ"], p["NW"]) for p in paths} == {(nj, nw) for nj in (2, 3, 4) for nw in (4, 8)}
    assert {min(p["nk"], 4) for p in paths} == {1, 2, 3, 4}
    assert all(c.B == 2 for c in pcx) and all(c.G == 4 and c.Kw <= 16 for c, p in zip(pcx, paths) if p["chunks"] > 1)
    assert {(c.cg, c.Kw, c.G, c.Tp) for c in pcx} >= {(48, 128, 16, 70), (64, 128, 16, 70)} and {(c.cg, c.Kw) for c in pcx} >= {(32, 2), (32, 4), (48, 4), (64, 4), (64, 1), (64, 3)}
    for Tp, edge in ((582, 256), (812, 512)):
        v = {n for c in pcx if c.Tp == Tp for n in c.valid}
        assert {edge - 1, edge, edge + 1} <= v and {255, 256, 257} <= {n for c in pcx if c.Tp in (582, 812) for n in c.valid}
    allv = [(n, c.Tp) for c in pcx for n in c.valid]
    assert any(n == 0 for n, _ in allv) and any(n == 1 for n, _ in allv) and any(n == Tp for n, Tp in allv) and any(n > Tp for n, Tp in allv)
    assert set(K.PC_FALLBACK) == {(64, 4, 4), (272, 4, 16), (100, 5, 4)}
    # conv0: channel-chunk counts, frame blocks, both forms, every mode
    c0 = K.c0_cases()
    mf = [c for c in c0 if c.form == "mfma"]
    assert {c.C // 64 for c in mf} == {1, 2, 3, 7, 8} and {(c.T0, c.P) for c in mf} >= set(K.C0_MFMA_TP) and {c.mode for c in mf} == {0, 1, 2}
    assert all({(c.C, c.T0, c.P) for c in mf if c.mode == m} >= {(C, T0, P) for C in K.C0_MFMA_C for T0, P in K.C0_MFMA_TP} for m in (0, 1, 2))
    va = [c for c in c0 if c.form == "valu"]
    assert {(c.C, c.P) for c in va} == {(8, 64), (72, 128), (512, 70), (64, 100)} and {c.mode for c in va} == {0, 1}
    assert all(K.c0_form(c.C, c.P) == c.form for c in c0) and any(c.extra for c in c0) and any(c.pad for c in c0) and any(not c.bias for c in c0 if c.mode == 1)
    assert [c for c in c0 if c.T0 == 31999] == [K.C0Case("c0-mfma-m0-C64-T31999-P32000", "mfma", 0, 64, 31999, 32000, 0, 0, True)]
    c0x = K.c0x_cases()
    assert {(c.form, c.kind, c.bias) for c in c0x} == {(f, k, b) for f in ("mfma", "valu") for k in ("xlo", "wlo") for b in (True, False)}
    assert {c.T0 for c in K.gn_cases()} == {1, 15, 16, 17, 4097, 31999} and any(c.pad % 2 for c in K.gn_cases()) and K.gn_wave_n(31999) == 512 and K.gn_wave_n(4097) == 128
    # finish: every template argument with both outputs, the partly filled chunks
    pf = K.pf_cases()
    assert {K.pf_kernel(c) for c in pf} == {(f, cg) for f in (False, True) for cg in (64, 48, 0)}
    assert {c.D for c in pf} == {80, 192, 768, 1020, 1024} and {c.D // c.G for c in pf} == {64, 48, 32, 20} and (K.PF_B * K.PF_TP) % 4 != 0
    assert set(K.PF_VALID) == {0, 4, K.PF_TP} and {(c.affine, c.f32) for c in pf} == {(a, f) for a in (False, True) for f in (False, True)}
    assert {(c.D, c.G, c.Kw, c.Tp, c.route) for c in K.E2E} == {(768, 16, 128, 70, "window"), (1024, 16, 128, 70, "window"), (64, 4, 16, 30, "pack"), (272, 4, 6, 33, "pack")}
    assert set(K.VE_D) == {4, 260, 768, 1020, 1024} and set(K.VE_NTOK) == {5, 10} and all((K.VE_B * n) % 4 for n in K.VE_NTOK)
    assert set(K.PT_CASES) == {(32, 64, 3072), (14, 42, 640), (16, 48, 768)} and {D // G for D, G, *_ in K.PACK_CASES} == {4, 20, 68}
    assert (K.IN_HW[1] * K.IN_HW[2]) % 256 != 0 and K.IN_HW[0] == 2 and len(K.IN_STATS) == 2
    # the reduced list: all six (NJ, NW) pairs need not be in it, but every nk corner, chunk count and channel-chunk count of its groups is asserted above on the full lists
    red = [c for c in pcx if c.id in tool.REDUCED]
    assert {K.pc_path(c)["chunks"] for c in red} == {1, 2, 3} and {c.form for c in c0 if c.id in tool.REDUCED} == {"mfma", "valu"}

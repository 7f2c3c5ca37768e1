"""CPU: the self-check of tools/attention_rows_bounds.py on the whole case list of tests/attention_rows_ref.py -- the fp32 emulation of the kernel's arithmetic stays within the
derived bound in both summation orders, the census cases are exact, every mutant statement leaves the bound on at least 90 % of the rows it changes -- and: the case list holds
every length, head dim, mask, layout and score profile the issue of record names (checked on the INPUTS, not on the names), the constants restated from the kernel source are the
source's, the MODEL constants of the GPU test are the tool's, and the argument contract of sc_attention_rows_fwd (codes with a message, no launch: the library loads without a GPU)."""
import ctypes
import functools
import importlib.util
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("attention_rows_bounds", os.path.join(ROOT, "tools", "attention_rows_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _report():
    return _tool().run(quiet=True)


def test_emulation_stays_within_the_derived_bound_on_every_case_in_both_orders():
    import attention_rows_ref as A
    table, failures, _, _ = _report()
    assert sorted(table) == sorted(c.id for c in A.cases())                          # no case skipped or excluded
    assert not failures, failures
    worst = max(table, key=table.get)
    print(f"worst fp32-emulation err / bound {table[worst]:.4f} on {worst}")
    assert all(0 <= v <= 1.0 for v in table.values()), table


def test_census_cases_are_exact_in_the_emulation_and_compare_every_element():
    import attention_rows_ref as A
    census = [c for c in A.cases() if c.family == "census"]
    assert {c.mask for c in census} >= {"first_chunk", "mid_chunk", "last_chunk", "only64"} and {72, 1024} <= {c.hd for c in census}
    for c in census:
        inp = A.inputs(c)
        want = A.census_expected(c, inp)
        assert want.numel() == c.B * c.L * c.H * c.hd and bool((A.bound(c, inp)["out"].bound == 0).all())
        for order in A.ORDERS:
            assert bool((A.emulate(c, inp, order)["out"] == want).all()), (c.id, order)
        for b in range(c.B):
            n = int((~inp["pad"][b]).sum())
            assert n == 0 or n & (n - 1) == 0, (c.id, b, n)                          # a power of two of live keys
        assert bool((inp["q"] == 0).all()) and float(inp["v"].abs().max()) <= 8 and bool((inp["v"] == inp["v"].round()).all())


def test_every_mutant_leaves_the_bound_on_nine_rows_in_ten_of_those_it_changes():
    import attention_rows_ref as A
    shares = _report()[2]
    assert set(shares) == set(A.MUTANTS) and len(A.MUTANTS) == 8
    for m, (changed, rejected) in shares.items():
        print(f"{m:28s} {rejected} of {changed} rows")
        assert changed > 0 and rejected >= 0.9 * changed, (m, changed, rejected)


def test_a_mutant_no_row_rejects_is_a_failure_of_the_tool(monkeypatch):
    import attention_rows_ref as A
    tool = _tool()
    monkeypatch.setattr(A, "BF_STORE", 1.0)                                           # a bound as wide as the reference itself: the scale mutant must get through
    c = A.case("rows/L65-hd96-holes-sentinel")
    inp = A.inputs(c)
    r, bd = A.ref(c, inp)["out"], A.bound(c, inp)["out"]
    changed, rejected = tool.mutant_rows(c, inp, r, bd, "no_log2e")
    assert changed > 0 and rejected < 0.9 * changed


def test_case_list_covers_what_it_claims():
    import attention_rows_ref as A
    cs = A.cases()
    real = [c for c in cs if c.family != "census"]
    assert all(c.B <= 3 and c.H <= 4 and c.L <= 200 for c in cs)
    assert {c.L for c in real} == set(A.LENGTHS) == {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 200}
    assert {c.hd for c in real} == set(A.HEAD_DIMS) == {8, 16, 32, 64, 72, 96, 128, 768, 1024}
    assert all(c.L <= 65 and c.H == 1 for c in cs if c.hd >= 768) and any(c.hd == 1024 and c.L == 65 for c in real)
    assert {c.mask for c in real} == set(A.MASKS) and {c.profile for c in real} == set(A.PROFILES)
    assert {c.family for c in cs} == {"sentinel", "poison", "census"}
    for c in real:                                                                     # every mask shape in the three families' first two, census where the issue asks
        if c.mask != "none":
            assert {k.family for k in cs if k.base == c.base} >= {"sentinel", "poison"}, c.base
    assert any(c.layout == "wide" for c in real) and {c.mbyte for c in real} >= {1, 2, 255, "mix"} and any(c.scale not in (None, c.hd ** -0.5) for c in real)
    # the masks, on the arrays themselves
    for c in real:
        pad = A.mask_for(c.mask, c.B, c.L)
        if pad is None:
            continue
        assert c.B >= 2 and any(not torch.equal(pad[0], pad[b]) for b in range(1, c.B)), c.id      # a row read from the wrong b shows
        live = [(~pad[b]).nonzero().flatten().tolist() for b in range(c.B)]
        nch = -(-c.L // A.CHUNK)
        dead = [[t for t in range(nch) if t not in A.live_chunks(pad[b], c.L)] for b in range(c.B)]
        if c.mask == "prefix":
            assert all(l == list(range(len(l))) and 0 < len(l) < c.L for l in live)
        elif c.mask == "holes" and c.L >= 67:
            assert all(bool(pad[0, j]) for j in (0, 63, 64, 65, c.L - 1)) and all(len(l) > c.L - 8 for l in live)
        elif c.mask == "only0":
            assert live[0] == [0]
        elif c.mask == "onlylast":
            assert live[0] == [c.L - 1]
        elif c.mask == "only64":
            assert live[0] == [64] and dead[0][0] == 0
        elif c.mask == "first_chunk":
            assert dead[0] == [0] and nch >= 2 and (c.L > 101) == (dead[1] == [0])       # (short L: the odd entries keep key 7 of that chunk live)
        elif c.mask == "mid_chunk":
            assert all(d == [1] and nch >= 3 for d in dead)
        elif c.mask == "last_chunk":
            assert all(d == [nch - 1] and nch >= 2 for d in dead)
        elif c.mask == "one_full":
            assert live[0] == [] and len(live[1]) > 0
    assert any(A.skipped_after_live(A.mask_for(c.mask, c.B, c.L), c.B, c.L) for c in real if c.profile == "fall")
    # the score profiles, on the fp64 scores of the inputs
    seen = set()
    for c in real:
        if c.family != "sentinel" or c.profile == "plain":
            continue
        inp = A.inputs(c)
        for b in range(c.B):
            lv = A.live_keys(c, inp, b)
            s, _ = A._scores(inp, b, lv, inp["c"])
            assert float(s.abs().max()) <= 1e4
            cmax = [s[..., (lv // A.CHUNK) == t].amax(-1) for t in sorted(set((lv // A.CHUNK).tolist()))]
            if c.profile == "flat":
                assert bool((s == 0).all())
            elif c.profile == "rise":
                assert len(cmax) >= 2 and all(bool((cmax[t + 1] > cmax[t] + 1).all()) for t in range(len(cmax) - 1)), c.id
            elif c.profile == "fall":
                assert len(cmax) >= 2 and all(bool((cmax[t + 1] < cmax[t]).all()) for t in range(len(cmax) - 1)), c.id
            elif c.profile == "jump" and len(cmax) >= 2:
                assert bool((cmax[-1] > torch.stack(cmax[:-1]).amax(0) + 160).all()), c.id
            elif c.profile == "underflow":
                a = s - s.amax(-1, keepdim=True)
                assert bool(((a < -160).sum(-1) >= 1).all()) and bool(((a > -100) | (a < -160)).all()), c.id
            seen.add(c.profile)
    assert seen == set(A.PROFILES) - {"plain"}
    # the sentinels: a masked key outscores every live key and carries -50; the poison twin has NaN exactly in the masked K / V rows
    for c in real:
        if c.family == "sentinel" and c.mask != "none" and c.profile == "plain":
            inp = A.inputs(c)
            assert bool((inp["v"][inp["pad"]] == A.MASKED_V).all())
            twin = A.inputs(A.case(c.id.replace("-sentinel", "-poison")))
            assert bool(torch.isnan(twin["k"][inp["pad"]]).all() and torch.isnan(twin["v"][inp["pad"]]).all())
            assert bool(torch.equal(twin["k"][~inp["pad"]], inp["k"][~inp["pad"]]) and torch.equal(twin["q"], inp["q"]))
    assert {(x.hd, x.L) for x in A.PROBS_CASES} == {(8, 65), (8, 130), (96, 65), (96, 130)} and all(x.mask == "holes" for x in A.PROBS_CASES)
    assert {(x.hd, x.L) for x in A.HD_CASES} == {(h, l) for h in (64, 96, 128) for l in (65, 129)} and all(x.mask == "prefix" for x in A.HD_CASES)
    mods = A.MOD_CASES
    assert {(m.n_layers, m.norm_first) for m in mods if m.kind == "encoder"} == {(1, False), (1, True), (2, False), (2, True)}
    assert {m.nhead for m in mods if m.kind == "mha"} == {1, 4} and all(m.d == 128 and m.B == 3 and m.L == 70 for m in mods) and all(m.nhead == 4 for m in mods if m.kind == "encoder")
    pad = A.mod_mask(3, 70)
    assert not bool(pad[:, 0].any()) and all(bool((pad[b, 1:] & ~pad[b, :-1]).any() and (~pad[b, 1:] & pad[b, :-1]).any()) for b in range(2))      # holes, not prefixes


def test_constants_restated_from_the_sources_are_the_sources():
    import attention_rows_ref as A
    hip = open(os.path.join(ROOT, "speechclip_amd", "csrc", "attention_rows.hip")).read()
    assert int(re.search(r"constexpr int ROWS_PER_BLOCK = (\d+);", hip).group(1)) == A.ROWS_PER_BLOCK
    assert int(re.search(r"constexpr int MAX_HD = (\d+);", hip).group(1)) == A.MAX_HD == max(A.HEAD_DIMS)
    assert "j0 += 64" in hip and A.CHUNK == 64 and "scale * 1.44269504088896341f" in hip
    common = open(os.path.join(ROOT, "speechclip_amd", "csrc", "common.h")).read()
    assert re.search(r"bf16_t f2bf\(float f\) \{\s*__bf16 b = \(__bf16\)f;", common)          # the compiler's conversion: round to nearest even


def test_model_constants_of_the_gpu_test_are_the_tools():
    import test_attention_rows_parity_gpu as G
    models = _report()[3]
    assert set(models) == set(G.HD_MODEL) | set(G.MOD_MODEL)
    for k, v in {**G.HD_MODEL, **G.MOD_MODEL}.items():
        assert abs(v - models[k]) <= 0.02 * models[k], (k, v, models[k])


def test_argument_errors_are_codes_that_name_the_entry_and_empty_shapes_touch_nothing():
    from speechclip_amd import _lib
    L = _lib.lib()
    sent = torch.full((64,), -77.0, dtype=torch.bfloat16)
    buf = torch.zeros(4096, dtype=torch.bfloat16)
    p, o = buf.data_ptr(), sent.data_ptr()
    assert p % 16 == 0

    def call(q=p, k=p, v=p, out=o, B=1, H=1, L_=2, hd=8, ld=24):
        return L.sc_attention_rows_fwd(q, k, v, out, None, B, H, L_, hd, ld, H * hd, 0.5, None)
    for kw in (dict(hd=0), dict(hd=12), dict(hd=1032, ld=3 * 1032), dict(ld=4), dict(q=p + 2), dict(q=None), dict(k=None), dict(v=None), dict(out=None)):
        assert call(**kw) < 0 and b"sc_attention_rows_fwd" in L.sc_last_error(), kw
    for kw in (dict(B=0), dict(L_=0), dict(H=0)):
        assert call(**kw) == 0, kw
    assert bool((sent == -77.0).all())

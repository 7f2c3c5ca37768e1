"""CPU: the self-check of tools/vq_mode_bounds.py on its reduced case list -- the fp64 statements of tests/vq_modes_parity_ref.py are well-posed (finite, no output
whose rms is below 10x its mean bound), a torch fp32 emulation of each kernel's arithmetic (two summation orders, the bf16 (hi, lo) pairs of the product emulated)
stays within half the fp32 part of its bound, every mutant of every group leaves the bound on a case the tool names, and the exact statements (the fragment-ordered
table, the one-hot / two-hot products) are exact in fp32.  Then: the case lists hold every shape and path csrc/vq_modes.hip branches on, by construction -- the host-side
rules of sc_vq_soft_embed (soft_ne, the grid, the split clamp) are restated in the reference module and asked which path each case takes."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_MUTANTS = {
    "probs": ("noise_row_base_dropped", "noise_missing_in_second_pass", "masked_in_denominator", "inv_temp_twice", "no_inv_temp"),
    "soft": ("noise_row_base_dropped", "noise_missing_in_second_pass", "masked_in_denominator", "inv_temp_twice", "no_inv_temp", "table_lo_dropped", "last_step_short",
             "rows_64_127_take_rows_0_63", "wave_column_shifted"),
    "modebwd": ("noise_row_base_dropped", "noise_missing_in_second_pass", "masked_in_denominator", "inv_temp_twice", "no_inv_temp", "rowdot_z_with_cos"),
    "argmax": ("ties_to_highest_index",),
}


def _tool():
    spec = importlib.util.spec_from_file_location("vq_mode_bounds", os.path.join(ROOT, "tools", "vq_mode_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_vq_mode_bounds_self_check_reduced_cases():
    import vq_modes_parity_ref as P
    tool = _tool()
    ids = tool.reduced_ids()
    table, failures, margins = tool.run(ids, quiet=True)
    assert sorted(table) == sorted(ids)
    assert not failures, failures
    assert all(0 <= v <= 0.5 for v in table.values()), table
    for name, wanted in REQUIRED_MUTANTS.items():
        assert set(wanted) <= set(P.GROUPS[name].mutants), name
    for G in P.GROUPS.values():
        for m in G.mutants:
            margin, cid = margins[(G.name, m)]
            assert margin > 1 and cid in ids, (G.name, m, margin, cid)


def test_case_lists_hold_the_required_shapes_and_paths():
    import vq_modes_parity_ref as P
    # the dispatcher restated: soft_ne, the grid and the split clamp
    assert [P.soft_ne(E) for E in P.GRID_E] == [1, 2, 3, 4, 1, 6, 8, 6] and [P.grid_y(E) for E in P.GRID_E] == [1, 1, 1, 1, 5, 1, 1, 2]
    assert {P.soft_ne(E) for E in P.GRID_E} == {1, 2, 3, 4, 6, 8} and {P.grid_y(E) for E in P.GRID_E} == {1, 2, 5}
    assert set(P.GRID_R) >= {1, 64, 65, 129, 200} and set(P.GRID_NSPLIT) >= {1, 2, 5, 0}
    assert P.nsteps(333) == 11 and P.nsteps(1031) == 33 and P.nsteps(32) == 1 and P.nsteps(33) == 2
    assert all(any(ns > P.nsteps(V) for ns in P.GRID_NSPLIT) for V in (P.HOT_V,) + P.SOFT_V)                      # a split count above the steps: the clamp
    assert P.soft_nsplit(200, 333, 64, 64) == 11 and P.soft_nsplit(200, 333, 64, 0) == 11 and P.soft_nsplit(200, 1031, 320, 0) == 25
    assert P.soft_nsplit(200, 333, 64, 5) == 5 and P.split_of(332, 333, 5) == 3                                    # 11 steps in chunks of 3: the fifth chunk is empty
    paths = {Rr: P.row_paths(Rr) for Rr in P.GRID_R}
    assert paths[1] == {"partial_wm0"} and paths[64] == {"partial_wm0"} and paths[65] == {"partial_wm1", "wm1"}
    assert paths[129] == {"full_tile", "partial_wm0", "second_tile", "wm1"} and paths[200] == {"full_tile", "partial_wm1", "second_tile", "wm1"}
    assert paths[256] == {"full_tile", "second_tile", "wm1"}
    rem = {Rr % 128 for Rr in P.GRID_R}
    assert any(0 < x <= 64 for x in rem) and any(64 < x < 128 for x in rem) and 0 in rem

    # the exact products
    hot = P.hot_cases()
    assert {(c.kind, c.R, c.E) for c in hot} == {(k, Rr, E) for k in ("one", "two") for Rr in P.GRID_R for E in P.GRID_E}
    assert {c.temp for c in hot} == {1.0, 0.1}
    W, V = P.hot_winner_list(), P.HOT_V
    assert {v % 32 for v in W} == set(range(32)) and W[0] == 1 and V - 1 in W and not set(W) & set(P.R.MASK)
    for ns in (2, 5, 11):
        sps = (P.nsteps(V) + ns - 1) // ns
        for b in range(sps * 32, V, sps * 32):                                                                     # both sides of every split boundary
            assert b - 1 in W and b in W and P.split_of(b - 1, V, ns) + 1 == P.split_of(b, V, ns), (ns, b)
            assert (b - 1, b) in P.hot_pair_list(), (ns, b)                                                        # and a two-hot pair across it
    assert all(a != b and not {a, b} & set(P.R.MASK) for a, b in P.hot_pair_list())
    assert all(P.split_of(a, V, 11) != P.split_of(b, V, 11) for a, b in P.hot_pair_list())
    for c in hot:
        if c.R >= 64 and c.kind == "one":
            assert {w[0] for w in P.hot_winners(c)} == set(W), c.id                                                  # every winner in every case with 64 rows or more
        if c.R >= 64 and c.kind == "two":
            assert set(P.hot_winners(c)) == set(P.hot_pair_list()), c.id
    assert {P.hot_winners(c)[0] for c in hot if c.R == 1 and c.kind == "one"} >= {(W[(7 * i) % len(W)],) for i in range(8)}
    emb = P.hot_table(V, 768)
    assert emb.unique().numel() == V * 768                                                                         # the entries differ in every (v, e)
    bits = emb.to(torch.float32).view(torch.int32)
    assert torch.equal(emb.to(torch.float32).to(torch.float64), emb) and bool(((bits & 0xff) == 0).all())          # at most 16 significant bits
    hi = emb.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    lo = (emb - hi).to(torch.float32).to(torch.bfloat16).to(torch.float64)
    assert torch.equal(hi + lo, emb)                                                                               # hi + lo is exact
    x = P.hot_inputs(hot[0])["x"]
    assert float(x[:, 2].min()) == P.HOT_MASKED and float(x.min()) == P.HOT_LOW and 2 in P.R.MASK

    # the table
    assert P.TABLE_V == (5, 31, 32, 33, 333) and P.TABLE_E == (64, 192)
    t = P.table_bits(torch.arange(1, 21 * 64 + 1, dtype=torch.float32).view(21, 64))                                # emb[v][e] = 64 v + e + 1: hi + lo holds it
    assert t.numel() == P.table_elems(21, 64) == 2 * 32 * 64
    v = t.view(torch.bfloat16).to(torch.float64).view(2, 1, 4, 64, 8)
    v = v[0] + v[1]
    assert float(v[0, 1, 17, 3]) == (8 * 1 + 3) * 64 + 16 * 1 + 1 + 1 and float(v[0, 3, 37, 4]) == (8 * 2 + 4) * 64 + 16 * 3 + 5 + 1      # [vb][et][lane][j]
    assert bool((v[0, :, 32:, 5:] == 0).all()) and bool((v[0, :, 48:] == 0).all()) and bool((v[0, :, :32] > 0).all())  # rows 21 .. 31 of the padded table are zero

    # the parity lists
    pr = P.prob_cases()
    assert {(c.V, c.R, c.temp, c.nmask, c.noise) for c in pr} == {(V_, Rr, t_, m, nz) for V_ in (5, 255, 256, 257, 1031) for Rr in (1, 7) for t_ in (1.0, 0.5, 0.1)
                                                                for m in (0, 3, 8) for nz in (False, True)}
    assert all(c.nmask == 0 or {0, c.V - 1} <= set(P.vq_mask_ids(c)) for c in pr)
    sf = P.soft_cases()
    grid = {(c.R, c.V, c.E, c.temp, c.noise) for c in sf if c is not P.SOFT_BIG}
    assert grid == {(Rr, V_, E, t_, nz) for Rr in P.GRID_R for V_ in (333, 1031) for E in P.GRID_E for t_ in (1.0, 0.1) for nz in (False, True)}
    assert all(c.nsplits == P.GRID_NSPLIT for c in sf if c is not P.SOFT_BIG)
    assert (P.SOFT_BIG.R, P.SOFT_BIG.V, P.SOFT_BIG.E, P.SOFT_BIG.nsplits) == (129, 49408, 512, (0,)) and P.SOFT_BIG in sf
    assert sum(c.V == 49408 for c in sf) == 1
    xs = P.soft_inputs([c for c in sf if c.R == 65 and c.V == 333][0])["x"]
    assert float(xs[0].argmax()) == 1 and float(xs[1].argmax()) == 332 and float(xs[3].argmax()) == 2 and len(xs[2, 4:].unique()) == 1   # the planted rows
    bw = P.bwd_cases()
    assert {(c.R, c.V, c.temp, c.nmask) for c in bw} == {(Rr, V_, t_, m) for (Rr, V_) in ((1, 5), (7, 255), (7, 256), (7, 257), (3, 49408)) for t_ in (0.1, 1.0)
                                                        for m in (0, 3, 8)}
    assert all(bool(c.zero) == (c.V == 49408) for c in bw)
    nz = P.noise_cases()
    assert {(c.R, c.V, c.seed) for c in nz} == {(5, 333, 77), (16, 49408, 12), (16, 49408, 9)}
    for c in nz:
        if c.extreme:
            u = P.R.uniform(c.seed, torch.tensor([c.extreme[0]]).numpy().astype("uint64"))[0]
            assert u == (2.0 ** -24 if c.extreme[1] == "low" else 1 - 2.0 ** -24), c.id

    # the arg-max: where the planted ties sit in the block
    wave = lambda v: (v % 256) // 64        # noqa: E731
    a, b = P.ARG_TIES["later_wave"]
    assert (a, b) == (70, 300) and a < b and wave(a) > wave(b)                                                      # the lowest index sits in a LATER wave than its equal
    a, b = P.ARG_TIES["same_thread"]
    assert b == a + 256
    a, b = P.ARG_TIES["one_wave"]
    assert wave(a) == wave(b) and a % 256 != b % 256
    ac = P.arg_cases()
    assert {len(c.ids) for c in ac if c.V == P.ARG_V} == {0, 3, 8} and all({0, c.V - 1} <= set(c.ids) for c in ac if c.V == P.ARG_V and c.ids)
    assert any(c.V == 5 and set(c.ids) == set(range(5)) for c in ac)
    for c in ac:
        if c.V == P.ARG_V:
            inp = P.arg_inputs(c)
            t = P.arg_ref(c, inp)["targets"].tolist()
            assert t[:4] == [70, 10, 5, 70] and t[4] == (0 if not c.ids else 33) and t[5] == (c.V - 1 if not c.ids else 1), (c.id, t)
            assert int(inp["x"][4].argmax()) == 0                                                                  # a masked column holds the row's largest score
        elif c.ids:
            assert P.arg_ref(c, P.arg_inputs(c))["targets"].tolist() == [0, 0]                                     # the all-masked row: target 0
    assert {V_ for V_, _ in P.ALLMASKED} == {5, 8} and all(set(ids) == set(range(V_)) for V_, ids in P.ALLMASKED)

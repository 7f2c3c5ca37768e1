"""CPU: the self-check of tools/front_bwd_bounds.py on its reduced case list -- the fp64 statements of tests/front_bwd_ref.py ARE the operations (conv layer 0's contract equals
fp64 autograd of conv1d -> group_norm -> gelu, the transposed positional conv and its weight gradient equal fp64 autograd of the grouped conv1d, the literal split-K chains equal
the direct statement, conv_layer_backward's equals fp64 autograd of the strided view), the cap of conv layer 0's bound holds on the reference alone, a torch fp32 emulation in
the kernel's summation split (both directions) stays within half the fp32 part of every bound and reproduces the exact cases bit for bit, and every mutant (variance over T0 - 1,
m1 / m2 over the frames with a gradient, the mean-subtraction terms skipped on frames without one, m1 dropped, tanh-form GELU', an fp32 one-sweep variance, mask t <= valid,
reversal by rows_b - t, slab row t, gap Kw - 1, lead Kw / 2 - 1, the last split chunk dropped, Tq padding rows not zero, an overlapping tap overwriting, the slack-row tap dropped)
leaves its bound or changes a bit on a named case.  The case lists must hold the shapes, layouts and host decisions the issue names."""
import dataclasses
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("front_bwd_bounds", os.path.join(ROOT, "tools", "front_bwd_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_front_bwd_bounds_self_check_reduced_cases():
    tool = _tool()
    table, failures = tool.run(tool.REDUCED, quiet=True)
    assert sorted(table) == sorted(tool.REDUCED)
    assert not failures, failures
    assert all(0 <= v <= 0.5 for v in table.values()), table


def test_the_cap_holds_on_every_capped_case_and_the_dc_case_is_a_dc_case():
    import front_bwd_ref as FB
    import torch
    for c in FB.c0b_cases():
        if not c.cap or c.T0 > 1217:            # (the T0 = 4801 case is checked by the tool's full run and by the GPU test itself)
            continue
        inp = FB.c0b_inputs(c)
        ref, bound = FB.c0b_ref(c, inp)
        assert not FB.c0b_cap(ref, bound)[1], (c.id, FB.c0b_cap(ref, bound))
        if "dc" in c.kinds and 4 <= c.T0 <= 64:
            u = torch.einsum("tj,cj->ct", FB.frames(inp["x"], c.T0)[c.kinds.index("dc")], inp["w"])
            assert int((u.mean(-1) ** 2 / u.var(-1, unbiased=False) >= 100).sum()) >= 1, c.id


def test_case_lists_hold_the_required_shapes_and_decisions():
    import front_bwd_ref as FB
    tool = _tool()
    # ---- conv layer 0
    c0 = FB.c0b_cases()
    uni = [c for c in c0 if c.rows is None]
    assert {c.T0 for c in uni} == {1, 2, 3, 4, 5, 7, 64, 1217, 4801, 31999} and {c.C for c in c0} == {64, 128} and max(len(c.kinds) for c in c0) == 4
    assert any(c.P > c.T0 for c in uni) and any(c.pad for c in c0) and all(set(c.kinds) <= set(FB.KINDS4) for c in c0) and any(set(c.kinds) == set(FB.KINDS4) for c in c0)
    assert [(c.C, len(c.kinds), c.cap) for c in c0 if c.T0 == 31999] == [(64, 1, False)] and all(c.cap == (c.T0 > 2) for c in c0 if c.T0 != 31999)
    pk = [c for c in c0 if c.rows is not None]
    assert {c.rows for c in pk} >= {FB.GEO_ROWS, FB.TRAP_ROWS} and any(len(c.rows) == 1 for c in pk) and any(c.scale * c.rows[0] >= c.T0 for c in pk)
    trap = next(c for c in pk if c.rows == FB.TRAP_ROWS)
    assert c0_trapped(trap, 1) > 400
    assert [c.id for c in FB.c0w_cases()] == [c.id for c in c0 if c.T0 <= 4801]
    # the tiny model's own allotment
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    enc = HubertModel(HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())))
    lens = [6091, 5200, 3040, 330]
    T = enc.frame_geometry(6091)[1]
    geo = enc.packed_geometry(lens, 6091, need_rows=[min(round(n / 320), T) for n in lens])
    assert tuple(geo["rows"]) == FB.GEO_ROWS and geo["T0"] == 1217 and geo["scale0"] == 64
    # ---- row kernels
    rows = FB.row_cases()
    assert {(c.D, c.G) for c in rows} == set(FB.ROW_SHAPES) and {len(c.rows) for c in rows if c.packed} == set(FB.ROW_B) == {len(c.rows) for c in rows if not c.packed}
    assert {FB.row_vec(c.D, c.G) for c in rows if not c.packed} == {4, 8} and all((c.D // c.G) % 8 == 0 for c in rows if c.packed)
    assert all((sum(c.rows) * c.D // FB.row_vec(c.D, c.G)) % 256 for c in rows)
    for c in rows:
        if c.packed and len(c.rows) >= 5:
            assert c.rows[0] == 1 and 1 in c.rows[1:-1]
            kinds = {k for v, r in zip(c.valid, c.rows) for k, hit in (("zero", v == 0), ("one", v == 1), ("all", v == r), ("above", v > r)) if hit}
            assert kinds >= {"zero", "one", "all", "above"}, (c.id, kinds)
    assert any(c.packed and c.rows[-1] == 1 for c in rows)
    # ---- the adjoint chain
    adj = FB.adj_cases()
    assert {(c.cg, c.Kw) for c in adj if not c.packed} == {(cg, Kw) for cg in (32, 48, 64) for Kw in (2, 3, 16)}
    # packed batches have the windowed kernel alone, which takes Kw D/G % 64 == 0: every cg and every Kw still occurs, the three other pairs must be refused (GPU test)
    assert {(c.cg, c.Kw) for c in adj if c.packed} == {(32, 2), (64, 2), (64, 3), (32, 16), (48, 16), (64, 16)} and set(FB.ADJ_PACKED_DECLINED) == {(32, 3), (48, 2), (48, 3)}
    for c in adj:
        if c.packed:
            assert {1, max(1, c.Kw // 2), 70, 582} <= set(c.rows)
    assert {c.rows[0] for c in adj if not c.packed and c.Kw == 16} == {1, 8, 70, 582}
    import front_kernels_ref as K
    assert K.pc_path(K.PCCase("x", 2, 2, 32, 2, 582, (582, 582)))["chunks"] == 3
    # ---- the positional conv's weight gradient: the host's decisions
    pw = [c for c in FB.pw_cases() if not c.real]
    assert {(len(c.rows), FB.pw_split(c)["S"]) for c in pw if not c.packed} == {(1, 1), (2, 2), (3, 1), (4, 4), (16, 16)}
    assert {(c.rows[0], FB.pw_split(c)["Tq"]) for c in pw if not c.packed} == {(5, 64), (64, 64), (70, 128)}
    assert {(FB.pw_split(c)["Rg"], FB.pw_split(c)["S"]) for c in pw if c.packed and len(c.rows) == 3} == {(511, 1), (512, 1), (1023, 1), (1024, 2), (2047, 2), (2048, 4)}
    assert any(c.packed and len(c.rows) == 1 for c in pw) and all(c.rows[0] == 1 for c in pw if c.packed and len(c.rows) == 3)
    assert all(any(v < r for v, r in zip(c.valid, c.rows)) for c in pw if c.packed) and {(c.cg, c.Kw, c.G) for c in pw} == {(8, 4, 2), (32, 16, 2)}
    assert any(v == 0 for c in pw if not c.packed for v in c.valid) and any(v >= c.rows[0] for c in pw if not c.packed for v in c.valid)
    assert len([c for c in FB.pw_cases() if c.real]) == 2
    # ---- conv_layer_backward
    cl = FB.cl_cases()
    assert {(c.k, c.s, c.rows_out) for c in cl if not c.real} == {(k, s, r) for (k, s) in ((3, 2), (2, 2)) for r in (5, 64, 65)} and all(c.B == 2 for c in cl)
    assert {c.C for c in cl} == {64, 128} == {c.dim for c in cl} and sorted((c.k, c.s) for c in cl if c.real) == [(2, 2), (3, 2)]
    # ---- every mutant the issue names has a home, and the reduced list covers every group
    named = {m for ms in tool.MUTANTS.values() for m in ms}
    assert named >= {"var_T0m1", "m_over_grad_frames", "mean_terms_skipped", "m1_dropped", "tanh_gelu", "one_sweep_f32", "mask_t_le_valid", "reverse_rows_b_minus_t", "slab_row_t",
                     "gap_Kw_minus_1", "lead_minus_1", "last_chunk_dropped", "tq_padding_not_zero", "tap_overwrites", "slack_tap_dropped"}
    assert {g for cid, g, _ in tool.all_checks() if cid in tool.REDUCED} == {"c0b", "c0w", "rows", "adj", "pw", "cl"}


def c0_trapped(c, b):
    """frames of utterance b without a gradient (the layout does not hold them) that exist on the padded layout: all of them see samples in these cases"""
    return c.T0 - min(c.T0, c.scale * c.rows[b])

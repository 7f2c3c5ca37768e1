"""CPU: the self-check of tools/row_kernel_bounds.py on its reduced case list -- the fp64 statements of tests/row_kernels_ref.py are well-posed (finite, no row whose
rms is below 10x its mean bound), a torch fp32 emulation of each kernel's arithmetic (two summation orders) stays within half the fp32 part of its bound, every mutant
(variance over D - 1, eps outside the root, biased mean, neighbour's statistics, shifted affine, GELU before the affine; mask without the row term, missing keep scale;
dropped / mis-strided layer, softmax over n - 1, biased normalize; Tp for T, per-layer mean, eps inside the root; len +- 1, fp32 single-pass and unbiased variance; bias and
residual swapped, ldr ignored; key count +- 1, CLS keys left out, transposed CLS scores, a wave's last four keys dropped, lo block zero) leaves the bound or the slope /
offset allowance, and the reduced list reaches every dispatch path of sc_layernorm.  Keeps the bounds and the mutants honest when someone edits the inputs."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("row_kernel_bounds", os.path.join(ROOT, "tools", "row_kernel_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_row_kernel_bounds_self_check_reduced_cases():
    tool = _tool()
    table, failures = tool.run(tool.REDUCED, quiet=True)
    assert sorted(table) == sorted(tool.REDUCED)
    assert not failures, failures
    assert all(0 <= v <= 0.5 for v in table.values()), table


def test_case_lists_hold_the_required_shapes_and_paths():
    import row_kernels_ref as R
    tool = _tool()
    ln = R.ln_cases()
    assert {c.path for c in ln} == set(R.LN_PATHS) and all(R.ln_dispatch(c) == c.path for c in ln)
    assert {c.path for c in ln if c.id in tool.REDUCED} == set(R.LN_PATHS)
    gen = [c for c in ln if c.path.startswith("gen_")]
    for path in ("gen_bf_bf", "gen_bf_f32", "gen_f32_bf", "gen_f32_f32", "gen_f32_half"):
        mine = [c for c in gen if c.path == path]
        assert {c.D for c in mine} >= set(R.LN_GENERIC_D), path
        assert any(c.gelu for c in mine) and any(not c.affine for c in mine) and any(c.ld_in > c.D for c in mine) and any(c.ld_out > c.D for c in mine), path
    assert all(set(c.rows) == set(R.LN_ROWS) for c in ln if not c.path.startswith("gen_"))
    assert any(c.ld_in == 5 * 768 for c in gen) and any(c.x_off == 4 and c.D == 768 for c in gen) and any(c.D == 512 and c.out_dt == R.F32 for c in gen)
    ws = R.ws_cases()
    assert {c.n for c in ws} == set(R.WS_N) and {c.D for c in ws} == set(R.WS_D) and {c.wkind for c in ws} == set(R.WS_KINDS)
    assert {(c.f32, c.normalize) for c in ws} == {(False, False), (False, True), (True, False), (True, True)}
    sk = R.sk_cases()
    assert {c.S for c in sk} == {1, 2, 7} and {c.res for c in sk} == {None, "ldN", "ldwide", "ld0"} and {(c.bias, c.gelu) for c in sk} == {(a, b) for a in (False, True) for b in (False, True)}
    for ld in R.WV_LDS:
        lens = R.wv_lens(ld)
        assert {0, 1, ld} <= set(lens) and max(lens) <= ld
    assert {(c.NQ, c.R, c.D) for c in R.pool_cases()} == set(R.POOL_SHAPES) and any(c.ld_x > c.D for c in R.pool_cases())
    assert {(c.NQ, c.H, c.hd) for c in R.attn_cases()} == set(R.ATTN_SHAPES)
    assert all(c.lens == R.POOL_LENS70 or c.lens == (499, 498) for c in R.pool_cases() + R.attn_cases())

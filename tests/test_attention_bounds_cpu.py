"""CPU: the self-check of tools/attention_bounds.py on a reduced case list -- the MODEL constants of tests/test_attention_fwd_parity_gpu.py are reproduced, its fp64
references are well-posed (finite, no tiny row, sentinel shares in range) and every mutant reference (key length +-1, causal diagonal +-1, tile count, skipped
rescale, swapped V heads, the dropout-mask variants) falls outside the bound of its case.  Keeps the bounds and the mutants honest when someone edits the inputs."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("attention_bounds", os.path.join(ROOT, "tools", "attention_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_attention_bounds_self_check_reduced_cases():
    tool = _tool()
    models, failures = tool.run(tool.REDUCED, quiet=True)
    assert sorted(models) == sorted(tool.REDUCED)
    assert not failures, failures
    assert all(0 < m < 1e-2 for m in models.values()), models


def test_every_case_has_a_model_constant_and_the_required_lengths():
    import test_attention_fwd_parity_gpu as T
    ids = {c.id for c in T.all_cases()}
    assert ids == set(T.MODEL), ids ^ set(T.MODEL)
    causal = {c.T for c in T.all_cases() if c.causal and c.group == "causal"}
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257} <= causal
    for c in T.all_cases():
        if c.group in ("fwd", "drop") and c.T > 64:
            assert c.T in c.klens and 1 in c.klens and any(abs(k % 64 - 32) >= 31 for k in c.klens if 1 < k < c.T) and len(c.klens) == 4, c

"""CPU: the self-check of tools/train_mode_bounds.py on a reduced case list -- the MODEL constants of tests/test_train_mode_parity_gpu.py are reproduced, its fp64
references are well-posed (finite, no tiny row, no gradient left out except k_b by name, every mask site with a dropped and a kept element per judged row) and every
mutant reference (swapped site seeds, a mask on the residual, a missing rescale, a backward without the forward's mask, wrong seed counts per layer, the packed-mask
and pooling-mask strides, ds from the dropped probabilities, d alpha without ds . u) falls outside the bound of its case.  Keeps the bounds and the mutants honest
when someone edits the inputs."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("train_mode_bounds", os.path.join(ROOT, "tools", "train_mode_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_mode_bounds_self_check_reduced_cases():
    tool = _tool()
    models, failures = tool.run(tool.REDUCED, quiet=True)
    assert sorted(models) == sorted(tool.REDUCED)
    assert not failures, failures
    worst = {cid: max(m.values()) for cid, m in models.items()}
    assert all(0 < w < 3e-2 for w in worst.values()), worst          # a model error of several per cent would mean the model, not the product, is off


def test_every_judged_tensor_has_a_model_constant_and_the_cases_hold_the_required_edges():
    import test_train_mode_parity_gpu as T
    tool = _tool()
    models, _ = tool.run(quiet=True, mutants=False)
    keys = {k for m in models.values() for k in m}
    assert keys == set(T.MODEL), keys ^ set(T.MODEL)
    for c in T.POOL_CASES:
        assert c.lens[0] == c.T and 1 in c.lens and (c.B < 3 or 0 in c.lens) and (c.B < 4 or any(n % 4 and n % 64 and 1 < n < c.T for n in c.lens)), c
    assert any(c.n > 16 and c.f32 and c.normalize for c in T.POOL_CASES) and any(c.D % 256 for c in T.POOL_CASES) and any(c.n == 0 and c.NQ > 1 for c in T.POOL_CASES)
    assert 0.0 in T.POOL_P and any(p > 0 for p in T.POOL_P) and 1 in T.POOL_NSPLIT and None in T.POOL_NSPLIT
    assert T.NODE_RATES["activation"] > 0 and any(c.packed and 1 in c.rows and 2 in c.rows for c in T.NODE_CASES) and any(not all(c.train) for c in T.NODE_CASES)
    dims = {dict(c.over).get("encoder_embed_dim", 128) for c in T.FROZEN_CASES}
    assert 768 in dims and any(dict(c.over).get("activation_dropout", 0) > 0 for c in T.FROZEN_CASES)

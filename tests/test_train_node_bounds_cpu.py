"""CPU: the self-check of tools/train_node_bounds.py on EVERY case of tests/test_train_nodes_parity_gpu.py (the whole table takes a few seconds, so no subset):
the MODEL constants pasted into the GPU test are the ones the tool computes now, every judged row and tensor is well-posed (max|ref| >= 1e-2, nothing left out
but the analytically zero k-bias slices), every mutant wiring of the references falls outside its bound, and the fp64 image-tower node is
vit_train_ref.oracle_visual_grads.  Keeps the bounds and the mutants honest when someone edits the inputs or the references."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("train_node_bounds", os.path.join(ROOT, "tools", "train_node_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_constants_well_posedness_and_every_mutant():
    import test_train_nodes_parity_gpu as T
    tool = _tool()
    models, failures, mutants = tool.run(quiet=True)
    assert not failures, failures
    assert sorted(models) == sorted([c.id for c in T.NODE_CASES] + list(T.WSUM_CASES) + [c.id for c in T.BRANCH_CASES] + list(T.TOWER_CASES))
    keys = {k for m in models.values() for k in m}
    assert keys == set(T.MODEL), keys ^ set(T.MODEL)
    assert set(mutants) == set(tool.ALL_MUTANTS)
    for name, rows in mutants.items():
        assert any(outside > 0 for _, outside, _ in rows), (name, rows)


def test_fp64_image_tower_node_is_the_oracle():
    import test_train_nodes_parity_gpu as T
    tool = _tool()
    for cid in T.TOWER_CASES:
        assert tool.tower_vs_oracle(cid) < 1e-10, cid


def test_cases_hold_the_required_edges():
    import test_train_nodes_parity_gpu as T
    ids = {c.id for c in T.NODE_CASES}
    assert {"node-nodrop-padded", "node-nodrop-packed", "node-preln-padded", "node-preln-packed", "node-preln-quickgelu", "node-n3-mixed", "node-preln-n3-mixed"} <= ids
    assert T.node_case("node-n3-mixed").train == (False, True, False) and T.node_case("node-n3-mixed").drop and not T.node_case("node-n3-mixed").pre_ln
    assert T.node_case("node-preln-n3-mixed").train == (False, True, False) and T.node_case("node-preln-n3-mixed").pre_ln
    assert T.node_case("node-nodrop-padded").lens == (70, 64, 33) and T.node_case("node-nodrop-packed").rows == (70, 65, 2, 1)
    assert (T.WSUM_N, T.WSUM_M, T.WSUM_D) == (4, 137, 128) and min(T.WSUM_W) <= -3.0 and max(T.WSUM_W) - sorted(T.WSUM_W)[-2] >= 1.0
    B = T.BRANCH_CASES
    assert {c.D // c.H for c in B if c.n == 2} == {64, 96, 128} and {c.n for c in B} == {1, 2, 3}
    assert {(c.pre_ln, c.p > 0) for c in B} == {(False, False), (False, True), (True, False), (True, True)}
    assert T.BRANCH_T == 69 and T.BRANCH_LEN == (69, 63, 64, 1)
    assert T.TOWER_CASES == ("tower-T17", "tower-T65") and T.TOWER_B == 3

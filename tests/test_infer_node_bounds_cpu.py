"""CPU: the self-check of tools/infer_node_bounds.py on EVERY case of tests/test_infer_nodes_parity_gpu.py (the whole table takes some ten seconds, so no subset):
the MODEL constants pasted into the GPU test are the ones the tool computes now, every judged row and tensor is well-posed (max|ref| >= 1e-2, nothing left out but
the rows behind an utterance's valid frames), every mutant wiring of the references falls outside its bound, the fp64 references are the oracle classes
(HubertModelRef, ClipRef) in double to 1e-10, and the half-range case reaches 2^15 .. 6e4 without leaving the half format.  Keeps the bounds and the mutants honest
when someone edits the inputs or the references."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("infer_node_bounds", os.path.join(ROOT, "tools", "infer_node_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_model_constants_well_posedness_oracle_and_every_mutant():
    import test_infer_nodes_parity_gpu as T
    tool = _tool()
    models, failures, mutants = tool.run(quiet=True)          # includes the oracle comparisons and the half-range report
    assert not failures, failures
    assert sorted(models) == sorted([c.id for c in T.ENC_CASES] + list(T.WRAP_MIX) + list(T.WRAP_METHODS) + list(T.TOWER_CASES) + [c.id for c in T.BRANCH_CASES] + list(T.TEXT_CASES))
    keys = {k for m in models.values() for k in m}
    assert keys == set(T.MODEL), keys ^ set(T.MODEL)
    assert set(mutants) == set(tool.ALL_MUTANTS)
    for name, rows in mutants.items():
        assert any(outside > 0 for _, outside, _, _ in rows), (name, rows)


def test_fp64_references_are_the_oracle_classes():
    import test_infer_nodes_parity_gpu as T
    tool = _tool()
    for cid in tool.ORACLE_ENC:
        assert tool.encoder_vs_oracle(cid) < 1e-10, cid
    for cid in T.TOWER_CASES:
        assert tool.tower_vs_oracle(cid) < 1e-10, cid
    for c in T.BRANCH_CASES:
        assert tool.branch_vs_torch(c.id) < 1e-10, c.id
    for cid in T.TEXT_CASES:
        assert tool.text_vs_oracle(cid) < 1e-10, cid


def test_cases_hold_the_required_edges():
    import test_infer_nodes_parity_gpu as T
    ids = {c.id for c in T.ENC_CASES}
    assert {"enc-post-tiny3", "enc-post-768", "enc-pre-tiny-f16", "enc-pre-tiny-bf16", "enc-pre-tiny-f16-conv0sep", "enc-pre-1024-f16", "enc-pre-1024-bf16",
            "slot-post-drop1", "slot-post-stop1", "slot-pre-drop1", "slot-pre-stop1", "half-f16", "half-bf16"} <= ids
    assert T.ENC_LENS == (8000, 6000, 3000, 400) and T.LAYOUTS == ("padded", "packed")
    enc, wav, pack, valid, need = T.enc_setup("enc-post-tiny3")
    assert enc.cfg.encoder_layers == 3 and enc.cfg.encoder_embed_dim == 128 and not enc.cfg.layer_norm_first
    assert list(valid) == [24, 19, 10, 2] and list(need) == [24, 19, 9, 1] and pack["rows"] == [25, 20, 11, 3]          # the 400-sample wave: feat_len 1
    c768 = T.enc_setup("enc-post-768")[0].cfg
    assert (c768.encoder_embed_dim, c768.encoder_attention_heads, c768.encoder_ffn_embed_dim, c768.conv_pos_groups, c768.encoder_layers) == (768, 12, 1536, 16, 2)
    pre = T.enc_setup("enc-pre-tiny-f16")
    assert pre[0].cfg.layer_norm_first and pre[0].cfg.extractor_mode == "layer_norm" and pre[0].cfg.conv_bias and pre[0].cfg.normalize
    assert abs(pre[1][0].mean().item() - 0.05) < 0.02 and bool((pre[1][1, 5000:6000] == 0.05).all()), "the DC offset and the silent tail inside utterance 1"
    c1024 = T.enc_setup("enc-pre-1024-f16")[0].cfg
    assert (c1024.encoder_embed_dim, c1024.encoder_attention_heads, c1024.encoder_ffn_embed_dim, c1024.conv_pos_groups, c1024.encoder_layers) == (1024, 16, 2048, 16, 2)
    assert {(c.fmt, c.conv0_fused) for c in T.ENC_CASES if c.id.startswith("enc-pre-tiny")} == {("f16", True), ("bf16", True), ("f16", False)}
    assert T.enc_case("slot-post-drop1").drop == (1,) and T.enc_case("slot-pre-stop1").stop == 1 and T.enc_setup("slot-pre-drop1")[0].cfg.encoder_layers == 3
    assert len(T.enc_reference_cached("slot-post-drop1")[0]) == 3 and len(T.enc_reference_cached("slot-post-stop1")[0]) == 2
    assert T.enc_case("half-f16").boost == T.enc_case("half-bf16").boost and T.REPORT_ONLY == ("half-bf16",)
    assert T.WRAP_W == (2.0, 0.25, -3.0, 0.5) and T.WRAP_LIST == [0, 2] and T.TOWER_CASES == ("tower-T17", "tower-T65")
    B = T.BRANCH_CASES
    assert {c.D // c.H for c in B} == {64, 96, 128} and {c.n for c in B} == {1, 2, 3} and {c.pre_ln for c in B} == {False, True}
    assert T.BRANCH_T == 69 and T.BRANCH_LEN == (69, 63, 64, 1)
    assert T.TEXT_CASES == ("text-w64-h1-l2", "text-w128-h2-l3") and T.TEXT_MODES == ("packed", "packed-general", "padded")
    assert T.text_setup("text-w64-h1-l2")[1].argmax(-1).tolist() == [1, 4, 12, 31, 76, 12]


def test_dropped_layer_slots_are_what_the_issue_states():
    """drop_layers=(1,) on three layers: three states, and state 2 is layer 2 applied to state 1 (the reference's own wiring, checked against a direct statement)"""
    import infer_nodes_ref as I
    import test_infer_nodes_parity_gpu as T
    import train_mode_ref as R
    enc = T.enc_setup("slot-post-drop1")[0]
    hs = T.enc_reference_cached("slot-post-drop1")
    full = T.enc_reference_cached("enc-post-tiny3")
    P2 = R.layer_params_of(enc.encoder.layers[2])
    for b, h in enumerate(hs):
        assert len(h) == 3 and I.row_metric(h[1], full[b][1]).max().item() == 0.0
        want = R.post_ln_layer(h[1][None], P2, [h[1].shape[0]], None, False, heads=enc.cfg.encoder_attention_heads)[0]
        assert I.row_metric(h[2], want).max().item() < 1e-12

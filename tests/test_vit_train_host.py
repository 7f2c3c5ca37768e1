"""No GPU: the `clip.image_encoder_trainable` switch (which tensors train, what the optimizer is handed), the seed condition of the GPU gradient tests, and the
self-check of sc_vit_embed_bwd's fp64 statement and derived bounds (tests/vit_train_ref.py): the bounds accept the statement evaluated in fp32 and reject three mutants."""
import dataclasses

import pytest
import torch

import vit_train_ref as V

N_VISUAL = 1 + 1 + 1 + 2 + 2 * 12 + 2 + 1          # conv1, class, positional, ln_pre, 2 blocks of 12, ln_post, proj


def test_image_encoder_trainable_constructs_and_trains_exactly_the_visual_tensors():
    from speechclip_amd.module.clip_official import ClipModel
    m = ClipModel("ViT-B/32", image_encoder_trainable=True, clip_config=V.tower_config("T17"))
    tp = m.trainable_params()
    assert len(tp) == N_VISUAL == 32
    visual = list(m.model.visual.parameters())
    assert len(visual) == 32 and all(any(p is q for q in visual) for p in tp)
    named = dict(m.model.named_parameters())
    assert all(p.requires_grad == k.startswith("visual.") for k, p in named.items())
    assert sum(p.requires_grad for p in named.values()) == 32
    frozen = ClipModel("ViT-B/32", clip_config=V.tower_config("T17"))
    assert frozen.trainable_params() == [] and not any(p.requires_grad for p in frozen.model.parameters())


def test_node_argument_order_covers_every_visual_tensor_once():
    from speechclip_amd.module.clip_official import ClipModel
    from speechclip_amd.train_vit import visual_params
    m = ClipModel("ViT-B/32", image_encoder_trainable=True, clip_config=V.tower_config("T65"))
    mine, theirs = visual_params(m.model.visual), list(m.model.visual.parameters())
    assert len(mine) == len(theirs) == 32 and {id(p) for p in mine} == {id(p) for p in theirs}


def test_text_encoder_trainable_still_raises_and_names_the_text_tower():
    from speechclip_amd.module.clip_official import ClipModel
    with pytest.raises(NotImplementedError, match="text"):
        ClipModel("ViT-B/32", text_encoder_trainable=True, clip_config=V.tower_config("T17"))
    with pytest.raises(NotImplementedError, match="text"):
        ClipModel("ViT-B/32", image_encoder_trainable=True, text_encoder_trainable=True, clip_config=V.tower_config("T17"))


def test_get_trainable_params_includes_the_image_tower():
    from helpers import make_config
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.hubert import HubertConfig
    cfg = make_config(d_model=128, branch_heads=4, hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())), clip_config=V.tower_config("T17"))
    cfg.clip.image_encoder_trainable = True
    model = KWClip_GeneralTransformer(cfg)
    tp = model.getTrainableParams()
    visual = list(model.clip.model.visual.parameters())
    assert len(visual) == 32 and all(any(p is q for q in tp) for p in visual)
    assert not any(p.requires_grad for k, p in model.clip.model.named_parameters() if not k.startswith("visual."))
    branch = list(model.parallel_branch.parameters())
    assert len(tp) == 32 + len(branch) + len(model.audio_encoder.trainable_params())          # + the layer-mix weights of the frozen speech encoder


@pytest.mark.parametrize("name", sorted(V.TOWERS))
def test_the_seed_leaves_no_reference_gradient_at_zero(name):
    """The GPU gradient test checks all 32 tensors and skips none: every fp64 reference norm is above 1e-7 for the seed in use."""
    _, ref, image, w = V.make_tower(name)
    _, grads = V.oracle_visual_grads(ref, image, w)
    assert len(grads) == 32
    norms = {k: g.norm().item() for k, g in grads.items()}
    assert min(norms.values()) > 1e-7, sorted(norms.items(), key=lambda kv: kv[1])[:3]
    d = 128
    for k, g in grads.items():              # softmax is invariant to a key bias: the exact gradient of the k slice is 0
        if k.endswith("in_proj_bias"):
            assert g[d:2 * d].abs().max().item() < 1e-12 * g.abs().max().item()


@pytest.mark.parametrize("B,ntok,D", V.EMBED_SHAPES)
def test_embed_bwd_bounds_accept_fp32_and_reject_the_mutants(B, ntok, D):
    x = V.embed_bwd_inputs(B, ntok, D)
    ref = V.embed_bwd_ref(**x)
    bound = V.embed_bwd_bounds(ref, x["gamma"], B, ntok, D)
    f32 = V.embed_bwd_ref(**x, dt=V.F32)
    f32["dpatch"] = f32["dpatch"].to(V.BF)          # the kernel's store
    for k in ("dpatch", "dpos", "dgamma", "dbeta"):
        r, i = V.worst_ratio(f32[k], ref[k], bound[k])
        print(f"fp32 statement {k:7s} [{B},{ntok},{D}] worst err/bound {r:.4f} at {i}")
        assert r <= 1.0, (k, r, i)
    for mutant, key in (("no_mean", "dpatch"), ("dpos_no_cls", "dpos"), ("dgamma_dy", "dgamma")):
        bad = V.embed_bwd_ref(**x, mutant=mutant)
        r, _ = V.worst_ratio(bad[key], ref[key], bound[key])
        print(f"mutant {mutant:12s} [{B},{ntok},{D}] worst err/bound of {key}: {r:.1f}")
        assert r > 1.0, (mutant, r)


def test_quickgelu_bwd_statement_is_the_derivative():
    u = V.every_bf16_in(-12.0, 12.0)
    assert u.numel() == 2 * (0x4140 + 1) and u.min().item() == -12.0 and u.max().item() == 12.0
    x = u.clone().requires_grad_(True)
    (x * torch.sigmoid(1.702 * x)).sum().backward()
    assert (V.quickgelu_bwd_ref(u, torch.ones_like(u)) - x.grad).abs().max().item() < 1e-14

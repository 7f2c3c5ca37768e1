"""GPU: a training step in deterministic mode (ops.set_deterministic / SC_DETERMINISTIC=1) repeats bit for bit.

Tiny models built by the helpers of the existing training tests; the batch is 16 ragged utterances of about 3 s (B x T = 16 x 149 = 2384 padded rows).  Every
configuration takes the fixed-order pooling backward and the chunked column sums (the head's 16 x 16 partial rows, the bias gradients over the frames).  The
split-K rule of sc_sgemm looks at the contraction length alone (K >= 2048), and every fp32 product of the tail contracts over the model width, the branch's
feed-forward width 4 d or the batch -- never over the frames -- so at d = 128 no step reaches it however many rows the batch has.  One configuration therefore
widens the tiny model to d = 512: the branch's feed-forward products then contract over K = 2048 with 8 output tiles and are split 8 ways, forward and backward,
one of them with beta = 1.  ops.det_counters() proves which of the three paths a step took.

  * four steps from the same torch seed: equal loss, torch.equal on EVERY gradient -- the four tensors test_finetune_packed_gpu.ATOMIC_HEAD_GRADS exempts included
    -- and another seed changes the gradients: P-base tail with its dropouts on, C-base (train-mode BatchNorm, straight-through quantizer, gradients through the
    text tower), layer fine-tuning under SC_VARLEN_PACK=0 and =1, whole-encoder training, image_encoder_trainable;
  * twenty steps of TrainKWClip_GeneralTransformer.fit, twice: equal loss history, parameters and FusedAdam moments;
  * the oracle / golden-gradient tests of the default path, run as they are (their own thresholds) with the mode on;
  * with the mode off the counters stay at zero."""
import numpy as np
import pytest
import torch

import test_finetune_gpu as TF
import test_finetune_packed_gpu as TP
import test_train_gpu as TT
import test_vit_train_gpu as TV
import test_vq_modes_gpu as TQ

pytestmark = pytest.mark.gpu

SAMPLES = 48000                                   # 3 s at 16 kHz: 149 frames
LENS16 = [48000, 41230, 47999, 33100, 48000, 44800, 39017, 46000, 36500, 48000, 42424, 45111, 30007, 47000, 43210, 40960]
REPEATS = 4


def _batch16(image_shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    wav = torch.zeros(16, SAMPLES)
    for i, n in enumerate(LENS16):
        wav[i, :n] = 0.3 * torch.randn(n, generator=g)
    return {"wav": wav.cuda(), "wav_len": torch.tensor(LENS16).cuda(), "image": torch.randn(16, *image_shape, generator=g).cuda(), "id": torch.arange(16).cuda() + 100}


@pytest.fixture
def det():
    """the mode on and the counters at zero; the mode as it was afterwards"""
    from speechclip_amd import ops
    was = ops._DETERMINISTIC[0]
    ops.set_deterministic(True)
    ops.det_counters(reset=True)
    yield ops
    ops.set_deterministic(was)
    ops.det_counters(reset=True)


def _step(model, batch, seed, pack="0"):
    torch.manual_seed(seed)
    np.random.seed(0)
    with TP._Env(SC_VARLEN_PACK=pack):
        model.zero_grad(set_to_none=True)
        feats, _, _ = model(batch)
        loss = model.compute_loss(feats)["loss"]
        loss.backward()
    return loss.item(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _p_base(tmp_path):
    model, _, b4 = TV._pbase_pair(False)
    return model.cuda().train(), _batch16(b4["image"].shape[1:]), "0"


def _wide_pair():
    """_pbase_pair's recipe at d = 512 (8 heads of 64; the branch's feed-forward width is 4 d = 2048), tiny CLIP, frozen towers"""
    import dataclasses
    from helpers import make_config
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.hubert import HubertConfig
    href = dataclasses.replace(HubertRefConfig.tiny(), encoder_embed_dim=512, encoder_attention_heads=8, encoder_ffn_embed_dim=1024)
    cfg = make_config(d_model=512, branch_heads=8, hubert_config=HubertConfig(**dataclasses.asdict(href)),
                      clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))
    torch.manual_seed(5)
    return KWClip_GeneralTransformer(cfg)


def _p_base_wide(tmp_path):
    return _wide_pair().cuda().train(), _batch16((3, 64, 64)), "0"


def _c_base(tmp_path):
    model, b4 = TQ._cascaded_model(tmp_path, None)
    model.cascaded_branch.train()                 # train-mode BatchNorm, the branch's dropouts on; the frozen towers stay in eval mode
    model.clip.eval()
    return model, _batch16(b4["image"].shape[1:]), "0"


def _layers(pack):
    def make(tmp_path):
        model, _, b4 = TP._pair([1, 2])
        return model.cuda().train(), _batch16(b4["image"].shape[1:]), pack
    return make


def _whole_encoder(tmp_path):
    model, _, b4 = TF._finetune_pair([], everything=True)
    return model.cuda().train(), _batch16(b4["image"].shape[1:]), "0"


def _image_tower(tmp_path):
    model, _, b4 = TV._pbase_pair(True)
    return model.cuda().train(), _batch16(b4["image"].shape[1:]), "0"


CONFIGS = {"p_base_tail": _p_base, "p_base_tail_wide": _p_base_wide, "c_base": _c_base, "layers_padded": _layers("0"), "layers_packed": _layers("1"), "whole_encoder": _whole_encoder,
           "image_tower": _image_tower}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_four_steps_from_one_seed_are_bitwise_equal(name, det, tmp_path):
    model, batch, pack = CONFIGS[name](tmp_path)
    l0, g0 = _step(model, batch, 3, pack)
    counts = det.det_counters()
    print(name, "loss", l0, "gradients", len(g0), "deterministic paths taken in one step:", counts)
    assert np.isfinite(l0) and g0 and all(bool(torch.isfinite(v).all()) for v in g0.values())
    head = TP.ATOMIC_HEAD_GRADS & set(g0)
    if name != "c_base":
        assert head == TP.ATOMIC_HEAD_GRADS, sorted(TP.ATOMIC_HEAD_GRADS - head)
    assert counts["cls_pool_bwd"] >= 1, counts          # every configuration trains a pooling head
    assert counts["colsum_chunks"] >= 1, counts         # ... whose 16 x nsplit = 256 partial rows are summed in 4 chunks
    if name == "p_base_tail_wide":                      # all three paths in one step
        assert counts["sgemm_split"] >= 2, counts       # K = 2048: linear2 forward, and the gradient through linear1 added onto the residual's (beta = 1)
    for _ in range(REPEATS - 1):
        l1, g1 = _step(model, batch, 3, pack)
        assert l1 == l0 and set(g1) == set(g0)
        diff = sorted(k for k in g0 if not torch.equal(g0[k], g1[k]))
        assert not diff, (name, "gradients that differ between two steps from one seed", diff)
    l2, g2 = _step(model, batch, 4, pack)
    assert any(not torch.equal(g0[k], g2[k]) for k in g0), "another seed gave the same gradients: the dropouts are not on"


def _fit_once():
    from speechclip_amd.task import TrainKWClip_GeneralTransformer
    model = _wide_pair()
    batch = _batch16((3, 64, 64))
    model.config.audio_encoder.optim.args.lr = 1e-3
    model.config.audio_encoder.scheduler.warmup = 1
    opts, orig = [], model.configure_optimizers

    def capture():
        r = orig()
        opts.append(r[0][0])
        return r
    model.configure_optimizers = capture
    torch.manual_seed(7)
    np.random.seed(0)
    hist = TrainKWClip_GeneralTransformer.fit(model, [batch] * 20)
    torch.cuda.synchronize()
    (opt,) = opts
    return hist, {k: v.detach().clone() for k, v in model.state_dict().items()}, opt.m.clone(), opt.v.clone()


def test_twenty_fit_steps_twice_give_equal_losses_parameters_and_moments(det):
    from speechclip_amd.train_tail import FusedAdam  # noqa: F401
    h0, sd0, m0, v0 = _fit_once()
    c = det.det_counters()
    h1, sd1, m1, v1 = _fit_once()
    print("loss history:", h0)
    assert len(h0) == 20 and all(np.isfinite(h0)) and h0[-1] < h0[0] and c["cls_pool_bwd"] == 20 and c["colsum_chunks"] >= 20 and c["sgemm_split"] >= 20, (h0, c)
    assert h1 == h0
    assert set(sd0) == set(sd1)
    diff = sorted(k for k in sd0 if not torch.equal(sd0[k], sd1[k]))
    assert not diff, diff
    assert torch.equal(m0, m1) and torch.equal(v0, v1) and bool(m0.abs().sum() > 0) and bool(v0.abs().sum() > 0)


def _existing(name, tmp_path):
    return {
        "tail_vs_reference_glue": lambda: TT.test_tail_gradients_vs_reference_glue("tiny_base_p", False),
        "tail_vs_reference_glue_large": lambda: TT.test_tail_gradients_vs_reference_glue("tiny_large_p", True),
        "tail_isolated_vs_oracle": lambda: TT.test_tail_backward_isolated_vs_oracle_autograd("tiny_base_p", False),
        "cascaded_vs_reference_glue": lambda: TT.test_cascaded_tail_gradients_vs_reference_glue(tmp_path),
        "cascaded_isolated_vs_oracle": lambda: TT.test_cascaded_tail_backward_isolated_vs_oracle_autograd(tmp_path),
        "layers_vs_oracle": lambda: TF.test_finetune_gradients_vs_oracle_autograd([1, 2]),
        "layers_packed_vs_oracle": lambda: TP.test_packed_finetune_gradients_vs_oracle_autograd([1, 2], False),
        "whole_encoder_vs_oracle": lambda: TF.test_full_encoder_training_gradients_vs_oracle_autograd(False),
        "image_tower_vs_oracle": lambda: TV.test_end_to_end_gradients_vs_the_oracles_autograd(),
    }[name]


EXISTING = ("tail_vs_reference_glue", "tail_vs_reference_glue_large", "tail_isolated_vs_oracle", "cascaded_vs_reference_glue", "cascaded_isolated_vs_oracle",
            "layers_vs_oracle", "layers_packed_vs_oracle", "whole_encoder_vs_oracle", "image_tower_vs_oracle")


@pytest.mark.parametrize("name", EXISTING)
def test_gradient_checks_of_the_default_path_pass_with_the_mode_on(name, det, tmp_path):
    """the existing test's own body and thresholds, nothing restated; the counter shows that its backward took the fixed-order pooling backward"""
    _existing(name, tmp_path)()
    c = det.det_counters()
    print(name, c)
    assert c["cls_pool_bwd"] >= 1, c


def test_torchs_flag_alone_selects_the_mode_and_the_step_runs_under_it(tmp_path):
    """torch.use_deterministic_algorithms(True) with the project's own switch off: the step takes the three fixed-order paths, none of the project's torch
    plumbing raises under the flag, and two steps from one seed are bitwise equal.  The flag is read, never set: it is as the test left it afterwards."""
    from speechclip_amd import ops
    was, torch_was = ops._DETERMINISTIC[0], torch.are_deterministic_algorithms_enabled()
    ops.set_deterministic(False)
    torch.use_deterministic_algorithms(True)
    try:
        ops.det_counters(reset=True)
        model, batch, pack = _p_base_wide(tmp_path)
        l0, g0 = _step(model, batch, 3, pack)
        c = ops.det_counters()
        assert c["sgemm_split"] >= 2 and c["colsum_chunks"] >= 1 and c["cls_pool_bwd"] == 1, c
        assert torch.are_deterministic_algorithms_enabled() and ops._DETERMINISTIC[0] is False
        l1, g1 = _step(model, batch, 3, pack)
        assert l1 == l0 and not [k for k in g0 if not torch.equal(g0[k], g1[k])]
    finally:
        torch.use_deterministic_algorithms(torch_was)
        ops.set_deterministic(was)


def test_counters_stay_at_zero_with_the_mode_off(tmp_path):
    from speechclip_amd import ops
    if torch.are_deterministic_algorithms_enabled():
        pytest.fail("torch.use_deterministic_algorithms is on in this process: the mode cannot be switched off")
    was = ops._DETERMINISTIC[0]
    ops.set_deterministic(False)
    try:
        ops.det_counters(reset=True)
        model, batch, pack = _layers("0")(tmp_path)
        loss, grads = _step(model, batch, 3, pack)
        assert np.isfinite(loss) and TP.ATOMIC_HEAD_GRADS <= set(grads)
        assert ops.det_counters() == {"sgemm_split": 0, "colsum_chunks": 0, "cls_pool_bwd": 0}
    finally:
        ops.set_deterministic(was)

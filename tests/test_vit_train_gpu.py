"""GPU: fine-tuning the CLIP image tower (`clip.image_encoder_trainable: true`, speechclip_amd/train_vit.py) on the two tiny towers of tests/vit_train_ref.py:
the differentiable forward is the eval forward bit for bit, all 32 `visual` gradients against fp64 autograd, the whole P-base step against the oracle's autograd,
bitwise reproducibility, a short optimizer run with the eval path repacking, and the frozen model still on its old path.

Bounds of the gradient tests: cosine > 0.97 and |norm ratio - 1| < 0.12 per tensor, the project's bounds for the same pre-LN layer bodies on a bf16 gradient
stream (test_finetune_gpu.py::test_finetune_pre_ln_layers_vs_oracle_autograd).  Measured on MI355X: profiles/vit_train_parity.txt."""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

import vit_train_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS_MIN, RATIO_TOL = 0.97, 0.12


@pytest.fixture(scope="module")
def towers():
    """name -> (ClipModel on the GPU, image on the GPU, w on the GPU, fp64 oracle feat, fp64 oracle gradients): built once, left unchanged"""
    out = {}
    for name in sorted(V.TOWERS):
        model, ref, image, w = V.make_tower(name)
        feat, grads = V.oracle_visual_grads(ref, image, w)
        out[name] = (model.cuda(), image.cuda(), w.float().cuda(), feat, grads)
    return out


def _backward(model, image, w):
    for p in model.parameters():
        p.grad = None
    feat = model.encode_image(image)
    assert feat.requires_grad
    (feat * w).sum().backward()
    return feat.detach(), {k: p.grad.clone() for k, p in model.model.visual.named_parameters()}


@pytest.mark.parametrize("name", sorted(V.TOWERS))
def test_differentiable_forward_is_bitwise_the_eval_forward(towers, name):
    model, image, w, ref_feat, _ = towers[name]
    with torch.no_grad():
        ev = model.encode_image(image)
    assert not ev.requires_grad
    tr = model.encode_image(image)
    assert tr.requires_grad and tr.grad_fn is not None
    assert torch.equal(tr.detach(), ev)
    c, ratio = V.cos_ratio(ev, ref_feat)
    print(f"{name}: forward vs the fp64 oracle: cosine {c:.5f} norm ratio {ratio:.4f}")
    assert c > 0.999


@pytest.mark.parametrize("name", sorted(V.TOWERS))
def test_all_32_gradients_vs_fp64_autograd(towers, name):
    model, image, w, _, ref = towers[name]
    _, got = _backward(model, image, w)
    assert sorted(got) == sorted(ref) and len(ref) == 32
    rows = []
    for k, r in ref.items():
        assert r.norm().item() > 1e-7, k                    # by the seed (test_vit_train_host.py): nothing is skipped
        assert got[k] is not None and got[k].shape == r.shape and got[k].dtype == torch.float32, k
        rows.append((k, *V.cos_ratio(got[k], r)))
    worst_c, worst_r = min(rows, key=lambda t: t[1]), max(rows, key=lambda t: abs(t[2] - 1))
    print(f"{name}: worst cosine {worst_c[1]:.5f} ({worst_c[0]}); worst norm ratio {worst_r[2]:.4f} ({worst_r[0]})")
    for k, c, ratio in rows:
        print(f"    {k:55s} cos {c:.5f} ratio {ratio:.4f}")
    for k, c, ratio in rows:
        assert c > COS_MIN and abs(ratio - 1) < RATIO_TOL, (name, k, c, ratio)
    # softmax is invariant to a key bias: the exact gradient of in_proj_bias's k slice is 0; here it is the rounding noise of the bf16 dK rows
    d = 128
    for k, gk in got.items():
        if k.endswith("in_proj_bias"):
            q, kk, v = gk[:d].norm().item(), gk[d:2 * d].norm().item(), gk[2 * d:].norm().item()
            print(f"    {k}: |q| {q:.3e} |k| {kk:.3e} |v| {v:.3e}")
            assert kk < 0.05 * min(q, v), (k, q, kk, v)


@pytest.mark.parametrize("name", sorted(V.TOWERS))
def test_two_backward_passes_are_bitwise_equal(towers, name):
    model, image, w, _, _ = towers[name]
    f1, g1 = _backward(model, image, w)
    f2, g2 = _backward(model, image, w)
    assert torch.equal(f1, f2) and len(g1) == 32
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _pbase_pair(trainable):
    """Tiny P-base model with the T17 image tower + the fp32 oracle with the same weights, B = 4."""
    from helpers import make_config
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from oracle.speechclip_ref import SpeechClipRef
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.hubert import HubertConfig
    href, ccfg = HubertRefConfig.tiny(), V.tower_config("T17")
    cfg = make_config(d_model=128, branch_heads=4, hubert_config=HubertConfig(**dataclasses.asdict(href)), clip_config=ccfg)
    cfg.clip.image_encoder_trainable = trainable
    torch.manual_seed(5)
    model = KWClip_GeneralTransformer(cfg)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for k, p in model.clip.model.visual.named_parameters():
            if "ln_" in k or k.endswith(".bias") or k.endswith("in_proj_bias"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    ref = SpeechClipRef(href, ClipRefConfig(**dataclasses.asdict(ccfg)), parallel=True, branch_heads=4).eval()
    sd = model.state_dict()
    ref.encoder.load_state_dict({k[len("audio_encoder.encoder."):]: v for k, v in sd.items() if k.startswith("audio_encoder.encoder.")})
    ref.clip.load_state_dict({k[len("clip.model."):]: v for k, v in sd.items() if k.startswith("clip.model.")})
    ref.parallel_branch.load_state_dict({k[len("parallel_branch."):]: v for k, v in sd.items() if k.startswith("parallel_branch.")})
    with torch.no_grad():
        ref.ws_weights.copy_(sd["audio_encoder.weightedsum_layer.weights"])
    lens = [8000, 5200, 8000, 3100]
    wav = torch.zeros(4, 8000)
    for i, l in enumerate(lens):
        wav[i, :l] = 0.3 * torch.randn(l, generator=g)
    batch = {"wav": wav, "wav_len": torch.tensor(lens), "image": torch.randn(4, 3, 56, 56, generator=g), "id": torch.tensor([1, 2, 3, 4])}
    return model, ref, batch


def test_end_to_end_gradients_vs_the_oracles_autograd():
    from oracle import speechclip_ref as R
    model, ref, batch = _pbase_pair(True)
    model = model.cuda().eval()                                  # eval(): no dropout in the branch; gradients still flow (grad mode is on)
    feats, _, _ = model({k: v.cuda() for k, v in batch.items()})
    assert feats["image_feat"].requires_grad and feats["parallel_audio_feat"].requires_grad
    loss = model.compute_loss(feats)["loss"]
    loss.backward()
    for p in ref.parameters():
        p.requires_grad_(False)
    for p in list(ref.clip.visual.parameters()) + list(ref.parallel_branch.parameters()):
        p.requires_grad_(True)
    audio_feat, audio_len, _ = ref.forward_audio(batch["wav"], batch["wav_len"])          # the frozen speech encoder
    with torch.enable_grad():
        pa = R.l2_normalize(ref.parallel_branch(audio_feat, audio_len))
        img = R.l2_normalize(ref.clip.encode_image(batch["image"]))
        ref_loss = R.masked_contrastive_loss(pa, img, batch["id"], ref.inv_temperature)
    ref_loss.backward()
    print(f"loss hip {loss.item():.5f} oracle {ref_loss.item():.5f}")
    assert abs(loss.item() - ref_loss.item()) < 2e-2
    mine = dict(model.named_parameters())
    rows = []
    for k, p in ref.clip.visual.named_parameters():
        got = mine["clip.model.visual." + k].grad
        assert got is not None and p.grad.norm().item() > 1e-7, k
        rows.append((k, *V.cos_ratio(got, p.grad)))
    worst_c, worst_r = min(rows, key=lambda t: t[1]), max(rows, key=lambda t: abs(t[2] - 1))
    print(f"end to end: worst cosine {worst_c[1]:.5f} ({worst_c[0]}); worst norm ratio {worst_r[2]:.4f} ({worst_r[0]})")
    assert len(rows) == 32
    for k, c, ratio in rows:
        assert c > COS_MIN and abs(ratio - 1) < RATIO_TOL, (k, c, ratio)
    for k, p in ref.parallel_branch.named_parameters():         # the branch's gradients: the assertion of test_finetune_gpu.py's gradient tests
        got = mine["parallel_branch." + k].grad
        if p.grad.norm().item() > 1e-6:
            assert V.cos_ratio(got, p.grad)[0] > 0.98, k
    assert all(p.grad is None for k, p in mine.items() if k.startswith("clip.model.") and not k.startswith("clip.model.visual."))


def test_short_run_trains_the_tower_and_the_eval_path_repacks():
    model, _, batch = _pbase_pair(True)
    model = model.cuda().eval()                                  # deterministic steps: no branch dropout
    batch = {k: v.cuda() for k, v in batch.items()}
    clip, image = model.clip, batch["image"]
    model.config.audio_encoder.optim.args.lr = 1e-3
    model.config.audio_encoder.scheduler.warmup = 1
    (opt,), (sch,) = model.configure_optimizers()
    from speechclip_amd.train_tail import FusedAdam
    assert isinstance(opt, FusedAdam)
    vis = clip.model.visual
    conv0, last0 = vis.conv1.weight.detach().clone(), vis.transformer.resblocks[-1].mlp.c_proj.weight.detach().clone()
    text0 = clip.model.text_projection.detach().clone()
    with torch.no_grad():
        before = clip.encode_image(image).clone()               # packs the eval operands
    losses = []
    for step in range(5):
        opt.zero_grad()
        loss = model.training_step_end(model.training_step(batch, step))["loss"]
        loss.backward()
        opt.step()
        sch["scheduler"].step()
        losses.append(loss.item())
    print("losses:", losses)
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert not torch.equal(conv0, vis.conv1.weight) and not torch.equal(last0, vis.transformer.resblocks[-1].mlp.c_proj.weight)
    assert torch.equal(text0, clip.model.text_projection)
    with torch.no_grad():
        after = clip.encode_image(image).clone()
    assert not torch.equal(after, before), "the eval path still runs on the pre-step packed operands"
    assert torch.equal(after, clip.encode_image(image).detach())          # the differentiable forward reads the parameters themselves
    # the same after one plain torch optimizer step (it moves the tensors' _version, not the parameter epoch)
    sgd = torch.optim.SGD(clip.trainable_params(), lr=0.05)
    sgd.zero_grad()
    clip.encode_image(image).square().sum().backward()
    sgd.step()
    with torch.no_grad():
        after_sgd = clip.encode_image(image)
    assert not torch.equal(after_sgd, after), "the eval path still runs on the operands packed before the SGD step"
    assert torch.equal(after_sgd, clip.encode_image(image).detach())


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_vit_train_gpu as T
model, _, batch = T._pbase_pair(False)
model = model.cuda().eval()
with torch.no_grad():
    f = model({k: v.cuda() for k, v in batch.items()})[0]
torch.save({k: f[k].cpu() for k in ("image_feat", "parallel_audio_feat")}, sys.argv[2])
"""


def test_frozen_towers_take_the_old_path(tmp_path):
    """Both flags false: forward() gives the image feature of the unchanged eval function (ops.l2norm of CLIP.encode_image under no_grad), nothing of the image
    side carries a gradient, and the side-stream forward equals the serial one (SC_OVERLAP_VIT=0) of a fresh process bit for bit."""
    from speechclip_amd import ops
    from speechclip_amd.model import kwClip
    model, _, batch = _pbase_pair(False)
    model = model.cuda().eval()
    batch = {k: v.cuda() for k, v in batch.items()}
    assert model.clip.trainable_params() == [] and not model.clip.image_encoder_trainable
    feats = model(batch)[0]                                     # grad mode on, as in a training step of the branch
    assert not feats["image_feat"].requires_grad and feats["parallel_audio_feat"].requires_grad
    with torch.no_grad():
        direct = ops.l2norm(model.clip.model.encode_image(batch["image"]))
        f0 = model(batch)[0]
    assert torch.equal(feats["image_feat"], direct) and torch.equal(f0["image_feat"], direct)
    if kwClip._OVERLAP_IMAGE_TOWER:
        out = str(tmp_path / "serial.pt")
        env = dict(os.environ, SC_OVERLAP_VIT="0")
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=env, cwd=ROOT, timeout=300)
        serial = torch.load(out)
        for k in serial:
            assert torch.equal(f0[k].cpu(), serial[k]), k

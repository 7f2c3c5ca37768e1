"""Padding-free WHOLE-ENCODER training (bare `audio_encoder.trainable: true` under SC_VARLEN_PACK=1): the front-end node (train_front.HubertFront[LN]TrainFn
with meta["pack"]), every transformer layer and the layer mix run on packed rows.  That the step ran packed, its gradients against the padded step and against
the fp32 oracle's autograd (base and large), that a gradient stays inside its utterance at every conv level, train-mode determinism with the two front-end
dropouts, and the hidden states handed back in the reference's [B, T, d] layout."""
import dataclasses
import functools

import pytest
import torch

from test_finetune_gpu import _finetune_pair
from test_finetune_packed_gpu import ATOMIC_HEAD_GRADS, LENS, _cos, _Env, _step

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_LAYERS = 3


@functools.lru_cache(maxsize=None)
def _steps(large):
    """The whole-encoder model of test_finetune_gpu (`_finetune_pair([], everything=True)`: tiny, 3 layers, lens [8000, 5200, 8000, 3100]), one step under
    SC_VARLEN_PACK=0 and one under =1, and the oracle's autograd on the same weights and batch -- computed once, shared by the tests below, not modified."""
    from oracle import hubert_ref as HR
    from oracle import speechclip_ref as R
    model, ref, batch = _finetune_pair([], everything=True, large=large)
    model = model.cuda().eval()
    assert model.audio_encoder.train_front
    spy0, spy1 = dict(attention_bwd_packed=0, attn_bwd_probs=0), dict(attention_bwd_packed=0, attn_bwd_probs=0)
    padded_step = _step(model, batch, "0", spy0)
    packed_step = _step(model, batch, "1", spy1)
    for p in ref.parameters():
        p.requires_grad_(False)
    for k, p in ref.encoder.named_parameters():
        p.requires_grad_(not k.startswith(("mask_emb", "final_proj", "label_embs_concat") + (("encoder.layer_norm",) if large else ())))
    for p in ref.parallel_branch.parameters():
        p.requires_grad_(True)
    ref.ws_weights.requires_grad_(True)
    ref.encoder.feature_grad_mult = 1.0 if large else 0.1
    wavs = [batch["wav"][b, :int(batch["wav_len"][b])] for b in range(4)]
    padded, mask = HR.preprocess_input(wavs, ref.hubert_cfg.normalize)
    with torch.enable_grad():
        hidden = HR.hubert_forward.__wrapped__(ref.encoder, padded, mask)["layer_results"]
        flen = HR.feat_lengths([len(w) for w in wavs], 320, hidden[-1].shape[1])
        pa = R.l2_normalize(ref.parallel_branch(R.weighted_sum(hidden, ref.ws_weights, large), flen))
        with torch.no_grad():
            img = R.l2_normalize(ref.clip.encode_image(batch["image"]))
        ref_loss = R.masked_contrastive_loss(pa, img, batch["id"], ref.inv_temperature)
    ref_loss.backward()
    return dict(padded=padded_step, packed=packed_step, spy0=spy0, spy1=spy1, ref=ref, ref_loss=ref_loss.item())


@pytest.mark.parametrize("large", [False, True])
def test_whole_encoder_step_ran_packed(large):
    s = _steps(large)
    plans0, plans1 = s["padded"][2], s["packed"][2]
    assert len(plans1) == 1 and plans1[0] is not None and plans1[0]["total"] < plans1[0]["padded_rows"], plans1
    assert s["spy1"] == dict(attention_bwd_packed=N_LAYERS, attn_bwd_probs=0), s["spy1"]
    assert len(plans0) == 1 and plans0[0] is None, plans0
    assert s["spy0"] == dict(attention_bwd_packed=0, attn_bwd_probs=N_LAYERS), s["spy0"]
    geo = plans1[0]
    b = LENS.index(3100)
    assert geo["rows"][b] == max(geo["valid"][b], min(round(3100 / 320), geo["T"])) + 1


@pytest.mark.parametrize("large", [False, True])
def test_packed_whole_encoder_step_matches_the_padded_step(large):
    """Loss and EVERY gradient (all 18 / 35 front-end tensors, all layers, the branch, the mix weights) at the thresholds of
    test_finetune_packed_gpu.test_packed_step_matches_padded_step_and_runs_the_new_backward."""
    s = _steps(large)
    (loss0, g0, _), (loss1, g1, _) = s["padded"], s["packed"]
    print("loss padded", loss0, "packed", loss1)
    assert abs(loss0 - loss1) < 2e-2, (loss0, loss1)
    assert set(g0) == set(g1)
    front = [k for k in g0 if k.startswith("audio_encoder.encoder.") and ".layers." not in k]
    assert len(front) == (35 if large else 18), front
    assert len([k for k in g0 if ".encoder.layers." in k]) == 16 * N_LAYERS and "audio_encoder.weightedsum_layer.weights" in g0
    for k in g0:
        n0 = g0[k].norm().item()
        if n0 < 1e-7:
            assert g1[k].norm().item() < 1e-4, k
            continue
        c, ratio = _cos(g1[k], g0[k]), g1[k].norm().item() / n0
        print(f"{k}: cosine {c:.5f} ratio {ratio:.4f}")
        assert c > 0.98 and abs(ratio - 1) < 0.1, (k, c, ratio)


@pytest.mark.parametrize("large", [False, True])
def test_packed_whole_encoder_gradients_vs_oracle_autograd(large):
    """The assertions and thresholds of test_finetune_gpu.test_full_encoder_training_gradients_vs_oracle_autograd on the packed step."""
    s = _steps(large)
    loss, mine, plans = s["packed"]
    ref = s["ref"]
    assert plans[0] is not None
    print("loss", loss, "oracle", s["ref_loss"])
    assert abs(loss - s["ref_loss"]) < 2e-2
    checked, worst = 0, (1.0, "")
    for k, p in ref.encoder.named_parameters():
        got = mine.get("audio_encoder.encoder." + k)
        if not p.requires_grad:
            assert got is None, k
            continue
        assert got is not None and p.grad is not None, k
        if p.grad.norm().item() < 1e-7:
            assert got.norm().item() < 1e-4, k
            continue
        c, ratio = _cos(got, p.grad), got.norm().item() / p.grad.norm().item()
        print(f"{k}: cosine {c:.5f} norm ratio {ratio:.4f}")
        worst = min(worst, (c, k))
        assert c > 0.97 and abs(ratio - 1) < 0.12, (k, c, ratio)
        checked += 1
    print("full-encoder gradients checked:", checked, "worst cosine:", worst)
    assert checked >= (35 if large else 18) + 3 * 12
    assert _cos(mine["audio_encoder.weightedsum_layer.weights"], ref.ws_weights.grad) > 0.97


def _front_model(large):
    from oracle.hubert_ref import HubertModelRef, HubertRefConfig, randomize_norm_affine
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    href = HubertRefConfig.tiny(layer_norm_first=True, extractor_mode="layer_norm", conv_bias=True) if large else HubertRefConfig.tiny()
    torch.manual_seed(11)
    ref = HubertModelRef(href)
    randomize_norm_affine(ref, torch.Generator().manual_seed(5))
    enc = HubertModel(HubertConfig(**dataclasses.asdict(href)))
    enc.load_state_dict(ref.state_dict())
    return enc.cuda()


@pytest.mark.parametrize("large", [False, True])
def test_gradient_stays_inside_its_utterance(large):
    """The front node's backward driven with a dh0 that is non-zero on the rows < valid_b of utterance 1 only: at every conv level the input gradient is
    exactly zero outside that utterance's row range (the halo row and the rows that read a neighbour's samples meet a zero gradient), the other utterances'
    conv0 partials are exactly zero, and changing the NEIGHBOUR's wave (utterance 2, whose samples utterance 1's last rows read) changes neither utterance 1's
    partials nor its dxp rows by a bit."""
    from speechclip_amd import ops
    from speechclip_amd.train_front import HubertFrontLNTrainFn, HubertFrontTrainFn, front_params, front_params_ln
    enc = _front_model(large)
    cfg = enc.cfg
    L, B, who = 8000, len(LENS), 1
    T0, T, P0, Tp = enc.frame_geometry(L)
    geo = enc.packed_geometry(LENS, L, need_rows=[min(round(l / 320), T) for l in LENS])
    off, total, valid = geo["row_off"], geo["total"], geo["valid"]
    dev = torch.device("cuda")
    off_d, valid_d = ops.dev_ints(off, torch.int32, dev), ops.dev_ints(valid, torch.int32, dev)
    g = torch.Generator().manual_seed(3)
    wav = torch.zeros(B, L)
    for i, l in enumerate(LENS):
        wav[i, :l] = 0.3 * torch.randn(l, generator=g)
    d = cfg.encoder_embed_dim
    dh0 = torch.zeros(total, d)
    dh0[off[who]:off[who] + valid[who]] = torch.randn(valid[who], d, generator=g)
    prm = front_params_ln(enc) if large else front_params(enc)
    for p in prm:
        p.requires_grad_(True)

    def run(w):
        trace = {}
        meta = dict(conv_layers=[tuple(c) for c in cfg.conv_layers], T0=T0, P0=P0, Tp=Tp, d=d, G=cfg.conv_pos_groups, Kw=cfg.conv_pos, grad_mult=0.1,
                    normalize=bool(cfg.normalize), trace=trace, pack=dict(row_off=off_d, rows_max=geo["rows_max"], total=total, scale0=geo["scale0"]))
        for p in prm:
            p.grad = None
        if large:
            h0 = HubertFrontLNTrainFn.apply(meta, w.cuda(), ops.dev_ints(LENS, torch.int32, dev), valid_d, *prm)
        else:
            h0 = HubertFrontTrainFn.apply(meta, w.cuda(), valid_d, *prm)
        assert h0.shape == (total, d) and bool(torch.isfinite(h0.float()).all())
        h0.backward(dh0.to(h0.dtype).cuda())
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in trace.items()}, [p.grad.detach().clone() for p in prm]

    tr, grads = run(wav)
    assert all(bool(torch.isfinite(x).all()) for x in grads) and grads[0].abs().sum().item() > 0
    assert set(tr) == {"dxp", "conv0_part"} | {f"dx{l}" for l in range(6)}
    lo, hi = off[who], off[who + 1]
    dxp = tr["dxp"]
    assert dxp.shape == (total, d) and bool((dxp[:lo] == 0).all()) and bool((dxp[hi:] == 0).all()) and bool((dxp[lo + valid[who]:hi] == 0).all())
    assert dxp[lo:hi].abs().sum().item() > 0
    for l in range(6):          # dx{l}: the gradient of conv layer l's output = the input gradient of layer l + 1, 2^(6 - l) rows per transformer row
        sc = 2 ** (6 - l)
        gl = tr[f"dx{l}"]
        assert gl.shape[0] == sc * total, (l, gl.shape)
        assert bool((gl[:sc * lo] == 0).all()) and bool((gl[sc * hi:] == 0).all()), l
        assert gl[sc * lo:sc * hi].abs().sum().item() > 0, l
    part = tr["conv0_part"]
    assert part.shape == (B, cfg.conv_layers[0][0], 12)
    for b in range(B):
        assert (b == who) == bool((part[b] != 0).any()), b
    wav2 = wav.clone()
    wav2[who + 1, :LENS[who + 1]] = 0.5 * torch.randn(LENS[who + 1], generator=g) + 0.2
    tr2, _ = run(wav2)
    assert torch.equal(tr2["conv0_part"][who], part[who]) and torch.equal(tr2["dxp"][lo:hi], dxp[lo:hi])
    for l in range(6):
        sc = 2 ** (6 - l)
        assert torch.equal(tr2[f"dx{l}"][sc * lo:sc * hi], tr[f"dx{l}"][sc * lo:sc * hi]), l


def test_packed_whole_encoder_train_mode_with_dropouts_is_reproducible():
    """Train mode, base model (dropout_input on the projected features, F.dropout on hidden state 0, the layers' own dropouts): the same torch seed gives a
    bitwise equal loss and bitwise equal gradients over three repeats, except the four head gradients that fp32 atomics reduce (ATOMIC_HEAD_GRADS); another
    seed changes the front end's gradients."""
    import numpy as np
    model, _, batch = _finetune_pair([], everything=True)
    model = model.cuda().train()
    rates = model.audio_encoder.encoder.dropout_rates()
    assert rates["features"] > 0 and rates["hidden"] > 0, rates

    def run(seed):
        torch.manual_seed(seed)
        np.random.seed(0)
        return _step(model, batch, "1")

    l0, g0, plans = run(3)
    assert len(plans) == 1 and plans[0] is not None
    assert np.isfinite(l0) and all(bool(torch.isfinite(v).all()) for v in g0.values())
    front = [k for k in g0 if k.startswith("audio_encoder.encoder.") and ".layers." not in k]
    assert len(front) == 18
    for _ in range(3):
        l1, g1, _ = run(3)
        assert l1 == l0 and set(g1) == set(g0)
        diff = {k for k in g0 if not torch.equal(g0[k], g1[k])}
        assert diff <= ATOMIC_HEAD_GRADS, sorted(diff - ATOMIC_HEAD_GRADS)
    l2, g2, _ = run(4)
    assert any(not torch.equal(g0[k], g2[k]) for k in front)


@pytest.mark.parametrize("large", [False, True])
def test_packed_whole_encoder_returns_padded_hidden_states(large):
    """The assertions of test_finetune_packed_gpu.test_packed_finetune_returns_padded_hidden_states with the whole encoder trainable: every state, hidden state 0
    (the front-end node's output) included, comes back as [B, T, d] attached to the graph."""
    model, _, batch = _finetune_pair([], everything=True, large=large)
    model = model.cuda().eval()
    enc = model.audio_encoder
    wav, wl = batch["wav"].cuda(), batch["wav_len"].cuda()
    outs, attached = {}, {}
    for pack in ("0", "1"):
        with _Env(SC_VARLEN_PACK=pack):
            feat, flen, hidden = enc(wav, wl, return_hidden_states=True)
        assert feat.requires_grad
        attached[pack] = [bool(h.requires_grad) for h in hidden]
        outs[pack] = (feat.detach().float().cpu(), flen.cpu(), [h.detach().float().cpu() for h in hidden])
    nl = enc.encoder.cfg.encoder_layers
    assert attached["1"] == attached["0"] and all(attached["1"])
    (f0, l0, h0), (f1, l1, h1) = outs["0"], outs["1"]
    assert torch.equal(l0, l1) and len(h1) == nl + 1 and f1.shape == f0.shape
    B, T, d = f0.shape
    for a, b in zip(h0, h1):
        assert b.shape == (B, T, d) and a.shape == (B, T, d)
        for u in range(B):
            n = int(l0[u])
            err = (a[u, :n] - b[u, :n]).abs().max().item()
            print(f"utterance {u}: max|packed - padded| {err:.3e} (max|state| {a[u, :n].abs().max().item():.3f})")
            assert err < 5e-2, (u, err)
            valid = enc.encoder.valid_frames(LENS, 8000, T)[u]
            assert bool((b[u, max(n, valid):] == 0).all()), u
    for u in range(B):
        n = int(l0[u])
        assert (f0[u, :n] - f1[u, :n]).abs().max().item() < 5e-2

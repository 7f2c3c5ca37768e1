"""GPU checks of the quantizer's soft / gumbel modes (csrc/vq_modes.hip) through the C ABI wrappers, each against the float64 restatement of
tests/vq_modes_ref.py on the same fp32 inputs (my_vector_quantizer.py:75-79, :124-131; F.gumbel_softmax; kwClip.py:889-911), the reference class's own
outputs (tests/golden/vq_modes.npz) and, at branch level, one train step of the tiny cascaded model per mode.

Bounds.  keywords: |kw - ref| / |ref| < 2e-5 (the fp32-grade bound of the three-term bf16 products, tests/test_boundary_gpu.py).  Noise: 1e-5 (4 ulp at 16.6).
Probabilities: 1e-6 absolute where the arithmetic allows it -- an fp32 noise value carries up to one ulp, 4.8e-7 for g in [4, 8) where a row's winner sits, and
a probability moves by p (1 - p) / T <= 1 / (4 T) times the error of a logit difference: with noise the 1e-6 bound needs T >= 0.5 (2 * 4.8e-7 / (4 * 0.5) = 4.8e-7),
so the noisy cases run at T = 1.0 and 0.5 and the T = 0.1 case runs noise-free; against the fixture at T = 0.1 with noise, where the reference's fp32 logits
carry the same error again, the bound is 2 * 2 * 4.8e-7 / (4 * 0.1) = 4.8e-6 -> 5e-6 (measured for gumbel_soft at T = 0.1: |gpu - reference class| 2.74e-6,
|gpu - float64| 1.65e-6, |reference class - float64| 1.23e-6; every other fixture case is below 3e-7 and held to 1e-6).  Gradients: max |d| < 2e-4 max(scale, 1e-3), the bound of
test_train_kernels_gpu.py::test_vq_straight_through_and_cosine_bwd; d loss / d T: 1e-3 relative."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vq_modes_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 11          # every row of every arg-max case below has a float64 top-2 gap of x + g above 1e-4 at this seed (asserted where it is used)


def dev():
    return torch.device("cuda", 0)


def _scores(Rr, V):
    return np.clip(np.random.default_rng(Rr + V).normal(0, 0.3, (Rr, V)), -1, 1).astype(np.float32)          # cosine-like


def _table(V, E):
    return np.random.default_rng(V * 1000 + E).normal(0, 0.02, (V, E)).astype(np.float32)                    # CLIP's token-embedding scale (init std 0.02)


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _rel(a, ref):
    return float(np.linalg.norm(a.astype(np.float64) - ref) / np.linalg.norm(ref))


# ------------------------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("Rr,V,seed,extreme", [(5, 333, 77, None), (16, 49408, 12, (8981, "low")), (16, 49408, 9, (486993, "high"))])
def test_gumbel_noise_matches_the_contract(Rr, V, seed, extreme):
    """sc_vq_gumbel_noise vs the float64 restatement; the two big cases hold the smallest and the largest uniform the 23-bit draw can give (found by a host
    search over seeds): near u = 1 the inner logarithm is 6e-8, where a fast log's absolute error would be an order-one relative error."""
    from speechclip_amd import ops
    ref = R.gumbel_matrix(seed, Rr, V)
    if extreme is not None:
        idx, which = extreme
        u = R.uniform(seed, np.array([idx], dtype=np.uint64))[0]
        assert u == (2.0 ** -24 if which == "low" else 1 - 2.0 ** -24)
        assert abs(ref.reshape(-1)[idx] - (-2.82 if which == "low" else 16.64)) < 0.01
    g = ops.vq_gumbel_noise(Rr, V, seed, dev()).cpu().numpy().astype(np.float64)
    err = np.abs(g - ref)
    print("noise", Rr, V, seed, "max |err|", err.max(), "at g =", ref.reshape(-1)[err.argmax()])
    assert err.max() <= 1e-5
    if extreme is not None:
        assert err.reshape(-1)[extreme[0]] <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ noisy arg-max
@pytest.mark.parametrize("Rr,V", [(7, 333), (40, 1031), (16, 49408)])
def test_noisy_argmax_equals_float64_on_every_row(Rr, V):
    from speechclip_amd import ops
    x = _scores(Rr, V)
    x[0, 2] = 30.0                                                   # a masked column never wins, however large
    z = R.masked_logits(x, R.gumbel_matrix(SEED, Rr, V), 1.0)
    top = np.sort(z, -1)
    assert (top[:, -1] - top[:, -2]).min() > 1e-4                    # decisive on every row: no row is excluded
    t = ops.vq_noisy_argmax(_gpu(x), SEED).cpu().numpy()
    assert np.array_equal(t, z.argmax(-1))
    t0 = ops.vq_noisy_argmax(_gpu(x), None).cpu().numpy()            # noise off: the plain masked arg-max
    assert np.array_equal(t0, R.masked_logits(x, None, 1.0).argmax(-1))
    assert (t != t0).any()


def test_argmax_ties_go_to_the_lowest_unmasked_index():
    from speechclip_amd import ops
    x = np.full((3, 700), 0.25, np.float32)
    x[1, 5:] = 0.2
    x[2, :600] = -1.0
    assert ops.vq_noisy_argmax(_gpu(x), None).cpu().tolist() == [1, 1, 600]


# ------------------------------------------------------------------------------------------------------------------ probabilities
@pytest.mark.parametrize("Rr,V,T,seed", [(7, 333, 1.0, None), (40, 1031, 0.1, None), (7, 333, 1.0, SEED), (40, 1031, 0.5, SEED)])
def test_probs_against_float64(Rr, V, T, seed):
    from speechclip_amd import ops
    x = _scores(Rr, V)
    x[1, 0] = 9.0
    ref = R.softmax(R.masked_logits(x, R.gumbel_matrix(seed, Rr, V) if seed else None, T))
    p = ops.vq_probs(_gpu(x), T, seed).cpu().numpy().astype(np.float64)
    print("probs", Rr, V, T, seed, "max |err|", np.abs(p - ref).max())
    assert (p[:, list(R.MASK)] == 0).all()
    assert np.abs(p.sum(-1) - 1).max() < 1e-5
    assert np.abs(p - ref).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ fused soft embed
def _planted(Rr, V):
    x = _scores(Rr, V)
    x[0, 1] = 1.5                      # winner at the first unmasked column
    x[1, V - 1] = 1.5                  # winner at the last column (the short last tile of most splits)
    x[2, :] = 0.25                     # all unmasked scores equal
    x[2, list(R.MASK)] = -0.5
    x[3, 2] = 7.0                      # the largest raw score sits in a masked column
    x[4, 0] = 7.0
    x[4, 3] = 6.0
    return x


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("Rr,V,E,T", [(7, 333, 64, 1.0), (40, 1031, 512, 0.1), (24, 8112, 768, 0.07), (16, 49408, 512, 0.1)])
def test_soft_embed_against_float64(Rr, V, E, T, noise):
    from speechclip_amd import ops
    x, emb = _planted(Rr, V), _table(V, E)
    seed = SEED if noise else None
    g = R.gumbel_matrix(SEED, Rr, V) if noise else None
    z = R.masked_logits(x, g, T)
    ref = R.softmax(z) @ emb.astype(np.float64)
    s = z * T                                                          # x + g, masked at -inf
    ref_max = s.max(-1)
    ref_den = np.exp((s - ref_max[:, None]) / T).sum(-1)
    xg, eg = _gpu(x), _gpu(emb)
    mean = emb.astype(np.float64)[[v for v in range(V) if v not in R.MASK]].mean(0)
    for nsplit in (1, 2, 5, 0):                                        # 5 leaves a last chunk shorter than the others; 0 = auto
        kw, rmax, rden = ops.vq_soft_embed(xg, eg, T, seed, nsplit=nsplit, want_stats=True)
        kw = kw.cpu().numpy()
        rows = np.linalg.norm(kw - ref, axis=1) / np.linalg.norm(ref, axis=1)
        print("soft_embed", (Rr, V, E, T), "noise", noise, "nsplit", nsplit, "rel", _rel(kw, ref), "worst row", rows.max())
        assert _rel(kw, ref) < 2e-5 and rows.max() < 2e-5, (nsplit, rows)
        assert np.abs(rmax.cpu().numpy() - ref_max).max() <= (1e-5 if noise else 1e-6)       # the noise's own bound
        assert np.abs(rden.cpu().numpy() / ref_den - 1).max() < (3e-5 if noise else 1e-5)      # a logit moves by <= 2 * 4.8e-7 / T with fp32 noise
        if not noise:                                                  # the row of equal scores: the mean of the unmasked table rows
            assert np.linalg.norm(kw[2] - mean) / np.linalg.norm(mean) < 2e-5, nsplit
    again = ops.vq_soft_embed(xg, eg, T, seed)
    assert torch.equal(again, ops.vq_soft_embed(xg, eg, T, seed)) and np.array_equal(again.cpu().numpy(), kw)          # bitwise run to run


def test_soft_embed_of_a_decisive_winner_is_the_gathered_row():
    """A winner ahead by 3.0 at T = 0.05 (e^-60 for everything else): the product is that row of the table, 1e-6 absolute at the table's scale
    (|emb| <= ~0.1: the (hi, lo) bf16 pair keeps 2^-18 of it)."""
    from speechclip_amd import ops
    Rr, V, E = 7, 333, 64
    x, emb = _scores(Rr, V) * 0.1, _table(V, E)
    win = np.array([1, V - 1, 4, 17, 100, 256, 332])
    x[np.arange(Rr), win] = 3.2
    assert (np.sort(R.masked_logits(x, None, 1.0), -1)[:, -1] - np.sort(R.masked_logits(x, None, 1.0), -1)[:, -2]).min() >= 3.0
    got = ops.gather_rows(_gpu(emb), _gpu(win))
    for nsplit in (1, 2, 5, 0):
        assert (ops.vq_soft_embed(_gpu(x), _gpu(emb), 0.05, nsplit=nsplit) - got).abs().max().item() <= 1e-6, nsplit


@pytest.mark.parametrize("noise", [False, True])
def test_uncovered_table_width_goes_through_probs_and_a_gemm(noise):
    from speechclip_amd import _lib, ops
    Rr, V, E, T = 7, 333, 48, 1.0
    x, emb = _planted(Rr, V), _table(V, E)
    import ctypes
    assert _lib.lib().sc_vq_soft_embed(None, None, None, None, None, None, Rr, V, E, ctypes.c_float(T), 1, 1, None, 0, 0, None) == 1
    ref = R.softmax(R.masked_logits(x, R.gumbel_matrix(SEED, Rr, V) if noise else None, T)) @ emb.astype(np.float64)
    kw, rmax, rden = ops.vq_soft_embed(_gpu(x), _gpu(emb), T, SEED if noise else None, want_stats=True)
    assert rmax is None and _rel(kw.cpu().numpy(), ref) < 2e-5


def test_both_routes_of_the_product_agree_with_float64(monkeypatch):
    """The composed route (sc_vq_probs, then the three-term split GEMM) is what a measurement may make the default: it holds the same bound."""
    from speechclip_amd import ops
    Rr, V, E, T = 40, 1024, 512, 0.1
    x, emb = _planted(Rr, V), _table(V, E)
    ref = R.softmax(R.masked_logits(x, R.gumbel_matrix(SEED, Rr, V), T)) @ emb.astype(np.float64)
    for route in ("fused", "probs"):
        monkeypatch.setattr(ops, "VQ_SOFT_ROUTE", route)
        assert _rel(ops.vq_soft_embed(_gpu(x), _gpu(emb), T, SEED).cpu().numpy(), ref) < 2e-5, route


# ------------------------------------------------------------------------------------------------------------------ backward
def _autograd64(a, emb, dkw, T, use_gumbel, hard, seed):
    """float64 autograd of cosine -> masked (x + g) / T -> softmax -> (hard ? one-hot + y - y.detach() : y) @ emb; returns (kw, da, dT)."""
    a64 = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
    e64 = torch.from_numpy(emb.astype(np.float64))
    t64 = torch.tensor(float(T), dtype=torch.float64, requires_grad=True)
    cos = (a64 / a64.norm(dim=1, keepdim=True).clamp_min(1e-8)) @ (e64 / e64.norm(dim=1, keepdim=True).clamp_min(1e-8)).t()     # F.cosine_similarity, kwClip.py:889-897
    if use_gumbel:
        cos = cos + torch.from_numpy(R.gumbel_matrix(seed, *cos.shape))
    z = cos / t64
    msk = torch.zeros(cos.shape[1], dtype=torch.bool)
    msk[list(R.MASK)] = True
    y = torch.softmax(z.masked_fill(msk, float("-inf")), -1)
    prob = y
    if hard:
        prob = torch.zeros_like(y).scatter_(-1, y.argmax(-1, keepdim=True), 1.0) + y - y.detach()
    kw = prob @ e64
    kw.backward(torch.from_numpy(dkw.astype(np.float64)))
    return kw.detach().numpy(), a64.grad.numpy(), float(t64.grad)


@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("Rr,V,E,T", [(48, 1000, 64, 0.1), (16, 49408, 512, 0.1), (7, 333, 64, 1.0)])
def test_keyword_vq_fn_backward_against_float64_autograd(Rr, V, E, T, mode):
    from speechclip_amd import ops
    from speechclip_amd.train_tail import KeywordVQFn
    use_gumbel, hard = R.MODES[mode]
    g = torch.Generator().manual_seed(Rr + V)
    emb = torch.randn(V, E, generator=g).numpy()
    a = (torch.randn(Rr, E, generator=g) + 0.3).numpy()
    dkw = torch.randn(Rr, E, generator=g).numpy()
    seed = SEED if use_gumbel else 0
    ref_kw, ref_da, ref_dt = _autograd64(a, emb, dkw, T, use_gumbel, hard, seed)
    ag = _gpu(a).requires_grad_(True)
    eg = _gpu(emb)
    temp = torch.nn.Parameter(torch.tensor([T], device=dev()))
    cos = ops.cosine_scores(ag.detach(), eg)
    targets = ops.vq_noisy_argmax(cos, seed if use_gumbel else None)
    kw = KeywordVQFn.apply(ag, cos, targets, eg, temp, R.MASK, not hard, seed)
    kw.backward(_gpu(dkw))
    if not hard:
        assert _rel(kw.detach().cpu().numpy(), ref_kw) < 2e-5
    else:
        assert torch.equal(kw.detach(), eg[targets])
    da = ag.grad.cpu().numpy().astype(np.float64)
    scale = np.abs(ref_da).max()
    print("bwd", mode, (Rr, V, E, T), "max |d da|", np.abs(da - ref_da).max(), "scale", scale, "dT", float(temp.grad), ref_dt)
    assert np.abs(da - ref_da).max() < 2e-4 * max(scale, 1e-3), (np.abs(da - ref_da).max(), scale)
    assert abs(float(temp.grad) - ref_dt) <= 1e-3 * abs(ref_dt), (float(temp.grad), ref_dt)
    if V == 49408:          # every product of this shape runs on the MFMA GEMM (the small ones take the SIMT sgemm, whose split-K adds atomically): bitwise run to run
        ag2 = _gpu(a).requires_grad_(True)
        KeywordVQFn.apply(ag2, cos, targets, eg, float(T), R.MASK, not hard, seed).backward(_gpu(dkw))
        assert torch.equal(ag2.grad, ag.grad)


@pytest.mark.parametrize("Rr,V,T", [(48, 1000, 0.1), (7, 333, 1.0)])
def test_mode_bwd_without_noise_is_the_straight_through_kernel_bitwise(Rr, V, T):
    from speechclip_amd import ops
    g = torch.Generator().manual_seed(Rr * V)
    cos = (torch.rand(Rr, V, generator=g) * 2 - 1).to(dev())
    dprob = torch.randn(Rr, V, generator=g).to(dev())
    d1, d2 = dprob.clone(), dprob.clone()
    rowdot = ops.vq_st_bwd_(cos, d1, T)
    rd, rz = ops.vq_mode_bwd_(cos, d2, T, None)
    assert torch.equal(d1, d2) and torch.equal(rowdot, rd) and torch.equal(rd, rz)
    d3 = dprob.clone()
    rd3, rz3 = ops.vq_mode_bwd_(cos, d3, T, SEED)                    # with noise: another distribution, and rowdot_z takes the noise along
    assert not torch.equal(d3, d1) and not torch.equal(rd3, rz3) and (d3[:, list(R.MASK)] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ the reference class's own outputs
@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("temp", [0.1, 0.5])
def test_fixture_of_the_reference_class(mode, temp):
    from speechclip_amd import ops
    g = np.load(os.path.join(GOLD, "vq_modes.npz"))
    x = g["x_q"].astype(np.float32) / 2 ** 10
    emb = g["emb_q"].astype(np.float32) / 2 ** 6
    use_gumbel, hard = R.MODES[mode]
    seed = int(g["seed"]) if use_gumbel else None
    tag = f"{mode}/T{temp}/"
    xg, eg = _gpu(x), _gpu(emb)
    targets = ops.vq_noisy_argmax(xg, seed)
    assert np.array_equal(targets.cpu().numpy(), g[tag + "targets"])
    ref_prob = R.unpack_f32(g[tag + "subword_prob"], x.shape)
    if hard:
        onehot = torch.zeros_like(xg).scatter_(-1, targets.view(-1, 1), 1.0).cpu().numpy()
        assert np.array_equal(onehot, np.round(ref_prob)) and np.abs(ref_prob - onehot).max() < 1e-6      # the reference's 1 - y + y is 1 to an ulp
        kw = ops.gather_rows(eg, targets)
    else:
        p = ops.vq_probs(xg, temp, seed).cpu().numpy()
        p64 = R.mode_forward(x, emb, temp, use_gumbel, hard, int(g["seed"]))[0]
        print("fixture probs", mode, temp, "max |gpu - reference class|", np.abs(p - ref_prob).max(), "max |gpu - float64|", np.abs(p - p64).max(),
              "max |reference class - float64|", np.abs(ref_prob - p64).max())
        assert np.abs(p - ref_prob).max() <= (5e-6 if use_gumbel and temp < 0.5 else 1e-6), np.abs(p - ref_prob).max()
        kw = ops.vq_soft_embed(xg, eg, temp, seed)
    assert _rel(kw.cpu().numpy(), g[tag + "keywords"].astype(np.float64)) < 2e-5
    dprob = _gpu((np.broadcast_to(g["w"].astype(np.float64), (x.shape[0], emb.shape[1])) @ emb.astype(np.float64).T).astype(np.float32))
    ops.vq_mode_bwd_(xg, dprob, temp, seed)
    ref_dx = R.unpack_f32(g[tag + "dx"], x.shape)
    scale = np.abs(ref_dx).max()
    assert np.abs(dprob.cpu().numpy() - ref_dx).max() < 2e-4 * max(scale, 1e-3)


# ------------------------------------------------------------------------------------------------------------------ branch level
def _cascaded_model(tmp_path, vq_args):
    """The tiny cascaded model of tests/test_train_gpu.py::_load_cascaded (decisive-margin fixture, reduced vocabulary), its quantizer built with `vq_args`,
    and the fixture's batch at B = 4."""
    from helpers import make_config
    from speechclip_amd.model import KWClip_GeneralTransformer
    from test_e2e_gpu import _tiny_cfgs
    vocab = np.array([0, 320, 510, 511] + list(range(5, 300, 3)))
    vp = str(tmp_path / "vocab.npy")
    np.save(vp, np.stack([vocab, np.arange(len(vocab))[::-1] + 1], axis=1))
    g = np.load(os.path.join(GOLD, "e2e_tiny_base_c2.npz"))
    hc, cc = _tiny_cfgs(False)
    cfg = make_config(d_model=128, branch_heads=4, parallel=False, cascaded=True, hubert_config=hc, clip_config=cc, hubert_name="hubert",
                      normalize_hiddenstates=False, reduce_vocab=vp, vq_args=vq_args)
    model = KWClip_GeneralTransformer(cfg)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/") and "vector_quantizer" not in k}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    model = model.cuda().eval()
    batch = {k: torch.from_numpy(g[k]) for k in ("wav", "wav_len", "image", "id")}
    n = batch["wav"].shape[0]
    pick = [i % n for i in range(4)]
    batch = {k: v[pick].clone().cuda() for k, v in batch.items()}
    batch["id"] = torch.arange(4, device="cuda") + 100                       # distinct ids: no masked positives
    return model, batch


TEMP_KEY = "cascaded_branch.vector_quantizer.curr_temp"


def _train_mode(model):
    cb = model.cascaded_branch
    cb.train()
    model.clip.eval()
    cb.self_att.multihead_attn_layer.dropout = 0.0
    return cb


def _step(model, batch, manual_seed):
    torch.manual_seed(manual_seed)
    model.zero_grad(set_to_none=True)
    feats, _, others = model(batch)
    model.compute_loss(feats)["loss"].backward()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()
             if k.startswith("cascaded_branch.") and not k.startswith("cascaded_branch.clip.") and p.requires_grad}
    return feats["cascaded_audio_feat"].detach().clone(), others["vq_results"], grads


@pytest.fixture(scope="module")
def shipped_eval(tmp_path_factory):
    model, batch = _cascaded_model(tmp_path_factory.mktemp("shipped"), None)
    with torch.no_grad():
        feats, _, others = model(batch)
    return feats["cascaded_audio_feat"].clone(), others["vq_results"]["targets"].clone(), others["keywords"].clone()


@pytest.mark.parametrize("mode", list(R.MODES))
def test_branch_trains_in_every_mode(tmp_path, mode, shipped_eval):
    use_gumbel, hard = R.MODES[mode]
    model, batch = _cascaded_model(tmp_path, {"use_gumbel": use_gumbel, "hard": hard, "temp": "learnable=0.1"})
    # eval: the shipped mode's outputs, bitwise
    with torch.no_grad():
        feats, _, others = model(batch)
    assert others["vq_results"]["gumbel_seed"] == 0
    assert torch.equal(feats["cascaded_audio_feat"], shipped_eval[0]) and torch.equal(others["vq_results"]["targets"], shipped_eval[1])
    assert torch.equal(others["keywords"], shipped_eval[2])
    onehot = others["vq_results"]["subword_prob"]
    assert onehot.sum().item() == onehot.shape[0] * onehot.shape[1] and set(onehot.unique().tolist()) == {0.0, 1.0}

    _train_mode(model)
    feat, vq, grads = _step(model, batch, 5)
    seed, (soft, scores, mask) = vq["gumbel_seed"], vq["vq_mode"]
    assert (seed != 0) == use_gumbel and soft == (not hard) and tuple(mask) == R.MASK
    Rr, V = scores.shape
    z = R.masked_logits(scores.cpu().numpy(), R.gumbel_matrix(seed, Rr, V) if use_gumbel else None, 1.0)
    assert np.array_equal(vq["targets"].reshape(-1).cpu().numpy(), z.argmax(-1))               # the returned seed reproduces the targets on the host
    prob = vq["subword_prob"].reshape(Rr, V).cpu().numpy()
    if hard:
        assert np.array_equal(prob.argmax(-1), z.argmax(-1)) and prob.sum() == Rr
    else:
        assert np.abs(prob - R.softmax(z / vq["temp"])).max() < 1e-4 and (prob[:, list(R.MASK)] == 0).all()
    assert torch.isfinite(feat).all() and len(grads) >= 12
    for k, gr in grads.items():
        assert torch.isfinite(gr).all(), k
        if k.endswith(("attentionBlock_Norm.bias", "linear_proj.bias")):
            continue        # a constant shift ahead of a batch-statistics BatchNorm: the gradient is zero up to fp32 noise (tests/test_train_gpu.py)
        assert gr.abs().max().item() > 0, k
    assert TEMP_KEY in grads

    feat2, vq2, grads2 = _step(model, batch, 5)                                                # the same host seed: the same step, bitwise
    # (the first step updated the BatchNorm running statistics, which train mode does not read)
    assert vq2["gumbel_seed"] == seed and torch.equal(vq2["targets"], vq["targets"]) and torch.equal(feat2, feat)
    assert torch.equal(vq2["subword_prob"], vq["subword_prob"]) and torch.equal(grads2[TEMP_KEY], grads[TEMP_KEY])
    # The parameter gradients behind the pooling backward are NOT bitwise repeatable in any mode, the shipped one included: cls_pool_bwd_frames_kernel, colsum_kernel
    # and the split-K sgemm add with float atomics.  Everything this feature computes is (asserted above and in the KeywordVQFn test); here: equal to that reordering.
    for k in grads:
        d, n = (grads2[k] - grads[k]).norm().item(), grads[k].norm().item()
        if d:
            print("not bitwise:", k, d / max(n, 1e-30))
        assert d <= 1e-4 * n + 1e-7, (k, d, n)
    if use_gumbel:
        _, vq3, _ = _step(model, batch, 6)
        assert vq3["gumbel_seed"] != seed and not torch.equal(vq3["targets"], vq["targets"])

    with torch.no_grad():                                                                      # train() under no_grad: the same forward kernels
        torch.manual_seed(5)
        feats_ng, _, others_ng = model(batch)
        vq_ng = others_ng["vq_results"]
        assert vq_ng["gumbel_seed"] == seed and vq_ng["vq_mode"][0] == soft and torch.isfinite(feats_ng["cascaded_audio_feat"]).all()
        # (the inference-style pooling in front of it rounds elsewhere than the training path: a near-tie may flip, most rows may not)
        assert (vq_ng["targets"] == vq["targets"]).float().mean().item() >= 0.75
        from speechclip_amd import ops
        emb = model.cascaded_branch.clip.model.token_embedding.weight
        kw_ng = others_ng["keywords"].reshape(Rr, -1)
        if soft:
            assert torch.equal(kw_ng, ops.vq_soft_embed(vq_ng["vq_mode"][1], emb, vq_ng["temp"], seed))
        else:
            assert torch.equal(kw_ng, ops.gather_rows(emb, vq_ng["targets"].reshape(-1)))

"""Training the stacked parallel branch (TransformerEncoder.forward_cls_train -> train_branch.BranchStackTrainFn): output and gradients against fp32
CPU autograd of torch.nn.TransformerEncoder with the same weights; train-mode dropout against fp32 CPU autograd of the same graph with the masks
restated on the host; the reference's own gradients from tests/golden/branch_stack_grad_*.npz.

Gradient bounds: those of tests/test_finetune_gpu.py::test_finetune_gradients_vs_oracle_autograd for encoder-layer tensors (the same bf16 chain):
cosine > 0.98 and |norm ratio - 1| < 0.1; a reference gradient of norm < 1e-7 asks for a norm < 1e-4."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import assert_rows_match

pytestmark = pytest.mark.gpu

CONFIGS = [(192, 2, 2, False), (128, 1, 3, True), (128, 2, 1, True)]          # d, heads, n_layers, norm_first
BATCHES = [(4, 40, (40, 1, 33, 17)), (3, 70, (70, 5, 64))]                    # B, T, lens


def _branch(d, heads, n_layers, norm_first, seed=0):
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    torch.manual_seed(seed)
    m = TransformerEncoder(n_layers=n_layers, d_model=d, nhead=heads, dim_feedforward=4 * d, dropout=0.1, norm_first=norm_first)
    cls = torch.randn(1, 1, d)
    return m.eval(), cls


def _torch_ref(m, d, heads, n_layers, norm_first):
    layer = nn.TransformerEncoderLayer(d, heads, 4 * d, 0.1, "gelu", 1e-5, batch_first=True, norm_first=norm_first)
    ref = nn.TransformerEncoder(layer, n_layers, nn.LayerNorm(d, eps=1e-5), enable_nested_tensor=False)
    ref.load_state_dict(m.model.state_dict())
    return ref.eval()


def _frames(B, T, d, lens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, d, generator=g)
    for b, l in enumerate(lens):
        x[b, l:] = 0
    return x.to(torch.bfloat16)


def _cos(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


def _check_grad(got, want, name):
    assert got is not None, name
    gn, wn = got.detach().double().norm().item(), want.detach().double().norm().item()
    print(f"{name}: cos {_cos(got, want):.5f} norm ratio {gn / max(wn, 1e-300):.4f} (ref norm {wn:.3e})")
    if wn < 1e-7:
        assert gn < 1e-4, (name, gn)
        return
    c, ratio = _cos(got, want), gn / wn
    assert c > 0.98 and abs(ratio - 1) < 0.1, (name, c, ratio)


def _valid(t, lens):
    return torch.cat([t[b, :l].reshape(-1).float().cpu() for b, l in enumerate(lens)])


def _run_device(m, cls, x, lens, G, seed=None):
    """-> (out, {name: grad}) of loss = (out * G).sum() on the device; the module keeps its mode."""
    m.zero_grad(set_to_none=True)
    c = cls.detach().cuda().requires_grad_(True)
    xx = x.detach().cuda().requires_grad_(True)
    out = m.forward_cls_train(c, xx, torch.tensor(lens).cuda(), seed=seed)
    (out * G.cuda()).sum().backward()
    grads = {k: p.grad for k, p in m.model.named_parameters()}
    grads["cls"], grads["frames"] = c.grad, xx.grad
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def _eval_case(ci, bi):
    """CPU reference (computed once, shared, never modified): output and gradients of nn.TransformerEncoder autograd."""
    d, heads, n_layers, norm_first = CONFIGS[ci]
    B, T, lens = BATCHES[bi]
    m, cls = _branch(d, heads, n_layers, norm_first, seed=ci)
    ref = _torch_ref(m, d, heads, n_layers, norm_first)
    x = _frames(B, T, d, lens, seed=10 * ci + bi)
    G = torch.randn(B, d, generator=torch.Generator().manual_seed(77 + ci))
    c = cls.clone().requires_grad_(True)
    xf = x.float().requires_grad_(True)
    src = torch.cat([c.expand(B, 1, d), xf], 1)
    mask = torch.arange(T + 1)[None, :] >= (torch.tensor(lens)[:, None] + 1)
    want = ref(src, src_key_padding_mask=mask)[:, 0]
    (want * G).sum().backward()
    wg = {k: p.grad for k, p in ref.named_parameters()}
    wg["cls"], wg["frames"] = c.grad, xf.grad
    return m, cls, x, G, want.detach(), wg


@pytest.mark.parametrize("bi", range(len(BATCHES)))
@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_stack_output_and_gradients_match_torch_autograd(ci, bi):
    m, cls, x, G, want, wg = _eval_case(ci, bi)
    B, T, lens = BATCHES[bi]
    m = m.cuda().eval()
    got, grads = _run_device(m, cls, x, lens, G)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = (got.cpu() - want).abs().max().item()
    print("forward max abs", err)
    assert err < 5e-2
    assert_rows_match(got, want, 0.999, "branch CLS row, training forward")
    with torch.no_grad():
        ev = m.forward_cls(cls.cuda(), x.cuda(), torch.tensor(lens).cuda())
    assert (got - ev).abs().max().item() < 5e-2
    assert_rows_match(got, ev, 0.999, "forward_cls_train vs forward_cls")
    # the node reports a gradient for exactly the parameters of m.model
    assert set(k for k, p in m.model.named_parameters() if p.grad is not None) == set(k for k, _ in m.model.named_parameters())
    for k, _ in m.model.named_parameters():
        _check_grad(grads[k], wg[k], k)
    _check_grad(grads["cls"], wg["cls"], "cls")
    assert grads["frames"].shape == x.shape
    _check_grad(_valid(grads["frames"], lens), _valid(wg["frames"], lens), "frames")
    for b, l in enumerate(lens):
        assert not grads["frames"][b, l:].any(), b                      # exact zeros on padded frames


def test_node_parameters_are_those_of_the_model():
    from speechclip_amd.train_branch import stack_params
    m, _ = _branch(192, 2, 2, False)
    assert sorted(id(p) for p in stack_params(m.model)) == sorted(id(p) for p in m.model.parameters())


# ---- dropout: the masks restated on the host (csrc/common.h: hash32, keep_elem, hash_pair; the pair index of sc_attention_hd_fwd)
def _hash32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def _row_keep(seed, rows, cols, p):
    """[rows, cols] kept set of sc_dropout_bf16 / sc_dropout_f32: element index row * cols + column."""
    idx = np.arange(rows * cols, dtype=np.uint64)
    h = _hash32(np.uint64(seed & 0xffffffff) ^ _hash32((idx + np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)))
    return torch.from_numpy((h >= np.uint64(min(4294967295, int(p * 4294967296.0)))).astype(np.float32)).view(rows, cols)


def _prob_keep(seed, B, H, Tq, Tk, p):
    """[B, H, Tq, Tk] kept set of the attention probabilities: pair index ((b*H + h)*Tk + query) * ceil(Tk / 2) + key / 2, 16 bits per key."""
    rows = ((np.arange(B * H, dtype=np.uint64) * np.uint64(Tk)).reshape(-1, 1) + np.arange(Tq, dtype=np.uint64)[None, :]).reshape(-1, 1)
    keys = np.arange(Tk, dtype=np.uint64)[None, :]
    pair = (rows * np.uint64((Tk + 1) // 2) + (keys >> np.uint64(1))) & np.uint64(0xffffffff)
    hsh = _hash32(((pair * np.uint64(0x9E3779B1)) + np.uint64(seed & 0xffffffff)) & np.uint64(0xffffffff))
    bits = np.where((keys & np.uint64(1)) == 1, hsh >> np.uint64(16), hsh & np.uint64(0xffff))
    return torch.from_numpy((bits >= np.uint64(min(65535, int(p * 65536.0)))).astype(np.float32)).view(B, H, Tq, Tk)


def _host_stack(model, cls, x, lens, heads, norm_first, p, seed):
    """fp32 CPU graph of nn.TransformerEncoder(+ final norm) on [CLS; x] with the node's dropout masks (p = 0: none): layers 0..n-2 on every row,
    the last layer on the CLS rows (the only rows whose masks the node draws there).  -> [B, D]."""
    from speechclip_amd.train_hubert import _site_seeds
    B, T, D = x.shape
    Lq, hd, n = T + 1, D // heads, len(model.layers)
    seeds = _site_seeds(seed, 4 * n) if p > 0 else [0] * (4 * n)
    kmask = (torch.arange(Lq)[None, :] >= (torch.tensor(lens)[:, None] + 1))[:, None, None, :]
    drop = lambda t, s: t if p == 0 else t * _row_keep(s, t.numel() // t.shape[-1], t.shape[-1], p).view(t.shape) / (1 - p)   # noqa: E731

    def attend(L, xq, xkv, s):
        a = L.self_attn
        W, b = a.in_proj_weight, a.in_proj_bias
        Tq = xq.shape[1]
        q = F.linear(xq, W[:D], b[:D]).view(B, Tq, heads, hd).transpose(1, 2)
        k = F.linear(xkv, W[D:2 * D], b[D:2 * D]).view(B, Lq, heads, hd).transpose(1, 2)
        v = F.linear(xkv, W[2 * D:], b[2 * D:]).view(B, Lq, heads, hd).transpose(1, 2)
        P = torch.softmax((q @ k.transpose(-1, -2) * hd ** -0.5).masked_fill(kmask, float("-inf")), -1)
        if p > 0:
            P = P * _prob_keep(s, B, heads, Tq, Lq, p) / (1 - p)
        return a.out_proj((P @ v).transpose(1, 2).reshape(B, Tq, D))

    h = torch.cat([cls.expand(B, 1, D), x], 1)
    for li, L in enumerate(model.layers):
        sa, s1, s2, s3 = seeds[4 * li:4 * li + 4]
        hq = h if li < n - 1 else h[:, :1]
        ff = lambda t: drop(L.linear2(drop(F.gelu(L.linear1(t)), s2)), s3)   # noqa: E731
        if norm_first:
            hq = hq + drop(attend(L, L.norm1(hq), L.norm1(h), sa), s1)
            h = hq + ff(L.norm2(hq))
        else:
            hq = L.norm1(hq + drop(attend(L, hq, h, sa), s1))
            h = L.norm2(hq + ff(hq))
    return model.norm(h[:, 0])


@pytest.mark.parametrize("norm_first", [False, True])
def test_train_mode_dropout_is_seeded_and_matches_host_masks(norm_first):
    d, heads, n_layers = 192, 2, 2
    B, T, lens = BATCHES[1]
    m, cls = _branch(d, heads, n_layers, norm_first, seed=3)
    x = _frames(B, T, d, lens, seed=21)
    G = torch.randn(B, d, generator=torch.Generator().manual_seed(5))
    import copy
    mc = copy.deepcopy(m)
    # the host restatement at p = 0 is nn.TransformerEncoder's CLS row (CPU fp32 both)
    src = torch.cat([cls.expand(B, 1, d), x.float()], 1)
    with torch.no_grad():
        ref0 = _torch_ref(m, d, heads, n_layers, norm_first)(src, src_key_padding_mask=torch.arange(T + 1)[None, :] >= (torch.tensor(lens)[:, None] + 1))[:, 0]
        assert (_host_stack(mc.model, cls, x.float(), lens, heads, norm_first, 0.0, 0) - ref0).abs().max().item() < 1e-4
    # host reference with the same masks
    c = cls.clone().requires_grad_(True)
    xf = x.float().requires_grad_(True)
    want = _host_stack(mc.model, c, xf, lens, heads, norm_first, 0.1, 1234)
    (want * G).sum().backward()
    wg = {k: p.grad for k, p in mc.model.named_parameters()}
    m = m.cuda().train()
    out1, g1 = _run_device(m, cls, x, lens, G, seed=1234)
    g1 = {k: v.clone() for k, v in g1.items()}
    out2, g2 = _run_device(m, cls, x, lens, G, seed=1234)
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    out3, g3 = _run_device(m, cls, x, lens, G, seed=1235)
    assert not torch.equal(out1, out3)
    assert not torch.equal(g1["layers.0.linear1.weight"], g3["layers.0.linear1.weight"])
    err = (out1.cpu() - want.detach()).abs().max().item()
    print("train forward max abs", err)
    assert err < 5e-2
    assert_rows_match(out1, want.detach(), 0.999, "branch CLS row, dropout")
    for k, _ in m.model.named_parameters():
        _check_grad(g1[k], wg[k], k)
    _check_grad(g1["cls"], c.grad, "cls")
    _check_grad(_valid(g1["frames"], lens), _valid(xf.grad, lens), "frames")
    for b, l in enumerate(lens):
        assert not g1["frames"][b, l:].any(), b


def test_two_step_fused_adam_trajectory():
    from speechclip_amd.train_tail import FusedAdam
    d, heads, n_layers, norm_first = CONFIGS[0]
    B, T, lens = BATCHES[0]
    m, cls = _branch(d, heads, n_layers, norm_first, seed=4)
    m = m.cuda().eval()
    c = nn.Parameter(cls.cuda())
    x = _frames(B, T, d, lens, seed=2).cuda()
    G = torch.randn(B, d, generator=torch.Generator().manual_seed(6)).cuda()
    opt = FusedAdam(list(m.parameters()) + [c], lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = (m.forward_cls_train(c, x, torch.tensor(lens).cuda()) * G).sum()
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[1] < losses[0]


@pytest.mark.parametrize("tag", ["hd96", "hd128"])
def test_stack_gradients_against_the_reference_fixture(tag):
    """tests/golden/branch_stack_grad_<tag>.npz (make_golden_branch_grad.py: the reference's own TransformerEncoder under autograd)."""
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"branch_stack_grad_{tag}.npz"))
    d, heads, n_layers, norm_first, ffn = (int(v) for v in z["cfg"])
    lens = z["lens"].tolist()
    m = TransformerEncoder(n_layers=n_layers, d_model=d, nhead=heads, dim_feedforward=ffn, norm_first=bool(norm_first)).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd_")})
    m = m.cuda()
    x = torch.from_numpy(z["x"]).view(torch.bfloat16).cuda().requires_grad_(True)
    cls = torch.from_numpy(z["cls"]).float().cuda().requires_grad_(True)
    y = m.forward_cls_train(cls, x, torch.tensor(lens).cuda())
    emb = _linear(y, torch.from_numpy(z["proj_w"]).float().cuda(), torch.from_numpy(z["proj_b"]).float().cuda())
    want = torch.from_numpy(z["out"])
    assert (emb.detach().cpu() - want).abs().max().item() < 5e-2
    assert_rows_match(emb.detach(), want, 0.999, "branch embedding vs reference fixture")
    (emb * torch.from_numpy(z["G"]).cuda()).sum().backward()
    for k, p in m.named_parameters():
        _check_grad(p.grad, _stored_grad(z, k), k)
    _check_grad(cls.grad, _stored_grad(z, "cls"), "cls")
    _check_grad(_valid(x.grad, lens), _valid(_stored_grad(z, "x"), lens), "frames")
    for b, l in enumerate(lens):
        assert not x.grad[b, l:].any(), b


def _stored_grad(z, name):
    """A gradient of the fixture: fp32 ("grad_"), or int8 with one fp32 scale per row of the first dimension ("gq_" / "gs_")."""
    if "grad_" + name in z.files:
        return torch.from_numpy(z["grad_" + name])
    q = torch.from_numpy(z["gq_" + name]).float()
    return q * torch.from_numpy(z["gs_" + name]).view(-1, *[1] * (q.dim() - 1))


def _linear(y, w, b):
    """linear_proj of the fixture on the fp32 CLS rows (elementwise fp32, no vendor BLAS: [B, D] x [E, D])."""
    return (y[:, None, :] * w[None]).sum(-1) + b

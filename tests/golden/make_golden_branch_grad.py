#!/usr/bin/env python3
"""Generate tests/golden/branch_stack_grad_hd96.npz / branch_stack_grad_hd128.npz: gradients of the REFERENCE's own TransformerEncoder (loaded from
its file, as make_golden_branch.py does) on that script's two cases, eval mode with autograd on.  loss = (linear_proj(CLS row) * G).sum() with a
fixed random G.  Per case: the inputs, the state dict and the projection (fp16, rounded BEFORE the run, so the stored values are the ones used), G,
the output and the gradient of every parameter, of the CLS token and of the frames.  To keep each file under the size limit for a committed file,
a gradient of 10 000 elements or more is stored as int8 with one fp32 scale per row of its first dimension ("gq_" / "gs_" keys: value = q * scale,
error <= row max / 254 per element, which moves a cosine by < 1e-4); smaller ones are fp32 ("grad_" keys).

Runs where the reference checkout exists (not on the GPU box; the GPU test reads only the .npz).
Usage:  python tests/golden/make_golden_branch_grad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_branch import B, CASES, E, LENS, T, _ref_models  # noqa: E402


def _store(out, name, g):
    if g.numel() < 10000:
        out["grad_" + name] = g.numpy()
        return
    rows = g.reshape(g.shape[0], -1)
    scale = rows.abs().amax(1, keepdim=True).clamp_min(1e-30) / 127.0
    out["gq_" + name] = torch.round(rows / scale).to(torch.int8).reshape(g.shape).numpy()
    out["gs_" + name] = scale.reshape(-1).numpy()


def main():
    tm = _ref_models()
    for ci, (tag, d, heads, n_layers, norm_first, ffn) in enumerate(CASES):
        torch.manual_seed(200 + ci)
        enc = tm.TransformerEncoder(n_layers=n_layers, d_model=d, nhead=heads, dim_feedforward=ffn, dropout=0.1, norm_first=norm_first).eval()
        proj = torch.nn.Linear(d, E)
        with torch.no_grad():
            for prm in list(enc.parameters()) + list(proj.parameters()):
                prm.copy_(prm.half().float())
        cls = torch.randn(1, 1, d).half().float().requires_grad_(True)
        x = torch.randn(B, T, d).to(torch.bfloat16).float()
        for b, l in enumerate(LENS):
            x[b, l:] = 0
        x.requires_grad_(True)
        G = torch.randn(B, E)
        src = torch.cat([cls.expand(B, 1, d), x], 1)
        mask = torch.arange(T + 1)[None, :] >= (torch.tensor(LENS)[:, None] + 1)
        emb = proj(enc(src=src, key_padding_mask=mask)[:, :1].reshape(-1, d))
        (emb * G).sum().backward()
        out = {"lens": np.array(LENS, dtype=np.int64), "cfg": np.array([d, heads, n_layers, int(norm_first), ffn], dtype=np.int64),
               "x": x.detach().to(torch.bfloat16).view(torch.int16).numpy(), "cls": cls.detach().half().numpy(), "G": G.numpy(),
               "out": emb.detach().numpy(), "grad_cls": cls.grad.numpy()}
        for k, v in enc.state_dict().items():
            out["sd_" + k] = v.half().numpy()
        for k, v in list(enc.named_parameters()) + [("x", x)]:
            _store(out, k, v.grad)
        out["proj_w"], out["proj_b"] = proj.weight.detach().half().numpy(), proj.bias.detach().half().numpy()
        path = os.path.join(HERE, f"branch_stack_grad_{tag}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

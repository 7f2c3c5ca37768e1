#!/usr/bin/env python3
"""Generate tests/golden/branch_stack_hd96.npz / branch_stack_hd128.npz: the REFERENCE's own TransformerEncoder
(avssl/module/kw_modules/TransformerModels.py, loaded from its file: it imports torch only) on head dims the new kernel takes -- d = 192 /
2 heads (head_dim 96), 2 post-LN layers; d = 128 / 1 head (head_dim 128), 3 pre-LN layers -- with ragged lengths, eval mode.  Per case it stores the inputs, the state dict, the branch
output (KW_ParallelBranch.forward, kwClip.py:1088-1108: [CLS; frames], key-padding mask of len + 1, CLS row, linear_proj) and the
hidden states of extract_hidden_states (kwClip.py:1049-1076, CLS position dropped).  Forward only: the stack has no training path.

Runs where the reference checkout exists (not on the GPU box; the GPU test reads only the .npz).
Usage:  python tests/golden/make_golden_branch.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
# (file tag, d, heads, n_layers, norm_first, dim_feedforward): head_dim 96 post-LN and head_dim 128 pre-LN; one file each keeps every
# fixture well under the size limit for a committed file (weights stored as fp16: they are rounded to fp16 BEFORE the reference runs, so
# the stored values are exactly the ones it used)
CASES = [("hd96", 192, 2, 2, False, 64), ("hd128", 128, 1, 3, True, 64)]
B, T, E = 4, 40, 32
LENS = [40, 1, 33, 17]


def _ref_models():
    spec = importlib.util.spec_from_file_location("ref_TransformerModels", os.path.join(REF, "avssl/module/kw_modules/TransformerModels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    tm = _ref_models()
    for ci, (tag, d, heads, n_layers, norm_first, ffn) in enumerate(CASES):
        torch.manual_seed(100 + ci)
        enc = tm.TransformerEncoder(n_layers=n_layers, d_model=d, nhead=heads, dim_feedforward=ffn, dropout=0.1, norm_first=norm_first).eval()
        proj = torch.nn.Linear(d, E)
        with torch.no_grad():
            for prm in list(enc.parameters()) + list(proj.parameters()):
                prm.copy_(prm.half().float())
        cls = torch.randn(1, 1, d).half().float()
        x = torch.randn(B, T, d).to(torch.bfloat16).float()          # the frames the branch receives are bf16 on the product path
        for b, l in enumerate(LENS):
            x[b, l:] = 0
        src = torch.cat([cls.expand(B, 1, d), x], 1)
        mask = torch.arange(T + 1)[None, :] >= (torch.tensor(LENS)[:, None] + 1)
        with torch.no_grad():
            y = enc(src=src, key_padding_mask=mask)[:, :1].reshape(-1, d)
            emb = proj(y)
            hidden = enc.extract_hidden_states(src=src, key_padding_mask=mask)
        out = {"lens": np.array(LENS, dtype=np.int64), "cfg": np.array([d, heads, n_layers, int(norm_first), ffn], dtype=np.int64),
               "x": x.to(torch.bfloat16).view(torch.int16).numpy(), "cls": cls.half().numpy()}
        for k, v in enc.state_dict().items():
            out["sd_" + k] = v.half().numpy()
        out["proj_w"], out["proj_b"] = proj.weight.detach().half().numpy(), proj.bias.detach().half().numpy()
        out["out"] = emb.numpy()
        for i, h in enumerate(hidden):
            out[f"hidden{i}"] = h[:, 1:].half().numpy()
        path = os.path.join(HERE, f"branch_stack_{tag}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

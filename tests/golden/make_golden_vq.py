#!/usr/bin/env python
"""Generate tests/golden/vq_modes.npz by running the REFERENCE's own SimpleVectorQuantizer (my_vector_quantizer.py:12-165) in train mode in its three
unshipped settings: soft (hard: false), gumbel hard, gumbel soft.

Runs ONLY in the build container (needs the reference tree, as make_golden.py does).  F.gumbel_softmax draws its noise with `torch.Tensor.exponential_`; for
the call that method is patched to fill in e = -log u from the host restatement of the project's noise contract (tests/vq_modes_ref.py) at a fixed seed, so the
reference class computes on exactly the noise the HIP kernels regenerate.  Size B=3, K=4, V=331, emb [331, 64], T = 0.1 and 0.5.  Stored per mode and T:
subword_prob, targets, keywords = subword_prob @ emb, and d/dx of (keywords * W).sum().  Inputs are stored in the integer grids they were drawn on
(x = x_q / 2^10, emb = emb_q / 2^6) and the dense fp32 [B*K, V] arrays as their four byte planes (vq_modes_ref.pack_f32 / unpack_f32: the same bits, the
exponent bytes together so that the archive's deflate finds them) to keep the file under 200 KB."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vq_modes_ref as R  # noqa: E402

REF = os.environ.get("SPEECHCLIP_REFERENCE", "/root/reference")
SEED, B, K, V, E = 20260, 3, 4, 331, 64
TEMPS = (0.1, 0.5)


def main():
    spec = importlib.util.spec_from_file_location("ref_my_vector_quantizer", f"{REF}/avssl/module/speechclip_c_modules/my_vector_quantizer.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(7)
    x_q = np.clip(np.round(rng.normal(0, 0.3, (B * K, V)) * 2 ** 10), -2 ** 10 + 1, 2 ** 10 - 1).astype(np.int16)      # cosine-like scores in (-1, 1)
    emb_q = np.clip(np.round(rng.normal(0, 0.05, (V, E)) * 2 ** 6), -127, 127).astype(np.int8)                        # CLIP's token-embedding scale
    w = rng.normal(0, 0.1, (1, E)).astype(np.float32)              # one direction for every row; small, so that |d/dx| stays below ~0.3: the reference's own
    # fp32 rounding of (x + g) / T (1e-5 relative at T = 0.1, F.gumbel_softmax computes in fp32) then sits under the 1e-6 the host test asks of a float64 restatement
    x = torch.from_numpy(x_q.astype(np.float32) / 2 ** 10)
    emb = torch.from_numpy(emb_q.astype(np.float32) / 2 ** 6)
    e_host = R.exponential(SEED, np.arange(B * K * V, dtype=np.uint64)).reshape(B * K, V)
    arrays = {"x_q": x_q, "emb_q": emb_q, "w": w, "seed": np.int64(SEED), "temps": np.asarray(TEMPS, np.float64), "e": R.pack_f32(e_host.astype(np.float32))}
    drawn = []

    def fill(self, *a, **k):
        assert tuple(self.shape) == (B * K, V) and self.dtype == torch.float32
        self.copy_(torch.from_numpy(e_host).to(self.dtype))
        drawn.append(self.clone())
        return self

    orig = torch.Tensor.exponential_
    for name, (use_gumbel, hard) in R.MODES.items():
        for temp in TEMPS:
            vq = mod.SimpleVectorQuantizer(temp=f"fixed={temp}", time_first=True, use_gumbel=use_gumbel, hard=hard).train()
            leaf = x.clone().requires_grad_(True)
            torch.Tensor.exponential_ = fill
            try:
                res = vq((leaf * 1.0).view(B, K, V))          # the reference masks its input in place: hand it a non-leaf
            finally:
                torch.Tensor.exponential_ = orig
            prob = res["subword_prob"].reshape(B * K, V)
            kw = prob @ emb                                    # kwClip.py:909
            (kw * torch.from_numpy(w)).sum().backward()
            tag = f"{name}/T{temp}/"
            arrays[tag + "subword_prob"] = R.pack_f32(prob.detach().numpy().astype(np.float32))
            arrays[tag + "targets"] = res["targets"].reshape(-1).numpy().astype(np.int64)
            arrays[tag + "keywords"] = kw.detach().numpy().astype(np.float32)
            dx = leaf.grad.numpy().astype(np.float32)
            assert np.isfinite(dx).all() and (dx[:, list(R.MASK)] == 0).all()
            arrays[tag + "dx"] = R.pack_f32(dx)
    assert len(drawn) == 4 and all(torch.equal(d, drawn[0]) for d in drawn)     # one draw per gumbel call, all the patched values
    out = os.path.join(HERE, "vq_modes.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 200 * 1024


if __name__ == "__main__":
    main()

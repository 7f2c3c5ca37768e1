"""Bits of the fused attention backward, for comparing two builds of the library: for seeded inputs, one JSON line per case with the sha256 of the output
bytes of each entry (sc_attention_bwd_packed, sc_attention_hd_bwd).  Cases: the small shapes of tests/test_attn_bwd_packed_gpu.py and
tests/test_attention_hd_bwd_gpu.py (row_off and uniform rows, head_dim 64 / 96 / 128, Tq == Tk and Tq == 1) and the shapes tools/attn_bwd_bench.py and
tools/branch_bench.py --train time, each with drop_p 0 and 0.1.  Run it once per build in a fresh process (SPEECHCLIP_HIP_LIB selects the build) and
compare the lines.
    python tools/attn_bwd_digest.py [--match REGEX] [--dump DIR]
--match keeps the cases whose name matches; --dump DIR also writes every output tensor as DIR/<case>.<entry>.<i>.npy (the bf16 bit patterns as uint16:
dqkv [rows, 3D] of a full-row call, or dq, dk, dv of a Tq == 1 call as i = 0, 1, 2), to size a difference."""
import argparse
import hashlib
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechclip_amd import ops  # noqa: E402

BF = torch.bfloat16
DROPS = ((0.0, 0), (0.1, 77))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


class Out:
    def __init__(self, match, dump):
        self.match, self.dump = re.compile(match), dump

    def wants(self, case):
        return self.match.search(case) is not None

    def emit(self, case, **entries):
        """entries: name -> tensor or tuple of tensors (hashed in order)"""
        rec = dict(case=case)
        for name, ts in entries.items():
            ts = ts if isinstance(ts, (tuple, list)) else (ts,)
            h = hashlib.sha256()
            arrs = [_bits(t) for t in ts]
            for a in arrs:
                h.update(a.tobytes())
            rec[name] = h.hexdigest()
            for i, a in enumerate(arrs if self.dump else ()):
                np.save(os.path.join(self.dump, f"{case}.{name}.{i}.npy"), a)
        print(json.dumps(rec), flush=True)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).cuda()


def packed_cases(out, tag, rows, klens, H, seed, layouts):
    """sc_attention_bwd_packed over `rows` (head_dim 64): layout "row_off", and "uniform" where every utterance has the same number of rows."""
    names = [f"{tag}.{lay}.p{p}" for lay in layouts for p, _ in DROPS]
    if not any(out.wants(n) for n in names):
        return
    g = torch.Generator().manual_seed(seed)
    B, Tmax, tot, d = len(rows), max(rows), sum(rows), H * 64
    qkv, dO, kl = _rand(g, tot, 3 * d), _rand(g, tot, d), _i32(klens)
    off = _i32(np.concatenate([[0], np.cumsum(rows)]))
    for lay in layouts:
        ro = off if lay == "row_off" else None
        for p, s in DROPS:
            name = f"{tag}.{lay}.p{p}"
            if out.wants(name):
                drop = (p, s) if p else None
                att = ops.attention(qkv, B, Tmax, H, kl, row_off_i32=ro, drop=drop)
                out.emit(name, sc_attention_bwd_packed=ops.attention_bwd_packed(qkv, att, dO, B, Tmax, H, kl, ro, drop))


def hd_cases(out, tag, B, L, H, hd, klens, seed, cls_query=True, packed_beside=False):
    """sc_attention_hd_bwd on full rows (Tq == Tk) and on one query per utterance (Tq == 1); at head_dim 64 optionally sc_attention_bwd_packed beside it."""
    names = [f"{tag}.hd{hd}.{form}.p{p}" for form in ("full", "cls") for p, _ in DROPS]
    if not any(out.wants(n) for n in names):
        return
    g = torch.Generator().manual_seed(seed)
    d = H * hd
    qkv, dO, kl = _rand(g, B * L, 3 * d), _rand(g, B * L, d), _i32(klens)
    for p, s in DROPS:
        name = f"{tag}.hd{hd}.full.p{p}"
        if out.wants(name):
            att = ops.attention_hd_qkv(qkv, B, L, H, kl, drop_p=p, seed=s)
            e = dict(sc_attention_hd_bwd=ops.attention_hd_qkv_bwd(qkv, att, dO, B, L, H, kl, drop_p=p, seed=s))
            if packed_beside:
                e["sc_attention_bwd_packed"] = ops.attention_bwd_packed(qkv, att, dO, B, L, H, kl, None, (p, s))
            out.emit(name, **e)
    if not cls_query:
        return
    q1, d1, kv = _rand(g, B, d), _rand(g, B, 1, d), qkv[:, d:].contiguous()
    qs, ks = (d, d), (L * 2 * d, 2 * d)
    for p, s in DROPS:
        name = f"{tag}.hd{hd}.cls.p{p}"
        if out.wants(name):
            o1 = ops.attention_hd(q1, kv, kv[:, d:], B, H, 1, L, hd, qs, ks, kl, drop_p=p, seed=s)
            out.emit(name, sc_attention_hd_bwd=ops.attention_hd_bwd(q1, kv, kv[:, d:], o1, d1, B, H, 1, L, hd, qs, ks, kl, drop_p=p, seed=s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--match", default="", help="regular expression: only the cases whose name it matches")
    ap.add_argument("--dump", default=None, help="directory for the outputs as .npy")
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    out = Out(a.match, a.dump)
    # the tests' shapes
    packed_cases(out, "test_rows", [2, 64, 65, 66, 131, 40, 1], [1, 63, 64, 65, 131, 30, 1], 2, 1, ("row_off",))
    packed_cases(out, "test_equal_rows", [70, 70, 70], [70, 33, 64], 2, 2, ("row_off", "uniform"))
    for hd in (64, 96, 128):
        hd_cases(out, "test", 6, 131, 2, hd, [131, 1, 63, 64, 65, 30], 10 + hd, packed_beside=hd == 64)
    # the timed shapes: tools/attn_bwd_bench.py (B = 256, H = 12, L = 499; full, and bench.py --varlen's lengths padded and packed) ...
    from bench import make_batch
    B, T = 256, 499
    ragged = [min(T, (n - 400) // 320 + 1) for n in make_batch(B, 160000, 0, "cpu", True)[1]]
    packed_cases(out, "timed_full", [T] * B, [T] * B, 12, 3, ("uniform",))
    packed_cases(out, "timed_varlen_padded", [T] * B, ragged, 12, 4, ("uniform",))
    packed_cases(out, "timed_varlen_packed", [n + 1 if n < T else n for n in ragged], ragged, 12, 5, ("row_off",))
    # ... and tools/branch_bench.py --train (B = 256, L = 500; full and ragged lengths; Tq == 1 on the ragged ones)
    L = 500
    lens = torch.randint(200, L + 1, (B,), generator=torch.Generator().manual_seed(0)).tolist()
    for d, hd in ((768, 64), (768, 96), (1024, 128)):
        hd_cases(out, "timed_full", B, L, d // hd, hd, [L] * B, 20 + hd, cls_query=False, packed_beside=hd == 64)
        hd_cases(out, "timed_ragged", B, L, d // hd, hd, lens, 30 + hd, packed_beside=hd == 64)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Speech-text retrieval gallery: what the CLIP text tower costs on padded and on packed rows (ViT-B/32 text tower: width 512, 8 heads, 12 layers, random init).

Workload: N = 5000 captions whose row counts (SOT + tokens + EOT) are drawn with a fixed seed uniformly from 6 .. 30, plus ONE caption of 77 rows so that the
padded path pays L = 77.  This is a STAND-IN for caption lengths: no caption corpus is on the machines this runs on.

Arms, timed after warm-up in three interleaved passes in one process (device events around `--iters` back-to-back calls):
  1  padded   ClipModel.encode_text with SC_TEXT_PACK=0: every caption through all 12 layers at L = 77 (the path before the packed tower existed)
  2  packed   CLIP.encode_text_ids with SC_ATTN_TEXT_GENERAL (attn_fwd_kernel with row_off and the causal bit)
  3  packed   CLIP.encode_text_ids with default flags (the entry's own choice of attention form)
and the attention entry alone on random q | k | v at the same rows, both flag values, plus the padded path's causal attention at N x 77 rows.

Rules this file settles (the verdict lines at the end):
  * a short-row attention form is sc_attention_fwd_text's default below its row limit only if arm 3 beats arm 2 in 3 of 3 passes;
  * SC_TEXT_PACK=auto packs only if the better packed arm beats arm 1 in 3 of 3 passes (speechclip_amd/module/clip_official.py: _TEXT_PACK_AUTO).

Usage: python tools/text_tower_bench.py [--n 5000] [--passes 3] [--iters 5] [--out profiles/text_tower_bench.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def make_captions(n, vocab, seed=7122):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(6, 31, (n,), generator=g)
    rows[n // 2] = 77
    text = torch.zeros(n, 77, dtype=torch.long)
    body = torch.randint(1, vocab - 2, (n, 77), generator=g)
    for b, r in enumerate(rows.tolist()):
        text[b, 1:r - 1] = body[b, 1:r - 1]
        text[b, 0], text[b, r - 1] = vocab - 2, vocab - 1
    return text, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_tower_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("text_tower_bench: needs the GPU (a CPU run measures nothing)")
    from speechclip_amd import ops
    from speechclip_amd.module.clip_official import ClipModel
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(7122)
    clip = ClipModel("ViT-B/32").cuda().eval()
    m = clip.model
    text, rows = make_captions(args.n, m.cfg.vocab_size)
    text = text.cuda()
    plan = m.text_pack_plan(text)
    N, total, H, D = args.n, plan["total"], m.transformer.heads, m.cfg.text_width
    say(f"# device {torch.cuda.get_device_name(0)}; ViT-B/32 text tower (width {D}, {H} heads, {m.cfg.text_layers} layers), random init")
    say(f"# N = {N} captions; rows per caption uniform 6 .. 30 (seed 7122) plus one caption of 77: a stand-in for caption lengths, not a corpus")
    say(f"# rows processed: padded {N * 77} (N x 77), packed {total} ({100.0 * total / (N * 77):.1f} % of padded; mean {total / N:.1f}, max {plan['rows_max']} rows per caption)")
    say(f"# {args.passes} interleaved passes x {args.iters} calls each, device-event time per call in ms")

    def padded():
        os.environ["SC_TEXT_PACK"] = "0"
        return clip.encode_text(text)

    def packed_general():
        return m.encode_text_ids(text, plan, general=True)

    def packed_default():
        return m.encode_text_ids(text, plan)

    with torch.no_grad():
        ref, a, b = padded(), packed_general(), packed_default()
        cos = torch.nn.functional.cosine_similarity(a.double(), ref.double(), dim=-1).min().item()
        say(f"# outputs: packed (SC_ATTN_TEXT_GENERAL) vs padded min cosine over captions {cos:.6f}, bitwise equal: {bool(torch.equal(a, ref))}; packed default flags vs "
            f"SC_ATTN_TEXT_GENERAL max|diff| / max|out| {((a - b).abs().max() / a.abs().max()).item():.2e}")
        for _ in range(2):
            padded(), packed_general(), packed_default()
        res = []
        arms = (padded, packed_general, packed_default)
        for r in range(args.passes):
            t = [0.0, 0.0, 0.0]
            for i in range(3):                     # the order rotates from pass to pass: no arm always runs behind the same neighbour
                a_ = (i + r) % 3
                t[a_] = timed(arms[a_], args.iters)
            t1, t2, t3 = t
            res.append((t1, t2, t3))
            say(f"pass {r}: (1) padded {t1:8.3f} ms | (2) packed, SC_ATTN_TEXT_GENERAL {t2:8.3f} ms | (3) packed, default flags {t3:8.3f} ms | padded / best packed {t1 / min(t2, t3):.2f}")
        # the attention entry alone, at the same rows
        g = torch.Generator().manual_seed(1)
        qkv = torch.randn(total, 3 * D, generator=g).to(torch.bfloat16).cuda()
        off = torch.tensor(plan["row_off"], dtype=torch.int32).cuda()
        out = torch.empty(total, D, dtype=torch.bfloat16, device="cuda")
        qkv_pad = torch.randn(N * 77, 3 * D, generator=g).to(torch.bfloat16).cuda()
        out_pad = torch.empty(N * 77, D, dtype=torch.bfloat16, device="cuda")
        forms = (("sc_attention_fwd_text, SC_ATTN_TEXT_GENERAL", lambda: ops.attention_text(qkv, N, plan["rows_max"], H, off, out=out, general=True)),
                 ("sc_attention_fwd_text, default flags", lambda: ops.attention_text(qkv, N, plan["rows_max"], H, off, out=out)),
                 ("sc_attention_fwd causal, N x 77 padded rows", lambda: ops.attention(qkv_pad, N, 77, H, None, out=out_pad, causal=True)))
        for _, fn in forms:
            fn()
        for r in range(args.passes):
            ta = {}
            for i in range(3):
                name, fn = forms[(i + r) % 3]
                ta[name] = timed(fn, 4 * args.iters)
            say(f"attention alone, pass {r}: " + " | ".join(f"{name} {ta[name]:.4f} ms" for name, _ in forms))
    short_wins = all(t3 < t2 for _, t2, t3 in res)
    pack_wins = all(min(t2, t3) < t1 for t1, t2, t3 in res)
    say(f"verdict: arm (3) beats arm (2) in {sum(t3 < t2 for _, t2, t3 in res)} of {len(res)} passes -> a short-row form {'may be' if short_wins else 'is not'} the entry's default")
    say(f"verdict: the better packed arm beats arm (1) in {sum(min(t2, t3) < t1 for t1, t2, t3 in res)} of {len(res)} passes -> SC_TEXT_PACK=auto {'packs' if pack_wins else 'stays padded'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

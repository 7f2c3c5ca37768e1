#!/usr/bin/env python
"""What `clip.image_encoder_trainable: true` costs, at the headline sizes (ViT-B/32, B = 256 images; P-base, 10 s waves):

  eval         CLIP.encode_image on the frozen path (what every step of a frozen-tower model runs)
  train tower  the differentiable forward + backward of the tower alone (train_vit.ImageTowerTrainFn, sum(feat * w) as the loss): by flop count the backward
               is about twice the forward, so forward + backward is about three eval forwards plus the recomputed fc1 product
  step         the whole P-base training step (bench.py --train: forward in train mode, loss.backward(), FusedAdam) with the tower frozen and trainable
  table        per library entry (each launches one to three kernels) of one tower forward + backward: calls, device time, share

Interleaved rounds in one process, warmed, device-event times of `--iters` back-to-back calls per round.  The per-entry table comes from a run of its own with
an event pair around every library call (it serialises nothing, but the host work between launches grows: its total is not a step time).
Usage: python tools/vit_train_bench.py [--rounds 3] [--iters 10] [--batch 256] [--no-step] > profiles/vit_train_bench.txt"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


class _TimedLib:
    """The ctypes library with a device-event pair around every sc_* call that takes a stream (the last argument)."""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("sc_") or "workspace" in name or name.endswith(("_bytes", "_partials", "_path", "_error", "_version")):
            return fn

        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self._log.append((name, e0, e1))
            return rc
        return call


def entry_table(fn):
    from speechclip_amd import _lib
    real, log = _lib.lib(), []
    _lib._lib = _TimedLib(real, log)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    agg = {}
    for name, e0, e1 in log:
        c, t = agg.get(name, (0, 0.0))
        agg[name] = (c + 1, t + e0.elapsed_time(e1))
    total = sum(t for _, t in agg.values())
    print(f"{'library entry':34s} {'calls':>6s} {'ms':>9s} {'share':>7s}")
    for name, (c, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{name:34s} {c:6d} {t:9.3f} {100 * t / total:6.1f}%")
    print(f"{'sum of the entries':34s} {sum(c for c, _ in agg.values()):6d} {total:9.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--audio-len", type=int, default=160000)
    ap.add_argument("--no-step", action="store_true", help="skip the two whole-step legs (they build the P-base model twice)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vit_train_bench: needs the GPU (a CPU run measures nothing)")
    from speechclip_amd.module.clip_official import ClipModel
    from speechclip_amd.util.shipped_configs import make_config
    from speechclip_amd.model import KWClip_GeneralTransformer
    B = args.batch
    print(f"# device {torch.cuda.get_device_name(0)}; ViT-B/32, B = {B}; {args.rounds} interleaved rounds x {args.iters} calls each")
    torch.manual_seed(7122)
    clip = ClipModel("ViT-B/32", image_encoder_trainable=True).cuda()
    g = torch.Generator().manual_seed(7122)
    image = torch.randn(B, 3, 224, 224, generator=g).cuda()
    w = torch.randn(B, clip.model.cfg.embed_dim, generator=g).cuda()

    def ev():
        with torch.no_grad():
            return clip.encode_image(image)

    def fwd():
        return clip.encode_image(image)

    def fwd_bwd():
        for p in clip.model.visual.parameters():
            p.grad = None
        (clip.encode_image(image) * w).sum().backward()

    assert torch.equal(ev(), fwd().detach()), "the differentiable forward is not the eval forward"
    for _ in range(3):
        ev(), fwd_bwd()
    for r in range(args.rounds):
        te, tf, tb = timed(ev, args.iters), timed(fwd, args.iters), timed(fwd_bwd, args.iters)
        print(f"tower round {r}: eval encode_image {te:.3f} ms | train forward {tf:.3f} ms | train forward + backward {tb:.3f} ms | "
              f"(forward + backward) / eval {tb / te:.2f} | backward / eval {(tb - tf) / te:.2f}")
    print("# one tower forward + backward, per library entry:")
    entry_table(fwd_bwd)
    if args.no_step:
        return
    del clip
    torch.cuda.empty_cache()
    steps = {}
    for name, flag in (("frozen", False), ("trainable", True)):
        cfg = make_config()
        cfg.clip.image_encoder_trainable = flag
        torch.manual_seed(7122)
        model = KWClip_GeneralTransformer(cfg).cuda().train()
        (opt,), (sch,) = model.configure_optimizers()
        gb = torch.Generator().manual_seed(7122)
        batch = {"wav": (0.1 * torch.randn(B, args.audio_len, generator=gb)).cuda(), "wav_len": torch.full((B,), args.audio_len, dtype=torch.long),
                 "image": image, "id": torch.arange(B).cuda()}

        def step(model=model, opt=opt, sch=sch, batch=batch):
            opt.zero_grad()
            loss = model.training_step_end(model.training_step(batch, 0))["loss"]
            loss.backward()
            opt.step()
            sch["scheduler"].step()
        steps[name] = step
        for _ in range(3):
            step()
    for r in range(args.rounds):
        t0, t1 = timed(steps["frozen"], args.iters), timed(steps["trainable"], args.iters)
        print(f"P-base training step round {r}: image tower frozen {t0:.2f} ms | trainable {t1:.2f} ms | difference {t1 - t0:.2f} ms")


if __name__ == "__main__":
    main()

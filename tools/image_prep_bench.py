"""Where should CLIP's resize + centre crop run?  Times ClipModel.prep_image (PNG files) and ClipModel.prep_image_arrays (decoded frames) under
SC_IMAGE_PREP=host (PIL on one host thread, the path before the device entry existed) and SC_IMAGE_PREP=device (decode only on the host, sc_image_prep_u8).

Workload: 256 images, half 500 x 375 and half 375 x 500, a stand-in for Flickr8k photographs (smooth random fields plus noise, fixed seed; no corpus is read).
Timing: wall clock around the whole call with a device synchronise on both sides -- the host work is what is measured -- after a warm-up of both arms, three
interleaved passes with rotating order, one process.  Also: the device entry alone (events around sc_image_prep_u8) and the bytes that cross PCIe per image.

    python tools/image_prep_bench.py [--images 256] [--passes 3] [--out profiles/image_prep_bench.txt]

The rule the result feeds (README, 'Image hand-over'): `auto` may mean `device` only if the device arm is faster in every pass on both legs."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_MS = 42.0          # the speech tower's step at B = 256 (bench.py --gpus 1): the rate an image path has to feed


def make_images(n, seed=0):
    """Photo-like stand-ins: a 16 x 12 random field blown up bicubically (smooth regions, edges) plus +-8 of noise."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = (500, 375) if i % 2 == 0 else (375, 500)
        low = Image.fromarray(rng.integers(0, 256, (12, 16, 3), dtype=np.uint8), "RGB").resize((w, h), Image.BICUBIC)
        img = np.asarray(low, dtype=np.int16) + rng.integers(-8, 9, (h, w, 3), dtype=np.int16)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_prep_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_prep_bench.py measures on the GPU: no device found (nothing is estimated on the CPU)")
    from PIL import Image
    import PIL
    from speechclip_amd import ops
    from speechclip_amd.data.image_transforms import plan_image_batch
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.clip_official import ClipModel
    # prep_image needs the resolution and the device only: a one-layer tower at 224 x 224
    clip = ClipModel("ViT-B/32", clip_config=ClipConfig(vision_layers=1, text_layers=1)).to("cuda")
    n_px = clip.model.cfg.image_resolution
    arrays = make_images(args.images)
    lines = []
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, a in enumerate(arrays):
            paths.append(os.path.join(d, f"{i:04d}.png"))
            Image.fromarray(a, "RGB").save(paths[-1])
        png_bytes = sum(os.path.getsize(p) for p in paths) / len(paths)
        print(f"# {len(paths)} PNG files written, {png_bytes / 1e3:.0f} KB each", file=sys.stderr, flush=True)
        legs = {"png_files": lambda: clip.prep_image(paths), "decoded_arrays": lambda: clip.prep_image_arrays(arrays)}
        arms = ["host", "device"]
        results = {leg: {a: [] for a in arms} for leg in legs}
        equal = {}
        for leg, fn in legs.items():
            outs = {}
            for a in arms:          # warm-up: code objects, pinned and device allocations, PIL's and the plan's caches
                os.environ["SC_IMAGE_PREP"] = a
                for _ in range(2):
                    outs[a] = fn()
            equal[leg] = bool(torch.equal(outs["host"], outs["device"]))
            del outs
            for p in range(args.passes):
                for a in (arms[p % 2:] + arms[:p % 2]):
                    os.environ["SC_IMAGE_PREP"] = a
                    ms, _ = timed(fn)
                    results[leg][a].append(ms)
                    print(f"# {leg} pass {p} {a}: {ms:.1f} ms", file=sys.stderr, flush=True)
        # the device entry alone: events around the library call
        os.environ["SC_IMAGE_PREP"] = "device"
        ops.PROFILE_HBM = []
        for _ in range(args.passes):
            clip.prep_image_arrays(arrays)
        torch.cuda.synchronize()
        entry_ms = [e0.elapsed_time(e1) for (e0, e1, _, tag, _) in ops.PROFILE_HBM if tag == "image_prep"]
        ops.PROFILE_HBM = None
        os.environ.pop("SC_IMAGE_PREP")
    plan = plan_image_batch(arrays, n_px)
    dev_bytes = (plan.packed_bytes + plan.offsets.nbytes + plan.geom.nbytes + plan.tables.nbytes) / len(arrays)
    faster = {leg: [d < h for h, d in zip(r["host"], r["device"])] for leg, r in results.items()}
    device_wins = all(all(f) for f in faster.values())
    lines.append(f"# tools/image_prep_bench.py on one {torch.cuda.get_device_name(0)}, Pillow {PIL.__version__}, {args.images} images (half 500 x 375, half 375 x 500; synthetic stand-ins"
                 f" for photographs, {png_bytes / 1e3:.0f} KB per PNG), n_px = {n_px}")
    lines.append(f"# wall clock around the whole call (device synchronise on both sides), {args.passes} interleaved passes with rotating order after a warm-up of both arms, one process")
    lines.append(f"# rule: auto = device only if the device arm is faster in every pass on both legs -> {'device' if device_wins else 'host'}")
    for leg, r in results.items():
        for a in arms:
            ms = r[a]
            lines.append(json.dumps({"leg": leg, "arm": a, "ms_per_call": [round(x, 2) for x in ms], "ms_per_image_median": round(float(np.median(ms)) / args.images, 4),
                                     "images_per_s_median": round(args.images / float(np.median(ms)) * 1e3, 1)}))
        lines.append(json.dumps({"leg": leg, "device_faster_per_pass": faster[leg], "outputs_bitwise_equal": equal[leg],
                                 "speedup_median": round(float(np.median(r["host"]) / np.median(r["device"])), 2)}))
    lines.append(json.dumps({"item": "device_entry_alone_ms", "events": [round(x, 3) for x in entry_ms], "images": args.images}))
    lines.append(json.dumps({"item": "bytes_over_pcie_per_image", "host_arm_uint8_crop": n_px * n_px * 3, "device_arm_decoded_image_and_tables": round(dev_bytes)}))
    need = {leg: {a: round(float(np.median(r[a])) / (STEP_MS * args.images / 256), 2) for a in arms} for leg, r in results.items()}
    lines.append(json.dumps({"item": "call_time_over_step_time", "step_ms_at_256_pairs": STEP_MS, "ratio": need,
                             "note": "a ratio above 1 means one thread of this path does not feed the speech tower's rate; compared, not assumed to be met"}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

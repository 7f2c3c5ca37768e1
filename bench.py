#!/usr/bin/env python3
"""bench.py -- speech-image pairs/s of the Parallel SpeechCLIP base forward + InfoNCE step on MI355X.

Workload (BASELINE.json configs[1] / SURVEY.md section 8d "C2"): HuBERT-base + CLIP ViT-B/32 + parallel CLS head, bf16 MFMA
compute, per-GPU batch 256, every wave exactly 160000 samples (10 s @ 16 kHz => T = 499), 224^2 images, unique ids,
random-init weights (no network), synthetic inputs resident in HBM before the timed region.  One "step" = the full
forward of both towers + head + L2 norms + (N > 1: RCCL all-gather of the embeddings) + masked InfoNCE on the global batch.
N > 1: one process per GPU, weak scaling (256 pairs per GPU), value = all pairs / max-over-ranks time.  `python bench.py --gpus N` works
both under an external `python -m torch.distributed.run ...` (RANK / WORLD_SIZE in the environment) and on its own: with --gpus N > 1 and
no WORLD_SIZE it re-executes itself under torch.distributed.run (one rank per GPU, 127.0.0.1 rendezvous) and rank 0 prints the line.
Every GEMM of the step runs on the hand-written kernels (gemm8p_pers_kernel for the large bf16-output shapes, gemm256_kernel / gemm_bf16_kernel for the rest); hipBLASLt on the plain shapes is measured BESIDE the headline as
`vendor_comparator` (never part of `value`).

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times --steps steps and prints the
headline fields (metric, value, unit, higher_is_better, dtype, ms_per_step, ...); everything measured beside the headline is filled in
only with --full (null otherwise):
  "roofline":     dominant kernel (the bf16 MFMA GEMM): algorithmic FLOPs of all its launches / their HIP-event time (events on every
                  third timed step), with "hbm_segments" from the same events
  "cpu_baseline": the fp32 CPU oracle (oracle/, a port of the reference's CPU path) timed on a bounded sample, and "parity_check" against it
  "vendor_comparator", "varlen_padded_comparator", "measured_ceiling_8k_cubed", "clock", "other_configs", "exchange_ms_per_step".
--dump-outputs DIR writes what the last timed step computed (the loss and the floating-point loss features the caller receives) as
DIR/<name>.npy; inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0  # dense MFMA bf16, MI355X_MICROARCH.md


def conv_lens(L):
    out = []
    for k, s in [(10, 5)] + [(3, 2)] * 4 + [(2, 2)] * 2:
        L = (L - k) // s + 1
        out.append(L)
    return out


def algorithmic_gflop_per_pair(L=160000, d=768, ffn=3072, layers=12, vit_w=768, vit_layers=12, patch=32, res=224, E=512):
    """SURVEY.md section 8(d) formulas (2*MACs of the dense contractions; softmax/LN/GELU excluded)."""
    Ts = conv_lens(L)
    T = Ts[-1]
    cnn0 = 2 * Ts[0] * 512 * 1 * 10
    cnn = sum(2 * Ts[i] * 512 * 512 * k for i, k in zip(range(1, 7), [3, 3, 3, 3, 2, 2]))
    proj = 2 * T * 512 * d
    pos = 2 * T * d * (d // 16) * 128
    lin = layers * 2 * T * (4 * d * d + 2 * d * ffn)
    att = layers * 4 * T * T * d
    n = (res // patch) ** 2 + 1
    vit_lin = 2 * (n - 1) * 3 * patch * patch * vit_w + vit_layers * 2 * n * (4 * vit_w * vit_w + 8 * vit_w * vit_w) + 2 * vit_w * E
    vit_att = vit_layers * 4 * n * n * vit_w
    branch_lin = 2 * (T + 1) * d * 2 * d + 2 * (d * d + d * d + 2 * d * ffn) + 2 * d * E   # K/V of all frames + CLS-row-only rest
    branch_att = 4 * (T + 1) * d
    total = cnn + proj + pos + lin + vit_lin + branch_lin + cnn0 + att + vit_att + branch_att     # 158.1 GF
    # FLOPs that actually run on the MFMA GEMM kernel (roofline numerator).  The pooling head is evaluated in its algebraic form
    # (score = x.u_r, value projection of 8 pooled vectors), so its K/V GEMM over all frames (1.18 GF/pair) is NOT executed and
    # is not credited to the kernel: 8 score columns + per-head value projection + out_proj + FFN + final projection.
    branch_gemm = 2 * T * d * 8 + 2 * d * d + 2 * (d * d + 2 * d * ffn) + 2 * d * E
    # The grouped positional conv (`pos`, 4.7 GF/pair) runs in its own windowed MFMA kernel (csrc/posconv.hip), not in the GEMM kernel: not credited.
    gemm = cnn + proj + lin + vit_lin + branch_gemm
    return total / 1e9, gemm / 1e9


LARGE = dict(d=1024, ffn=4096, layers=24, vit_w=1024, vit_layers=24, patch=14, E=768)   # HuBERT-large + ViT-L/14 (BASELINE configs[4])


def bench_vocab_ids(vocab=8112, seed=7122):
    """The synthetic reduced sub-word vocabulary of --model cascaded (original CLIP ids; rows 0/2/3 = pad / SOT / EOT as my_vector_quantizer.py:64 assumes)."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.tensor([0, 320, 49406, 49407]), torch.randperm(49000, generator=g)[:vocab - 4] + 321])


def build_model(seed=7122, large=False, cascaded=False, vocab=8112, finetune_layers=(), finetune_all=False):
    from speechclip_amd.util.shipped_configs import make_config
    from speechclip_amd.model import KWClip_GeneralTransformer
    torch.manual_seed(seed)
    if cascaded:      # C-base (BASELINE configs[2]): 8 keyword queries -> BatchNorm -> VQ over the sub-word table -> CLIP text tower
        # spchclp_c.yaml:94 ships a REDUCED vocabulary of 8112 sub-words (`reduce_subword_embbedding`); --vocab 49408 = the full table (stress)
        vp = None
        if vocab and vocab < 49408:
            import tempfile
            import numpy as np
            ids = bench_vocab_ids(vocab, seed).numpy()
            vp = os.path.join(tempfile.gettempdir(), f"bench_vocab_{vocab}_{os.getpid()}.npy")
            np.save(vp, np.stack([ids, np.arange(len(ids))[::-1] + 1], axis=1))
        cfg = make_config(parallel=False, cascaded=True, reduce_vocab=vp)
    elif large:
        cfg = make_config(d_model=1024, branch_heads=8, hubert_name="hubert_large_ll60k", clip_name="ViT-L/14", normalize_hiddenstates=True,
                          temperature_trainable=True)
    else:
        cfg = make_config()
    if finetune_all:          # audio_encoder.trainable: true with no layer lists: the whole encoder trains (speech_encoder_plus.py:399-401)
        cfg.audio_encoder.trainable = True
    elif finetune_layers:
        cfg.audio_encoder.trainable = True
        cfg.audio_encoder.unfreeze_layers = [int(i) for i in finetune_layers]
    return KWClip_GeneralTransformer(cfg).eval()


def make_batch(B, L, rank=0, dev="cuda", varlen=False, lo=32000):
    """The synthetic batch of the timed region: seed 7122 + rank, waves 0.1 * randn (every wave L samples, or
    L_i ~ U{32000..L} zero-padded to the batch maximum as collate_general hands it over), images randn [B, 3, 224, 224], unique ids.
    tests/test_headline_parity_gpu.py checks the HIP path against the fp32 oracle on THIS batch."""
    g = torch.Generator(device="cpu").manual_seed(7122 + rank)
    wav = (0.1 * torch.randn(B, L, generator=g)).to(dev)
    lens = [L] * B
    if varlen:
        lens = [int(x) for x in torch.randint(min(lo, L), L + 1, (B,), generator=g)]
        wav = wav[:, :max(lens)].contiguous()
        wav *= (torch.arange(wav.shape[1], device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None])
    batch = {"wav": wav, "wav_len": torch.tensor(lens, dtype=torch.long), "image": torch.randn(B, 3, 224, 224, generator=g).to(dev),
             "id": (torch.arange(B) + rank * B).to(dev)}
    return batch, lens


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(model_sd, n_pairs, L, iters=3, keep=None):
    """fp32 CPU oracle (port of the reference's CPU path) on the host cores, SURVEY.md section 8(d) protocol: 1 warm-up + `iters` timed
    iterations of (a) `n_pairs` fixed-length pairs of the headline workload and (b) the C1 batch (BASELINE configs[0]: 16 pairs, variable
    lengths); os.cpu_count() and the CPU model stated; per-segment split (CNN / transformer / layer mix + branch / ViT / loss) from module
    hooks.  The thread count is what torch uses after a probe (its CPU kernels do not scale to all hardware threads on this workload)."""
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from oracle.speechclip_ref import SpeechClipRef
    ncpu = os.cpu_count() or 1
    ref = SpeechClipRef(HubertRefConfig.base(), ClipRefConfig.vit_b32(), parallel=True, branch_heads=8).eval()
    ref.encoder.load_state_dict({k[len("audio_encoder.encoder."):]: v for k, v in model_sd.items() if k.startswith("audio_encoder.encoder.")})
    ref.clip.load_state_dict({k[len("clip.model."):]: v for k, v in model_sd.items() if k.startswith("clip.model.")})
    ref.parallel_branch.load_state_dict({k[len("parallel_branch."):]: v for k, v in model_sd.items() if k.startswith("parallel_branch.")})
    g = torch.Generator().manual_seed(7122)

    def mk(b, lens=None):
        lens = [L] * b if lens is None else lens
        wav = torch.zeros(b, max(lens))
        for i, n in enumerate(lens):
            wav[i, :n] = 0.1 * torch.randn(n, generator=g)
        return {"wav": wav, "wav_len": torch.tensor(lens), "image": torch.randn(b, 3, 224, 224, generator=g), "id": torch.arange(b)}
    # segment timers: forward hooks on the oracle's own modules
    seg = {"cnn": 0.0, "transformer": 0.0, "vit": 0.0, "branch": 0.0}
    t_in = {}

    def hook(name, mod):
        mod.register_forward_pre_hook(lambda m, a: t_in.__setitem__(name, time.perf_counter()))
        mod.register_forward_hook(lambda m, a, o: seg.__setitem__(name, seg[name] + time.perf_counter() - t_in[name]))
    hook("cnn", ref.encoder.feature_extractor)
    hook("transformer", ref.encoder.encoder)
    hook("vit", ref.clip.visual)
    hook("branch", ref.parallel_branch)
    best, cores = 0.0, 1
    probe_rates = {}
    with torch.no_grad():
        for n in (sorted({min(ncpu, c) for c in (8, 16, 32, 64, ncpu)}) if n_pairs >= 8 else [min(16, ncpu)]):   # (tiny samples: the contract test)
            torch.set_num_threads(n)
            t0 = time.perf_counter()
            ref(mk(1))
            r_warm = 1 / (time.perf_counter() - t0)
            if r_warm < 0.25 * best:                        # hopeless candidate (all hardware threads: ~40 s per pair): its warm-up pass is its measurement
                probe_rates[n] = (r_warm, 1, "un-warmed")
                continue
            t0 = time.perf_counter()
            ref(mk(2))
            r = 2 / (time.perf_counter() - t0)
            probe_rates[n] = (r, 2, "after a 1-pair warm-up")
            if r > best:
                best, cores = r, n
    torch.set_num_threads(cores)

    def run(batch_fn, n):
        with torch.no_grad():
            ref.compute_loss(ref(batch_fn()))                 # warm-up
            for k in seg:
                seg[k] = 0.0
            times, t_loss = [], 0.0
            for _ in range(iters):
                b = batch_fn()
                t0 = time.perf_counter()
                o = ref(b)
                t1 = time.perf_counter()
                loss = ref.compute_loss(o)["loss"].item()
                t2 = time.perf_counter()
                if keep is not None and n == n_pairs:          # the fixed-length sample: inputs + oracle outputs of the LAST timed iteration (parity_check)
                    keep.update(batch=b, out={k: o[k] for k in ("parallel_audio_feat", "image_feat")}, loss=loss)
                times.append(t2 - t0)
                t_loss += t2 - t1
        tot = sum(times)
        split = {k: round(v / tot, 4) for k, v in seg.items()}
        split["loss"] = round(t_loss / tot, 4)
        split["mix_and_glue"] = round(max(0.0, 1.0 - sum(split.values())), 4)
        return {"pairs_per_s": round(n * iters / tot, 3), "iter_s": [round(t, 2) for t in times], "segments_frac": split, "loss": round(loss, 4)}
    fixed = run(lambda: mk(n_pairs), n_pairs)
    n_c1 = 16 if n_pairs >= 16 else max(2, n_pairs)           # C1 = 16 pairs (BASELINE configs[0]); smaller only for the quick contract test
    c1_lens = [int(x) for x in torch.randint(L // 4, L + 1, (n_c1,), generator=g)]
    c1 = run(lambda: mk(n_c1, c1_lens), n_c1)
    # SURVEY.md section 8(d) asks for ALL host cores: that is the thread-count probe's own last candidate (torch.set_num_threads(os.cpu_count()): a 1-pair
    # warm-up, then 2 timed pairs -- or the warm-up pass alone when that is already 4x slower than the best candidate), reported beside the best-of-probe figure (`value` stays the best thread count's).  (Until late round 3 this was a
    # separate un-warmed 1-pair pass: 72 s of the default run for a number the probe already had.)
    all_cores = None
    if ncpu != cores and ncpu in probe_rates:
        r_all, n_all, how = probe_rates[ncpu]
        all_cores = {"cores": ncpu, "pairs_per_s": round(r_all, 3), "iter_s": [round(n_all / r_all, 2)], "pairs": n_all,
                     "note": f"{n_all} timed pair(s) {how} (forward only; the thread-count probe's all-cores candidate): torch's CPU kernels "
                             "collapse at this thread count, the probe picks the best count"}
    return {"value": fixed["pairs_per_s"], "unit": "pairs/s", "cores": cores, "kind": "port", "host_hw_threads": ncpu, "cpu_model": _cpu_model(),
            "all_host_cores": all_cores,
            "timed_iterations": iters, "fixed_length": fixed, "c1_varlen_b16": dict(c1, pairs=n_c1, lens_min_max=[min(c1_lens), max(c1_lens)]),
            "sample": f"{iters} timed iterations (after 1 warm-up) of {n_pairs} pairs (10 s audio + 224^2 image) through oracle/speechclip_ref.py fp32 "
                      f"with {cores} torch threads (best of 8/16/32/64/all on a 2-pair probe; host: {ncpu} hardware threads, {_cpu_model()}), "
                      f"{sum(fixed['iter_s']):.1f} s; plus the C1 batch ({n_c1} pairs, variable lengths) {c1['pairs_per_s']} pairs/s"}


def parity_check(model, keep, dev):
    """The HIP path against the CPU baseline's OWN outputs: the same 32 pairs and the same weights the `cpu_baseline` leg just ran through the fp32
    oracle go through the GPU model; centred cosine per embedding row (tests/helpers.py: the reference's batch mean removed from both sides; the
    same rows rotated by one as the negative control), loss difference and the largest logit difference.  Thresholds = the test-suite's
    (tests/test_headline_parity_gpu.py); `ok` says whether this very run met them."""
    import torch.nn.functional as F
    b, o = keep["batch"], keep["out"]
    with torch.no_grad():
        lf, _, _ = model({k: v.to(dev) for k, v in b.items()})
        loss = model.compute_loss(lf)["loss"].item()

    def ccos(got, ref):
        got, ref = got.float().cpu(), ref.float().cpu()
        mu = ref.mean(0, keepdim=True)
        return F.cosine_similarity(got - mu, ref - mu, dim=-1), F.cosine_similarity(torch.roll(got, 1, 0) - mu, ref - mu, dim=-1)
    ca, wa = ccos(lf["parallel_audio_feat"], o["parallel_audio_feat"])
    ci, wi = ccos(lf["image_feat"], o["image_feat"])
    lg = ((lf["parallel_audio_feat"].float().cpu() @ lf["image_feat"].float().cpu().t()) - (o["parallel_audio_feat"] @ o["image_feat"].t())) / 0.07
    raw = F.cosine_similarity(lf["parallel_audio_feat"].float().cpu(), o["parallel_audio_feat"], dim=-1).min().item()
    out = {"pairs": int(b["id"].shape[0]), "against": "cpu_baseline's own fp32 oracle outputs on the same inputs and weights (last timed iteration)",
           "audio_centred_cos_min": round(ca.min().item(), 5), "audio_centred_cos_mean": round(ca.mean().item(), 5),
           "image_centred_cos_min": round(ci.min().item(), 5), "rotated_rows_centred_cos_max": round(max(wa.max().item(), wi.max().item()), 4),
           "audio_raw_cos_min": round(raw, 7), "loss_gpu": round(loss, 5), "loss_cpu": round(keep["loss"], 5), "loss_abs_diff": round(abs(loss - keep["loss"]), 6),
           "logit_max_abs_diff": round(lg.abs().max().item(), 5),
           "thresholds": {"centred_cos_min": 0.99, "rotated_rows_max": 0.9, "loss_abs_diff": 2e-2, "logit_max_abs_diff": 5e-2}}
    out["ok"] = bool(out["audio_centred_cos_min"] >= 0.99 and out["image_centred_cos_min"] >= 0.99 and out["rotated_rows_centred_cos_max"] < 0.9
                     and out["loss_abs_diff"] <= 2e-2 and out["logit_max_abs_diff"] <= 5e-2)
    return out


MFMA_POWER_CAPPED_TFLOPS = 2150.0          # profiles/r06_mfma_power_ceiling.txt: 16x16x32 bf16, random operands, MFMA-only, power-capped socket
MFMA_POWER_CAPPED_LDS_TFLOPS = 1750.0      # the same with the GEMM k-loop's fragment reads (ds_read_b128 at the loop's read : MFMA ratio)
OTHER_CONFIGS = ("cascaded_v8112", "large_b64", "large_b64_ragged", "varlen_packed", "varlen_padded", "train")


def other_config(kind, dev, batch=None, steps=5, warmup=2):
    """One of the NON-headline configurations, timed the same way (fences, wall clock, inputs resident) with a short run, so that the driver's one
    line carries every BASELINE.json config.  Never part of `value`.
      cascaded_v8112  configs[2]  Cascaded SpeechCLIP base, reduced vocabulary of 8112 sub-words, B = 256, 10 s
      large_b64       configs[4]  Parallel SpeechCLIP large (HuBERT-large + ViT-L/14), 64 pairs per GPU (model_large/coco/spchclp_p.yaml:10 over 4 GPUs), 10 s
      large_b64_ragged  configs[4] as SURVEY.md section 8d C5 specifies it: SpokenCOCO-shaped RAGGED batch, L_i ~ U{48000..160000}, padding-free engine
      varlen_packed / varlen_padded   configs[1] with L_i ~ U{32000..160000}: padding-free engine vs the reference's padded layout (SC_VARLEN_PACK=0)
      train           configs[1] training step of the trainable tail (train-mode crop to 102400 samples, loss.backward(), clip, Adam, LR schedule)"""
    from speechclip_amd import parallel
    large, casc, train = kind.startswith("large_b64"), kind == "cascaded_v8112", kind == "train"
    varlen = kind.startswith("varlen") or kind == "large_b64_ragged"
    model = build_model(large=large, cascaded=casc).to(dev)
    B = batch or (64 if large else 256)
    L = 160000
    b, lens = make_batch(B, L, 0, dev, varlen, lo=48000 if kind == "large_b64_ragged" else 32000)
    old_pack = os.environ.get("SC_VARLEN_PACK")
    if kind == "varlen_padded":
        os.environ["SC_VARLEN_PACK"] = "0"
    try:
        if train:
            model.train()
            (opt,), (sch,) = model.configure_optimizers()

            def step():
                opt.zero_grad()
                loss = model.training_step_end(model.training_step(b, 0))["loss"]
                loss.backward()
                opt.step()
                sch["scheduler"].step()
                return loss.detach()
        else:
            def step():
                with torch.no_grad():
                    lf, _, _ = model(b)
                    return model.compute_loss(parallel.gather_loss_feats(lf))["loss"]
        for _ in range(warmup):
            loss = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        if kind == "varlen_padded":
            if old_pack is None:
                os.environ.pop("SC_VARLEN_PACK", None)
            else:
                os.environ["SC_VARLEN_PACK"] = old_pack
    mal = int(getattr(model.audio_encoder, "max_audio_len", -1))
    eff = [min(n, mal) if (train and mal > 0) else n for n in lens]
    cache = {}
    for n in set(eff):
        cache[n] = algorithmic_gflop_per_pair(n, **(LARGE if large else {}))[0]
    gf = sum(cache[n] for n in eff) / B + (0.9 if casc else 0.0)     # cascaded head: + ~2.1 GF instead of the parallel head's 1.19
    pps = B * steps / dt
    out = {"ms_per_step": round(dt / steps * 1e3, 3), "pairs_per_s": round(pps, 2), "pairs_per_gpu": B, "steps": steps, "warmup": warmup,
           "algorithmic_gflop_per_pair": round(gf, 2), "e2e_tflops": round(gf * pps / 1e3, 1), "e2e_frac": round(gf * pps / 1e3 / PEAK_BF16_TFLOPS, 4),
           "audio_samples_mean": int(sum(eff) / B), "loss": round(float(loss), 5)}
    if large:      # the pre-LN speech tower's layers take IEEE-half GEMM / attention operands (module/hubert.py _PRELN_F16; same dense MFMA peak as bf16)
        from speechclip_amd.module import hubert as _hb
        out["layer_operands"] = "f16" if _hb._PRELN_F16 else "bf16"
    del model
    torch.cuda.empty_cache()
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, loss, feats):
    """--dump-outputs: the loss and every floating-point tensor of the loss features of the last timed step as <out_dir>/<name>.npy (float32; the
    loss float64).  Rows beyond the 64 MB budget are replaced by a fixed, seeded sample of rows (its row indices are written beside it)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": np.asarray([float(loss)], dtype=np.float64)}
    for k in sorted(feats):
        v = feats[k]
        if torch.is_tensor(v) and v.is_floating_point():
            arrays[k] = v.detach().float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        for k in [k for k in arrays if k != "loss"]:
            a = arrays[k]
            keep = max(1, int(a.shape[0] * DUMP_MAX_BYTES / total / 2))
            if keep < a.shape[0]:
                rows = np.sort(np.random.default_rng(7122).choice(a.shape[0], keep, replace=False))
                arrays[k] = a[rows]
                arrays[k + "_rows"] = rows.astype(np.float64)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher: re-execute under torch.distributed.run, one rank per GPU, loopback rendezvous."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def dry_run(args, world, rank):
    """Launcher / exchange-protocol check without a GPU (tests, CPU container): `gloo` process group, random unit embeddings instead of
    the towers, the SAME packed all-gather (speechclip_amd.parallel), barrier + max-over-ranks timing and JSON contract.  No kernel runs
    and nothing here is a throughput claim (`data` says so)."""
    import torch.distributed as dist
    from speechclip_amd import parallel
    if world > 1:
        dist.init_process_group("gloo")
    if args.global_batch is not None:
        if args.global_batch % world:
            sys.exit(f"bench.py: --global-batch {args.global_batch} is not divisible by {world} ranks")
        args.batch = args.global_batch // world
    B, E = args.batch or 8, (768 if args.model == "large" else 512)      # embedding width of the CLIP tower (ViT-L/14: 768)
    g = torch.Generator().manual_seed(7122 + rank)

    def step():
        a = torch.nn.functional.normalize(torch.randn(B, E, generator=g), dim=-1)
        i = torch.nn.functional.normalize(torch.randn(B, E, generator=g), dim=-1)
        f = parallel.gather_loss_feats({"id": torch.arange(B) + rank * B, "image_feat": i, "parallel_audio_feat": a})
        lg = f["parallel_audio_feat"] @ f["image_feat"].t() / 0.07
        return 0.5 * ((torch.logsumexp(lg, 1) - lg.diagonal()).mean() + (torch.logsumexp(lg, 0) - lg.diagonal()).mean()), f["id"].shape[0], f
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, bg, feats = step()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, feats)
    seen = torch.ones(1)
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
        dist.all_reduce(seen)
    if rank == 0:
        print(json.dumps({"metric": "speech-image pairs/sec/node (dry run)", "value": round(world * B * args.steps / dt, 2), "unit": "pairs/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
                          "scaling": "strong" if args.global_batch is not None else "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "dry-run: launcher + exchange protocol on CPU/gloo, no kernels, not a measurement",
                          "config": {"workload": "dry run", "pairs_per_gpu": B, "global_batch": int(bg), "parallelism": f"dp{world}"},
                          "ranks_seen": int(seen.item()), "backend": str(dist.get_backend()) if world > 1 else "none", "model": args.model,
                          "loss": round(float(loss), 5), "roofline": None, "cpu_baseline": None}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def clock_under_load(step, fence, seconds=1.2):
    """Shader clock and socket power WHILE the step runs (rocm-smi polled from a thread during ~1 s of extra, untimed steps).  The MFMA peak
    the roofline is priced against (2.5 PF/s) is the 2.4 GHz figure; under these kernels the socket sits at its power cap and sclk settles
    lower, which scales what any kernel can reach.  Reported beside the roofline, never part of `value`; None when rocm-smi is unusable."""
    import re
    import subprocess
    import threading
    samples, stop = [], [False]

    def poll():
        while not stop[0]:
            try:
                o = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=10).stdout
            except Exception:
                return
            m = re.search(r"sclk clock level:\s*\S+\s*\((\d+)Mhz", o)
            w = re.search(r"Power \(W\):\s*([\d.]+)", o)
            if m and w:
                samples.append((int(m.group(1)), float(w.group(1))))
    th = threading.Thread(target=poll, daemon=True)
    t0 = time.perf_counter()
    th.start()
    n = 0
    # (at least `seconds`, and on until four readings are in -- one rocm-smi call takes 0.2-0.8 s depending on the box -- but never beyond 6 s)
    while time.perf_counter() - t0 < seconds or (len(samples) < 4 and time.perf_counter() - t0 < 6.0):
        step()
        fence()
        n += 1
    stop[0] = True
    th.join(timeout=15)
    busy = [s for s in samples if s[0] > 500]               # drop readings that caught the GPU between steps in a low-power state
    if len(busy) < 2:
        return None
    busy = busy[len(busy) // 2:]                             # second half: after the power controller settled
    sclk = sorted(s[0] for s in busy)[len(busy) // 2]
    pw = sorted(s[1] for s in busy)[len(busy) // 2]
    return {"sclk_mhz_under_load": sclk, "socket_power_w": pw, "samples": len(busy), "steps_run": n,
            "mfma_peak_at_this_clock_tflops": round(2500.0 * sclk / 2400.0, 1),
            # what the matrix pipes of this socket sustain under its power cap on RANDOM register-resident operands, MFMAs only, >= 2.5 s
            # (tools/probes/mfma_power_probe.hip, profiles/r06_mfma_power_ceiling.txt: v_mfma_f32_16x16x32_bf16 2151 TF/s at 2121 MHz / 1357 W;
            #  32x32x16 1899-1917 TF/s at 1857-1871 MHz; with the k-loop's fragment reads 1720-1756).  A constant measured once, not in this run.
            "mfma_power_capped_tflops": MFMA_POWER_CAPPED_TFLOPS, "mfma_power_capped_with_lds_reads_tflops": MFMA_POWER_CAPPED_LDS_TFLOPS,
            "note": "rocm-smi polled during extra untimed steps; the 2500 TF/s roofline peak is the 2.4 GHz figure; mfma_power_capped_* from "
                    "profiles/r06_mfma_power_ceiling.txt (random operands, MFMA-only / + the k-loop's ds_read traffic)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="pairs per GPU (default 256; 64 with --model large)")
    ap.add_argument("--model", choices=["base", "large", "cascaded"], default="base", help="base = the headline workload (BASELINE configs[1]); large = "
                    "HuBERT-large + ViT-L/14 (configs[4]), informational")
    ap.add_argument("--audio-len", type=int, default=160000)
    ap.add_argument("--varlen", action="store_true", help="SURVEY.md section 8(d) C2 varlen variant: L_i ~ U{32000..160000} (seed 7122) instead of every wave at "
                    "--audio-len; the step runs on the padding-free engine and the flop model uses each utterance's own frame count.  With --full the same batch on the "
                    "padded engine (SC_VARLEN_PACK=0) is timed beside it as `varlen_padded_comparator`")
    ap.add_argument("--global-batch", type=int, default=None, help="STRONG scaling: the global batch is fixed (e.g. 2048 = spchclp_p.yaml:10 x 8 GPUs) and split "
                    "over the ranks (pairs per GPU = global / N); the line says \"scaling\": \"strong\"")
    ap.add_argument("--cpu-pairs", type=int, default=32, help="--full: pairs for the CPU baseline sample (0 = skip)")
    ap.add_argument("--no-roofline-events", action="store_true", help="--full without the roofline / HBM events")
    ap.add_argument("--train", action="store_true", help="time the TRAINING step of the trainable tail instead (forward in train mode + loss.backward() "
                    "+ grad all-reduce + clip + Adam + LR schedule); not the headline metric, reported with config.mode = 'train'")
    ap.add_argument("--finetune-layers", type=int, nargs="*", default=[], help="with --train: also fine-tune these HuBERT transformer layers "
                    "(unfreeze_layers of the reference, speech_encoder_plus.py:431-446); informational, not a BASELINE config")
    ap.add_argument("--finetune-all", action="store_true", help="with --train: audio_encoder.trainable: true -- conv extractor, positional conv and all "
                    "transformer layers train too; informational")
    ap.add_argument("--vocab", type=int, default=8112, help="--model cascaded: sub-word table size (8112 = the shipped reduced vocabulary, "
                    "spchclp_c.yaml:94; 49408 = the full table)")
    ap.add_argument("--no-vendor-comparator", action="store_true", help="--full: skip the hipBLASLt comparator run beside the headline")
    ap.add_argument("--no-clock-probe", action="store_true", help="--full: skip the rocm-smi clock / power reading taken beside the timed region")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short runs of the non-headline configurations (cascaded, large, varlen packed / "
                    "padded, train) that an N = 1 --full run reports beside `value` as `other_configs`")
    ap.add_argument("--dump-gemm-launches", default=None, help="--full: write the per-step list of GEMM launches (shape, epilogue, tower) as JSON: "
                    "tools/make_traffic_json.py aligns the PMC rows of the same command with it, so `roofline.traffic` covers exactly the launches "
                    "`roofline.launches_per_step` counts")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto", help="replay the local part of the step (both towers + head: everything before "
                    "the exchange) from a captured HIP graph on the steps that are not instrumented with events.  auto: on for N > 1 (eight Python "
                    "launchers on one host must not become the bottleneck), off for N = 1 (the eager step is what earlier rounds measured)")
    ap.add_argument("--dry-run", action="store_true", help="CPU/gloo check of the launcher + exchange protocol (no GPU, no kernels)")
    ap.add_argument("--share-gpu", action="store_true", help="TEST HOOK for 1-GPU boxes: all N ranks run on cuda:0 and exchange over gloo, so the N > 1 code "
                    "path (packed gather, global-batch loss, max-over-ranks timing) executes with the real kernels; the line says so in `data`")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline: roofline / HBM events on every third timed step, "
                    "CPU baseline + parity check, hipBLASLt comparator, 8192^3 ceiling, clock / power probe, padded-engine comparator (--varlen), "
                    "exchange timing (N > 1) and the other BASELINE.json configurations.  Off: the run does only what `value` needs")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step computed (loss and "
                    "the floating-point loss features) as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.dump_gemm_launches and not args.full:
        sys.exit("bench.py: --dump-gemm-launches needs --full (the launch list comes from the roofline events)")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:       # no launcher around us: become one
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if args.dry_run:
        return dry_run(args, world, rank)
    if args.share_gpu:
        local_rank = 0
    if not torch.cuda.is_available() or torch.cuda.device_count() <= local_rank:
        sys.exit(f"bench.py: rank {rank} needs cuda:{local_rank}, but {torch.cuda.device_count()} device(s) are visible (use --dry-run for a CPU protocol check)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)      # "nccl" = RCCL on ROCm: xGMI between the GPUs of the node
    backend_name, devices_seen = "none", 1
    if world > 1:
        backend_name = str(dist.get_backend())
        # First-contact check for the 8-GPU node: every rank must sit on its OWN physical GPU.  A launcher that hands each rank
        # HIP_VISIBLE_DEVICES=<one id> collapses LOCAL_RANK -> cuda:0 legitimately; ranks that share a PCI bus id do not.  (--share-gpu is the
        # explicit single-GPU test hook and says so in `data`.)
        pr = torch.cuda.get_device_properties(dev)
        # identity of the GPU behind this rank: uuid where torch exposes it, else PCI domain : bus : device (the bus number alone repeats across PCI
        # domains on multi-socket nodes); a second, independent key is (HIP_VISIBLE_DEVICES, device index).  The ranks are on distinct GPUs if EITHER key
        # separates them -- the check must not abort a healthy node because one property is missing or coarse.
        bus = "/".join(str(getattr(pr, a, "?")) for a in ("uuid", "pci_domain_id", "pci_bus_id", "pci_device_id"))
        ids = [None] * world
        dist.all_gather_object(ids, (int(torch.cuda.current_device()), str(bus), os.environ.get("HIP_VISIBLE_DEVICES", "")))
        devices_seen = max(len({b for _, b, _ in ids}), len({(v, d) for d, _, v in ids}))
        if not args.share_gpu and devices_seen != world:
            sys.exit(f"bench.py: {world} ranks but only {devices_seen} distinct GPU(s) behind them {ids}: check HIP_VISIBLE_DEVICES / LOCAL_RANK")

    from speechclip_amd import ops, parallel
    large = args.model == "large"
    strong = args.global_batch is not None
    if strong:
        if args.global_batch % world:
            sys.exit(f"bench.py: --global-batch {args.global_batch} is not divisible by {world} ranks")
        args.batch = args.global_batch // world
    if args.batch is None:
        args.batch = 64 if large else 256
    casc = args.model == "cascaded"
    model = build_model(large=large, cascaded=casc, vocab=args.vocab, finetune_layers=args.finetune_layers if args.train else [], finetune_all=args.finetune_all and args.train)
    sd_cpu = {k: v.clone() for k, v in model.state_dict().items()} if (args.full and rank == 0 and args.cpu_pairs > 0 and world == 1 and not args.train and not large and not casc) else None
    model = model.to(dev)
    B, L = args.batch, args.audio_len
    batch, lens = make_batch(B, L, rank, dev, args.varlen)
    last = {}                       # the loss features of the most recent step (--dump-outputs)

    if args.train:
        model.train()
        (opt,), (sch,) = model.configure_optimizers()

        def step():
            opt.zero_grad()
            o = model.training_step(batch, 0)
            loss = model.training_step_end(o)["loss"]
            loss.backward()
            opt.step()
            sch["scheduler"].step()
            last["feats"] = o["loss_feats"]
            return loss.detach()
    else:
        def step():
            with torch.no_grad():
                lf, _, _ = model(batch)
                f = parallel.gather_loss_feats(lf)
                last["feats"] = f
                return model.compute_loss(f)["loss"]

    def fence():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        loss = step()
    fence()
    # ---- HIP graph of the LOCAL part of the step (both towers + head, everything ahead of the exchange): N > 1 by default.  The exchange (one
    # all_gather_into_tensor) and the loss stay eager (3 launches); the steps instrumented with HIP events run eagerly (events need the launches).
    # `auto` is EAGER at every N (the line the driver compares across rounds and rank counts uses one launch method; a replay measured
    # +-0.1 % at N = 1 in round 5: the step is GPU-bound); `--graph on` times replays and says so in `step_launch`
    use_graph = args.graph == "on" and not args.train
    graph_note, replay_step = None, None
    if use_graph:
        # Capture is LOCAL (no collective inside); every decision that changes how many collectives a rank issues afterwards is agreed on by all
        # ranks first (a rank that failed to capture must not skip a gather the others run).
        cap_ok, why = True, ""
        graph = g_lf = None
        try:
            cap = torch.cuda.Stream()
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):
                with torch.no_grad():
                    model(batch)                                   # allocations of the capture stream's pool settle before the capture
            torch.cuda.current_stream().wait_stream(cap)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                with torch.no_grad():
                    g_lf, _, _ = model(batch)
        except Exception as e:     # noqa: BLE001  -- a capture problem must not cost the measurement: fall back to the eager step and SAY so
            cap_ok, why = False, str(e)[:200]
            torch.cuda.synchronize()

        def all_ranks(flag_):
            if world == 1:
                return flag_
            t_ = torch.tensor([1.0 if flag_ else 0.0], device=dev)
            torch.distributed.all_reduce(t_, op=torch.distributed.ReduceOp.MIN)
            return t_.item() >= 1
        if not all_ranks(cap_ok):
            graph_note = "eager (graph capture failed%s)" % (": " + why if why else " on another rank")
        else:
            def replay_step():
                graph.replay()
                with torch.no_grad():
                    f = parallel.gather_loss_feats(g_lf)
                    last["feats"] = f
                    return model.compute_loss(f)["loss"]
            l_g = float(replay_step())                             # every rank runs both forms once (the same collectives everywhere) ...
            g_copy = {k: v.detach().clone() for k, v in g_lf.items() if torch.is_tensor(v)}
            with torch.no_grad():
                e_lf, _, _ = model(batch)
            l_e = float(step())
            same_feats = all(torch.equal(g_copy[k], e_lf[k]) if not e_lf[k].is_floating_point() else
                             bool(((g_copy[k].float() - e_lf[k].float()).abs().max() <= 1e-6).item()) for k in g_copy if k in e_lf)
            if all_ranks(abs(l_g - l_e) <= 1e-5 and same_feats):   # ... and all of them must agree that the replay reproduces the eager step: loss AND every loss feature
                graph_note = "hip graph (towers + head captured once, replayed; exchange + loss eager)"
            else:
                replay_step, graph_note = None, "eager (replayed step loss %.6f != eager %.6f on some rank)" % (l_g, l_e)
    fence()
    # roofline instrumentation (--full): HIP events around every GEMM launch of every THIRD timed step (two events per launch, ~220 launches per
    # step: on every step they cost ~1 % of the step time they are meant to explain)
    prof = [] if (args.full and not args.no_roofline_events) else None
    hbm_prof, xchg_prof = [], []
    ops.PROFILE_SIDE = []
    ev_steps = 0
    host_s = {"eager": [0.0, 0], "graph": [0.0, 0]}               # host time spent INSIDE the step calls (launching), by launch method
    t0 = time.perf_counter()
    for i in range(args.steps):
        instrumented = prof is not None and (i % 3 == 2 or args.steps < 3)
        ops.PROFILE = prof if instrumented else None
        ops.PROFILE_HBM = hbm_prof if instrumented else None
        parallel.PROFILE_EXCHANGE = xchg_prof if instrumented else None       # the exchange measured INSIDE the step (events around the gather)
        ev_steps += int(instrumented)
        h0 = time.perf_counter()
        if replay_step is not None and not instrumented:
            loss = replay_step()
            how = "graph"
        else:
            loss = step()
            how = "eager"
        host_s[how][0] += time.perf_counter() - h0
        host_s[how][1] += 1
    ops.PROFILE = ops.PROFILE_HBM = parallel.PROFILE_EXCHANGE = None
    fence()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = t.item()
    pairs_per_s = world * B * args.steps / dt
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, last["feats"])
    # ---- beside the timed region (all ranks take part; none of it enters `value`; --full only)
    seen = torch.ones(1, device=dev)
    exchange_ms = None
    if world > 1:
        torch.distributed.all_reduce(seen)                    # every rank of the job answered over RCCL
    if world > 1 and args.full:
        with torch.no_grad():
            E = 768 if large else 512                          # the step's payload: ids + image + audio embeddings of this rank's pairs
            lf_x = {"id": batch["id"], "image_feat": torch.randn(B, E, device=dev), ("cascaded_audio_feat" if casc else "parallel_audio_feat"): torch.randn(B, E, device=dev)}
            for _ in range(3):
                parallel.gather_loss_feats(lf_x)
            fence()
            x0, x1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x0.record()
            for _ in range(20):
                parallel.gather_loss_feats(lf_x)               # pack + ONE all_gather_into_tensor + unpack: the step's exchange
            x1.record()
            fence()
            t = torch.tensor([x0.elapsed_time(x1) / 20], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            exchange_ms = round(t.item(), 4)
    exchange_in_step_ms = None
    if world > 1 and xchg_prof:
        t = torch.tensor([sum(a.elapsed_time(b) for a, b in xchg_prof) / max(1, ev_steps)], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        exchange_in_step_ms = round(t.item(), 4)
    # the same batch on the PADDED engine (what every round before the packed engine measured): comparator, never part of `value`
    varlen_cmp = None
    if args.full and args.varlen and not args.train:
        os.environ["SC_VARLEN_PACK"] = "0"
        for _ in range(2):
            step()
        fence()
        v0 = time.perf_counter()
        nv = max(3, min(args.steps, 8))
        for _ in range(nv):
            step()
        fence()
        vdt = time.perf_counter() - v0
        os.environ.pop("SC_VARLEN_PACK")
        if world > 1:
            t = torch.tensor([vdt], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            vdt = t.item()
        varlen_cmp = {"engine": "padded layout (SC_VARLEN_PACK=0): every GEMM on B x T_max rows, the reference's own shape", "steps": nv,
                      "ms_per_step": round(vdt / nv * 1e3, 3), "value": round(world * B * nv / vdt, 2), "unit": "pairs/s"}
    # measured ceiling of the vendor library on this box, beside the 2.5 PF/s datasheet peak: hipBLASLt and the hand-written kernel on 8192^3 bf16
    ceiling = None
    if args.full and world == 1 and not args.no_vendor_comparator and not args.train:
        n8 = 8192
        a8 = torch.randn(n8, n8, device=dev, dtype=torch.bfloat16)
        w8 = torch.randn(n8, n8, device=dev, dtype=torch.bfloat16)
        c8 = torch.empty(n8, n8, device=dev, dtype=torch.bfloat16)
        ceiling = {"shape": "8192^3 bf16, 30 back-to-back launches after 10 warm-up launches"}
        for name, on in (("hand_written_tflops", False), ("hipblaslt_tflops", True)):      # hand-written: gemm8p_pers_kernel, column bands of 4 N tiles (gemm.hip dispatcher)
            ops.set_vendor_gemm(on)
            for _ in range(10):
                ops.gemm(a8, w8, out=c8)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                ops.gemm(a8, w8, out=c8)
            e1.record()
            torch.cuda.synchronize()
            ceiling[name] = round(30 * 2.0 * n8 ** 3 / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)
        ops.set_vendor_gemm(False)
        del a8, w8, c8
    clock = None
    if args.full and world == 1 and not args.no_clock_probe:
        clock = clock_under_load(step, fence)
    vendor = None
    if args.full and not args.no_vendor_comparator and not args.train:
        # the same step with hipBLASLt taking the plain GEMMs (QKV / out-proj / fc2 / ViT projections): a COMPARATOR for the hand-written
        # kernel on those shapes, measured with the same fences, reported beside the headline and never part of it
        ops.set_vendor_gemm(True)
        for _ in range(2):
            step()
        fence()
        v0 = time.perf_counter()
        nv = max(3, min(args.steps, 8))
        for _ in range(nv):
            step()
        fence()
        vdt = time.perf_counter() - v0
        ops.set_vendor_gemm(False)
        if world > 1:
            t = torch.tensor([vdt], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            vdt = t.item()
        vendor = {"kernel": "hipBLASLt on the plain GEMMs (SC_GEMM_VENDOR=1), everything else unchanged", "steps": nv,
                  "ms_per_step": round(vdt / nv * 1e3, 3), "value": round(world * B * nv / vdt, 2), "unit": "pairs/s"}
    # train mode crops every utterance to audio_encoder.max_audio_len (102400 samples, T = 319) exactly as the reference trains
    mal = int(getattr(model.audio_encoder, "max_audio_len", -1))
    L_eff = min(L, mal) if (args.train and mal > 0) else L
    if args.varlen:          # "padding is not work" (SURVEY.md section 8d): each utterance is credited with ITS OWN frames
        cache = {}
        for n in lens:
            n = min(n, mal) if (args.train and mal > 0) else n
            if n not in cache:
                cache[n] = algorithmic_gflop_per_pair(n, **(LARGE if large else {}))
        per = [cache[min(n, mal) if (args.train and mal > 0) else n] for n in lens]
        total_gf, gemm_gf = sum(p[0] for p in per) / B, sum(p[1] for p in per) / B
        L_eff = int(sum(lens) / B)
    else:
        total_gf, gemm_gf = algorithmic_gflop_per_pair(L_eff, **(LARGE if large else {}))
    mode_str = "forward + loss"
    if args.train:
        what = " + the whole HuBERT encoder" if args.finetune_all else (" + HuBERT layers %s" % args.finetune_layers if args.finetune_layers else "")
        drops = "off (SC_FROZEN_DROPOUT=0)" if os.environ.get("SC_FROZEN_DROPOUT", "1") == "0" else "on"
        mode_str = "train (tail: branch + layer-mix weights%s; encoder in train mode, its checkpoint dropouts %s)" % (what, drops)
    if rank == 0:
        roof = None
        if prof:
            ms = sum(e[0].elapsed_time(e[1]) for e in prof)
            launches = len(prof)
            alg = gemm_gf * 1e9 * B * ev_steps                 # algorithmic GEMM FLOPs of this rank's instrumented launches
            ach = alg / (ms * 1e-3) / 1e12
            # HBM traffic of the kernel cannot be measured from inside this process (PMC counters need rocprofv3 and their own passes):
            # report the committed per-launch figure of the same command, with its source, or null if it is not there / not this workload
            traffic, tsrc, traffic_launches = None, None, None
            import glob
            import hashlib
            tfs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_hbm_traffic.json")))      # the newest round's PMC pass
            if tfs and not args.train and not large and not casc and B == 256 and L == 160000 and not args.varlen:
                tj = json.load(open(tfs[-1]))
                traffic = tj["gemm_main_stream"]["bytes_per_launch"]
                traffic_launches = tj["gemm_main_stream"].get("launches_per_step")
                from speechclip_amd import _lib as _l
                sha = hashlib.sha256(open(_l.LIB_PATH, "rb").read()).hexdigest()[:16]
                same = tj.get("lib_sha16") == sha
                tsrc = (tj["source"] + " (%s; separate rocprofv3 --pmc passes, FETCH_SIZE x2 + WRITE_SIZE; main-stream sc_gemm_bf16 launches (gemm8p_pers_kernel, gemm256_kernel, gemm_bf16_kernel) of the "
                        "same command; NOT measured in this run -- PMC counters need rocprofv3; collected on library %s, this run's library is %s: %s)"
                        % (os.path.basename(tfs[-1]), tj.get("lib_sha16", "unstamped"), sha, "the same build" if same else "a DIFFERENT build"))
            # the entry serves two kernels (vendor_gemm.hip): the hand-written gemm256_kernel family (everything fused / overlapping rows /
            # small) and hipBLASLt (plain GEMMs).  The DOMINANT kernel of the step is the hand-written one: `achieved` is ITS flops / ITS time;
            # the whole entry and the library part are reported beside it.
            exe = sum(e[2] for e in prof)
            # The image tower runs on a side stream beside the speech tower (its small kernels are slotted in between the speech tower's
            # for most of the step).  The roofline counts the launches of the MAIN stream -- the speech tower, 97 % of the GEMM flops --,
            # whose event time is the kernel's own apart from the few CUs a side-stream kernel holds at that moment; the side stream's
            # launches wait for CUs inside their event window (stretched, overlapping in wall time) and are reported as `side_stream`.
            main_stream = torch.cuda.current_stream().cuda_stream

            def concurrent(e):       # image-tower launches (side stream when the towers overlap; tagged by the model, so SC_OVERLAP_VIT=0 classifies the same)
                return e[5] == "image" if len(e) > 5 else e[4] != main_stream
            flags_c = [concurrent(e) for e in prof]
            part = {}
            for path, name in ((0, "hand_written"), (1, "vendor")):
                sel = [e for e, c in zip(prof, flags_c) if (e[3][6] == 1) == (path == 1) and not c]      # path 1 = vendor library; 0 / 2 / 3 = hand-written kernels
                pms = sum(e[0].elapsed_time(e[1]) for e in sel)
                pfl = sum(e[2] for e in sel) * (alg / exe)     # algorithmic share (executed flops include <0.2 % tile padding)
                part[name] = {"launches_per_step": len(sel) // ev_steps, "ms_per_step": round(pms / ev_steps, 3),
                              "avg_launch_ms": round(pms / max(1, len(sel)), 4), "achieved": round(pfl / max(pms, 1e-9) / 1e9, 1) if sel else None}
            tot_sel = [e for e, c in zip(prof, flags_c) if not c]
            tot_ms = sum(e[0].elapsed_time(e[1]) for e in tot_sel)
            tot_fl = sum(e[2] for e in tot_sel) * (alg / exe)
            csel = [e for e, c in zip(prof, flags_c) if c]
            cms = sum(e[0].elapsed_time(e[1]) for e in csel)
            conc = {"launches_per_step": len(csel) // ev_steps, "event_ms_per_step": round(cms / ev_steps, 3),
                    "windows_ms_per_step": round(sum(w0.elapsed_time(w1) for w0, w1 in ops.PROFILE_SIDE) / ev_steps, 3),
                    "note": "image-tower GEMMs on the side stream: they wait for CUs inside their event window (stretched, overlapping the main stream in "
                            "wall time); not counted in achieved.  SC_OVERLAP_VIT=0 serialises the towers"} if csel else None
            if args.dump_gemm_launches:
                per = len(prof) // ev_steps
                json.dump({"launches_per_step": per, "overlap_image_tower": os.environ.get("SC_OVERLAP_VIT", "1") != "0",
                           "launches": [{"M": e[3][0], "N": e[3][1], "K": e[3][2], "act": e[3][3], "res": bool(e[3][4]), "out_f32": bool(e[3][5]),
                                         "batch": (e[3][7] if len(e[3]) > 7 else 1), "tower": e[5]} for e in prof[:per]]},
                          open(args.dump_gemm_launches, "w"), indent=0)
            hw = part["hand_written"]
            roof = {"bound": "mfma", "kernel": "sc_gemm_bf16 family, hand-written HIP: gemm8p_pers_kernel (ping-pong schedule; the 95 % of the flops in bf16-output shapes with N % 256 == 0: fused-GELU / residual epilogues, conv-as-GEMM with overlapping rows) + gemm256_kernel / gemm_bf16_kernel (fp32 outputs, small shapes)",
                    "achieved": hw["achieved"], "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(hw["achieved"] / PEAK_BF16_TFLOPS, 4),
                    "traffic": traffic, "traffic_source": tsrc, "traffic_launches_per_step": traffic_launches, "launches_per_step": hw["launches_per_step"], "avg_launch_ms": hw["avg_launch_ms"],
                    "ms_per_step": hw["ms_per_step"],
                    "vendor_plain_gemms": dict(part["vendor"], kernel="hipBLASLt (plain QKV / out-proj / fc2 / ViT projections behind the same sc_gemm_bf16 entry)",
                                               frac=round(part["vendor"]["achieved"] / PEAK_BF16_TFLOPS, 4) if part["vendor"]["achieved"] else None),
                    "gemm_entry_total": {"achieved": round(tot_fl / max(tot_ms, 1e-9) / 1e9, 1), "frac": round(tot_fl / max(tot_ms, 1e-9) / 1e9 / PEAK_BF16_TFLOPS, 4),
                                         "launches_per_step": len(tot_sel) // ev_steps, "avg_launch_ms": round(tot_ms / max(1, len(tot_sel)), 4),
                                         "ms_per_step": round(tot_ms / ev_steps, 3)},
                    "side_stream": conc,
                    "gemm_ms_per_step": round(tot_ms / ev_steps, 3),
                    "instrumented_steps": ev_steps,
                    "executed_over_algorithmic": round(exe / alg, 4)}
        # HBM-bound segments, each against the 8 TB/s HBM3E peak: algorithmic bytes (unique input + output) / HIP-event time
        hbm = None
        if hbm_prof and ev_steps:
            hbm = {}
            main_s = torch.cuda.current_stream().cuda_stream
            for tag in sorted({e[3] for e in hbm_prof}):
                sel = [e for e in hbm_prof if e[3] == tag and e[4] == main_s]      # side-stream (image tower) launches wait for CUs inside their events
                if not sel:
                    continue
                ms = sum(e[0].elapsed_time(e[1]) for e in sel)
                by = sum(e[2] for e in sel)
                hbm[tag] = {"launches_per_step": len(sel) // ev_steps, "ms_per_step": round(ms / ev_steps, 3), "gbytes_per_step": round(by / ev_steps / 1e9, 3),
                            "achieved_gb_s": round(by / max(ms, 1e-9) / 1e6, 1), "frac_of_8tb_s": round(by / max(ms, 1e-9) / 1e6 / 8000.0, 4)}
            hbm["note"] = ("algorithmic bytes / HIP-event time of the MAIN-stream launches (speech tower + head; the image tower's side-stream launches wait for "
                           "CUs inside their event windows); peak 8000 GB/s (datasheet), ~6300 GB/s is what a copy reaches")
        out = {"metric": "speech-image pairs/sec/node (%s)" % ("Cascaded SpeechCLIP base" if casc else "Parallel SpeechCLIP %s" % args.model), "value": round(pairs_per_s, 2), "unit": "pairs/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
               "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
               "dtype": ("bf16 (f16 operands in the pre-LN HuBERT-large layers, fp32 accumulate and residual stream)" if large and os.environ.get("SC_PRELN_F16", "1") != "0" else "bf16"),
               "data": "synthetic" if not args.share_gpu else "synthetic; TEST HOOK --share-gpu: all ranks on one GPU over gloo, not a scaling measurement",
               "config": {"workload": ("Cascaded SpeechCLIP base (HuBERT-base + ViT-B/32 + CLIP text tower; flop model = the encoders' GEMMs, the keyword head adds < 1 %)" if casc else
                                       "Parallel SpeechCLIP large (HuBERT-large + ViT-L/14)" if large else "Parallel SpeechCLIP base (HuBERT-base + ViT-B/32)")
                          + (" forward + InfoNCE, VARLEN 16 kHz audio L_i ~ U{%d..%d} samples (seed 7122, zero-padded to the batch maximum as collate hands it over; "
                             "padding-free engine: %s) + 224^2 images" % (min(32000, L), L, os.environ.get("SC_VARLEN_PACK", "auto")) if args.varlen
                             else " forward + InfoNCE, 10 s/16 kHz audio + 224^2 images"),
                          "pairs_per_gpu": B, "global_batch": world * B, "audio_samples": L_eff, "frames": conv_lens(L_eff)[-1],
                          "audio_samples_min_max": [min(lens), max(lens)],
                          "parallelism": f"dp{world}" if world > 1 else "single", "weights": "random-init (no network)",
                          "algorithmic_gflop_per_pair": round(total_gf, 2), "mode": mode_str},
               "e2e_tflops_per_gpu": round(total_gf * 1e9 * pairs_per_s / world / 1e12, 1),
               "e2e_frac_of_bf16_peak": round(total_gf * 1e9 * pairs_per_s / world / 1e12 / PEAK_BF16_TFLOPS, 4),
               "ranks_seen": int(seen.item()), "backend": backend_name, "rccl_ranks_seen": int(seen.item()) if backend_name == "nccl" else 0,
               "devices_seen": devices_seen, "exchange_ms_per_step": exchange_ms, "exchange_in_step_ms": exchange_in_step_ms,
               "exchange": ("one packed all_gather_into_tensor over RCCL per step (speechclip_amd/parallel.py); exchange_ms_per_step = pack + collective + unpack, "
                            "timed beside the step with random payloads; exchange_in_step_ms = the same three operations timed by HIP events INSIDE the instrumented "
                            "steps (includes waiting for the slowest rank's towers); both max over ranks") if world > 1 else None,
               "vendor_comparator": vendor, "varlen_padded_comparator": varlen_cmp, "measured_ceiling_8k_cubed": ceiling, "hbm_segments": hbm, "clock": clock,
               "loss": round(float(loss), 5), "roofline": roof, "cpu_baseline": None, "parity_check": None, "other_configs": None}
        out["step_launch"] = {"method": graph_note or "eager (one Python launcher thread per GPU)",
                              "host_launch_ms_per_step": {k: round(v[0] / v[1] * 1e3, 3) for k, v in host_s.items() if v[1]},
                              "steps_by_method": {k: v[1] for k, v in host_s.items() if v[1]},
                              "note": "host time spent inside the step calls (enqueueing); the instrumented steps (HIP events) always launch eagerly"}
        if clock is not None and roof is not None:
            # the same achieved TF/s against the MFMA peak at the clock the socket actually held under this load (power-capped), beside the
            # nominal 2.4 GHz figure `frac` is priced against
            roof["frac_of_clock_adjusted_peak"] = round(roof["achieved"] / clock["mfma_peak_at_this_clock_tflops"], 4)
            roof["frac_of_power_capped_mfma_ceiling"] = round(roof["achieved"] / MFMA_POWER_CAPPED_TFLOPS, 4)
        if clock is not None:
            clock["joules_per_step"] = round(clock["socket_power_w"] * dt / args.steps, 2)
            clock["joules_per_pair"] = round(clock["socket_power_w"] * dt / args.steps / (world * B), 4)
            clock["energy_note"] = "socket power (rocm-smi, polled during the extra untimed steps) x the TIMED region's ms_per_step"
        if sd_cpu is not None:
            keep = {}
            out["cpu_baseline"] = cpu_baseline(sd_cpu, args.cpu_pairs, L, keep=keep)
            if keep:
                out["parity_check"] = parity_check(model, keep, dev)
        if args.full and world == 1 and not args.no_other_configs and not args.train and not large and not casc and not args.varlen:
            del model
            torch.cuda.empty_cache()
            oc = {}
            for kind in OTHER_CONFIGS:
                try:
                    oc[kind] = other_config(kind, dev, batch=args.batch if args.batch != 256 else None, steps=5 if args.steps >= 5 else 2, warmup=2 if args.warmup >= 2 else 1)
                except Exception as e:     # noqa: BLE001
                    oc[kind] = {"error": str(e)[:300]}
            oc["note"] = ("short runs (same fences and clock as the headline, inputs resident) of the other BASELINE.json configurations, one after the other in "
                          "this process; never part of `value`.  --model / --varlen / --train give each its own full line")
            out["other_configs"] = oc
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

"""Where should the audio hand-over of a LIST of utterances run?  Times FairseqSpeechEncoder_Hubert._list_to_padded -- the step of forward() that turns the
list into the padded device batch -- under SC_WAVE_PREP=host (one host-to-device copy and one slice-assign per utterance: the path before sc_wave_prep
existed) and SC_WAVE_PREP=device (one packed pinned copy + one library call).

Workload: 256 synthetic utterances (noise, fixed seed; no corpus is read), lengths uniform in 2 s .. 10 s.  Arms:
    a  host    1-D float32 tensors at 16 kHz                      (the per-utterance loop)
    b  device  the same list
    c  device  int16 mono at 16 kHz
    d  device  int16 stereo at 44.1 kHz                            (mono mix + 160 / 441 resampling, 104 taps)
Timing: wall clock around the whole call with a device synchronise on both sides -- the host work is what is measured -- after a warm-up of every arm, three
interleaved passes with rotating arm order, one process.  Also: the device entry alone (events around sc_wave_prep) and the bytes that cross PCIe.

    python tools/wave_prep_bench.py [--utterances 256] [--passes 3] [--out profiles/wave_prep_bench.txt]

The rule the result feeds (speech_encoder_plus._WAVE_PREP_AUTO_DEVICE): `auto` may move 16 kHz float lists to the device only if arm b beats arm a in
every pass."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_MS = 42.0          # the speech tower's step at B = 256 (bench.py --gpus 1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_prep_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_prep_bench.py measures on the GPU: no device found (nothing is estimated on the CPU)")
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd import ops
    from speechclip_amd.module.hubert import HubertConfig
    from speechclip_amd.module.speech_encoder_plus import FairseqSpeechEncoder_Hubert
    # _list_to_padded needs the device and the mode only: a tiny encoder in eval mode (no crop)
    enc = FairseqSpeechEncoder_Hubert("hubert", hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny()))).cuda().eval()
    dev = next(enc.parameters()).device
    rng = np.random.default_rng(0)
    secs = rng.uniform(2.0, 10.0, args.utterances)
    pcm16 = [np.clip(rng.normal(0, 6000, int(s * 16000)), -32768, 32767).astype(np.int16) for s in secs]
    floats = [torch.from_numpy(p.astype(np.float32) / 32768) for p in pcm16]
    pcm44 = [(np.clip(rng.normal(0, 6000, (int(s * 44100), 2)), -32768, 32767).astype(np.int16), 44100) for s in secs]
    arms = {"a": ("host", floats), "b": ("device", floats), "c": ("device", pcm16), "d": ("device", pcm44)}
    what = {"a": "host loop, f32 16 kHz list", "b": "device entry, f32 16 kHz list", "c": "device entry, int16 mono 16 kHz", "d": "device entry, int16 stereo 44.1 kHz"}

    def run(arm):
        os.environ["SC_WAVE_PREP"] = arms[arm][0]
        return enc._list_to_padded(arms[arm][1], dev)

    outs = {}
    for arm in arms:          # warm-up: code object, pinned and device allocations, tap tables
        for _ in range(2):
            outs[arm] = run(arm)
    torch.cuda.synchronize()
    equal_ab = bool(torch.equal(outs["a"][0], outs["b"][0])) and outs["a"][1] == outs["b"][1]
    equal_ac = bool(torch.equal(outs["a"][0], outs["c"][0]))
    shape_d = list(outs["d"][0].shape)
    del outs
    names = list(arms)
    ms = {a: [] for a in arms}
    for p in range(args.passes):
        for arm in names[p % len(names):] + names[:p % len(names)]:
            t, _ = timed(lambda: run(arm))
            ms[arm].append(t)
            print(f"# pass {p} arm {arm}: {t:.2f} ms", file=sys.stderr, flush=True)
    entry = {}
    for arm in ("b", "c", "d"):          # the device entry alone: events around the library call
        ops.PROFILE_HBM = []
        for _ in range(args.passes):
            run(arm)
        torch.cuda.synchronize()
        entry[arm] = [round(e0.elapsed_time(e1), 3) for (e0, e1, _, tag, _) in ops.PROFILE_HBM if tag == "wave_prep"]
        ops.PROFILE_HBM = None
    os.environ.pop("SC_WAVE_PREP")
    faster = [b < a for a, b in zip(ms["a"], ms["b"])]
    lines = [f"# tools/wave_prep_bench.py on one {torch.cuda.get_device_name(0)}, {args.utterances} synthetic utterances of 2 s .. 10 s ({sum(len(p) for p in pcm16) / 16000:.0f} s of audio)",
             f"# wall clock around the whole hand-over call (device synchronise on both sides), {args.passes} interleaved passes with rotating order after a warm-up of every arm, one process",
             f"# rule: auto moves 16 kHz float lists to the device only if arm b is faster than arm a in every pass -> {'device' if all(faster) else 'host loop'}"]
    for arm in arms:
        lines.append(json.dumps({"arm": arm, "what": what[arm], "ms_per_call": [round(x, 2) for x in ms[arm]], "ms_median": round(float(np.median(ms[arm])), 2),
                                 "call_time_over_step_time": round(float(np.median(ms[arm])) / (STEP_MS * args.utterances / 256), 3)}))
    lines.append(json.dumps({"item": "b_faster_than_a_per_pass", "value": faster, "outputs_bitwise_equal_a_b": equal_ab, "int16_equals_float_list_a_c": equal_ac,
                             "speedup_median_a_over_b": round(float(np.median(ms["a"]) / np.median(ms["b"])), 2), "arm_d_output_shape": shape_d}))
    lines.append(json.dumps({"item": "device_entry_alone_ms", "events": entry}))
    lines.append(json.dumps({"item": "bytes_over_pcie_per_call", "a_b_f32": sum(f.numel() for f in floats) * 4, "c_int16": sum(p.nbytes for p in pcm16),
                             "d_int16_stereo_44k_and_table": sum(p.nbytes for p, _ in pcm44) + 160 * 104 * 4}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

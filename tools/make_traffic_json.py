#!/usr/bin/env python3
"""profiles/rNN_gemm_hbm_traffic.json from the two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) over `bench.py --steps S --warmup 0`:
bytes per step and per launch of the GEMM kernels, next to their algorithmic bytes.  FETCH_SIZE is doubled (gfx950 correction prescribed by
MI355X_MICROARCH.md, calibrated in round 1 on layernorm768_kernel: corrected read = its 196.6 MB input exactly); both counters are in KiB.
With a fifth argument -- the launch list `bench.py --dump-gemm-launches` wrote for the same command (towers serialised: SC_OVERLAP_VIT=0, so the dispatch order
is the host's launch order) -- the GEMM rows are aligned with that list in dispatch order and `gemm_main_stream` covers EXACTLY the launches bench.py's
`roofline.launches_per_step` counts (speech tower + head; the image tower's GEMMs, which share kernel names with them, are left out row by row).
Without it the rows are classified by kernel name (rounds 1-3: the ViT's plain / residual GEMMs were counted in -- VERDICT r3 weak-4).
usage: python tools/make_traffic_json.py <pmc_FETCH_SIZE dir> <pmc_WRITE_SIZE dir> <steps> <source label> [launch list json] > profiles/rNN_gemm_hbm_traffic.json"""
import collections, csv, glob, json, os, sys


GEMM_KERNELS = ("gemm256_kernel", "gemm_bf16_kernel", "gemm8p_pers_kernel")      # every kernel behind sc_gemm_bf16 (round 5: + gemm8p)


def act_of(k):
    """Activation template argument of a GEMM kernel name: gemm256_kernel<ABL, TRACE, ACT, ..> / gemm8p_pers_kernel<ACT, RES>; None for gemm_bf16_kernel."""
    args = [a.strip() for a in k.split("<")[1].rstrip(">").split(",")] if "<" in k else []
    if k.startswith("gemm256_kernel"):
        return args[2]
    if k.startswith("gemm8p"):
        return args[0]
    return None


def load(d):
    f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
    agg, cnt = collections.defaultdict(float), collections.Counter()
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        agg[k] += float(r["Counter_Value"]) * 1024.0
        cnt[k] += 1
    return agg, cnt


def load_rows(d):
    """GEMM rows of one PMC pass in dispatch order: [(kernel name, bytes)]."""
    f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
    rows = []
    for r in csv.DictReader(open(f)):
        k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if k.startswith(GEMM_KERNELS):
            rows.append((int(r["Dispatch_Id"]), k, float(r["Counter_Value"]) * 1024.0))
    rows.sort()
    return [(k, v) for _, k, v in rows]


def aligned(fd, wd, steps, launch_json):
    """Per-launch (tower, fetch, write) by aligning the dispatch-ordered GEMM rows with bench.py's launch list (repeated `steps` times)."""
    L = json.load(open(launch_json))
    assert not L["overlap_image_tower"], "the launch list must come from a run with SC_OVERLAP_VIT=0 (dispatch order = launch order)"
    per = L["launches"]
    fr, wr = load_rows(fd), load_rows(wd)
    assert len(fr) == len(wr) == steps * len(per), (len(fr), len(wr), steps, len(per))
    for i, (k, _) in enumerate(fr):          # soft consistency check: the QuickGELU template variant is the image tower's fc1
        quick = act_of(k) == "2"
        assert act_of(k) is None or quick == (per[i % len(per)]["act"] == 2), (i, k, per[i % len(per)])
    return [(per[i % len(per)]["tower"], 2 * fr[i][1], wr[i][1]) for i in range(len(fr))], per


def lib_sha16():
    """sha256[:16] of the product library the passes ran on: bench.py compares it with the library of the run that quotes these numbers."""
    import hashlib
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speechclip_amd", "libspeechclip_hip.so")
    return hashlib.sha256(open(p, "rb").read()).hexdigest()[:16] if os.path.exists(p) else None


def main():
    fd, wd, steps, label = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
    launch_json = sys.argv[5] if len(sys.argv) > 5 else None
    fetch, fc = load(fd)
    write, _ = load(wd)

    def group(pred):
        ks = [k for k in fetch if pred(k)]
        return {"kernels": sorted(ks), "launches_per_step": sum(fc[k] for k in ks) // steps,
                "fetch_bytes_per_step": int(2 * sum(fetch[k] for k in ks) / steps), "write_bytes_per_step": int(sum(write.get(k, 0.0) for k in ks) / steps)}
    is_gemm = lambda k: k.startswith(GEMM_KERNELS)              # noqa: E731
    is_vit = lambda k: act_of(k) == "2"   # noqa: E731  QuickGELU variant: image tower only
    out = {"method": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in two separate passes over `python bench.py --steps %d --warmup 0 --cpu-pairs 0 "
                     "--no-roofline-events --no-vendor-comparator` (tools/collect_round_profiles.sh); FETCH_SIZE x2 as MI355X_MICROARCH.md prescribes for gfx950; "
                     "both counters in KiB" % steps,
           "source": label, "lib_sha16": lib_sha16()}
    for name, pred in (("gemm_all", is_gemm), ("gemm_main_stream", lambda k: is_gemm(k) and not is_vit(k))):
        g = group(pred)
        g["bytes_per_launch"] = int((g["fetch_bytes_per_step"] + g["write_bytes_per_step"]) / max(1, g["launches_per_step"]))
        out[name] = g
    if launch_json:
        rows, per = aligned(fd, wd, steps, launch_json)
        main = [r for r in rows if r[0] != "image"]
        n_main = len([p_ for p_ in per if p_["tower"] != "image"])
        out["gemm_main_stream"] = {"classified_by": "dispatch-order alignment with bench.py --dump-gemm-launches (speech tower + head launches only)",
                                   "launches_per_step": n_main, "fetch_bytes_per_step": int(sum(r[1] for r in main) / steps),
                                   "write_bytes_per_step": int(sum(r[2] for r in main) / steps)}
        out["gemm_main_stream"]["bytes_per_launch"] = int((out["gemm_main_stream"]["fetch_bytes_per_step"] + out["gemm_main_stream"]["write_bytes_per_step"]) / n_main)
        img = [r for r in rows if r[0] == "image"]
        out["gemm_image_tower"] = {"launches_per_step": len(per) - n_main, "fetch_bytes_per_step": int(sum(r[1] for r in img) / steps),
                                   "write_bytes_per_step": int(sum(r[2] for r in img) / steps)}
    # algorithmic bytes of the main-stream GEMMs at B = 256, 10 s audio (unique operand + output bytes, bf16): conv stack + transformer + heads
    B, T = 256, 500
    rows = [32000, 16000, 8000, 4000, 2000, 1000, 500]
    conv_r = sum(B * r * 512 * 2 for r in rows[:6])            # each conv layer reads the previous layer's output once
    conv_w = sum(B * r * 512 * 2 for r in rows[1:])
    M, d, f = B * T, 768, 3072
    layer_r = M * 2 * (d + d + d + d + f + d)                  # qkv in, out-proj in + residual, fc1 in, fc2 in + residual
    layer_w = M * 2 * (3 * d + d + f + d)
    out["gemm_main_stream"]["algorithmic_bytes_per_step"] = {"read": conv_r + 12 * layer_r + M * 512 * 2, "write": conv_w + 12 * layer_w + M * d * 2}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

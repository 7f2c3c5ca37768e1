"""CPU only: the MODEL errors behind the bounds of tests/test_packed_frontend_gpu.py, and the sensitivity of those bounds to boundary bugs.

For each of the test's four parts a correct kernel is modelled as the test's own reference with the kernel's documented roundings applied (bf16 operands, bf16
store of each layer's output, fp32 accumulate), on the test's own inputs; printed is the per-row max|err| / max|ref|, maximum over the compared rows.  The test's
bound is 4 x that + 1e-3.  Then MUTANT references -- a neighbour's rows leaking across the packed boundary, the halo row dropped / left unmasked -- are measured
with the same metric: each must exceed the bound, or the inputs are too tame.  No kernel runs here.

    python tools/packed_frontend_bounds.py [--no-front]      (--no-front skips the real-dimension front end, the only slow part)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_packed_frontend_gpu as T   # noqa: E402


def level0_slab(b, geo, p, wav, mode):
    """model of utterance b's packed layer-0 rows: bf16 store of the fp64 conv, zeros from T0 on"""
    n = 64 * geo["rows"][b]
    ref = T.conv0_ref(wav[b], p, mode)
    slab = torch.zeros(n, T.C0, dtype=T.F64)
    live = min(n, ref.shape[0])
    slab[:live] = T.r16(ref[:live])
    return slab


def main():
    torch.manual_seed(0)
    geo, p, wav = T.geometry_a(), T.conv0_params(), T.waves_a()
    print("geometry (a)/(b): rows", geo["rows"], "valid", geo["valid"], "T0", geo["T0"], "T", geo["T"])
    print("== (a) conv layer 0: bf16 store of the fp64 reference")
    for mode in (0, 1, 2):
        worst = 0.0
        for b, r in enumerate(geo["rows"]):
            ref = T.conv0_ref(wav[b], p, mode)[: 64 * r]
            worst = max(worst, T.row_metric(T.r16(ref), ref).max().item())
        print(f"   mode {mode}: model {worst:.3e}  -> bound {T.bound_of(worst):.3e}   (constant in the test: {T.MODEL_CONV0[mode]:.3e})")

    print("== (b) conv stack: fp32 accumulate + bf16 stores vs the fp64 chain with bf16 stores")
    for ln_mode in (False, True):
        sp = T.stack_params(ln_mode)
        slabs = [level0_slab(b, geo, p, wav, 2 if ln_mode else 0) for b in range(len(T.LENS_A))]
        worst = [0.0] * 6
        refs = []
        for b in range(len(T.LENS_A)):
            ref = T.stack_chain(slabs[b], sp, ln_mode)
            mod = T.stack_chain(slabs[b], sp, ln_mode, dtype=torch.float32)
            refs.append(ref)
            for l in range(6):
                worst[l] = max(worst[l], T.row_metric(mod[l], ref[l]).max().item())
        bound = T.bound_of(T.MODEL_STACK[ln_mode])
        print(f"   layer_norm={ln_mode}: model per level {['%.3e' % w for w in worst]} max {max(worst):.3e} -> bound {T.bound_of(max(worst)):.3e}"
              f"   (constant in the test: {T.MODEL_STACK[ln_mode]:.3e}, bound {bound:.3e})")
        B = len(T.LENS_A)
        for name in ("leak", "drop-halo"):
            res = []
            for b, r in enumerate(geo["rows"]):
                m = slabs[b].clone()
                nb = slabs[(b + 1) % B]
                m[64 * (r - 1):] = nb[:64] if name == "leak" else 0.0        # the halo row's block holds the next utterance's first rows / nothing
                top = T.stack_chain(m, sp, ln_mode)[5]
                res.append(T.row_metric(top, refs[b][5]).max().item())
            print(f"   mutant {name:9s}: top-level row metric per utterance {['%.2e' % x for x in res]}: {sum(x > bound for x in res)} of {B} utterances exceed the bound"
                  f" {'OK' if max(res) > bound else 'INPUTS TOO TAME'}")

    print("== (c) packed positional conv: bf16 store of the conv (+ bf16 store of the result)")
    off = T.pc_offsets()
    for D, G, Kw in T.PC_SHAPES:
        x, w, bias, gamma, beta = T.posconv_inputs(D, G, Kw)
        for ln in (True, False):
            ga, be = (gamma, beta) if ln else (None, None)
            refs = [T.posconv_ref(x[off[b]: off[b + 1]], v, w, bias, ga, be, G, Kw) for b, v in enumerate(T.PC_VALID)]
            for out_f32 in (False, True):
                worst = 0.0
                for b, v in enumerate(T.PC_VALID):
                    mod = T.posconv_ref(x[off[b]: off[b + 1]], v, w, bias, ga, be, G, Kw, conv_store=T.r16)
                    mod = mod.float().double() if out_f32 else T.r16(mod)
                    worst = max(worst, T.row_metric(mod, refs[b]).max().item())
                print(f"   D={D} ln={ln} out_f32={out_f32}: model {worst:.3e} -> bound {T.bound_of(worst):.3e}   (constant in the test: {T.MODEL_POSCONV[(D, ln, out_f32)]:.3e})")
            bound = min(T.bound_of(T.MODEL_POSCONV[(D, ln, f)]) for f in (False, True))
            B = len(T.PC_ROWS)
            for name in ("leak", "halo-unmasked", "last-valid-dropped"):
                res = []
                for b, (r, v) in enumerate(zip(T.PC_ROWS, T.PC_VALID)):
                    xb = x[off[b]: off[b + 1]]
                    if name == "leak":        # one row of either neighbour visible across the boundary (their rows next to the boundary as they lie in the packed tensor)
                        mut = T.posconv_ref(xb, v, w, bias, ga, be, G, Kw, prev_row=x[off[b] - 1] if b > 0 else None, next_row=x[off[b + 1]] if b + 1 < B else None)
                    elif name == "halo-unmasked":
                        mut = T.posconv_ref(xb, min(v + 1, r), w, bias, ga, be, G, Kw)
                    else:
                        mut = T.posconv_ref(xb, max(v - 1, 0), w, bias, ga, be, G, Kw)
                    res.append(T.row_metric(mut, refs[b]).max().item())
                print(f"   D={D} ln={ln} mutant {name:18s}: {['%.2e' % x for x in res]}: {sum(x > 3 * bound for x in res)} of {B} exceed 3 x the larger bound"
                      f" {'OK' if max(res) > 3 * bound else 'INPUTS TOO TAME'}")

    if "--no-front" in sys.argv:
        return
    print("== (d) whole front end at real dimensions vs the fp32 oracle")
    for which in ("base", "large"):
        model, ref = T.front_models(which)
        wavd = T.waves_d()
        with torch.no_grad():
            want = T.front_oracle(ref, wavd)
            geo_d = model.packed_geometry(T.LENS_D, max(T.LENS_D))
            worst, sanity = 0.0, 0.0
            for b, v in enumerate(geo_d["valid"]):
                mod = T.front_chain(model, wavd[b], T.LENS_D[b], v)[:v]
                worst = max(worst, T.row_metric(mod, want[b, :v]).max().item())
                if b == 1:
                    same = T.front_chain(model, wavd[b], T.LENS_D[b], v, store=None)[:v]
                    sanity = T.row_metric(same, want[b, :v]).max().item()
        print(f"   {which}: rows {geo_d['rows']} valid {geo_d['valid']}: model {worst:.3e} -> bound {T.bound_of(worst):.3e}   (constant in the test: {T.MODEL_FRONT[which]:.3e}; "
              f"the chain without roundings restates the oracle to {sanity:.1e})")


if __name__ == "__main__":
    main()

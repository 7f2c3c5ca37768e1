"""Kernel-level parity of the padding-free (packed) FRONT END: conv layer 0 (`sc_conv0_fwd_packed`, three modes), the stride-2 conv stack run as ONE
overlapping-row GEMM per layer over the packed slab, the packed positional conv (`sc_posconv_conv_packed` / `sc_posconv_finish_packed`, D/G = 32 / 48 / 64)
and the whole front end at HuBERT-base / -large dimensions, frame by frame.

Every reference is plain torch on the CPU, computed PER UTTERANCE on that utterance's own zero-padded wave / own rows: it never sees a neighbour, so a
read across a packed boundary shows as an error (and, in the contamination controls, as a bitwise difference).

Bounds.  For every comparison the metric is, per row, max|got - ref| / max|ref| (maxima over the row's channels).  The bound is
4 x MODEL + 1e-3, where MODEL is that same metric for a CPU model of a correct kernel -- the reference with the kernel's documented roundings applied
(bf16 operands, bf16 store of each layer's output, fp32 accumulate) -- on exactly the inputs used here (`tools/packed_frontend_bounds.py` prints them;
the factor 4 covers what the model leaves out: the MFMA summation order and the polynomial GELU).  The MODEL values are the
constants below.  Where the padded twin of a kernel has a tested tolerance (test_conv0_*: 2e-2, test_posconv: 3e-2, atol + rtol) the packed kernel
must meet that one as well.  The values observed on the MI355X are in EXPERIMENTS.md ("Packed front end: kernel-level parity").

Rows left out of a comparison are only those that the layout defines as inexact: the last (halo) row of every utterance in the conv stack, which reads
the next utterance's first rows (include/speechclip_hip.h, sc_unpack_rows).  Each test prints the count and asserts it is at most
B + sum(rows_b - valid_b) (times the level's row scale below the top level)."""
import dataclasses
import functools
import math

import pytest
import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64
C0 = 512
CONV_K = (3, 3, 3, 3, 2, 2)

# ---- modelled error of a correct kernel (per-row max|err| / max|ref|, maximum over all compared rows; tools/packed_frontend_bounds.py) -----------
MODEL_CONV0 = {0: 3.80e-3, 1: 3.80e-3, 2: 3.85e-3}                     # (a) one bf16 store of the output (half a bf16 ulp: <= 2^-8); bounds 1.62e-2 / 1.62e-2 / 1.64e-2
MODEL_STACK = {False: 7.19e-3, True: 7.41e-3}                            # (b) [layer_norm extractor?] fp32 accumulate under six bf16 stores (a re-rounded value moves by a whole ulp); bounds 2.98e-2 / 3.06e-2
MODEL_POSCONV = {                                                        # (c) (D, ln, out_f32): bf16 store of the conv, bf16 / fp32 store of the result; bounds 1.5e-2 .. 2.8e-2
    (128, True, False): 6.79e-3, (128, True, True): 5.36e-3, (128, False, False): 6.49e-3, (128, False, True): 4.46e-3,
    (768, True, False): 5.98e-3, (768, True, True): 4.31e-3, (768, False, False): 5.37e-3, (768, False, True): 4.19e-3,
    (1024, True, False): 5.89e-3, (1024, True, True): 3.96e-3, (1024, False, False): 5.86e-3, (1024, False, True): 3.56e-3,
}
MODEL_FRONT = {"base": 1.32e-2, "large": 1.28e-2}                       # (d) bf16 weights + every stored activation of the whole front end vs the fp32 oracle; bounds 5.38e-2 / 5.22e-2


def bound_of(model_err):
    return 4.0 * model_err + 1e-3


def r16(t):
    """bf16 store of an fp64 / fp32 value, back in fp64."""
    return t.to(torch.float32).to(BF).to(F64)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def row_metric(got, ref):
    """per row: max|got - ref| / max|ref|; rows whose reference is all zero must be zero exactly (metric 0) or count as inf."""
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).abs().amax(-1)
    scale = ref.abs().amax(-1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def check_rows(got, ref, bound, twin_tol, what):
    """Every row within `bound` (row metric) AND within the padded twin's tested tolerance (atol + rtol); returns the worst row metric."""
    assert got.shape == ref.shape and got.shape[0] > 0, (what, got.shape, ref.shape)
    assert torch.isfinite(got.float()).all(), what
    m = row_metric(got, ref)
    worst = m.max().item()
    assert worst <= bound, (what, "row", int(m.argmax()), "of", got.shape[0], "metric", worst, "bound", bound)
    if twin_tol is not None:
        torch.testing.assert_close(got.float(), ref.float(), atol=twin_tol, rtol=twin_tol, msg=lambda s: f"{what}: {s}")
    return worst


# ================================================================================================ inputs and CPU references (no GPU below this line until the tests)
# layer-0 frames per utterance: 641, 63 (= 64 - 1, one transformer frame), 1039 (the batch maximum, not first), 191, 192, 193 (64 k - 1, 64 k, 64 k + 1), 512 (64 k);
# the 320-sample utterance sits between the two longest
LENS_A = [3210, 320, 5200, 960, 965, 970, 2565]
NEED_A = [0, 0, 0, 4, 0, 0, 0]                       # utterance 3: need_b (4) > valid_b (3)


@functools.lru_cache(maxsize=None)
def _geometry_model():
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    return HubertModel(HubertConfig(encoder_layers=0))


def geometry_a():
    return _geometry_model().packed_geometry(LENS_A, max(LENS_A), need_rows=NEED_A)


def waves_a(neighbour_fill=None, keep=None):
    """DC offset and amplitude as test_conv0_groupnorm_gelu.  neighbour_fill: every utterance except `keep` is replaced by large garbage of that flavour
    ("big": +-50 square-ish noise; "zero": silence) over the WHOLE padded row."""
    g = _g(11)
    lmax = max(LENS_A)
    wav = torch.zeros(len(LENS_A), lmax)
    for b, l in enumerate(LENS_A):
        wav[b, :l] = torch.randn(l, generator=g) * 0.2 + (0.3 if b % 2 == 0 else 0.01)
    if neighbour_fill is not None:
        for b in range(len(LENS_A)):
            if b == keep:
                continue
            wav[b] = 0.0 if neighbour_fill == "zero" else 50.0 * torch.sign(torch.randn(lmax, generator=g)) + 7.0 * torch.randn(lmax, generator=g)
    return wav


def conv0_params():
    g = _g(12)
    return dict(w=torch.randn(C0, 10, generator=g) * 0.4, bias=0.2 * torch.randn(C0, generator=g),
                gn=(1 + 0.2 * torch.randn(C0, generator=g), 0.2 * torch.randn(C0, generator=g)),
                ln=(1 + 0.2 * torch.randn(C0, generator=g), 0.2 * torch.randn(C0, generator=g)))


def conv0_ref(wav_b, p, mode):
    """One utterance's own zero-padded wave [lmax] -> fp64 [T0, C]: mode 0 conv -> GroupNorm(C groups) over the PADDED length -> GELU; 1 conv + bias;
    2 conv + bias -> LayerNorm(C) -> GELU."""
    w = p["w"].double()[:, None]
    y = F.conv1d(wav_b.double()[None, None], w, None if mode == 0 else p["bias"].double(), stride=5)
    if mode == 0:
        y = F.gelu(F.group_norm(y, C0, p["gn"][0].double(), p["gn"][1].double(), 1e-5))
    elif mode == 2:
        y = F.gelu(F.layer_norm(y.transpose(1, 2), (C0,), p["ln"][0].double(), p["ln"][1].double(), 1e-5)).transpose(1, 2)
    return y[0].t().contiguous()


def stack_params(ln_mode):
    g = _g(13 + int(ln_mode))
    w = [(torch.randn(C0, C0, k, generator=g) * math.sqrt(2.0 / (k * C0))).to(BF) for k in CONV_K]          # [out, in, k], kaiming scale, real widths
    b = [0.05 * torch.randn(C0, generator=g) if ln_mode else None for _ in CONV_K]
    ln = [(1 + 0.2 * torch.randn(C0, generator=g), 0.1 * torch.randn(C0, generator=g)) for _ in CONV_K] if ln_mode else None
    return dict(w=w, b=b, ln=ln)


def stack_chain(x0, sp, ln_mode, dtype=F64, store=r16):
    """One utterance's OWN level-0 rows [n0, C] -> list of its level 1..6 outputs [n_l, C] (n_l = (n_{l-1} - k) // 2 + 1: every frame that the own rows determine),
    arithmetic in `dtype`, `store` applied to each layer's output (the bf16 store)."""
    x = x0.to(dtype)
    out = []
    for i, k in enumerate(CONV_K):
        y = F.conv1d(x.t()[None], sp["w"][i].to(dtype), None if sp["b"][i] is None else sp["b"][i].to(dtype), stride=2)[0].t()
        if ln_mode:
            y = F.layer_norm(y, (C0,), sp["ln"][i][0].to(dtype), sp["ln"][i][1].to(dtype), 1e-5)
        x = store(F.gelu(y)).to(dtype)
        out.append(x.to(F64))
    return out


# ---- positional conv
PC_ROWS = [129, 2, 300, 1, 63, 64, 65, 127]          # a 2-row utterance between 129 and 300, the longest not first; 300 > 256 spans two 256-frame chunks
PC_VALID = [128, 1, 297, 0, 62, 63, 60, 126]         # valid_b < rows_b everywhere (halo row; utterances 2 and 6: need_b > valid_b as well)
PC_SHAPES = [(128, 4, 16), (768, 16, 128), (1024, 16, 128)]


def pc_offsets():
    off = [0]
    for r in PC_ROWS:
        off.append(off[-1] + r)
    return off


def posconv_inputs(D, G, Kw):
    """x bf16 [total, D]: N(0, 1) on the valid rows, LARGE values on every row >= valid_b (halo rows hold whatever the conv stack left there: a kernel that
    fails to mask them shows at once); weights scaled as test_posconv."""
    g = _g(D + Kw)
    cg = D // G
    off = pc_offsets()
    x = torch.randn(off[-1], D, generator=g)
    for b, (r, v) in enumerate(zip(PC_ROWS, PC_VALID)):
        x[off[b] + v: off[b] + r] = 300.0 * torch.randn(r - v, D, generator=g)
    w = (torch.randn(D, cg, Kw, generator=g) * math.sqrt(4.0 / (Kw * D)) * 3).to(BF)
    bias = torch.randn(D, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    return x.to(BF), w, bias, gamma, beta


def posconv_ref(xb, valid, w, bias, gamma, beta, G, Kw, conv_store=None, prev_row=None, next_row=None):
    """One utterance's own rows xb bf16 [rows, D] -> fp64 [rows, D]: rows >= valid masked to zero, grouped conv with padding Kw/2 and the SamePad trim, + bias, GELU,
    residual add, optional LayerNorm (gamma None).  conv_store: rounding applied to the conv output before the bias (the kernel stores it as bf16).
    prev_row / next_row: MUTANTS only -- a neighbour's row made visible at t = -1 / t = rows."""
    rows, D = xb.shape
    xm = xb.double().clone()
    xm[valid:] = 0
    xin = xm
    lead = 0
    if prev_row is not None:
        xin, lead = torch.cat([prev_row.double()[None], xin]), 1
    if next_row is not None:
        xin = torch.cat([xin, next_row.double()[None]])
    conv = F.conv1d(xin.t()[None], w.double(), None, padding=Kw // 2, groups=G)[0, :, lead: lead + rows].t()
    if conv_store is not None:
        conv = conv_store(conv)
    s = xm + F.gelu(conv + bias.double())
    if gamma is not None:
        s = F.layer_norm(s, (D,), gamma.double(), beta.double(), 1e-5)
    return s


# ---- whole front end
LENS_D = [41000, 6500, 23000, 16000, 9000]


def front_config(which):
    from speechclip_amd.module.hubert import HubertConfig
    return dataclasses.replace(HubertConfig.from_name("hubert" if which == "base" else "hubert_large_ll60k"), encoder_layers=1)


def front_models(which):
    """(HubertModel, HubertModelRef) with the same random weights, non-trivial norm affines and biases."""
    from oracle.hubert_ref import HubertModelRef, HubertRefConfig, randomize_norm_affine
    from speechclip_amd.module.hubert import HubertModel
    cfg = front_config(which)
    torch.manual_seed(5)
    ref = HubertModelRef(HubertRefConfig(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(HubertRefConfig)})).eval()
    randomize_norm_affine(ref, _g(6))
    model = HubertModel(cfg).eval()
    model.load_state_dict(ref.state_dict())
    return model, ref


def waves_d():
    g = _g(2)
    wav = torch.zeros(len(LENS_D), max(LENS_D))
    for b, l in enumerate(LENS_D):
        wav[b, :l] = 0.2 * torch.randn(l, generator=g)
    return wav


def front_oracle(ref, wav):
    from oracle.hubert_ref import hubert_forward, preprocess_input
    padded, mask = preprocess_input([wav[b, :l] for b, l in enumerate(LENS_D)], ref.cfg.normalize)
    return hubert_forward(ref, padded, mask)["layer_results"][0]          # [B, T, d] fp32: the positional-conv output (+ LayerNorm for post-LN models)


def front_chain(model, wav_b, length, valid, store=r16):
    """MODEL of a correct packed front end for ONE utterance (own zero-padded wave [lmax]) in fp64: the 16-bit operands are rounded to bf16 (conv 1-6, projection and
    positional-conv weights) and `store` is applied wherever the engine stores a bf16 tensor.  store = identity and no weight rounding restates the oracle."""
    cfg = model.cfg
    ident = store is None
    st = (lambda t: t) if ident else store
    w16 = (lambda t: t.detach().double()) if ident else (lambda t: r16(t.detach()))
    d64 = lambda t: None if t is None else t.detach().double()
    ln_mode = cfg.extractor_mode == "layer_norm"
    convs = model.feature_extractor.conv_layers
    x = wav_b.double().clone()
    if cfg.normalize:
        x[:length] = F.layer_norm(x[:length], (length,))
    y = None
    for i, blk in enumerate(convs):
        c = getattr(blk, "0")
        src = x[None, None] if i == 0 else y
        y = F.conv1d(src, d64(c.weight) if i == 0 else w16(c.weight), d64(getattr(c, "bias", None)), stride=cfg.conv_layers[i][2])
        if ln_mode:
            ln = getattr(getattr(blk, "2"), "1")
            y = F.layer_norm(y.transpose(1, 2), (y.shape[1],), d64(ln.weight), d64(ln.bias), 1e-5).transpose(1, 2)
        elif i == 0:
            gn = getattr(blk, "2")
            y = F.group_norm(y, y.shape[1], d64(gn.weight), d64(gn.bias), 1e-5)
        y = st(F.gelu(y))
    f = y[0].t()                                                          # [T, 512]
    f = st(F.layer_norm(f, (f.shape[1],), d64(model.layer_norm.weight), d64(model.layer_norm.bias), 1e-5))
    xp = st(f @ w16(model.post_extract_proj.weight).t() + d64(model.post_extract_proj.bias))
    pc = getattr(model.encoder.pos_conv, "0")
    v = pc.weight_v.detach().float()
    wfold = pc.weight_g.detach().float() * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    wfold = wfold.double() if ident else r16(wfold)
    xm = xp.clone()
    xm[valid:] = 0
    conv = st(F.conv1d(xm.t()[None], wfold, None, padding=cfg.conv_pos // 2, groups=cfg.conv_pos_groups)[0, :, : xm.shape[0]].t())
    s = xm + F.gelu(conv + d64(pc.bias))
    if cfg.layer_norm_first:
        return s                                                          # fp32 residual stream, no LayerNorm here
    return st(F.layer_norm(s, (s.shape[1],), d64(model.encoder.layer_norm.weight), d64(model.encoder.layer_norm.bias), 1e-5))


# ================================================================================================ (a) conv layer 0, packed
def _conv0_packed(wav, geo, mode, p):
    """-> device bf16 [64 * total + 8, C] (the +8 slack rows of the engine's buffer, zero)."""
    from speechclip_amd import ops
    dev = "cuda"
    off = torch.tensor(geo["row_off"], dtype=torch.int32, device=dev)
    x = torch.zeros(geo["scale0"] * geo["total"] + 8, C0, device=dev, dtype=BF)
    kw = dict(out=x)
    if mode == 0:
        kw.update(gn_gamma=p["gn"][0].to(dev), gn_beta=p["gn"][1].to(dev))
    else:
        kw.update(bias=p["bias"].to(dev))
        if mode == 2:
            kw.update(ln_coef=torch.cat([p["ln"][0], p["ln"][1], torch.tensor([1e-5])]).to(dev))
    ops.conv0_packed(wav.to(dev), p["w"].to(dev), geo["T0"], off, geo["scale0"], geo["rows_max"], geo["total"], **kw)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv0_packed_every_row_vs_fp64(mode):
    """sc_conv0_fwd_packed, all 64 r_b rows of every utterance (a superset of the 64 valid_b + 15 rows a valid frame can read: conv layer 0 reads only the
    utterance's own wave, so no row of this level is inexact and none is excluded): rows t < T0 against fp64, rows t >= T0 exactly zero; and packed == padded
    sc_conv0_fwd on the same rows."""
    from speechclip_amd import ops
    geo, p, wav = geometry_a(), conv0_params(), waves_a()
    T0, sc = geo["T0"], geo["scale0"]
    assert sc == 64 and geo["rows"][1] == 2 and geo["rows"][3] == 5 and max(geo["rows"]) == geo["rows"][2]
    got = _conv0_packed(wav, geo, mode, p)
    assert got[sc * geo["total"]:].abs().max().item() == 0                      # nothing written past the slab
    got = got.cpu()
    P0 = (T0 + 63) // 64 * 64
    dev = "cuda"
    if mode == 0:
        pad = ops.conv0(wav.to(dev), p["w"].to(dev), T0, P0, p["gn"][0].to(dev), p["gn"][1].to(dev))
    else:
        pad = ops.conv0(wav.to(dev), p["w"].to(dev), T0, P0, bias=p["bias"].to(dev),
                        ln_coef=torch.cat([p["ln"][0], p["ln"][1], torch.tensor([1e-5])]).to(dev) if mode == 2 else None)
    pad = pad[: len(LENS_A) * P0].view(len(LENS_A), P0, C0).cpu()
    bound = bound_of(MODEL_CONV0[mode])
    worst, worst_pad, n_rows, bitwise = 0.0, 0.0, 0, True
    for b, r in enumerate(geo["rows"]):
        n = sc * r
        mine = got[sc * geo["row_off"][b]: sc * geo["row_off"][b] + n]
        live = min(n, T0)
        ref = conv0_ref(wav[b], p, mode)[:live]
        worst = max(worst, check_rows(mine[:live], ref, bound, 2e-2, f"conv0 packed mode {mode} utterance {b}"))
        assert mine[live:].abs().max().item() == 0 if live < n else True         # frames >= T0 are written as zeros
        m = min(n, P0)
        worst_pad = max(worst_pad, check_rows(mine[:m], pad[b, :m].double(), bound, 2e-2, f"conv0 packed vs padded mode {mode} utterance {b}"))
        bitwise = bitwise and torch.equal(mine[:m], pad[b, :m])
        n_rows += n
    print(f"conv0 packed mode {mode}: {n_rows} rows, 0 excluded; worst row metric vs fp64 {worst:.3e} (model {MODEL_CONV0[mode]:.2e}, bound {bound:.2e}); "
          f"vs padded kernel {worst_pad:.3e} (bitwise equal: {bitwise})")


# ================================================================================================ (b) conv layers 1-6 over the packed slab
def _run_stack(wav, geo, ln_mode, p, sp):
    """conv layer 0 (packed) + the six stride-2 layers exactly as HubertModel.extract_all_layers(pack=...) issues them -> list of 7 host tensors (levels 0..6)."""
    from speechclip_amd import ops
    from speechclip_amd.ops import ACT_GELU, ACT_NONE
    dev = "cuda"
    x = _conv0_packed(wav, geo, 2 if ln_mode else 0, p)
    rows_all = geo["scale0"] * geo["total"]
    levels = [x[:rows_all].cpu()]
    for i, k in enumerate(CONV_K):
        rows_all //= 2
        y = torch.zeros(rows_all + 8, C0, device=dev, dtype=BF)
        w = sp["w"][i].permute(0, 2, 1).reshape(C0, k * C0).contiguous().to(dev)          # [out, k*in], K index = tap*C + c_in
        ops.gemm(x, w, None if sp["b"][i] is None else sp["b"][i].to(dev), ACT_NONE if ln_mode else ACT_GELU, out=y[:rows_all], M=rows_all, K=k * C0, lda=2 * C0)
        if ln_mode:
            ops.layernorm(y[:rows_all], sp["ln"][i][0].to(dev), sp["ln"][i][1].to(dev), gelu=True, out=y[:rows_all])
        levels.append(y[:rows_all].cpu())
        x = y
    assert rows_all == geo["total"]
    return levels


def own_rows(levels, geo, b):
    """utterance b's slab at every level: 2^(6-l) r_b rows at 2^(6-l) row_off[b]."""
    return [lv[(64 >> l) * geo["row_off"][b]: (64 >> l) * geo["row_off"][b + 1]] for l, lv in enumerate(levels)]


@pytest.mark.gpu
@pytest.mark.parametrize("ln_mode", [False, True])
def test_packed_conv_stack_every_own_frame_vs_fp64(ln_mode):
    """Layers 1-6 as ONE overlapping-row GEMM per layer over the packed slab (row offsets double per level).  Reference: each utterance's own level-0 rows through an
    fp64 F.conv1d chain with a bf16 store after every layer.  At every level, EVERY frame that the utterance's own rows determine is compared (n_l = (n_{l-1} - k) // 2 + 1
    from n_0 = 64 r_b: all but the last row of the slab; at the top that is frames t < r_b - 1 >= valid_b, the last one reading into the halo row's block).  The slab's
    last row per level reads the next utterance and is the only one excluded."""
    geo, p, sp, wav = geometry_a(), conv0_params(), stack_params(ln_mode), waves_a()
    levels = _run_stack(wav, geo, ln_mode, p, sp)
    bound = bound_of(MODEL_STACK[ln_mode])
    B = len(LENS_A)
    worst = [0.0] * 7
    excluded = [0] * 7
    for b, r in enumerate(geo["rows"]):
        mine = own_rows(levels, geo, b)
        ref = stack_chain(mine[0], sp, ln_mode)
        for l in range(1, 7):
            n = ref[l - 1].shape[0]
            excluded[l] += mine[l].shape[0] - n
            worst[l] = max(worst[l], check_rows(mine[l][:n], ref[l - 1], bound, None, f"conv stack (layer_norm={ln_mode}) level {l} utterance {b}"))
        assert ref[5].shape[0] == r - 1 >= geo["valid"][b]                      # the top level: every frame below the halo row, the last valid one included
    for l in range(1, 7):
        assert excluded[l] <= (64 >> l) * (B + sum(r - v for r, v in zip(geo["rows"], geo["valid"]))) and excluded[l] == B
    print(f"packed conv stack (layer_norm={ln_mode}): excluded rows per level {excluded[1:]} (the slab's last row of each of {B} utterances); "
          f"worst row metric per level {['%.3e' % w for w in worst[1:]]} (model {MODEL_STACK[ln_mode]:.2e}, bound {bound:.2e})")


@pytest.mark.gpu
@pytest.mark.parametrize("ln_mode", [False, True])
@pytest.mark.parametrize("keep", [1, 3, 5])
def test_packed_conv_stack_neighbours_do_not_reach_own_frames(ln_mode, keep):
    """Contamination control: the neighbours' waves replaced by +-50 garbage vs by silence -- every own frame of utterance `keep` (1: the 2-row utterance between the
    two longest), at every level, is BITWISE unchanged: the rows a valid frame reads are the utterance's own."""
    geo, p, sp = geometry_a(), conv0_params(), stack_params(ln_mode)
    quiet = own_rows(_run_stack(waves_a("zero", keep), geo, ln_mode, p, sp), geo, keep)
    loud_all = _run_stack(waves_a("big", keep), geo, ln_mode, p, sp)
    loud = own_rows(loud_all, geo, keep)
    n = 64 * geo["rows"][keep]
    assert torch.equal(quiet[0], loud[0])
    for l, k in enumerate(CONV_K, start=1):
        n = (n - k) // 2 + 1
        assert n == quiet[l].shape[0] - 1
        assert torch.equal(quiet[l][:n], loud[l][:n]), (l, keep)
        assert torch.isfinite(loud_all[l].float()).all()
    # the control is live: the excluded last row of the top level does see the neighbour (unless `keep` is the last utterance)
    assert not torch.equal(quiet[6][n:], loud[6][n:])


# ================================================================================================ (c) packed positional conv
def _posconv_packed(x, w, bias, gamma, beta, D, G, Kw, out_f32):
    from speechclip_amd import ops
    dev = "cuda"
    cg = D // G
    off = pc_offsets()
    wg = w.float().view(G, cg, cg, Kw).permute(0, 1, 3, 2).reshape(G, cg, Kw * cg).contiguous().to(dev, BF)
    return ops.posconv_packed(x.to(dev), torch.tensor(PC_VALID, dtype=torch.int32, device=dev), torch.tensor(off, dtype=torch.int32, device=dev), wg, bias.to(dev),
                              None if gamma is None else gamma.to(dev), None if beta is None else beta.to(dev), len(PC_ROWS), max(PC_ROWS), off[-1], D, G, Kw,
                              out_f32=out_f32).cpu(), wg


@pytest.mark.gpu
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("D,G,Kw", PC_SHAPES)
def test_posconv_packed_every_row_vs_fp64(D, G, Kw, ln, out_f32):
    """sc_posconv_conv_packed + sc_posconv_finish_packed for D/G = 32 / 48 / 64, with and without the LayerNorm, bf16 and fp32 output.
    Contract of rows >= valid_b (include/speechclip_hip.h: out = [LayerNorm](mask(x) + gelu(conv + bias)) for EVERY row, the conv reading frames >= valid_b as zero):
    they hold [LayerNorm](gelu(conv + bias)) of the masked utterance -- neither zeros nor the input.  So all rows_b rows of every utterance are compared, halo row
    included, and no row is excluded.  The input carries values ~300 on the rows >= valid_b and the neighbours sit back to back: an unmasked halo row or a window
    reaching into a neighbour cannot stay inside the bound."""
    from speechclip_amd import ops
    x, w, bias, gamma, beta = posconv_inputs(D, G, Kw)
    if not ln:
        gamma = beta = None
    got, wg = _posconv_packed(x, w, bias, gamma, beta, D, G, Kw, out_f32)
    assert got.dtype == (torch.float32 if out_f32 else BF)
    off = pc_offsets()
    B, Tp = len(PC_ROWS), max(PC_ROWS)
    xpad = torch.zeros(B, Tp, D, dtype=BF)
    for b, r in enumerate(PC_ROWS):
        xpad[b, :r] = x[off[b]: off[b + 1]]
    dev = "cuda"
    pad = ops.posconv(xpad.view(B * Tp, D).to(dev), torch.tensor(PC_VALID, dtype=torch.int32, device=dev), wg, bias.to(dev), None if gamma is None else gamma.to(dev),
                      None if beta is None else beta.to(dev), B, Tp, D, G, Kw, out_f32=out_f32).cpu().view(B, Tp, D)
    bound = bound_of(MODEL_POSCONV[(D, ln, out_f32)])
    worst, worst_pad, bitwise = 0.0, 0.0, True
    for b, (r, v) in enumerate(zip(PC_ROWS, PC_VALID)):
        mine = got[off[b]: off[b + 1]]
        ref = posconv_ref(x[off[b]: off[b + 1]], v, w, bias, gamma, beta, G, Kw)
        worst = max(worst, check_rows(mine, ref, bound, 3e-2, f"posconv packed D={D} ln={ln} f32={out_f32} utterance {b} (rows {r}, valid {v})"))
        worst_pad = max(worst_pad, check_rows(mine, pad[b, :r].double(), bound, 3e-2, f"posconv packed vs padded D={D} utterance {b}"))
        bitwise = bitwise and torch.equal(mine, pad[b, :r])
    print(f"posconv packed D={D} G={G} Kw={Kw} ln={ln} out_f32={out_f32}: {off[-1]} rows, 0 excluded; worst row metric vs fp64 {worst:.3e} "
          f"(model {MODEL_POSCONV[(D, ln, out_f32)]:.2e}, bound {bound:.2e}); vs padded kernel {worst_pad:.3e} (bitwise equal: {bitwise})")


@pytest.mark.gpu
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("D,G,Kw", PC_SHAPES)
def test_posconv_packed_neighbours_do_not_reach_own_rows(D, G, Kw, ln):
    """Contamination control: every OTHER utterance's rows scaled by 1e3 -- all rows of the utterance left alone are bitwise unchanged, for each utterance in turn
    (the window of a packed block reaches Kw/2 rows to either side, far into both neighbours of the short utterances)."""
    x, w, bias, gamma, beta = posconv_inputs(D, G, Kw)
    if not ln:
        gamma = beta = None
    base, _ = _posconv_packed(x, w, bias, gamma, beta, D, G, Kw, False)
    off = pc_offsets()
    for keep in range(len(PC_ROWS)):
        x2 = (x.float() * 1e3).to(BF)
        x2[off[keep]: off[keep + 1]] = x[off[keep]: off[keep + 1]]
        got, _ = _posconv_packed(x2, w, bias, gamma, beta, D, G, Kw, False)
        assert torch.equal(got[off[keep]: off[keep + 1]], base[off[keep]: off[keep + 1]]), (D, keep)
        others = torch.cat([got[: off[keep]], got[off[keep + 1]:]]), torch.cat([base[: off[keep]], base[off[keep + 1]:]])
        assert not torch.equal(*others)                                             # the control is live


# ================================================================================================ (d) the whole packed front end at real dimensions, per frame
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["base", "large"])
def test_packed_front_end_real_dims_per_frame_vs_oracle(which):
    """HuBERT-base (D/G = 48, GroupNorm extractor, post-LN) and HuBERT-large (D/G = 64, LayerNorm extractor, wave normalisation, pre-LN fp32 output) layouts with ONE
    encoder layer, ragged batch, `extract_all_layers(pack=geo, stop_layer=0)`: hidden[0] (the positional-conv output) against the fp32 oracle FRAME BY FRAME.  The first
    two frames (the window reaches 64 rows back into the previous utterance unless masked), the last two valid frames (they read the halo row's block and sit next to the
    neighbour's first rows) and the interior are reported separately and must all meet the SAME bound."""
    model, ref = front_models(which)
    wav = waves_d()
    want = front_oracle(ref, wav)
    model = model.cuda()
    geo = model.packed_geometry(LENS_D, max(LENS_D))
    hidden, T, _, valid = model.extract_all_layers(wav.cuda(), LENS_D, stop_layer=0, pack=geo)
    assert hidden.shape[0] == 1 and hidden.shape[1] == geo["total"] and T == want.shape[1] and list(valid) == geo["valid"]
    got = hidden[0].float().cpu()
    bound = bound_of(MODEL_FRONT[which])
    groups = {"first 2": [], "last 2 valid": [], "interior": []}
    excluded = 0
    for b, (r, v) in enumerate(zip(geo["rows"], geo["valid"])):
        mine = got[geo["row_off"][b]: geo["row_off"][b] + v]
        excluded += r - v
        check_rows(mine, want[b, :v].double(), bound, None, f"packed front end ({which}) utterance {b}")
        m = row_metric(mine, want[b, :v])
        assert v >= 5
        groups["first 2"].append(m[:2].max().item())
        groups["last 2 valid"].append(m[v - 2:].max().item())
        groups["interior"].append(m[2: v - 2].max().item())
    assert excluded <= len(LENS_D) + sum(r - v for r, v in zip(geo["rows"], geo["valid"])) and excluded == len(LENS_D)
    for k, vals in groups.items():
        assert max(vals) <= bound, (which, k, vals, bound)
    print(f"packed front end ({which}): {geo['total'] - excluded} frames compared, {excluded} excluded (the halo row of each utterance); worst row metric per utterance: "
          + "; ".join(f"{k} {['%.3e' % x for x in vals]}" for k, vals in groups.items()) + f" (model {MODEL_FRONT[which]:.2e}, bound {bound:.2e})")

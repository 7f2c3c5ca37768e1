"""Inference nodes, per-row parity: WHAT the eval-mode host drivers compute -- which LayerNorm gets which affine, which buffer a residual is read from, which slot a
layer writes, what the padded view of a packed batch holds behind an utterance's frames.

  a. the encoder, post-LN     HubertModel.extract_all_layers on bf16 rows: three layers at d = 128, two at d = 768
  b. the encoder, pre-LN      the same function on the fp32 stream with IEEE-half and with bf16 operands, d = 128 and d = 1024, wave LayerNorm on
  c. slot wiring              drop_layers=(1,) and stop_layer=1 on three layers, both bodies
  d. the wrapper in eval      FairseqSpeechEncoder_Hubert.forward: the layer mix (plain, normalize_features), the state selections, method1 / method2
  f. the branch               TransformerEncoder.forward_cls and the full-row forward: head dims 64 / 96 / 128, 1 / 2 / 3 layers, post-LN and pre-LN
  e. the towers               CLIP.encode_image: the bits of encode_image_train's forward, and the fp64 forward of the training node; the text tower packed
                              (encode_text_ids, default and general=True) and padded (_encode_text_embeddings_eval): every caption's feature row and every row of
                              the residual stream entering ln_final
  g. half range               one fc1 channel whose stored GELU output reaches 2^15 .. 6e4 in the half format

The machinery is that of tests/test_train_nodes_parity_gpu.py: fp64 references on the CPU (tests/infer_nodes_ref.py, one utterance at a time, from the product's own
weights), per row max|got - ref| / max|ref| for hidden states, the same over the whole tensor for mix outputs and feature matrices, bound 4 x MODEL + 1e-3 with MODEL
the metric of the CPU model of a correct implementation (model="bf16" / "f16") on exactly these inputs.  `python tools/infer_node_bounds.py` prints every value,
checks well-posedness and every mutant (a wrong wiring of the reference must leave the bound); `--emit` prints the MODEL dict below.  No literal tolerance appears in
this file.  The rounding model alone is what the bounds are made of: the packed-half GELU polynomial of fc1's epilogue is NOT in the CPU model (no case needed it).
SC_INFER_PARITY_OUT=<file> appends the worst / bound lines (profiles/infer_nodes_parity.txt is such a file).

Left out of the row metrics, and nothing else: rows at or beyond an utterance's valid frames (fairseq's padding-mask rule, HubertModel.valid_frames).  Where the
driver defines them -- the padded view of a packed batch behind max(valid, feat_len) frames, the halo row included -- they must be exact zeros.  Every test asserts
how many rows and tensors it judged.  The 400-sample wave owns one frame by the round(len / 320) rule (feat_len = 1) and two by the padding-mask rule.

Which case reaches which branch:
    extract_all_layers   enc-post-*        `elif not pre_ln` (residual in the GEMM epilogue, a separate LayerNorm); d = 768 reaches the 768-wide LayerNorm kernel;
                                           the GroupNorm extractor (conv0 with gn_gamma), posconv with the encoder LayerNorm
                         enc-pre-*         the last branch (fp32 stream, xmid, lw = half or bf16); the "layer_norm" extractor with conv biases, conv 0 fused
                                           (ln_coef) and, in *-conv0sep, as conv + bias and a separate LayerNorm + GELU pass; cfg.normalize (ops.wave_layernorm);
                                           posconv without the encoder LayerNorm, fp32 out
                         */padded, */packed  conv0 / posconv / attention on uniform rows, conv0_packed / posconv_packed / attention with row offsets
                         slot-*            `continue` on a dropped layer with `kept` one behind i, the hidden[: kept + 1] returns; `break` at stop_layer
    the wrapper          wrap-plain/-norm  packed: ops.weighted_sum on packed rows, then ops.unpack_rows(halo=1); padded: weightedsum_layer on the [n, B, Tp, d] buffer
                         wrap-select       "all", a list, "last_hidden_state": the clone of the padded workspace, the unpacked copy of the packed one
                         wrap-method1/2    ops.hidden_normalize_ (these force the padded layout)
    run_tower            tower-*           uniform rows without a mask (the image tower); ln_post on the class rows through ld_in = ntok * W
    the branch           branch-*-n1-post  forward_cls: the algebraic CLS-rows head (sc_cls_pool_fwd, hi | lo split GEMMs); branch-* else: _forward_cls_stack (layers
                                           0 .. n-2 through _layer_rows on attention_hd_qkv, the last layer on the CLS rows); every case: the full-row forward
                                           (_layer_rows on attention_rows with the boolean mask, the final norm on every row)
                         text-*            packed rows (ops.attention_text, default and general=True) through encode_text_ids, uniform causal rows through
                                           _encode_text_embeddings_eval; the gather of the EOT rows, ln_final, the projection"""
import copy
import dataclasses
import functools
import os

import pytest
import torch

import infer_nodes_ref as I
import train_mode_ref as R
from test_train_mode_parity_gpu import _tiny_hubert, _waves

BF = torch.bfloat16
F64 = torch.float64

# ---- modelled error of a correct implementation per case and tensor: `python tools/infer_node_bounds.py --emit`
MODEL = {
    "enc-post-tiny3/h0": 1.87e-02, "enc-post-tiny3/h1": 1.54e-02, "enc-post-tiny3/h2": 1.46e-02, "enc-post-tiny3/h3": 1.19e-02,
    "enc-post-768/h0": 1.11e-02, "enc-post-768/h1": 1.36e-02, "enc-post-768/h2": 1.24e-02,
    "enc-pre-tiny-f16/h0": 2.06e-02, "enc-pre-tiny-f16/h1": 1.65e-02, "enc-pre-tiny-f16/h2": 2.23e-02, "enc-pre-tiny-f16/own1": 6.80e-04,
    "enc-pre-tiny-f16/own2": 7.92e-04,
    "enc-pre-tiny-bf16/h0": 2.06e-02, "enc-pre-tiny-bf16/h1": 1.64e-02, "enc-pre-tiny-bf16/h2": 1.99e-02, "enc-pre-tiny-bf16/own1": 6.12e-03,
    "enc-pre-tiny-bf16/own2": 5.17e-03,
    "enc-pre-tiny-f16-conv0sep/h0": 2.25e-02, "enc-pre-tiny-f16-conv0sep/h1": 1.47e-02, "enc-pre-tiny-f16-conv0sep/h2": 1.46e-02,
    "enc-pre-tiny-f16-conv0sep/own1": 6.64e-04, "enc-pre-tiny-f16-conv0sep/own2": 7.24e-04,
    "enc-pre-1024-f16/h0": 1.61e-02, "enc-pre-1024-f16/h1": 8.11e-03, "enc-pre-1024-f16/h2": 7.14e-03, "enc-pre-1024-f16/own1": 7.04e-04,
    "enc-pre-1024-f16/own2": 6.77e-04,
    "enc-pre-1024-bf16/h0": 1.61e-02, "enc-pre-1024-bf16/h1": 1.00e-02, "enc-pre-1024-bf16/h2": 1.04e-02, "enc-pre-1024-bf16/own1": 5.66e-03,
    "enc-pre-1024-bf16/own2": 6.90e-03,
    "slot-post-drop1/h0": 1.87e-02, "slot-post-drop1/h1": 1.54e-02, "slot-post-drop1/h2": 1.44e-02,
    "slot-post-stop1/h0": 1.87e-02, "slot-post-stop1/h1": 1.54e-02,
    "slot-pre-drop1/h0": 2.08e-02, "slot-pre-drop1/h1": 8.30e-03, "slot-pre-drop1/h2": 1.04e-02, "slot-pre-drop1/own1": 6.61e-04, "slot-pre-drop1/own2": 1.01e-03,
    "slot-pre-stop1/h0": 2.08e-02, "slot-pre-stop1/h1": 8.30e-03, "slot-pre-stop1/own1": 6.61e-04,
    "half-f16/h0": 1.57e-02, "half-f16/h1": 1.42e-02, "half-f16/h2": 1.27e-02, "half-f16/own1": 8.40e-04, "half-f16/own2": 8.77e-04,
    "half-bf16/h0": 1.57e-02, "half-bf16/h1": 1.55e-02, "half-bf16/h2": 1.69e-02, "half-bf16/own1": 5.96e-03, "half-bf16/own2": 1.02e-02,
    "wrap-plain/mixed": 9.05e-03,
    "wrap-norm/mixed": 1.00e-02,
    "wrap-method1/h0": 1.88e-02, "wrap-method1/h1": 1.47e-02, "wrap-method1/h2": 1.53e-02, "wrap-method1/h3": 1.27e-02,
    "wrap-method2/h0": 1.88e-02, "wrap-method2/h1": 1.48e-02, "wrap-method2/h2": 1.52e-02, "wrap-method2/h3": 1.20e-02,
    "tower-T17/feat": 3.72e-03,
    "tower-T65/feat": 3.28e-03,
    "branch-hd64-n1-post/cls": 2.26e-04, "branch-hd64-n1-post/full": 2.03e-03,
    "branch-hd96-n2-pre/cls": 1.87e-03, "branch-hd96-n2-pre/full": 3.75e-03,
    "branch-hd128-n2-post/cls": 2.40e-03, "branch-hd128-n2-post/full": 2.85e-03,
    "branch-hd64-n3-post/cls": 3.31e-03, "branch-hd64-n3-post/full": 4.21e-03,
    "branch-hd64-n1-pre/cls": 1.98e-03, "branch-hd64-n1-pre/full": 2.38e-03,
    "text-w64-h1-l2/feat": 6.35e-03, "text-w64-h1-l2/stream": 9.08e-03,
    "text-w128-h2-l3/feat": 5.48e-03, "text-w128-h2-l3/stream": 7.53e-03,
}


def _note(line):
    print(line)
    path = os.environ.get("SC_INFER_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Judge:
    """Counts what it judged; prints (and notes) key / worst / model / bound per tensor."""

    def __init__(self, tag):
        self.rows = self.tensors = 0
        self.tag = tag

    def check(self, key, kind, got, ref, report_only=False):
        assert got.shape == ref.shape and got.numel() > 0, (key, got.shape, ref.shape)
        assert torch.isfinite(got.double()).all(), key
        bound = R.bound_of(MODEL[key])
        if kind == "rows":
            m = R.row_metric(got.double().cpu(), ref)
            worst = m.max().item()
            self.rows += m.numel()
        else:
            worst = R.tensor_metric(got.double().cpu(), ref)
            self.tensors += 1
        _note(f"{self.tag:34s} {key:28s} {kind:6s} worst {worst:.3e}  model {MODEL[key]:.2e}  bound {bound:.3e}  worst/bound {worst / bound:6.3f}"
              + ("  (reported, not asserted)" if report_only else ""))
        if not report_only:
            assert worst <= bound, (self.tag, key, kind, "metric", worst, "bound", bound)
        return worst

    def all(self, cid, got, ref, report_only=False):
        """got / ref: name -> (kind, tensor)"""
        assert list(got) == list(ref), sorted(set(got) ^ set(ref))
        return max(self.check(f"{cid}/{name}", kind, got[name][1], r, report_only) for name, (kind, r) in ref.items())


# ================================================================================================ a - c, g. the encoder
ENC_LENS = (8000, 6000, 3000, 400)          # T = 24 frames; valid 24 / 19 / 10 / 2, feat_len 24 / 19 / 9 / 1
LAYOUTS = ("padded", "packed")
_PRE = (("layer_norm_first", True), ("extractor_mode", "layer_norm"), ("conv_bias", True), ("normalize", True))
_D768 = (("encoder_embed_dim", 768), ("encoder_attention_heads", 12), ("encoder_ffn_embed_dim", 1536), ("conv_pos_groups", 16))
_D1024 = (("encoder_embed_dim", 1024), ("encoder_attention_heads", 16), ("encoder_ffn_embed_dim", 2048), ("conv_pos_groups", 16))
_L3 = (("encoder_layers", 3),)
HALF_CHANNEL = 5              # the fc1 output channel of layer 0 the half-range case scales


@dataclasses.dataclass(frozen=True)
class EncCase:
    id: str
    over: tuple               # config overrides (name, value)
    fmt: str = "bf16"         # operand format of the layers (pre-LN: _PRELN_F16)
    conv0_fused: bool = True  # _CONV0_LN_FUSED
    drop: tuple = ()
    stop: int = None
    boost: float = None       # half range: the scale of fc1 channel HALF_CHANNEL of layer 0 (fc2's column scaled down by it)
    model_of: str = None      # the case whose setup (weights, waves) this one shares

    @property
    def pre_ln(self):
        return dict(self.over).get("layer_norm_first", False)


HALF_BOOST = 2.0 ** 16        # calibrated by tools/infer_node_bounds.py (half_range_report): the largest half-stored value must land in [2^15, 6e4]
ENC_CASES = (
    EncCase("enc-post-tiny3", _L3), EncCase("enc-post-768", _D768),
    EncCase("enc-pre-tiny-f16", _PRE, "f16"), EncCase("enc-pre-tiny-bf16", _PRE, "bf16", model_of="enc-pre-tiny-f16"),
    EncCase("enc-pre-tiny-f16-conv0sep", _PRE, "f16", conv0_fused=False, model_of="enc-pre-tiny-f16"),
    EncCase("enc-pre-1024-f16", _PRE + _D1024, "f16"), EncCase("enc-pre-1024-bf16", _PRE + _D1024, "bf16", model_of="enc-pre-1024-f16"),
    EncCase("slot-post-drop1", _L3, drop=(1,), model_of="enc-post-tiny3"), EncCase("slot-post-stop1", _L3, stop=1, model_of="enc-post-tiny3"),
    EncCase("slot-pre-drop1", _PRE + _L3, "f16", drop=(1,)), EncCase("slot-pre-stop1", _PRE + _L3, "f16", stop=1, model_of="slot-pre-drop1"),
    EncCase("half-f16", _PRE, "f16", boost=HALF_BOOST), EncCase("half-bf16", _PRE, "bf16", boost=HALF_BOOST, model_of="half-f16"),
)
REPORT_ONLY = ("half-bf16",)          # the issue: the bf16 twin of the half-range case reports its worst metric next to it, nothing is asserted on it


def enc_case(cid):
    return next(c for c in ENC_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def enc_setup(cid):
    """(module.hubert.HubertModel on the CPU, wav [4, 8000], packed geometry, valid frames, feat_len)"""
    c = enc_case(cid)
    if c.model_of is not None and enc_case(c.model_of).boost == c.boost:
        return enc_setup(c.model_of)
    seed = 700 + sum(map(ord, cid))
    enc = _tiny_hubert(seed, **dict(c.over)).eval()
    wav = _waves(ENC_LENS, seed + 5)
    if c.pre_ln:          # a DC offset inside every utterance (the wave LayerNorm has a mean to remove) and a silent tail inside utterance 1's length
        for b, l in enumerate(ENC_LENS):
            wav[b, :l] += 0.05
        wav[1, 5000:ENC_LENS[1]] = 0.05
    if c.boost is not None:
        with torch.no_grad():
            lyr = enc.encoder.layers[0]
            lyr.fc1.weight[HALF_CHANNEL] *= c.boost
            lyr.fc1.bias[HALF_CHANNEL] *= c.boost
            lyr.fc2.weight[:, HALF_CHANNEL] /= c.boost
    L = wav.shape[1]
    T = enc.frame_geometry(L)[1]
    need = [min(round(l / 320), T) for l in ENC_LENS]
    return enc, wav, enc.packed_geometry(ENC_LENS, L, need_rows=need), enc.valid_frames(ENC_LENS, L, T), need


def enc_reference(cid, model=False, wiring=(), rows="valid", probe=None, h0=None):
    """-> hidden[b][i] fp64 [valid_b, d].  model: False, True (the case's own format) or a format name (MUTANT: another format than the case claims).
    h0[b]: state 0 given, only the layers run."""
    c = enc_case(cid)
    enc, wav, pack, _, _ = enc_setup(cid)
    return I.encoder_eval(enc, wav, list(ENC_LENS), pack, c.drop, c.stop, c.fmt if model is True else model, rows, c.conv0_fused, wiring, probe, h0)


@functools.lru_cache(maxsize=None)
def enc_reference_cached(cid):
    return enc_reference(cid)


def enc_tensors(res, own=None):
    """hidden[b][i] -> name -> ("rows", the valid rows of every utterance, concatenated).  own: the states the layers give on a GIVEN state 0 (pre-LN cases):
    judged as own1 .. -- the layers alone, where the operand format shows (the front end in front of h1 .. is bf16 in every format)."""
    out = {f"h{i}": ("rows", torch.cat([hs[i] for hs in res])) for i in range(len(res[0]))}
    if own is not None:
        out.update({f"own{i}": ("rows", torch.cat([hs[i] for hs in own])) for i in range(1, len(own[0]))})
    return out


def enc_model_tensors(cid, model=True):
    """The tool's side of the judged tensors: the CPU model against the fp64 reference; for the pre-LN cases the layers alone run on the CPU MODEL's state 0, a
    tensor with the statistics of the driver's own (the GPU test feeds the reference the state 0 the driver produced).  -> (reference, model)"""
    ref, mod = enc_reference_cached(cid), enc_reference(cid, model=True)
    if not enc_case(cid).pre_ln:
        return enc_tensors(ref), enc_tensors(mod)
    h0 = [hs[0] for hs in mod]
    return enc_tensors(ref, enc_reference(cid, h0=h0)), enc_tensors(mod, enc_reference(cid, model=model, h0=h0))


def n_states(c, n_layers):
    return c.stop + 1 if c.stop is not None else n_layers + 1 - len(c.drop)


def _run_encoder(cid, layout, monkeypatch):
    from speechclip_amd.module import hubert as hb
    c = enc_case(cid)
    enc_cpu, wav, pack, valid, _ = enc_setup(cid)
    monkeypatch.setattr(hb, "_PRELN_F16", c.fmt == "f16")
    monkeypatch.setattr(hb, "_CONV0_LN_FUSED", c.conv0_fused)
    enc = copy.deepcopy(enc_cpu).cuda().eval()
    packed = layout == "packed"
    hidden, T, Tp, v = enc.extract_all_layers(wav.cuda(), list(ENC_LENS), stop_layer=c.stop, drop_layers=c.drop, pack=pack if packed else None)
    torch.cuda.synchronize()
    assert list(v) == list(valid)
    assert enc._packed["layer_dtype"] == (torch.float16 if (c.pre_ln and c.fmt == "f16") else BF)
    assert hidden.dtype == (torch.float32 if c.pre_ln else BF)
    n = n_states(c, enc.cfg.encoder_layers)
    assert hidden.shape[0] == n or (c.stop is not None and not packed and hidden.shape[0] == enc.cfg.encoder_layers + 1)
    hidden = hidden[:n].float().cpu()
    off = pack["row_off"]
    return [[(hidden[i, off[b]:off[b] + valid[b]] if packed else hidden[i, b, :valid[b]]) for i in range(n)] for b in range(len(valid))]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", [c.id for c in ENC_CASES if c.id not in REPORT_ONLY])
def test_encoder_eval_hidden_states_against_fp64(cid, layout, monkeypatch):
    c = enc_case(cid)
    _, _, _, valid, _ = enc_setup(cid)
    n = n_states(c, dict(c.over).get("encoder_layers", 2))

    def judge(case, report_only=False):
        got = _run_encoder(case, layout, monkeypatch)
        own = enc_reference(case, h0=[hs[0].double() for hs in got]) if c.pre_ln else None          # the fp64 layers on the driver's own state 0
        J = Judge(f"{case}/{layout}")
        J.all(case, enc_tensors(got, got if c.pre_ln else None), enc_tensors(enc_reference_cached(case), own), report_only)
        assert len(got[0]) == n and (J.rows, J.tensors) == ((n + (n - 1) * bool(c.pre_ln)) * sum(valid), 0)
    judge(cid)
    if cid == "half-f16":          # the same weights and waves on bf16 operands: its own worst metric against its own model, next to the half one
        judge(REPORT_ONLY[0], report_only=True)


# ================================================================================================ d. the wrapper in eval
WRAP_ENC = "enc-post-tiny3"
WRAP_W = (2.0, 0.25, -3.0, 0.5)          # test_train_nodes_parity_gpu.WSUM_W: one dominant weight, one near -3 (softmax 0.4 %)
WRAP_MIX = ("wrap-plain", "wrap-norm")
WRAP_METHODS = ("wrap-method1", "wrap-method2")
WRAP_LIST = [0, 2]


def mix_reference(cid, model=False, wiring=()):
    """-> ("tensor", the mixed valid rows of every utterance, concatenated)"""
    hs = enc_reference(WRAP_ENC, model=True) if model else enc_reference_cached(WRAP_ENC)
    w = torch.tensor(WRAP_W, dtype=F64)
    return dict(mixed=("tensor", torch.cat([I.mix_eval(torch.stack(h), w, cid == "wrap-norm", bool(model), wiring) for h in hs])))


def method_reference(cid, model=False):
    """normalize_type method1 / method2 on the padded layout: every state of every utterance on ALL T frames, normalised, then its valid rows"""
    _, _, _, valid, _ = enc_setup(WRAP_ENC)
    hs = enc_reference(WRAP_ENC, model=True if model else False, rows="all")
    T = hs[0][0].shape[0]
    out = [I.hidden_normalize(torch.stack(h), T, cid.split("-")[1], R.r16 if model else None)[:, :v] for h, v in zip(hs, valid)]
    return {f"h{i}": ("rows", torch.cat([o[i] for o in out])) for i in range(out[0].shape[0])}


def _wrapper(monkeypatch, layout, **kw):
    from speechclip_amd.module import FairseqSpeechEncoder_Hubert
    enc_cpu = enc_setup(WRAP_ENC)[0]
    monkeypatch.setenv("SC_VARLEN_PACK", "1" if layout == "packed" else "0")
    torch.manual_seed(3)
    mod = FairseqSpeechEncoder_Hubert("hubert", max_audio_len=100000, hubert_config=enc_cpu.cfg, **kw)
    mod.encoder.load_state_dict(enc_cpu.state_dict())
    if hasattr(mod, "weightedsum_layer"):
        with torch.no_grad():
            mod.weightedsum_layer.weights.copy_(torch.tensor(WRAP_W))
    return mod.cuda().eval()


def _other_batch():
    return _waves((7000, 2000), 99).cuda(), torch.tensor([7000, 2000])


def _zeros_behind(x, valid, need, what):
    """the padded view of a packed batch: exact zeros behind max(valid, feat_len) frames of every utterance (the halo row is not copied)"""
    for b, (v, n) in enumerate(zip(valid, need)):
        assert not bool(x[..., b, max(v, n):, :].any()), (what, b, "rows behind the utterance's frames must be exact zeros")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cid", WRAP_MIX)
def test_wrapper_layer_mix_against_fp64(cid, layout, monkeypatch):
    _, wav, _, valid, need = enc_setup(WRAP_ENC)
    mod = _wrapper(monkeypatch, layout, feat_select_idx="weighted_sum", normalize_hiddenstates=cid == "wrap-norm", normalize_type="s3prl")
    assert (mod._pack_plan(wav.cuda(), list(ENC_LENS)) is not None) == (layout == "packed")
    with torch.no_grad():
        mixed, feat_len = mod(wav.cuda(), torch.tensor(ENC_LENS))
        torch.cuda.synchronize()
        first = mixed.clone()
        mod(*_other_batch())          # a second forward on another batch must leave the first result alone
        torch.cuda.synchronize()
    assert torch.equal(mixed, first), "the mixed frames of the first forward changed under the second"
    T = mixed.shape[1]
    assert mixed.dtype == BF and mixed.shape == (len(ENC_LENS), T, mod.out_dim)
    assert feat_len.tolist() == [min(round(l / 320), T) for l in ENC_LENS] == list(need)
    got = mixed.float().cpu()
    if layout == "packed":
        _zeros_behind(got, valid, need, cid)
    J = Judge(f"{cid}/{layout}")
    J.all(cid, dict(mixed=("tensor", torch.cat([got[b, :v] for b, v in enumerate(valid)]))), mix_reference(cid))
    assert (J.rows, J.tensors) == (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wrapper_state_selections_against_fp64(layout, monkeypatch):
    _, wav, _, valid, need = enc_setup(WRAP_ENC)
    ref = enc_tensors(enc_reference_cached(WRAP_ENC))
    n = len(ref)
    J = Judge(f"wrap-select/{layout}")
    judged = 0
    for select in ("all", WRAP_LIST, "last_hidden_state"):
        mod = _wrapper(monkeypatch, layout, feat_select_idx=select)
        with torch.no_grad():
            out, feat_len = mod(wav.cuda(), torch.tensor(ENC_LENS))
            torch.cuda.synchronize()
            states = list(out["hidden_states"]) if select == "all" else list(out) if isinstance(select, list) else [out]
            which = list(range(n)) if select == "all" else WRAP_LIST if isinstance(select, list) else [n - 1]
            first = [s.clone() for s in states]
            mod(*_other_batch())
            torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(states, first)), (select, "states handed to the caller changed under a second forward")
        if select == "all":
            assert torch.equal(out["last_hidden_state"], states[-1])
        T = states[0].shape[1]
        assert feat_len.tolist() == list(need) and len(states) == len(which)
        for i, s in zip(which, states):
            got = s.float().cpu()
            assert s.dtype == BF and got.shape == (len(ENC_LENS), T, mod.out_dim)
            if layout == "packed":
                _zeros_behind(got, valid, need, (select, i))
            J.check(f"{WRAP_ENC}/h{i}", "rows", torch.cat([got[b, :v] for b, v in enumerate(valid)]), ref[f"h{i}"][1])
            judged += 1
    assert judged == n + len(WRAP_LIST) + 1 and (J.rows, J.tensors) == (judged * sum(valid), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", WRAP_METHODS)
def test_wrapper_hidden_state_normalisation_against_fp64(cid, monkeypatch):
    _, wav, _, valid, need = enc_setup(WRAP_ENC)
    ref = method_reference(cid)
    mod = _wrapper(monkeypatch, "packed", feat_select_idx="hidden_states", normalize_hiddenstates=True, normalize_type=cid.split("-")[1])      # packing is asked for ...
    with torch.no_grad():
        states, feat_len = mod(wav.cuda(), torch.tensor(ENC_LENS))
        torch.cuda.synchronize()
    assert feat_len.tolist() == list(need) and len(states) == len(ref)
    got = {f"h{i}": ("rows", torch.cat([s.float().cpu()[b, :v] for b, v in enumerate(valid)])) for i, s in enumerate(states)}
    if cid == "wrap-method2":      # ... and refused: method2 averages over all T frames of the padded batch, so the rows behind the valid frames are NOT zeros
        assert bool(states[0][2, valid[2]:].any())
    J = Judge(f"{cid}/padded")
    J.all(cid, got, ref)
    assert (J.rows, J.tensors) == (len(ref) * sum(valid), 0)


# ================================================================================================ e. the image tower
TOWER_CASES = ("tower-T17", "tower-T65")


def tower_eval_reference(cid, model=False, wiring=()):
    import test_train_nodes_parity_gpu as TN
    _, ref, image, _, cfg = TN.tower_setup(cid)
    params = {k: p.detach().double() for k, p in ref.visual.named_parameters()}
    return dict(feat=("tensor", I.image_tower_eval(image.double(), params, cfg, bool(model), wiring)))


@functools.lru_cache(maxsize=None)
def tower_eval_reference_cached(cid):
    return tower_eval_reference(cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", TOWER_CASES)
def test_encode_image_is_the_training_forward_bit_for_bit_and_the_fp64_tower(cid):
    import test_train_nodes_parity_gpu as TN
    from speechclip_amd.train_vit import encode_image_train
    model, _, image, _, _ = TN.tower_setup(cid)
    clip = copy.deepcopy(model.model).cuda().eval()
    feat = clip.encode_image(image.cuda())
    train = encode_image_train(clip, image.cuda()).detach()
    torch.cuda.synchronize()
    assert feat.dtype == torch.float32 and feat.shape == (TN.TOWER_B, clip.cfg.embed_dim)
    assert torch.equal(feat, train), (cid, "encode_image and encode_image_train's forward differ", (feat - train).abs().max().item())
    J = Judge(cid)
    J.all(cid, dict(feat=("tensor", feat.cpu())), tower_eval_reference_cached(cid))
    assert (J.rows, J.tensors) == (0, 1)


# ================================================================================================ f. the branch
@dataclasses.dataclass(frozen=True)
class BranchCase:
    id: str
    D: int
    H: int
    n: int
    pre_ln: bool

    @property
    def ffn(self):
        return 2 * self.D


# a cross, not the full product: each head dim once with two layers or the one-layer head, one and three layers, both norms; n1-post is the benchmarked shape
BRANCH_CASES = (BranchCase("branch-hd64-n1-post", 256, 4, 1, False), BranchCase("branch-hd96-n2-pre", 192, 2, 2, True), BranchCase("branch-hd128-n2-post", 256, 2, 2, False),
                BranchCase("branch-hd64-n3-post", 128, 2, 3, False), BranchCase("branch-hd64-n1-pre", 128, 2, 1, True))
BRANCH_T, BRANCH_LEN = 69, (69, 63, 64, 1)          # key counts 70, 64, 65, 2: both sides of the 64-key tile edge and the shortest utterance


def branch_case(cid):
    return next(c for c in BRANCH_CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def branch_inputs(cid):
    """as test_train_nodes_parity_gpu.branch_inputs: 12 tensors per layer and the final norm (matrices hold bf16 values, std 0.9 / sqrt(fan_in)), the CLS token and
    the frames (bf16 values, zero beyond the length)"""
    c = branch_case(cid)
    D, ffn, B = c.D, c.ffn, len(BRANCH_LEN)
    g = torch.Generator().manual_seed(1300 + c.D + 10 * c.n + int(c.pre_ln))
    mat = lambda o, i: (0.9 * i ** -0.5 * torch.randn(o, i, generator=g)).to(BF).float()      # noqa: E731
    vec = lambda k: 0.05 * torch.randn(k, generator=g)                                         # noqa: E731
    params = []
    for _ in range(c.n):
        params += [mat(3 * D, D), vec(3 * D), mat(D, D), vec(D), 1.0 + vec(D), vec(D), mat(ffn, D), vec(ffn), mat(D, ffn), vec(D), 1.0 + vec(D), vec(D)]
    params += [1.0 + vec(D), vec(D)]
    frames = torch.randn(B, BRANCH_T, D, generator=g).to(BF).float()
    for b, l in enumerate(BRANCH_LEN):
        frames[b, l:] = 0
    return dict(params=params, cls=torch.randn(D, generator=g).to(BF).float(), frames=frames)


def branch_reference(cid, model=False, wiring=()):
    """-> cls: ("rows", [B, D]), full: ("rows", the rows [CLS; frames < len] of every utterance, concatenated)"""
    c, d = branch_case(cid), branch_inputs(cid)
    rows, full = I.branch_eval(d["cls"].double(), [f.double() for f in d["frames"]], BRANCH_LEN, [p.double() for p in d["params"]], c.H, c.pre_ln, c.n, model, wiring)
    return dict(cls=("rows", rows), full=("rows", torch.cat(full)))


@functools.lru_cache(maxsize=None)
def branch_reference_cached(cid):
    return branch_reference(cid)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in BRANCH_CASES])
def test_branch_forward_cls_and_full_rows_against_fp64(cid):
    from speechclip_amd.module.kw_modules.TransformerModels import TransformerEncoder
    from speechclip_amd.train_branch import stack_params
    c, d = branch_case(cid), branch_inputs(cid)
    B, L = len(BRANCH_LEN), BRANCH_T + 1
    m = TransformerEncoder(n_layers=c.n, d_model=c.D, nhead=c.H, dim_feedforward=c.ffn, dropout=0.1, norm_first=c.pre_ln).eval()
    assert m.stacked == (c.n != 1 or c.pre_ln)
    with torch.no_grad():
        for p, v in zip(stack_params(m.model), d["params"]):
            p.copy_(v)
    m = m.cuda()
    lens = torch.tensor(BRANCH_LEN).cuda()
    cls = d["cls"].view(1, 1, c.D).cuda()
    with torch.no_grad():
        got_cls = m.forward_cls(cls, d["frames"].to(BF).cuda(), lens)
        src = torch.cat([cls.expand(B, 1, c.D), d["frames"].cuda()], 1)
        mask = torch.arange(L, device="cuda")[None, :] >= (lens[:, None] + 1)
        got_full = m(src, mask)
        torch.cuda.synchronize()
    assert got_cls.dtype == torch.float32 and got_cls.shape == (B, c.D) and got_full.dtype == torch.float32 and got_full.shape == (B, L, c.D)
    full = got_full.cpu()
    J = Judge(cid)
    J.all(cid, dict(cls=("rows", got_cls.cpu()), full=("rows", torch.cat([full[b, :l + 1] for b, l in enumerate(BRANCH_LEN)]))), branch_reference_cached(cid))
    assert (J.rows, J.tensors) == (B + sum(BRANCH_LEN) + B, 0)


# ================================================================================================ e. the text tower
TEXT_CASES = ("text-w64-h1-l2", "text-w128-h2-l3")
TEXT_MODES = ("packed", "packed-general", "padded")


@functools.lru_cache(maxsize=None)
def text_setup(cid):
    """(ClipModel on the CPU, ids [6, 77] with the EOT at test_text_tower_gpu.EOT_POS)"""
    import test_text_tower_gpu as TT
    cref = TT.tower_configs()[cid[len("text-"):]]
    return TT.make_clip(cref), TT.captions(cref.vocab_size), cref


def text_reference(cid, model=False, wiring=()):
    m, ids, _ = text_setup(cid)
    feat, streams = I.text_tower_eval(m.model, ids, model, wiring)
    return dict(feat=("rows", feat), stream=("rows", torch.cat(streams)))


@functools.lru_cache(maxsize=None)
def text_reference_cached(cid):
    return text_reference(cid)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", TEXT_MODES)
@pytest.mark.parametrize("cid", TEXT_CASES)
def test_text_tower_feature_rows_and_stream_against_fp64(cid, mode, monkeypatch):
    import test_text_tower_gpu as TT
    from speechclip_amd.module import clip_model as CM
    m, ids, cref = text_setup(cid)
    assert ids.argmax(-1).tolist() == list(TT.EOT_POS)
    clip = copy.deepcopy(m.model).cuda().eval()
    seen = {}
    run_tower = CM.run_tower

    def spy(packed, x, *a, **k):          # observes the residual stream run_tower hands back; changes nothing
        out = run_tower(packed, x, *a, **k)
        seen["x"], seen["general"] = out.detach().clone(), k.get("text_general")
        return out
    monkeypatch.setattr(CM, "run_tower", spy)
    B, L = ids.shape
    n = [e + 1 for e in TT.EOT_POS]
    with torch.no_grad():
        if mode == "padded":
            feat = clip._encode_text_embeddings_eval(clip.token_embedding(ids.cuda()), ids.cuda().argmax(-1))
            x = seen["x"].view(B, L, -1).float().cpu()
            streams = [x[b, :n[b]] for b in range(B)]
        else:
            feat = clip.encode_text_ids(ids.cuda(), general=mode == "packed-general")
            assert seen["general"] == (mode == "packed-general") and seen["x"].shape[0] == sum(n)
            streams = list(seen["x"].float().cpu().split(n))
        torch.cuda.synchronize()
    assert feat.dtype == torch.float32 and feat.shape == (B, cref.embed_dim)
    J = Judge(f"{cid}/{mode}")
    J.all(cid, dict(feat=("rows", feat.cpu()), stream=("rows", torch.cat(streams))), text_reference_cached(cid))
    assert (J.rows, J.tensors) == (B + sum(n), 0)

"""GPU: the full-row attention kernel (csrc/attention_rows.hip) through its C entry sc_attention_rows_fwd and through ops.attention_rows, against the plain fp64 statement of
tests/attention_rows_ref.py: element by element under the bound DERIVED there (no element is excluded, padded query positions included), bit for bit on the census cases.
tools/attention_rows_bounds.py is the CPU self-check of statement, emulation, bound and mutants; tests/test_attention_rows_bounds_cpu.py runs it and holds the argument contract.
Operands sit between NaN guard rows (the wide layout: NaN in the gap columns too; the poison family: NaN in the K and V rows of every masked key), the mask between guard bytes
that say "padding", the output in a sentinel-filled guarded window whose every byte outside the written region must still hold the sentinel.  Each case prints its worst
err / bound and where it occurred (-s); with SC_ATTN_ROWS_PARITY_OUT set the line is appended to that file (profiles/attention_rows_parity.txt is one such run).

Which case reaches which code of attention_rows_kernel:
    L 1 .. 5                         the 4-rows-per-block edge: waves with i >= L return early, L = 5 needs a second block with one live wave
    L 63 / 64 / 65, 127 .. 130, 200  jn and the `j < L` test of the last chunk; one, two, three and four chunks
    hd 8 .. 128, 72 / 96             nd = 1 / 2, the `d < hd` guard of a partly filled second accumulator; hd 768 / 1024: 12 / 16 accumulators, 12 / 16 KB of LDS (wave * hd)
    first_chunk / only64             the all-padding `continue` while run_max is still -inf; mid_chunk / last_chunk / only0: the state carried across skipped chunks
    one_full                         a row without a live key: zeros, next to a live batch entry
    rise / fall / jump / underflow   corr < 1 at every chunk / corr = 1 / corr = 0 (the earlier accumulators vanish) / the `pj == 0` skip
    wide, mbyte 2 / 255 / mix, scale separate q / k / v pointers with ld_qkv > 3 H hd and ld_out > H hd; any non-zero mask byte is padding; a scale other than hd^-0.5
The comparisons with sc_attention_probs_fwd and sc_attention_hd_fwd run on sentinel inputs of the same construction (attention_rows_ref.PROBS_CASES / HD_CASES).
Module level (attention_rows_ref.MOD_CASES): TransformerEncoder.forward / extract_hidden_states and MultiheadAttentionAndNorm.forward / extract_hidden_states /
extract_attention_map under a mask WITHOUT prefix structure, every row (masked query positions included) against the fp64 restatement attention_rows_ref.mod_ref under
4 x MODEL + 1e-3 of the per-row metric max|got - ref| / max|ref|."""
import os

import pytest
import torch

import attention_rows_ref as A
import row_kernels_ref as R

pytestmark = pytest.mark.gpu
F64, F32, BF = R.F64, R.F32, R.BF
NAN = float("nan")
# the modelled error of a correct flash kernel on attention_rows_ref.HD_CASES and of a correct module chain on attention_rows_ref.MOD_CASES (per-row max|err| / max|ref|):
# `python tools/attention_rows_bounds.py --emit`; tests/test_attention_rows_bounds_cpu.py recomputes them
HD_MODEL = {"hd-hd64-L65": 3.53e-03, "hd-hd64-L129": 4.44e-03, "hd-hd96-L65": 3.70e-03, "hd-hd96-L129": 4.40e-03, "hd-hd128-L65": 3.64e-03, "hd-hd128-L129": 4.48e-03}
MOD_MODEL = {"encoder-n1-post": 2.92e-03, "encoder-n1-pre": 2.86e-03, "encoder-n2-post": 4.45e-03, "encoder-n2-pre": 4.01e-03, "mha-h1": 1.94e-03, "mha-h4": 1.49e-03}


def bound_of(model_err):
    """the convention of tests/test_attention_fwd_parity_gpu.py: the factor covers what the model leaves out (fp32 summation orders, the GELU form), the floor never carries a
    row (the tool checks that no reference row has max|ref| < 1e-2)"""
    return 4.0 * model_err + 1e-3


def _note(line):
    print(line)
    path = os.environ.get("SC_ATTN_ROWS_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _layout(c):
    """-> (ld_qkv, column of q, of k, of v, ld_out)"""
    D = c.H * c.hd
    if c.layout == "wide":
        g = A.WIDE_GAP
        return 3 * D + 4 * g, g, D + 2 * g, 2 * D + 3 * g, D + 8
    return 3 * D, 0, D, 2 * D, D


def _device_operands(c, inp):
    """the bf16 row buffer [B L, ld_qkv] between two NaN guard rows (NaN wherever no operand lies) and the mask bytes between guard bytes of 1 -> (buffer view, mask | None)"""
    B, L, D = c.B, c.L, c.H * c.hd
    ld, cq, ck, cv, _ = _layout(c)
    host = torch.full((B * L + 2, ld), NAN, dtype=F64)
    rows = host[1:-1]
    rows[:, cq:cq + D] = inp["q"].reshape(B * L, D)
    rows[:, ck:ck + D] = inp["k"].reshape(B * L, D)
    rows[:, cv:cv + D] = inp["v"].reshape(B * L, D)
    dev = host.to(F32).to(BF).cuda()
    mask = None
    if inp["pad"] is not None:
        mb = torch.ones(B * L + 128, dtype=torch.uint8)
        byte = inp["pad"].reshape(-1).to(torch.uint8)
        if c.mbyte == "mix":
            byte = byte * torch.tensor([1, 2, 255], dtype=torch.uint8)[torch.arange(B * L) % 3]
        else:
            byte = byte * c.mbyte
        mb[64:64 + B * L] = byte
        mask = mb.cuda()[64:64 + B * L]
    return dev[1:-1], mask


def _run_abi(c, inp, dev=None, mask=None):
    """one call of sc_attention_rows_fwd into a guarded window -> fp64 [B, L, H, hd] (the guards checked)"""
    from speechclip_amd._lib import lib, check, ptr, stream
    if dev is None:
        dev, mask = _device_operands(c, inp)
    ld, cq, ck, cv, ld_out = _layout(c)
    D = c.H * c.hd
    go = R.Guarded(c.B * c.L, ld_out, BF, width=D)
    base = dev.data_ptr()
    assert base % 16 == 0 and dev.stride(0) == ld
    check(lib().sc_attention_rows_fwd(base + 2 * cq, base + 2 * ck, base + 2 * cv, go.win.data_ptr(), ptr(mask), c.B, c.H, c.L, c.hd, ld, ld_out, inp["scale"], stream()), c.id)
    torch.cuda.synchronize()
    return go.check(c.id).view(c.B, c.L, c.H, c.hd)


# ================================================================================================ parity and repeatability, every case
@pytest.mark.parametrize("c", A.cases(), ids=lambda c: c.id)
def test_attention_rows_every_element_vs_fp64(c):
    inp = A.inputs(c)
    dev, mask = _device_operands(c, inp)
    got = _run_abi(c, inp, dev, mask)
    ref, bd = A.ref(c, inp)["out"], A.bound(c, inp)["out"]
    assert got.numel() == ref.numel() == c.B * c.L * c.H * c.hd
    err = (got - ref).abs()
    r, i = R.worst(err, bd.bound)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    _note(f"{c.id:48s} worst err/bound {r:8.4f} at (b, i, h, d) = {idx}" + ("  bitwise" if c.family == "census" and r == 0 else ""))
    assert bool(torch.isfinite(got).all()), (c.id, "output not finite")
    assert r <= 1.0, (c.id, "err / bound", r, "at", idx, "got", float(got[idx]), "ref", float(ref[idx]), "bound", float(bd.bound[idx]))
    if c.family == "census":
        assert bool((got == A.census_expected(c, inp)).all()), c.id
    again = _run_abi(c, inp, dev, mask)
    assert bool((again == got).all()), (c.id, "two runs differ", int((again != got).sum()))


# ================================================================================================ ops.attention_rows
@pytest.mark.parametrize("cid", ["rows/L65-hd96-holes-sentinel", "rows/L129-hd72-mid_chunk-sentinel", "rows/L127-hd32-prefix-sentinel"])
def test_wrapper_equals_the_abi_call_and_its_argument_forms_agree(cid):
    from speechclip_amd import ops
    c = A.case(cid)
    c = c._replace(layout="packed", mbyte=1)
    inp = A.inputs(c)
    dev, _ = _device_operands(c, inp)
    qkv = dev.contiguous()
    pad = inp["pad"].cuda()
    explicit = None if c.scale is None else c.scale
    via_bool = ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, pad, scale=explicit)
    via_u8 = ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, pad.to(torch.uint8), scale=explicit)
    assert via_bool.dtype == BF and via_bool.shape == (c.B * c.L, c.H * c.hd)
    assert torch.equal(via_bool, via_u8), cid
    abi = _run_abi(c, inp)
    assert bool((via_bool.cpu().to(F64).view(abi.shape) == abi).all()), (cid, "the wrapper's bits are not the ABI call's")
    if c.scale is None:
        assert torch.equal(ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, pad, scale=c.hd ** -0.5), via_bool), cid
    nomask = ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, None, scale=explicit)
    assert torch.equal(nomask, ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, torch.zeros_like(pad), scale=explicit)), cid


# ================================================================================================ against the probabilities kernel
@pytest.mark.parametrize("x", A.PROBS_CASES, ids=lambda x: x.id)
def test_rows_agree_with_probabilities_times_v(x):
    """Both kernels lie within their own derived bound of the same fp64 softmax, so  |rows - probs_gpu @ V| <= bound_rows + sum_j bound_probs_j |v_jd|  per element, the
    product taken in fp64 from the kernel's fp32 probabilities.  (It is compared UNROUNDED: a second bf16 rounding of the product would need a store term of its own, which
    the inequality does not have.)"""
    import cascaded_fwd_ref as C
    from speechclip_amd import ops
    c = A.cross_case(x)
    inp = A.inputs(c)
    dev, _ = _device_operands(c, inp)
    qkv, pad = dev.contiguous(), inp["pad"].cuda()
    rows = ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, pad).cpu().to(F64).view(c.B, c.L, c.H, c.hd)
    probs = ops.attention_probs(qkv, c.B, c.L, c.H, c.hd, pad).cpu().to(F64)                      # [B, H, L, L]
    pc = C.PBCase(x.id, c.B, c.H, c.L, c.hd, c.L, 0, "holes", False)
    pinp = dict(q=inp["q"], k=inp["k"], pad=inp["pad"], scale=inp["scale"])
    pbound = C.pb_bound(pc, pinp)["probs"].bound
    assert bool((probs[inp["pad"][:, None, None, :].expand_as(probs)] == 0).all())
    pv = torch.einsum("bhij,bjhd->bihd", probs, inp["v"])
    allow = A.bound(c, inp)["out"].bound + torch.einsum("bhij,bjhd->bihd", pbound, inp["v"].abs())
    assert rows.numel() == c.B * c.L * c.H * c.hd
    R.judge(x.id + " rows vs probs @ V", rows, pv, allow)
    R.judge(x.id + " rows vs fp64", rows, A.ref(c, inp)["out"], A.bound(c, inp)["out"].bound)


# ================================================================================================ against sc_attention_hd_fwd
@pytest.mark.parametrize("x", A.HD_CASES, ids=lambda x: x.id)
def test_rows_and_flash_kernel_within_their_own_bounds_of_one_reference(x):
    import test_attention_fwd_parity_gpu as T
    from speechclip_amd import ops
    c = A.cross_case(x)
    inp = A.inputs(c)
    dev, _ = _device_operands(c, inp)
    qkv, pad = dev.contiguous(), inp["pad"].cuda()
    ref = A.ref(c, inp)["out"]
    rows = ops.attention_rows(qkv, c.B, c.L, c.H, c.hd, pad).cpu().to(F64).view(ref.shape)
    R.judge(x.id + " rows vs fp64", rows, ref, A.bound(c, inp)["out"].bound)
    klens = torch.tensor(A.prefix_lengths(inp["pad"]), dtype=torch.int32, device="cuda")
    flash = ops.attention_hd_qkv(qkv, c.B, c.L, c.H, klens).cpu().to(F64).view(ref.shape)
    m = T.row_metric(flash, ref)
    assert m.numel() == c.B * c.L * c.H
    print(f"{x.id:48s} flash kernel worst row metric {float(m.max()):.3e}  bound {T.bound_of(HD_MODEL[x.id]):.3e}")
    assert float(m.max()) <= T.bound_of(HD_MODEL[x.id]), (x.id, float(m.max()))


# ================================================================================================ the modules built on the kernel
def _module(m, inp):
    from speechclip_amd.module.kw_modules import TransformerModels as TM
    if m.kind == "mha":
        mod = TM.MultiheadAttentionAndNorm(d_model=m.d, nhead=m.nhead)
    else:
        mod = TM.TransformerEncoder(n_layers=1, d_model=m.d, nhead=m.nhead, dim_feedforward=m.ff)
        if m.n_layers != 1 or m.norm_first:
            # The constructor serves a stack at head dims 64 / 96 / 128 only: that is the flash kernel of forward_cls.  The full-row path under test runs on
            # sc_attention_rows_fwd at any head dim, so the stack of head dim 32 is put into a module built for the one-layer shape.
            mod.model = TM._EncoderStack(dict(d_model=m.d, nhead=m.nhead, dim_feedforward=m.ff, dropout=0.1, activation="gelu", layer_norm_eps=1e-5, batch_first=True,
                                              norm_first=m.norm_first), m.n_layers, m.d)
            mod.n_layers, mod.norm_first, mod.stacked = m.n_layers, m.norm_first, True
    mod.load_state_dict({k: v.to(F32) for k, v in inp["params"].items()}, strict=True)
    return mod.cuda().eval()


def _rows_within(what, got, want, model):
    got = got.detach().cpu().to(F64)
    assert got.shape == want.shape
    m = A.row_metric(got, want)
    print(f"{what:48s} {m.numel()} rows, worst max|err| / max|ref| {float(m.max()):.3e}  bound {bound_of(model):.3e}")
    assert bool(torch.isfinite(got).all()) and float(m.max()) <= bound_of(model), (what, float(m.max()), bound_of(model))
    return m.numel()


@pytest.mark.parametrize("m", [m for m in A.MOD_CASES if m.kind == "encoder"], ids=lambda m: m.id)
def test_transformer_encoder_full_rows_with_a_holed_mask_vs_fp64(m):
    inp = A.mod_inputs(m)
    ref = A.mod_ref(m, inp)
    enc = _module(m, inp)
    src, pad = inp["src"].to(F32).cuda(), inp["pad"].cuda()
    n = _rows_within(m.id + " forward", enc(src, pad), ref["out"], MOD_MODEL[m.id])
    hs = enc.extract_hidden_states(src, pad)
    assert len(hs) == m.n_layers + 1 and torch.equal(hs[0], src)
    for i, want in enumerate(ref["hidden"]):
        n += _rows_within(f"{m.id} hidden state {i + 1}", hs[i + 1], want, MOD_MODEL[m.id])
    assert n == (m.n_layers + 1) * m.B * m.L


@pytest.mark.parametrize("m", [m for m in A.MOD_CASES if m.kind == "mha"], ids=lambda m: m.id)
def test_mha_and_norm_full_rows_with_a_holed_mask_vs_fp64(m):
    inp = A.mod_inputs(m)
    ref = A.mod_ref(m, inp)
    mod = _module(m, inp)
    src, pad = inp["src"].to(F32).cuda(), inp["pad"].cuda()
    out = mod(src, pad)
    assert _rows_within(m.id + " forward", out, ref["out"], MOD_MODEL[m.id]) == m.B * m.L
    out2, probs = mod.extract_attention_map(src, pad)
    assert torch.equal(out2, out), (m.id, "extract_attention_map's output is not forward's")
    assert probs.shape == (m.B, m.nhead, m.L, m.L) and bool((probs[pad[:, None, None, :].expand_as(probs)] == 0).all())
    hs = mod.extract_hidden_states(src, pad)
    assert len(hs) == 2 and torch.equal(hs[0], src) and torch.equal(hs[1], out)

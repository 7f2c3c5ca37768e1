"""Kernel-level tests of the packed (padding-free) front-end BACKWARD entry points (csrc/train_front.hip), through the C ABI / `ops`:
sc_posconv_finish_train_packed, sc_reverse_rows_packed_bf16, sc_posconv_dgrad_finish_packed, sc_posconv_pack_gapped (bitwise against the uniform entries on
every utterance's own rows, exact zeros where the contract says zero, every row written: the outputs are poisoned first), sc_conv0_bwd_packed /
sc_conv0_wgrad_packed (fp64 restatement per utterance on its own zero-padded wave, at the tolerance the padded twins are tested at) and the packed
positional-conv weight gradient against the padded one.

Geometry: `packed_geometry` of the tiny model for LENS = [6091, 5200, 3040, 330] padded to 6091 samples: utterance 0 sets T0 (= 1217 frames, one more than
the 64 * 19 = 1216 its rows materialise, and frame 1216 still sees samples 6080 .. 6089: the T0-sum trap), utterance 2 has need_b = 10 > valid_b = 9,
utterance 3 has valid_b = 1."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LENS = [6091, 5200, 3040, 330]
LMAX = 6091
KW = 16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cos(a, b):
    return F.cosine_similarity(a.double().reshape(1, -1).cpu(), b.double().reshape(1, -1).cpu()).item()


def _close(name, mine, ref, cos, ratio):
    mine, ref = mine.double().cpu(), ref.double().cpu()
    assert mine.shape == ref.shape, (name, mine.shape, ref.shape)
    c, r = _cos(mine, ref), (mine.norm() / ref.norm()).item()
    print(f"{name}: cosine {c:.6f} norm ratio {r:.5f}")
    assert c > cos and abs(r - 1) < ratio, (name, c, r)


@functools.lru_cache(maxsize=None)
def _geo():
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.module.hubert import HubertConfig, HubertModel
    enc = HubertModel(HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())))
    T = enc.frame_geometry(LMAX)[1]
    need = [min(round(l / 320), T) for l in LENS]
    geo = enc.packed_geometry(LENS, LMAX, need_rows=need)
    geo["need"] = need
    geo["Tp"] = enc.frame_geometry(LMAX)[3]
    return geo


def test_geometry_has_the_cases_the_kernels_can_get_wrong():
    geo = _geo()
    rows, valid, need, T0 = geo["rows"], geo["valid"], geo["need"], geo["T0"]
    assert geo["scale0"] == 64 and T0 == (LMAX - 10) // 5 + 1
    assert need[2] > valid[2] and valid[3] == 1 and rows[3] == 2
    # the T0-sum trap: frames of utterance 0 the packed layout does not materialise (t >= 64 rows_0) that exist on the padded layout (t < T0) and still see
    # non-zero samples (5 t < len_0)
    trapped = [t for t in range(64 * rows[0], T0) if 5 * t < LENS[0]]
    assert trapped, (rows, T0)
    assert all(64 * r >= min(T0, -(-l // 5)) for r, l in zip(rows[1:], LENS[1:]))      # the other utterances have none


def _dev(xs, dtype=torch.int32):
    return torch.tensor(xs, dtype=dtype).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=BF).cuda()


def _pack_rows(x, rows):
    """padded [B, Tp, D] -> packed [sum rows_b, D]."""
    return torch.cat([x[b, :r] for b, r in enumerate(rows)], 0).contiguous()


@pytest.mark.parametrize("D,G", [(128, 4), (256, 4)])
def test_elementwise_packed_kernels_match_their_padded_twins_bitwise(D, G):
    from speechclip_amd import ops
    from speechclip_amd._lib import check, lib, ptr, stream
    geo = _geo()
    rows, valid, off, total, Tp = geo["rows"], geo["valid"], geo["row_off"], geo["total"], geo["Tp"]
    B, cg = len(rows), D // G
    g = _g(D)
    x = torch.randn(B, Tp, D, generator=g).to(BF).cuda()
    ds = torch.randn(B, Tp, D, generator=g).to(BF).cuda()
    conv = torch.randn(B, G, Tp, cg, generator=g).to(BF).cuda()
    bias = torch.randn(D, generator=g).cuda()
    valid_d, off_d, rows_d = _dev(valid), _dev(off), _dev(rows)
    xp, dsp = _pack_rows(x, rows), _pack_rows(ds, rows)
    # ---- finish-train: conv slab of utterance b = [G][rows_b][cg] at element row_off[b] * D
    u0, s0 = ops.posconv_finish_train(x.view(B * Tp, D), valid_d, conv.view(-1), bias, B, Tp, D, G)
    slab = torch.cat([conv[b, :, :r].reshape(-1) for b, r in enumerate(rows)]).contiguous()
    u1, s1 = _nan(total, D), _nan(total, D)
    check(lib().sc_posconv_finish_train_packed(ptr(xp), ptr(valid_d), ptr(off_d), ptr(slab), ptr(bias), ptr(u1), ptr(s1), B, total, D, G, stream()), "finish_train_packed")
    assert torch.equal(u1, _pack_rows(u0.view(B, Tp, D), rows)) and torch.equal(s1, _pack_rows(s0.view(B, Tp, D), rows))
    wu, ws_ = ops.posconv_finish_train(xp, valid_d, slab, bias, B, Tp, D, G, row_off_i32=off_d)
    assert torch.equal(wu, u1) and torch.equal(ws_, s1)
    # ---- reverse: inside each utterance's own rows
    r1 = _nan(total, D)
    check(lib().sc_reverse_rows_packed_bf16(ptr(xp), ptr(off_d), ptr(r1), B, total, D, stream()), "reverse_rows_packed")
    assert torch.equal(r1, torch.cat([x[b, :r].flip(0) for b, r in enumerate(rows)], 0))
    for b, r in enumerate(rows):      # the padded twin on an utterance of exactly rows_b frames
        assert torch.equal(r1[off[b]:off[b + 1]], ops.reverse_rows_bf16(x[b, :r].contiguous(), 1, r, D))
    assert torch.equal(ops.reverse_rows_bf16(xp, B, Tp, D, row_off_i32=off_d), r1)
    # ---- dgrad-finish: packed slab row rows_b - 1 - t <-> padded slab row Tp - 1 - t
    dx0 = ops.posconv_dgrad_finish(conv.view(-1), ds.view(B * Tp, D), valid_d, B, Tp, D, G).view(B, Tp, D)
    slabT = torch.cat([conv[b, :, Tp - r:].reshape(-1) for b, r in enumerate(rows)]).contiguous()
    dx1 = _nan(total, D)
    check(lib().sc_posconv_dgrad_finish_packed(ptr(slabT), ptr(dsp), ptr(valid_d), ptr(off_d), ptr(dx1), B, total, D, G, stream()), "dgrad_finish_packed")
    assert torch.equal(dx1, _pack_rows(dx0, rows))
    for b in range(B):                # exactly zero from valid_b on (the positional conv's input mask), non-zero below
        assert bool((dx1[off[b] + valid[b]:off[b + 1]] == 0).all()) and bool((dx1[off[b]:off[b] + valid[b]] != 0).any())
    assert torch.equal(ops.posconv_dgrad_finish(slabT, dsp, valid_d, B, Tp, D, G, row_off_i32=off_d), dx1)
    # ---- window pack: Kw zero rows between utterances; the padded twin's rows Kw/2 + t of utterance b at gapped row Kw/2 + row_off[b] + b Kw + t
    xg0 = ops.posconv_pack(x.view(B * Tp, D), valid_d, B, Tp, D, G, KW)[:B * G * (Tp + KW) * cg].view(B, G, Tp + KW, cg)
    slab_rows = KW // 2 + total + B * KW + 37             # more rows than the minimum: the tail must be written (zeros) too
    xg1 = _nan(slab_rows * D)
    check(lib().sc_posconv_pack_gapped(ptr(xp), ptr(valid_d), ptr(off_d), ptr(xg1), B, total, D, G, KW, KW // 2, slab_rows, stream()), "pack_gapped")
    xg1 = xg1.view(G, slab_rows, cg)
    want = torch.zeros_like(xg1)
    for b, r in enumerate(rows):
        p0 = KW // 2 + off[b] + b * KW
        want[:, p0:p0 + r] = xg0[b, :, KW // 2:KW // 2 + r]
        assert bool((xg0[b, :, KW // 2 + valid[b]:] == 0).all())
    assert torch.equal(xg1, want)
    # the gradient's form of the same kernel: G = 1, no lead, rows_b as the limit -> [slab_rows, D] with zero rows in the gaps
    dg1 = _nan(slab_rows * D)
    check(lib().sc_posconv_pack_gapped(ptr(dsp), ptr(rows_d), ptr(off_d), ptr(dg1), B, total, D, 1, KW, 0, slab_rows, stream()), "pack_gapped")
    want = torch.zeros(slab_rows, D, dtype=BF).cuda()
    for b, r in enumerate(rows):
        want[off[b] + b * KW:off[b] + b * KW + r] = ds[b, :r]
    assert torch.equal(dg1.view(slab_rows, D), want)


def _waves(B, g):
    wav = torch.zeros(B, LMAX)
    for i, l in enumerate(LENS):
        wav[i, :l] = 0.3 * torch.randn(l, generator=g) + 0.05
    return wav


def _packed_dy(rows_list, T0, C, g):
    """dy bf16 [64 * total + 8, C]: random on every utterance's materialised frames t < T0, 1e4 on frames in [T0, 64 rows_b) and in the slack rows (never read)."""
    total = sum(rows_list)
    dy = torch.full((64 * total + 8, C), 1e4, dtype=BF)
    r0 = 0
    for r in rows_list:
        n = min(T0, 64 * r)
        dy[64 * r0:64 * r0 + n] = torch.randn(n, C, generator=g).to(BF)
        r0 += r
    return dy


# rows of a second, hand-made geometry: utterance 1 (5200 samples = 1039 frames with samples) is allotted 9 rows = 576 frames only, so hundreds of frames the
# layout does not materialise still see its samples
TRAP_ROWS = [19, 9, 11, 2]


@pytest.mark.parametrize("rows_list", [None, TRAP_ROWS])
def test_conv0_bwd_packed_vs_fp64_per_utterance(rows_list):
    """GroupNorm extractor: per-utterance partials [B, C, 12] against fp64 autograd of conv1d -> group_norm -> gelu on the utterance's own zero-padded wave with
    dy = 0 on the frames the layout does not hold; cosine / norm-ratio thresholds of tests/test_finetune_front_gpu.py::test_conv0_backward_vs_autograd."""
    from speechclip_amd import ops
    geo = _geo()
    rows = list(geo["rows"]) if rows_list is None else rows_list
    T0, C, B = geo["T0"], 64, len(LENS)
    trapped = [sum(1 for t in range(64 * r, T0) if 5 * t < l) for r, l in zip(rows, LENS)]
    print("frames without a gradient that still see samples, per utterance:", trapped)
    assert trapped[0] >= 1 and (rows_list is None or trapped[1] > 400)
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    g = _g(17)
    wav = _waves(B, g)
    w = 0.3 * torch.randn(C, 1, 10, generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    dy = _packed_dy(rows, T0, C, g)
    dw, dg, db, part = ops.conv0_bwd(wav.cuda(), w.reshape(C, 10).cuda().contiguous(), gamma.cuda(), beta.cuda(), dy.cuda(), T0, 64 * off[-1],
                                      row_off_i32=_dev(off), row_scale=64)
    part = part.cpu()
    tot = torch.zeros(C, 12, dtype=torch.float64)
    for b in range(B):
        wd, gd, bd = (t.double().clone().requires_grad_(True) for t in (w, gamma, beta))
        y = F.gelu(F.group_norm(F.conv1d(wav[b].double()[None, None], wd, stride=5), C, gd, bd, 1e-5))      # [1, C, T0]
        dyb = torch.zeros(T0, C, dtype=torch.float64)
        n = min(T0, 64 * rows[b])
        dyb[:n] = dy[64 * off[b]:64 * off[b] + n].double()
        y.backward(dyb.t()[None])
        ref = torch.cat([wd.grad.view(C, 10), gd.grad[:, None], bd.grad[:, None]], 1)
        tot += ref
        _close(f"utterance {b} dw", part[b, :, :10], ref[:, :10], 0.999, 0.02)
        _close(f"utterance {b} dgamma", part[b, :, 10], ref[:, 10], 0.999, 0.02)
        _close(f"utterance {b} dbeta", part[b, :, 11], ref[:, 11], 0.999, 0.02)
    _close("dw", dw, tot[:, :10], 0.999, 0.02)
    _close("dgamma", dg, tot[:, 10], 0.999, 0.02)
    _close("dbeta", db, tot[:, 11], 0.999, 0.02)
    assert part.abs().max().item() < 1e3          # the 1e4 rows were not read


@pytest.mark.parametrize("rows_list", [None, TRAP_ROWS])
def test_conv0_wgrad_packed_vs_fp64_per_utterance(rows_list):
    """LayerNorm extractor: dw[c, j] = sum_t du[t, c] wav[5 t + j], dbias[c] = sum_t du[t, c] over the frames t < min(T0, 64 rows_b) per utterance, at the bound of
    tests/test_untested_entries_gpu.py::test_conv0_wgrad_vs_autograd_fp64: |err| <= (frames / 4 + 4) 2^-24 sum_t |du wav|."""
    from speechclip_amd import ops
    geo = _geo()
    rows = list(geo["rows"]) if rows_list is None else rows_list
    T0, C, B = geo["T0"], 64, len(LENS)
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    g = _g(23)
    wav = _waves(B, g)
    du = _packed_dy(rows, T0, C, g)
    dw, dbias, part = ops.conv0_wgrad(wav.cuda(), du.cuda(), C, T0, 64 * off[-1], row_off_i32=_dev(off), row_scale=64)
    part = part.cpu().double()
    for b in range(B):
        n = min(T0, 64 * rows[b])
        gout = du[64 * off[b]:64 * off[b] + n].double().t()[None]                                   # [1, C, n]
        seg = wav[b, :5 * (n - 1) + 10].double()[None, None]
        w = torch.zeros(C, 1, 10, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        F.conv1d(seg, w, bias, stride=5).backward(gout)
        wa = torch.zeros(C, 1, 10, dtype=torch.float64, requires_grad=True)
        F.conv1d(seg.abs(), wa, stride=5).backward(gout.abs())
        tol = (n / 4 + 4) * 2.0 ** -24
        err_w = (part[b, :, :10] - w.grad[:, 0]).abs()
        err_b = (part[b, :, 10] - bias.grad).abs()
        print(f"utterance {b}: {n} frames, max err dw {err_w.max().item():.3e} dbias {err_b.max().item():.3e}")
        assert (err_w <= tol * wa.grad[:, 0] + 1e-30).all(), (b, err_w.max().item(), tol)
        assert (err_b <= tol * gout.abs().sum((0, 2)) + 1e-30).all(), (b, err_b.max().item())
        assert bool((part[b, :, 11] == 0).all())
    _close("dw summed over the batch", dw, part[:, :, :10].sum(0), 0.999999, 1e-5)
    _close("dbias summed over the batch", dbias, part[:, :, 10].sum(0), 0.999999, 1e-5)
    assert part.abs().max().item() < 1e3          # the 1e4 rows were not read


@pytest.mark.parametrize("D,G", [(128, 4), (256, 4)])
def test_packed_posconv_weight_gradient_matches_the_padded_one(D, G):
    """dW of the grouped positional conv through the gapped slab (one [rows, cols] product for the batch) against posconv_wgrad on the padded layout of the same
    data (du zero beyond every utterance's rows, as it is in a step) and against fp64 autograd of conv1d."""
    from speechclip_amd.train_front import posconv_wgrad, posconv_wgrad_packed
    geo = _geo()
    rows, valid, off, total, Tp = geo["rows"], geo["valid"], geo["row_off"], geo["total"], geo["Tp"]
    B, cg = len(rows), D // G
    g = _g(D + 1)
    x = torch.randn(B, Tp, D, generator=g).to(BF)
    du = torch.randn(B, Tp, D, generator=g).to(BF)
    for b, r in enumerate(rows):
        du[b, r:] = 0
    valid_d, off_d, rows_d = _dev(valid), _dev(off), _dev(rows)
    dw0 = posconv_wgrad(du.cuda().view(B * Tp, D), x.cuda().view(B * Tp, D), valid_d, B, Tp, D, G, KW)
    dw1 = posconv_wgrad_packed(_pack_rows(du, rows).cuda(), _pack_rows(x, rows).cuda(), valid_d, rows_d, off_d, B, total, D, G, KW)
    dw2 = posconv_wgrad_packed(_pack_rows(du, rows).cuda(), _pack_rows(x, rows).cuda(), valid_d, rows_d, off_d, B, total, D, G, KW)
    assert torch.equal(dw1, dw2)                  # fixed summation order
    xm = x.double() * (torch.arange(Tp)[None, :, None] < torch.tensor(valid)[:, None, None])
    w = torch.zeros(D, cg, KW, dtype=torch.float64, requires_grad=True)
    F.conv1d(xm.permute(0, 2, 1), w, padding=KW // 2, groups=G)[:, :, :-1].backward(du.double().permute(0, 2, 1))
    _close("packed vs padded", dw1, dw0, 0.98, 0.1)
    _close("packed vs fp64", dw1, w.grad, 0.98, 0.1)


# ---------------------------------------------------------------------------------------------------------------- one kernel per operation
def _slab(B, G, Tp, cg, g):
    return torch.randn(B, G, Tp, cg, generator=g).to(BF).cuda()


@pytest.mark.parametrize("D,G", [(128, 4), (768, 16)])
def test_uniform_offsets_through_the_packed_entries_equal_the_uniform_entries_bitwise(D, G):
    """The padded layout is the packed one with row_off[b] = b * Tp: the *_packed entries on row_off = [0, 7, 14, 21] against the uniform entries on B = 3, Tp = 7
    (valid = [7, 3, 0]; D/G = 32 and 48, the second no power of two and straddling the 8-wide chunks), outputs poisoned first."""
    from speechclip_amd import ops
    from speechclip_amd._lib import check, lib, ptr, stream
    B, Tp, valid, off = 3, 7, [7, 3, 0], [0, 7, 14, 21]
    cg, total = D // G, B * Tp
    g = _g(D + 7)
    x = torch.randn(total, D, generator=g).to(BF).cuda()
    ds = torch.randn(total, D, generator=g).to(BF).cuda()
    conv = _slab(B, G, Tp, cg, g).view(-1)
    bias = torch.randn(D, generator=g).cuda()
    valid_d, off_d = _dev(valid), _dev(off)
    u0, s0 = ops.posconv_finish_train(x, valid_d, conv, bias, B, Tp, D, G)
    u1, s1 = _nan(total, D), _nan(total, D)
    check(lib().sc_posconv_finish_train_packed(ptr(x), ptr(valid_d), ptr(off_d), ptr(conv), ptr(bias), ptr(u1), ptr(s1), B, total, D, G, stream()), "finish_train_packed")
    assert torch.equal(u1, u0) and torch.equal(s1, s0)
    r1 = _nan(total, D)
    check(lib().sc_reverse_rows_packed_bf16(ptr(x), ptr(off_d), ptr(r1), B, total, D, stream()), "reverse_rows_packed")
    assert torch.equal(r1, ops.reverse_rows_bf16(x, B, Tp, D)) and torch.equal(r1.view(B, Tp, D), x.view(B, Tp, D).flip(1))
    dx1 = _nan(total, D)
    check(lib().sc_posconv_dgrad_finish_packed(ptr(conv), ptr(ds), ptr(valid_d), ptr(off_d), ptr(dx1), B, total, D, G, stream()), "dgrad_finish_packed")
    assert torch.equal(dx1, ops.posconv_dgrad_finish(conv, ds, valid_d, B, Tp, D, G))
    for b, v in enumerate(valid):
        assert bool((dx1.view(B, Tp, D)[b, v:] == 0).all()) and (v == 0 or bool((dx1.view(B, Tp, D)[b, :v] != 0).any()))


def test_uniform_offsets_through_the_packed_conv0_entries_equal_the_uniform_entries_bitwise():
    """sc_conv0_bwd_packed / sc_conv0_wgrad_packed with row_off = [0, 2, 4], row_scale = 64 (P = 128 rows per utterance) against sc_conv0_bwd / sc_conv0_wgrad
    with P = 128: B = 2, C = 64, L = 330 (T0 = 65 frames <= 128, so the packed frame limit min(T0, 64 * 2) is T0)."""
    from speechclip_amd import ops
    B, C, L, Tp, scale, P = 2, 64, 330, 2, 64, 128
    T0 = (L - 10) // 5 + 1
    assert T0 == 65 and scale * Tp == P
    g = _g(330)
    wav = (0.3 * torch.randn(B, L, generator=g) + 0.05).cuda()
    w = (0.3 * torch.randn(C, 10, generator=g)).cuda()
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.1 * torch.randn(C, generator=g)).cuda()
    dy = torch.randn(B * P + 8, C, generator=g).to(BF).cuda()
    off_d = _dev([0, Tp, 2 * Tp])
    uni = ops.conv0_bwd(wav, w, gamma, beta, dy, T0, P)
    pkd = ops.conv0_bwd(wav, w, gamma, beta, dy, T0, B * P, row_off_i32=off_d, row_scale=scale)
    for name, a, b in zip(("dw", "dgamma", "dbeta", "partials"), uni, pkd):
        assert torch.equal(a, b), name
    uni = ops.conv0_wgrad(wav, dy, C, T0, P)
    pkd = ops.conv0_wgrad(wav, dy, C, T0, B * P, row_off_i32=off_d, row_scale=scale)
    for name, a, b in zip(("dw", "dbias", "partials"), uni, pkd):
        assert torch.equal(a, b), name


def test_four_wide_instantiation_of_the_row_kernels():
    """D/G = 20 is a multiple of 4 but not of 8: the uniform entries run the 4-elements-per-thread instantiation.  reverse and dgrad-finish are exact (a copy; one
    fp32 add and one RNE rounding on both sides), finish-train is held to the bounds of tests/test_untested_entries_gpu.py::test_posconv_finish_train_both_outputs."""
    from speechclip_amd import ops
    D, G, B, Tp, valid = 80, 4, 2, 5, [5, 2]
    cg = D // G
    g = _g(80)
    x = torch.randn(B, Tp, D, generator=g).to(BF)
    ds = torch.randn(B, Tp, D, generator=g).to(BF)
    conv = (torch.randn(B, G, Tp, cg, generator=g) * 1.5).to(BF)
    bias = torch.randn(D, generator=g) * 0.3
    valid_d = _dev(valid)
    rev = ops.reverse_rows_bf16(x.cuda().view(B * Tp, D), B, Tp, D)
    assert torch.equal(rev.view(B, Tp, D).cpu(), x.flip(1))
    # dx[b, t] = t < valid[b] ? bf16(ds + conv[b, :, Tp - 1 - t, :] regrouped) : 0
    dx = ops.posconv_dgrad_finish(conv.cuda().view(-1), ds.cuda().view(B * Tp, D), valid_d, B, Tp, D, G).view(B, Tp, D).cpu()
    want = (conv.flip(2).permute(0, 2, 1, 3).reshape(B, Tp, D).float() + ds.float()).to(BF)
    for b, v in enumerate(valid):
        want[b, v:] = 0
    assert torch.equal(dx, want)
    for b, v in enumerate(valid):
        assert bool((dx[b, v:] == 0).all()) and bool((dx[b, :v] != 0).any())
    # finish-train
    half_ulp = 2.0 ** -8 * 1.001          # HALF_ULP_BF16 of tests/test_untested_entries_gpu.py
    xin = x.clone()
    for b, v in enumerate(valid):
        xin[b, v:] = 100.0                                                              # must be masked
    u, s = ops.posconv_finish_train(xin.cuda().view(B * Tp, D), valid_d, conv.cuda().view(-1), bias.cuda(), B, Tp, D, G)
    u, s = u.cpu().view(B, Tp, D), s.cpu().view(B, Tp, D)
    u_ref = conv.double().permute(0, 2, 1, 3).reshape(B, Tp, D) + bias.double()
    assert ((u.double() - u_ref).abs() <= half_ulp * u_ref.abs() + 1e-30).all()
    xm = xin.double().clone()
    for b, v in enumerate(valid):
        xm[b, v:] = 0
    s_ref = xm + F.gelu(u.double())
    assert ((s.double() - s_ref).abs() <= half_ulp * s_ref.abs() + 1e-6 * (1 + u.double().abs())).all(), (s.double() - s_ref).abs().max().item()
    for b, v in enumerate(valid):
        assert v == Tp or (s[b, v:].double() - F.gelu(u[b, v:].double())).abs().max().item() < 0.02      # rows >= valid: no trace of the 100.0 input

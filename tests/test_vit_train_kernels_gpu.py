"""GPU: the kernels behind image-tower training against their fp64 statements (tests/vit_train_ref.py; tests/test_vit_train_host.py is the CPU self-check of
statements, bounds and mutants): sc_quickgelu_bwd_bf16 on every bf16 pre-activation in [-12, 12], sc_vit_embed_bwd per element under derived bounds and twice
for its bits, and the image side of the InfoNCE backward.  Kernel outputs land in sentinel-guarded buffers.  Each test prints its worst err / bound (-s)."""
import pytest
import torch

import vit_train_ref as V

pytestmark = pytest.mark.gpu
F64, F32, BF = V.F64, V.F32, V.BF
DH = [1.0, -0.7109375, 0.005859375, 160.0]          # bf16-exact gradient magnitudes


def _quickgelu_inputs():
    u = V.every_bf16_in(-12.0, 12.0)
    uu = u.repeat(len(DH))
    dh = torch.tensor(DH, dtype=F64).repeat_interleave(u.numel())
    assert bool((uu.to(BF).to(F64) == uu).all()) and bool((dh.to(BF).to(F64) == dh).all())
    return uu, dh


def _run_quickgelu(u64, dh64, off_u=0, off_dh=0, off_out=0):
    """inputs as views `off` elements into their allocations (the allocations are 256-byte aligned), the output into a guarded window"""
    from speechclip_amd import ops
    n = u64.numel()
    ub = torch.zeros(n + off_u, dtype=BF, device="cuda")
    db = torch.zeros(n + off_dh, dtype=BF, device="cuda")
    ub[off_u:] = u64.to(BF).cuda()
    db[off_dh:] = dh64.to(BF).cuda()
    go = V.Guarded(n, BF, off_out)
    ops.quickgelu_bwd_bf16(ub[off_u:], db[off_dh:], out=go.win)
    return go.check(f"quickgelu_bwd n={n} offsets {off_u}/{off_dh}/{off_out}")


@pytest.mark.parametrize("what,n_cut,offs", [("whole", 0, (0, 0, 0)), ("odd_length", 1, (0, 0, 0)), ("short_odd", -1001, (0, 0, 0)), ("offset_view", 3, (1, 1, 1)),
                                             ("offset_4_bytes", 0, (2, 2, 2)), ("mixed_phase", 5, (1, 3, 0)), ("three_elements", -3, (5, 5, 5))])
def test_quickgelu_bwd_bf16_every_preactivation(what, n_cut, offs):
    u, dh = _quickgelu_inputs()
    if n_cut > 0:        # drop n_cut elements from the end
        u, dh = u[:-n_cut], dh[:-n_cut]
    elif n_cut < 0:      # keep -n_cut elements spread over the whole range
        idx = torch.linspace(0, u.numel() - 1, -n_cut).long()
        u, dh = u[idx], dh[idx]
    got = _run_quickgelu(u, dh, *offs)
    ref = V.quickgelu_bwd_ref(u, dh)
    r, i = V.worst_ratio(got, ref, V.quickgelu_bwd_bound(ref, dh))
    print(f"quickgelu_bwd {what:16s} n={u.numel():7d} worst err/bound {r:.4f} at u={u[i].item()} dh={dh[i].item()}")
    assert torch.isfinite(got).all() and r <= 1.0, (what, r, u[i].item(), dh[i].item(), got[i].item(), ref[i].item())


def test_quickgelu_bwd_far_tails_are_finite():
    """beyond the range of the parity test, up to the largest bf16: e^{-1.702 u} leaves fp32 for u < -52 and 1.702 u itself beyond 2e38; same bound"""
    u = torch.tensor([-3.0e38, -1000.0, -64.5, -60.0, -52.5, -40.0, 40.0, 52.5, 60.0, 64.5, 1000.0, 3.0e38], dtype=F64).to(BF).to(F64)
    dh = torch.full_like(u, 2.0)
    got = _run_quickgelu(u, dh)
    ref = V.quickgelu_bwd_ref(u, dh)
    r, i = V.worst_ratio(got, ref, V.quickgelu_bwd_bound(ref, dh))
    print(f"quickgelu_bwd far tails: {got.tolist()} worst err/bound {r:.4f}")
    assert torch.isfinite(got).all() and r <= 1.0, (r, u[i].item(), got[i].item(), ref[i].item())


def _run_embed_bwd(x):
    from speechclip_amd import ops
    B, ntok, D = x["B"], x["ntok"], x["D"]
    outs = [V.Guarded(B * (ntok - 1) * D, BF), V.Guarded(ntok * D, F32), V.Guarded(D, F32), V.Guarded(D, F32)]
    views = (outs[0].win.view(B * (ntok - 1), D), outs[1].win.view(ntok, D), outs[2].win, outs[3].win)
    res = ops.vit_embed_bwd(x["dx"].to(F32).cuda(), x["patch"].to(BF).cuda(), x["cls"].to(F32).cuda(), x["pos"].to(F32).cuda(), x["gamma"].to(F32).cuda(),
                            B, ntok, D, V.EPS, out=views)
    assert res[2].data_ptr() == res[1].data_ptr() and res[2].shape == (D,)          # dcls is row 0 of dpos
    return {k: o.check(f"vit_embed_bwd {k} [{B},{ntok},{D}]") for k, o in zip(("dpatch", "dpos", "dgamma", "dbeta"), outs)}


@pytest.mark.parametrize("B,ntok,D", V.EMBED_SHAPES)
def test_vit_embed_bwd_vs_fp64_statement(B, ntok, D):
    x = V.embed_bwd_inputs(B, ntok, D)
    for k in ("dx", "cls", "pos", "gamma"):
        x[k] = x[k].to(F32).to(F64)                        # what the kernel reads
    ref = V.embed_bwd_ref(**x)
    bound = V.embed_bwd_bounds(ref, x["gamma"], B, ntok, D)
    got = _run_embed_bwd(x)
    for k in ("dpatch", "dpos", "dgamma", "dbeta"):
        r, i = V.worst_ratio(got[k], ref[k].reshape(-1), bound[k].reshape(-1))
        print(f"vit_embed_bwd {k:7s} [{B},{ntok},{D}] worst err/bound {r:.4f} at {i}")
        assert torch.isfinite(got[k]).all() and r <= 1.0, (k, r, i, got[k][i].item(), ref[k].reshape(-1)[i].item())
    again = _run_embed_bwd(x)
    for k in got:
        assert torch.equal(got[k], again[k]), (k, "two runs differ")


def test_vit_embed_bwd_with_several_batch_splits():
    """B = 40 at ntok = 65: 7 batch splits of 6 entries per token (waves 0 and 1 take two rows each, the last split holds 4): the two-stage reduction proper."""
    B, ntok, D = 40, 65, 256
    x = V.embed_bwd_inputs(B, ntok, D, seed=7)
    for k in ("dx", "cls", "pos", "gamma"):
        x[k] = x[k].to(F32).to(F64)
    ref = V.embed_bwd_ref(**x)
    bound = V.embed_bwd_bounds(ref, x["gamma"], B, ntok, D)
    got = _run_embed_bwd(x)
    for k in ("dpatch", "dpos", "dgamma", "dbeta"):
        r, i = V.worst_ratio(got[k], ref[k].reshape(-1), bound[k].reshape(-1))
        print(f"vit_embed_bwd {k:7s} [{B},{ntok},{D}] worst err/bound {r:.4f} at {i}")
        assert r <= 1.0, (k, r, i)
    again = _run_embed_bwd(x)
    assert all(torch.equal(got[k], again[k]) for k in got)


GRID = [(256, 512, False, 0.0, False, True, True), (300, 768, True, 0.0, False, True, True), (64, 512, True, 0.2, False, True, False),
        (130, 512, True, 0.0, True, False, True)]          # the option grid of test_train_kernels_gpu.py::test_infonce_backward_matches_autograd


def _infonce_case(Bg, E, dup):
    g = torch.Generator().manual_seed(Bg + E)
    a = torch.nn.functional.normalize(torch.randn(Bg, E, generator=g), dim=-1)
    b = torch.nn.functional.normalize(torch.randn(Bg, E, generator=g), dim=-1)
    ids = torch.arange(Bg)
    if dup:
        ids[1::7] = ids[0::7][: len(ids[1::7])]
    return a, b, ids


def _close(got, ref):
    return (got.double().cpu() - ref.double()).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item() * 10)


@pytest.mark.parametrize("Bg,E,dup,margin,dcl,a2b,b2a", GRID)
def test_infonce_dfeat_b_matches_fp64_autograd(Bg, E, dup, margin, dcl, a2b, b2a):
    from oracle.speechclip_ref import masked_contrastive_loss
    from speechclip_amd import ops
    a, b, ids = _infonce_case(Bg, E, dup)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    masked_contrastive_loss(ar, br, ids, 1 / 0.07, margin=margin, dcl=dcl, a2b=a2b, b2a=b2a).backward()
    out, da, dinv, db = ops.infonce_fwd_bwd(a.cuda(), b.cuda(), ids.cuda(), 1 / 0.07, margin, dcl, a2b, b2a, want_dfeat_b=True)
    print(f"infonce dfeat_b [{Bg},{E}] max err {(db.double().cpu() - br.grad).abs().max().item():.3e}  max |ref| {br.grad.abs().max().item():.3e}")
    assert _close(db, br.grad) and _close(da, ar.grad)
    assert len(ops.infonce_fwd_bwd(a.cuda(), b.cuda(), ids.cuda(), 1 / 0.07, margin, dcl, a2b, b2a)) == 3


@pytest.mark.parametrize("Bg,E,dup,margin,dcl,a2b,b2a", GRID)
def test_masked_contrastive_loss_returns_both_gradients_and_swaps(Bg, E, dup, margin, dcl, a2b, b2a):
    from oracle.speechclip_ref import masked_contrastive_loss
    from speechclip_amd.module.losses import MaskedContrastiveLoss
    a, b, ids = _infonce_case(Bg, E, dup)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    masked_contrastive_loss(ar, br, ids, 1 / 0.07, margin=margin, dcl=dcl, a2b=a2b, b2a=b2a).backward()

    def run(x, y, x2y, y2x):
        crit = MaskedContrastiveLoss(temperature=0.07, temperature_trainable=False, margin=margin, dcl=dcl, a2b=x2y, b2a=y2x)
        xg, yg = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
        loss = crit(feat_A=xg, feat_B=yg, index=ids.cuda())
        loss.backward()
        return loss.item(), xg.grad, yg.grad

    loss, ga, gb = run(a, b, a2b, b2a)
    assert ga is not None and gb is not None and _close(ga, ar.grad) and _close(gb, br.grad)
    loss_s, gb_s, ga_s = run(b, a, b2a, a2b)               # the swapped call: the same pair, exchanged
    assert abs(loss - loss_s) < 1e-4 and _close(ga_s, ar.grad) and _close(gb_s, br.grad)
    # only the image side carries a gradient (a frozen speech side): still served
    crit = MaskedContrastiveLoss(temperature=0.07, temperature_trainable=False, margin=margin, dcl=dcl, a2b=a2b, b2a=b2a)
    yg = b.cuda().requires_grad_(True)
    crit(feat_A=a.cuda(), feat_B=yg, index=ids.cuda()).backward()
    assert _close(yg.grad, br.grad)

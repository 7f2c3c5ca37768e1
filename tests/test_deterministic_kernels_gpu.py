"""GPU: the three fixed-order reductions through the C ABI -- sc_sgemm_batched_det / sc_sgemm_det, sc_colsum_det, sc_cls_pool_bwd_det.

For the two workspace entries, per case:
  * five calls give equal bits;
  * the output equals, bit for bit, the fp32 restatement of the finish chain stated in include/speechclip_hip.h, computed with numpy float32 (one rounding per
    operation, no FMA) from the partials the test reads back from the workspace;
  * fp64 parity under the bound tests/tail_kernels_ref.py derives for the default entry (it allows any summation order, so it covers the fixed one);
  * a shape with one slice / one chunk returns the default entry's bits.
For the pooling backward, over the case list of tests/test_train_mode_parity_gpu.py (ragged batch with an empty utterance, NQ > 1, 13 and 25 layers without and with
normalize, bf16 and fp32 hidden states, key splits 1 / default / 64, dropout off and on): du, dcls_key and dalpha repeat over five calls; dcls_key, ds_ws and pp_ws
equal sc_cls_pool_bwd's bit for bit; du and dalpha stay inside the bound that test applies to sc_cls_pool_bwd and within twice that bound of sc_cls_pool_bwd.

Every output sits between sentinels; every workspace is NaN-filled over its stated size (a partial that is not written shows in the result) with sentinels behind
it (a write past the stated size shows)."""
import numpy as np
import pytest
import torch

import tail_kernels_ref as T
import test_train_mode_parity_gpu as TM
import train_mode_ref as R
from row_kernels_ref import GUARD, SENT32, Guarded, judge as _judge

pytestmark = pytest.mark.gpu
F64, F32, BF = T.F64, T.F32, T.BF
REPEATS = 5


def _L():
    from speechclip_amd._lib import check, lib, ptr, stream
    return lib(), check, ptr, stream


def _d(t):
    return t.to(F32).cuda().contiguous()


def _placed(stored, off):
    flat = torch.full((off + stored.numel(),), T.PAST_VALUE, dtype=F32, device="cuda")
    flat[off:] = stored.to(F32).reshape(-1).cuda()
    return flat[off:]


class Workspace:
    """`nbytes` of NaN between sentinels"""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.full((2 * GUARD + self.n,), SENT32, dtype=F32, device="cuda")
        self.buf[GUARD:GUARD + self.n] = float("nan")
        self.nbytes = nbytes

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def read(self, what, expect_written=True):
        flat = self.buf.cpu()
        assert bool((flat[:GUARD] == SENT32).all()) and bool((flat[GUARD + self.n:] == SENT32).all()), (what, "wrote outside the stated workspace size")
        win = flat[GUARD:GUARD + self.n]
        if expect_written:
            assert not bool(torch.isnan(win).any()), (what, "left part of the workspace unwritten")
        else:
            assert bool(torch.isnan(win).all()), (what, "touched a workspace it does not need")
        return win.numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ================================================================================================ sgemm
def _gc(tag, ta, tb, M, N, K, batch, layout, pad, abi):
    al, be, bias = T.GEMM_AB[abi]
    return T.GemmCase(f"det-sgemm-{tag}-{'t' if ta else 'n'}{'t' if tb else 'n'}-{M}x{N}x{K}-b{batch}-{layout}{'-ldc3' if pad else ''}-a{al:g}b{be:g}{'-bias' if bias else ''}",
                      ta, tb, M, N, K, batch, layout, pad, al, be, bias)


def _gemm_cases():
    """the smallest split shape (8 slices), a shape ragged in M, N and K (16 slices of 272, the last one short), a batch of 3 (9 slices each): all four transposes
    of each; the (alpha, beta, bias) triple, the operand layout and ldc rotate underneath, and beta != 0 with a bias meets every shape and every transpose"""
    out = []
    for ti, (ta, tb) in enumerate(((False, False), (False, True), (True, False), (True, True))):
        out.append(_gc("min", ta, tb, 64, 64, 2048, 1, T.GEMM_LAYOUTS[ti % 3], ti % 2 == 1, (ti + 1) % 3))
        out.append(_gc("ragged", ta, tb, 33, 70, 4099, 1, T.GEMM_LAYOUTS[(ti + 1) % 3], ti % 2 == 0, (ti + 2) % 3))
        out.append(_gc("batch", ta, tb, 16, 64, 2304, 3, T.GEMM_LAYOUTS[(ti + 2) % 3], ti >= 2, ti % 3))
    out.append(_gc("min", False, True, 64, 64, 2048, 1, "aligned", False, 1))
    out.append(_gc("ragged", True, False, 33, 70, 4099, 1, "aligned", True, 1))
    out.append(_gc("batch", True, True, 16, 64, 2304, 3, "off1", False, 1))
    return out


GEMM_CASES = _gemm_cases()


def test_sgemm_case_list_covers_what_it_claims():
    sl = {c.id: T.gemm_split(c.M, c.N, c.K, c.batch)[0] for c in GEMM_CASES}
    assert {(c.M, c.N, c.K, c.batch): sl[c.id] for c in GEMM_CASES} == {(64, 64, 2048, 1): 8, (33, 70, 4099, 1): 16, (16, 64, 2304, 3): 9}
    for shape in ((64, 64, 2048), (33, 70, 4099), (16, 64, 2304)):
        cs = [c for c in GEMM_CASES if (c.M, c.N, c.K) == shape]
        assert {(c.ta, c.tb) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
        assert any(c.beta != 0 and c.bias for c in cs) and any(c.beta == 0 for c in cs)
    for tt in ((False, False), (False, True), (True, False), (True, True)):
        assert any(c.beta != 0 and c.bias for c in GEMM_CASES if (c.ta, c.tb) == tt)


def _run_gemm_det(c, inp, det=True):
    """-> (C [batch, M, N] fp64, partials [batch, slices, M, N] float32 numpy or None)"""
    L, check, ptr, stream = _L()
    off = 1 if c.layout == "off1" else 0
    A, B = _placed(inp["A"], off), _placed(inp["B"], off)
    lda, ldb = inp["A"].shape[-1], inp["B"].shape[-1]
    sA, sB = inp["A"].shape[1] * lda, inp["B"].shape[1] * ldb
    ldc = c.N + 3 if c.ldc_pad else c.N
    C = Guarded(c.batch * c.M, ldc, F32, c.N)
    C.out().copy_(inp["C0"].reshape(c.batch * c.M, c.N).to(F32).cuda())
    bias = _d(inp["bias"]) if c.bias else None
    slices = T.gemm_split(c.M, c.N, c.K, c.batch)[0]
    if not det:
        check(L.sc_sgemm_batched(int(c.ta), int(c.tb), c.M, c.N, c.K, c.alpha, ptr(A), lda, sA, ptr(B), ldb, sB, c.beta, ptr(C.out()), ldc, c.M * ldc, ptr(bias),
                                 c.N if c.bias else 0, c.batch, stream()), c.id)
        return C.check(c.id).view(c.batch, c.M, c.N), None
    ws = Workspace(L.sc_sgemm_det_workspace_bytes(c.M, c.N, c.K, c.batch))
    assert ws.nbytes == slices * c.M * c.N * c.batch * 4
    if c.batch == 1:
        check(L.sc_sgemm_det(int(c.ta), int(c.tb), c.M, c.N, c.K, c.alpha, ptr(A), lda, ptr(B), ldb, c.beta, ptr(C.out()), ldc, ptr(bias), ws.ptr(), ws.nbytes,
                             stream()), c.id)
    else:
        check(L.sc_sgemm_batched_det(int(c.ta), int(c.tb), c.M, c.N, c.K, c.alpha, ptr(A), lda, sA, ptr(B), ldb, sB, c.beta, ptr(C.out()), ldc, c.M * ldc, ptr(bias),
                                     c.N if c.bias else 0, c.batch, ws.ptr(), ws.nbytes, stream()), c.id)
    torch.cuda.synchronize()
    parts = ws.read(c.id, expect_written=slices > 1).reshape(c.batch, slices, c.M, c.N)
    return C.check(c.id).view(c.batch, c.M, c.N), parts


def _gemm_chain(c, inp, parts):
    """include/speechclip_hip.h: t = beta * C (+0 when beta == 0), t = t + bias[n], then t = t + p_s in ascending s; numpy float32, one rounding per operation"""
    f = np.float32
    t = np.zeros((c.batch, c.M, c.N), dtype=f)
    if c.beta != 0:
        t = f(c.beta) * inp["C0"].to(F32).numpy()
    if c.bias:
        t = t + inp["bias"].to(F32).numpy()[:, None, :]
    for s in range(parts.shape[1]):
        t = t + parts[:, s]
    assert t.dtype == f
    return t


@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c.id)
def test_sgemm_det_repeats_matches_its_stated_chain_and_fp64(c):
    inp = T.gemm_inputs(c)
    runs = [_run_gemm_det(c, inp) for _ in range(REPEATS)]
    C0, parts0 = runs[0]
    for C, parts in runs[1:]:
        assert torch.equal(C, C0) and np.array_equal(_bits(parts), _bits(parts0)), (c.id, "differs between calls")
    got = C0.to(F32).numpy()
    want = _gemm_chain(c, inp, parts0)
    assert np.array_equal(_bits(got), _bits(want)), (c.id, "C is not the stated chain over the workspace partials", int((_bits(got) != _bits(want)).sum()))
    _judge(f"{c.id} C", C0, T.gemm_ref(c, inp)["C"], T.gemm_bound(c, inp)["C"].bound)


ONE_SLICE = ((64, 64, 2047, 1, False, True), (65, 5, 19, 3, True, False), (1024, 512, 2048, 1, True, True))


@pytest.mark.parametrize("M,N,K,batch,ta,tb", ONE_SLICE)
def test_sgemm_det_with_one_slice_returns_the_default_entrys_bits(M, N, K, batch, ta, tb):
    """K one below the threshold, a short K in a batch, 128 tiles with K at the threshold: the rule gives one slice, the entry is sc_sgemm_batched (same
    bits) and leaves the workspace alone"""
    c = _gc("one", ta, tb, M, N, K, batch, "aligned", False, 1)
    assert T.gemm_split(M, N, K, batch)[0] == 1
    inp = T.gemm_inputs(c)
    det, _ = _run_gemm_det(c, inp)
    ref, _ = _run_gemm_det(c, inp, det=False)
    assert torch.equal(det, ref), (c.id, int((det != ref).sum()))


# ================================================================================================ colsum
CS_CASES = [T.CSCase(f"det-colsum-{r}x{c_}-ld{ld}-{'acc' if acc else 'set'}", r, c_, ld, acc)
            for (r, c_, ld) in ((256, 64, 64), (1000, 70, 96), (257, 130, 130)) for acc in (0, 1)]
CS_ONE_CHUNK = [T.CSCase(f"det-colsum-{r}x{c_}-ld{ld}-{'acc' if acc else 'set'}", r, c_, ld, acc) for (r, c_, ld) in ((255, 64, 64), (255, 70, 96)) for acc in (0, 1)]


def test_colsum_case_list_covers_what_it_claims():
    assert [T.cs_chunks(c.rows, c.cols)[0] for c in CS_CASES] == [4, 4, 16, 16, 5, 5]
    assert all(T.cs_chunks(c.rows, c.cols)[0] == 1 for c in CS_ONE_CHUNK)


def _run_cs(c, inp, det=True):
    L, check, ptr, stream = _L()
    x = _d(inp["x"])
    out = Guarded(1, c.cols, F32)
    out.out().copy_(inp["out0"].to(F32).cuda().view(1, -1))
    if not det:
        check(L.sc_colsum(ptr(x), c.ld, c.rows, c.cols, ptr(out.out()), c.acc, stream()), c.id)
        return out.check(c.id), None
    chunks = T.cs_chunks(c.rows, c.cols)[0]
    ws = Workspace(L.sc_colsum_det_workspace_bytes(c.rows, c.cols))
    assert ws.nbytes == chunks * c.cols * 4
    check(L.sc_colsum_det(ptr(x), c.ld, c.rows, c.cols, ptr(out.out()), c.acc, ws.ptr(), ws.nbytes, stream()), c.id)
    torch.cuda.synchronize()
    return out.check(c.id), ws.read(c.id, expect_written=chunks > 1).reshape(chunks, c.cols)


@pytest.mark.parametrize("c", CS_CASES, ids=lambda c: c.id)
def test_colsum_det_repeats_matches_its_stated_chain_and_fp64(c):
    inp = T.cs_inputs(c)
    runs = [_run_cs(c, inp) for _ in range(REPEATS)]
    o0, p0 = runs[0]
    for o, p in runs[1:]:
        assert torch.equal(o, o0) and np.array_equal(_bits(p), _bits(p0)), (c.id, "differs between calls")
    t = p0[0].copy()
    for k in range(1, p0.shape[0]):
        t = t + p0[k]
    if c.acc:
        t = t + inp["out0"].to(F32).numpy()
    assert t.dtype == np.float32
    got = o0.to(F32).numpy().reshape(-1)
    assert np.array_equal(_bits(got), _bits(t)), (c.id, "out is not the stated chain over the workspace partials", int((_bits(got) != _bits(t)).sum()))
    _judge(f"{c.id} out", o0.reshape(-1), T.cs_ref(c, inp)["out"], T.cs_bound(c, inp)["out"].bound)


@pytest.mark.parametrize("c", CS_ONE_CHUNK, ids=lambda c: c.id)
def test_colsum_det_with_one_chunk_returns_the_default_entrys_bits(c):
    inp = T.cs_inputs(c)
    det, _ = _run_cs(c, inp)
    ref, _ = _run_cs(c, inp, det=False)
    assert torch.equal(det, ref)
    _judge(f"{c.id} out", det.reshape(-1), T.cs_ref(c, inp)["out"], T.cs_bound(c, inp)["out"].bound)


# ================================================================================================ pooling backward
def _pool_run(c, p, nsplit, det):
    """sc_cls_pool_bwd[_det] on the inputs of test_train_mode_parity_gpu -> dict of fp32 CPU tensors (partial rows as written)"""
    L, check, ptr, stream = _L()
    from speechclip_amd import ops
    d = TM.pool_inputs(c.id)
    dev = torch.device("cuda")
    x_rows = d["x"].to(BF).reshape(c.B * c.T, c.D).to(dev)
    cls, u, dzbar = d["cls"].to(dev).contiguous(), d["u"].to(dev).contiguous(), d["dzbar"].to(dev).contiguous()
    lens_i = torch.tensor(c.lens, dtype=torch.int32, device=dev)
    hid = None
    if c.n:
        hid = (d["hid"] if c.f32 else d["hid"].to(BF)).reshape(c.n, c.B * c.T, c.D).contiguous().to(dev)
    pk, _ = ops.cls_pool_train_fwd(x_rows, cls, d["scores"].to(dev), d["cls_scores"].to(dev), lens_i, c.B, c.T, c.NQ, c.R, c.D, p, TM.POOL_SEED)
    S = max(1, min(16, 512 // c.B)) if nsplit is None else nsplit
    K = c.NQ + c.T
    ds, pp = Guarded(c.B * c.R, K, F32), Guarded(c.B * c.R, K, F32)
    du, dck = Guarded(c.B * S, c.R * c.D, F32), Guarded(c.B * S, c.NQ * c.D, F32)
    da = Guarded(c.B * S, c.n, F32) if c.n else None
    entry = L.sc_cls_pool_bwd_det if det else L.sc_cls_pool_bwd
    check(entry(ptr(x_rows), x_rows.stride(0), ptr(cls), ptr(hid), int(bool(c.n) and c.f32), hid.stride(0) if c.n else 0, c.n, int(c.normalize), ptr(pk), ptr(dzbar),
                ptr(u), ptr(lens_i), ptr(ds.out()), ptr(pp.out()), ptr(du.out()), ptr(dck.out()), ptr(da.out()) if c.n else 0, c.B, c.T, c.NQ, c.R, c.D, S, float(p),
                TM.POOL_SEED, stream()), c.id)
    torch.cuda.synchronize()
    return dict(S=S, ds=ds.check(c.id), pp=pp.check(c.id), du=du.check(c.id).view(c.B, S, c.R, c.D), dck=dck.check(c.id).view(c.B, S, c.NQ, c.D),
                dalpha=da.check(c.id).view(c.B, S, c.n) if c.n else None)


def test_pool_case_list_is_the_existing_one_and_covers_what_the_issue_names():
    cs = TM.POOL_CASES
    assert any(c.NQ > 1 for c in cs) and any(c.n == 13 and not c.normalize for c in cs) and any(c.n > 16 and c.normalize and c.f32 for c in cs)
    assert any(c.n and not c.f32 for c in cs) and all(len(set(c.lens)) > 1 for c in cs) and any(0 in c.lens for c in cs)
    assert 1 in TM.POOL_NSPLIT and any(s is None or s > 1 for s in TM.POOL_NSPLIT) and any(p > 0 for p in TM.POOL_P) and 0.0 in TM.POOL_P
    assert {(c.D + 255) // 256 for c in cs} == {1, 3, 4}          # DCH 1, 3, 4 (DCH 2, D = 260, runs in the extra case below)


@pytest.mark.parametrize("p", TM.POOL_P)
@pytest.mark.parametrize("cid", [c.id for c in TM.POOL_CASES])
def test_cls_pool_bwd_det_repeats_and_matches_the_default_entry_and_fp64(cid, p):
    c = TM.pool_case(cid)
    ref = TM.pool_reference_cached(cid, p)
    for nsplit in TM.POOL_NSPLIT:
        runs = [_pool_run(c, p, nsplit, det=True) for _ in range(REPEATS)]
        g0 = runs[0]
        for g in runs[1:]:
            for k in ("du", "dck", "dalpha", "ds", "pp"):
                assert (g0[k] is None and g[k] is None) or torch.equal(g[k], g0[k]), (cid, p, nsplit, k, "differs between calls")
        dflt = _pool_run(c, p, nsplit, det=False)
        for k in ("dck", "ds", "pp"):          # one writer per element in both entries
            assert torch.equal(g0[k], dflt[k]), (cid, p, nsplit, k, "differs from sc_cls_pool_bwd", int((g0[k] != dflt[k]).sum()))
        for k, t in (("du", "du"), ("dalpha", "dalpha")):
            if g0[k] is None:
                continue
            bound = R.bound_of(TM.MODEL[f"{cid}/p{p}/{t}"])
            got = g0[k].sum(1) if k == "dalpha" else g0[k].sum((0, 1))
            other = dflt[k].sum(1) if k == "dalpha" else dflt[k].sum((0, 1))
            worst = R.tensor_metric(got, ref[k])
            apart = (got - other).abs().max().item() / ref[k].abs().max().item()
            print(f"{cid} p={p} nsplit={nsplit} {k}: vs fp64 {worst:.3e} (bound {bound:.3e}), vs the default entry {apart:.3e} (bound {2 * bound:.3e})")
            assert torch.isfinite(got).all() and worst <= bound, (cid, p, nsplit, k, worst, bound)
            assert apart <= 2 * bound, (cid, p, nsplit, k, apart, 2 * bound)
        for b, n in enumerate(c.lens):
            if n == 0 and c.n:
                assert bool((g0["dalpha"][b] == 0).all()), "an utterance without frames has no d alpha"


def test_cls_pool_bwd_det_two_chunk_width_and_partial_rows_against_the_default():
    """D = 260 (DCH 2, the second 256-chunk holds 4 elements), R = 7 (the last group of three rows holds one), 3 layers, two key splits: every PARTIAL row.
    An element of du / dalpha is the sum of the block's 8 wave partials w_i in one of two orders, each within 7 U sum|w_i| of the exact sum, so the entries differ by
    at most 14 U sum|w_i| <= 14 U MAG, with MAG the sum of the absolute terms over the block's keys, formed in fp64 from the (one-writer, shared) ds_ws / pp_ws:
    du: sum_t |ds_rt| |z_td|;  dalpha: sum_t sum_d (sum_r |pp_rt| |dzbar_rd| + |ds_rt| |u_rd|) |H_ntd|.  (x 1.01 for the second-order terms.)"""
    c = TM.PoolCase("det-pool-260", 3, 41, 260, 1, 7, 3)
    g = torch.Generator().manual_seed(260)
    L, check, ptr, stream = _L()
    from speechclip_amd import ops
    dev = torch.device("cuda")
    hid = (torch.randn(c.n, c.B * c.T, c.D, generator=g) + 0.2).to(BF)
    x16 = torch.randn(c.B * c.T, c.D, generator=g).to(BF)
    cls, u = torch.randn(c.NQ, c.D, generator=g), torch.randn(c.R, c.D, generator=g) * c.D ** -0.5
    dzbar = torch.randn(c.B, c.R, c.D, generator=g)
    lens = [41, 7, 30]
    x_rows, hid_d, cls_d, u_d, dzbar_d = x16.to(dev), hid.to(dev), cls.to(dev), u.to(dev), dzbar.to(dev)
    lens_i = torch.tensor(lens, dtype=torch.int32, device=dev)
    scores, cls_scores = (x_rows.float() @ u_d.t()).contiguous(), (cls_d @ u_d.t()).contiguous()
    pk, _ = ops.cls_pool_train_fwd(x_rows, cls_d, scores, cls_scores, lens_i, c.B, c.T, c.NQ, c.R, c.D, 0.1, 5)
    S, K = 2, c.NQ + c.T
    outs = {}
    for det in (True, False, True):
        ds, pp = Guarded(c.B * c.R, K, F32), Guarded(c.B * c.R, K, F32)
        du, dck, da = Guarded(c.B * S, c.R * c.D, F32), Guarded(c.B * S, c.NQ * c.D, F32), Guarded(c.B * S, c.n, F32)
        entry = L.sc_cls_pool_bwd_det if det else L.sc_cls_pool_bwd
        check(entry(ptr(x_rows), x_rows.stride(0), ptr(cls_d), ptr(hid_d), 0, hid_d.stride(0), c.n, 0, ptr(pk), ptr(dzbar_d), ptr(u_d), ptr(lens_i), ptr(ds.out()),
                    ptr(pp.out()), ptr(du.out()), ptr(dck.out()), ptr(da.out()), c.B, c.T, c.NQ, c.R, c.D, S, 0.1, 5, stream()), c.id)
        torch.cuda.synchronize()
        got = dict(du=du.check(c.id).view(c.B, S, c.R, c.D), dck=dck.check(c.id), dalpha=da.check(c.id).view(c.B, S, c.n),
                   ds=ds.check(c.id).view(c.B, c.R, K), pp=pp.check(c.id).view(c.B, c.R, K))
        if det and True in outs:
            assert all(torch.equal(got[k], outs[True][k]) for k in got), "differs between calls"
        outs[det] = got
    for k in ("dck", "ds", "pp"):
        assert torch.equal(outs[True][k], outs[False][k]), k
    # MAG per block (b, sp): the block owns the keys kk with (kk // 8) % S == sp, kk < NQ + lens[b]
    ds64, pp64 = outs[True]["ds"].abs(), outs[True]["pp"].abs()
    z = torch.cat([cls.double().abs().expand(c.B, c.NQ, c.D), x16.double().abs().view(c.B, c.T, c.D)], 1)          # [B, K, D]
    H = hid.double().abs().view(c.n, c.B, c.T, c.D)
    kk = torch.arange(K)
    mag_du, mag_da = torch.zeros(c.B, S, c.R, c.D, dtype=F64), torch.zeros(c.B, S, c.n, dtype=F64)
    for b in range(c.B):
        for sp in range(S):
            own = ((kk // 8) % S == sp) & (kk < c.NQ + lens[b])
            mag_du[b, sp] = torch.einsum("rk,kd->rd", ds64[b][:, own], z[b][own])
            fr = own & (kk >= c.NQ)
            dz = torch.einsum("rk,rd->kd", pp64[b][:, fr], dzbar[b].double().abs()) + torch.einsum("rk,rd->kd", ds64[b][:, fr], u.double().abs())
            mag_da[b, sp] = torch.einsum("kd,nkd->n", dz, H[:, b][:, fr[c.NQ:]])
    for k, mag in (("du", mag_du), ("dalpha", mag_da)):
        a, b_ = outs[True][k], outs[False][k]
        bound = 1.01 * 14 * T.U * mag
        r = ((a - b_).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"{c.id} {k}: partial rows, |det - default| / (14 U MAG) worst {r:.4f}")
        assert bool(((a - b_).abs() <= bound).all()), (k, r)

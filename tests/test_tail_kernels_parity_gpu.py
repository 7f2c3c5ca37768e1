"""GPU: the fp32 kernels of the trainable tail (csrc/train.hip below the pooling kernels, csrc/infonce.hip, csrc/sgemm.hip, csrc/train_cascaded.hip) against the plain fp64
statements of tests/tail_kernels_ref.py, element by element, under the bounds DERIVED there from the arithmetic (no element is excluded;
tools/tail_kernel_bounds.py is the CPU self-check of statements, bounds and mutants).  Every kernel is called through the C ABI of speechclip_amd._lib / ops, every
output lands in a sentinel-filled buffer, and everything outside the written region must still hold the sentinel bit for bit.  Each case prints its worst
err / bound and where it occurred (-s); profiles/tail_kernels_parity.txt keeps that table.

Which case reaches which code:
    sc_adam_step          adam_kernel: one and several blocks (n 1 / 257 / 100003), steps 1 .. 100000, clip_coef NULL and given (the SECOND float of sc_grad_norm's pair)
    sc_grad_norm          sumsq_kernel one pass per thread (n < 262144) and the grid-stride loop at 1024 blocks (n >= 262144); finish_norm_kernel's max_norm <= 0 branch
    sc_colsum             colsum_kernel with one row chunk (rows < 256, or 512 column blocks and more) and with atomics between chunks; cols % 64 != 0; ld > cols
    sc_layernorm_bwd      ln_bwd_rows_kernel<4> with a partly filled 256-column chunk (D 4 .. 1020), rows 1 .. 33, accumulate_dx; ln_bwd_cols_kernel and its absence
    sc_gelu_f32           gelu_fwd_kernel / gelu_bwd_kernel;   sc_quickgelu_f32: quickgelu_kernel forward f32, forward bf16, backward
    sc_l2norm_bwd, sc_add_rows_f32 (b_rows = rows and 1), sc_mix_softmax_bwd, sc_cosine_bwd_finish (a row below eps), sc_split_hilo_bf16 (nblk 2 / 3, lda > K)
    sc_sgemm / sc_sgemm_batched   sgemm_kernel<TA, TB> x 4, vector and scalar loads (ld % 4, a base pointer one element off), split-K with sgemm_prescale_kernel,
                          blockIdx.z decoded into (batch, k slice), ldc > N
    sc_kw_bn_train_fwd / sc_kw_bn_bwd   one and several blocks of columns (K E = 5 .. 771), running statistics present and NULL
    sc_vq_st_bwd          vq_st_bwd_kernel: V below, at and above the block's 256 threads, V = 49408; 0 / 3 / 8 masked ids with id 0 and id V - 1
    sc_attn_small_bwd     attn_small_bwd_kernel: L 1 .. 16 (L L below and above the 64 lanes), causal and full, peaked rows
    sc_infonce_fwd / sc_infonce_bwd   infonce_tile_kernel / infonce_bwd_kernel on 1 .. 32 x 32 tiles (Bg 1 .. 2048), the k0 + lk < E guard (E = 4, 20), ids NULL /
                          64-bit ids that collide in their low words / an id shared across a tile border / all equal; infonce_final_kernel's out3[1], out3[2];
                          dfeat_a and dfeat_b through ops.infonce_fwd_bwd (two sc_sgemm, split-K at Bg = 2048)"""
import pytest
import torch

import tail_kernels_ref as T
from row_kernels_ref import Guarded, judge as _judge

pytestmark = pytest.mark.gpu
F64, F32, BF = T.F64, T.F32, T.BF


def _d(t):
    return t.to(F32).cuda().contiguous()


def _filled(rows, ld, data=None, dt=F32, width=None):
    go = Guarded(rows, ld, dt, width)
    if data is not None:
        go.out().copy_(data.to(F32).to(dt).cuda().reshape(go.out().shape))
    return go


def _placed(stored, off):
    """a [.., rows, ld] operand as stored, `off` elements into its allocation (off 1: a base pointer that is 4- but not 16-byte aligned)"""
    flat = torch.full((off + stored.numel(),), T.PAST_VALUE, dtype=F32, device="cuda")
    flat[off:] = stored.to(F32).reshape(-1).cuda()
    return flat[off:]


def _check(group, c, run):
    G = T.GROUPS[group]
    inp = G.inputs(c)
    got = run(c, inp)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(got) == set(ref), (c.id, sorted(got), sorted(ref))
    for name, r in ref.items():
        _judge(f"{c.id} {name}", got[name], r, bd[name].bound)
    return got, ref, inp


def _L():
    from speechclip_amd._lib import check, lib, ptr, stream
    return lib(), check, ptr, stream


# ================================================================================================ sc_adam_step
def _run_adam(c, inp):
    L, check, ptr, stream = _L()
    p, m, v = (_filled(1, c.n, inp[k]) for k in "pmv")
    g = _d(inp["g"])
    clip = torch.tensor([T.ADAM_NORM, T.ADAM_COEF], dtype=F32, device="cuda") if c.clip else None
    check(L.sc_adam_step(ptr(p.out()), ptr(g), ptr(m.out()), ptr(v.out()), c.n, (ptr(clip) + 4) if c.clip else 0, T.ADAM_LR, T.ADAM_B1, T.ADAM_B2, T.ADAM_EPS, c.wd,
                         c.step, stream()), c.id)
    return dict(m=m.check(c.id), v=v.check(c.id), step=inp["p"].view(1, -1) - p.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["adam"].cases(), ids=lambda c: c.id)
def test_adam_step_m_v_and_the_step(c):
    _check("adam", c, _run_adam)


# ================================================================================================ sc_grad_norm
def _run_gn(c, inp):
    L, check, ptr, stream = _L()
    g = _d(inp["g"])
    ws = torch.empty(L.sc_grad_norm_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out = Guarded(1, 2, F32)
    check(L.sc_grad_norm(ptr(g), c.n, c.max_norm, ptr(ws), ptr(out.out()), stream()), c.id)
    return dict(out=out.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["gradnorm"].cases(), ids=lambda c: c.id)
def test_grad_norm_and_clip_coefficient(c):
    assert T.gn_blocks(c.n)[1] == ("stride" if c.n >= 262144 else "single")
    _check("gradnorm", c, _run_gn)


# ================================================================================================ sc_colsum
def _run_cs(c, inp):
    L, check, ptr, stream = _L()
    x = _d(inp["x"])
    out = _filled(1, c.cols, inp["out0"])
    check(L.sc_colsum(ptr(x), c.ld, c.rows, c.cols, ptr(out.out()), c.acc, stream()), c.id)
    return dict(out=out.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["colsum"].cases(), ids=lambda c: c.id)
def test_colsum(c):
    _check("colsum", c, _run_cs)


# ================================================================================================ sc_layernorm_bwd
def _run_lb(c, inp):
    L, check, ptr, stream = _L()
    rows, D = inp["x"].shape
    x, dy, gamma = _d(inp["x"]), _d(inp["dy"]), _d(inp["gamma"])
    dx = _filled(rows, D, inp["dx0"] if c.acc else None)
    dg, db = (_filled(1, D, inp["dg0"]), _filled(1, D, inp["db0"])) if c.params else (None, None)
    ws = torch.empty(2 * rows, dtype=F32, device="cuda")
    check(L.sc_layernorm_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(dx.out()), ptr(dg.out()) if dg else 0, ptr(db.out()) if db else 0, ptr(ws), rows, D, T.LN_EPS,
                             int(c.acc), stream()), c.id)
    out = dict(dx=dx.check(c.id))
    if c.params:
        out["dgamma"], out["dbeta"] = dg.check(c.id), db.check(c.id)
    return out


@pytest.mark.parametrize("c", T.lb_cases(), ids=lambda c: c.id)
def test_layernorm_bwd(c):
    for v in T.lbv_cases():
        if v.base == c:
            _check("lnbwd", v, _run_lb)


# ================================================================================================ sc_gelu_f32 / sc_quickgelu_f32
def _run_act(c, inp):
    L, check, ptr, stream = _L()
    z = _d(inp["z"])
    bwd, bf = c.kind.endswith("bwd"), c.kind == "qgelu_fwd_bf16"
    io = _filled(1, c.n, inp["dh"] if bwd else None, BF if bf else F32)
    if c.kind.startswith("gelu"):
        check(L.sc_gelu_f32(ptr(z), ptr(io.out()), c.n, int(bwd), stream()), c.id)
    else:
        check(L.sc_quickgelu_f32(ptr(z), ptr(io.out()), c.n, int(bwd), int(bf), stream()), c.id)
    return dict(out=io.check(c.id).reshape(-1))


@pytest.mark.parametrize("c", T.GROUPS["act"].cases(), ids=lambda c: c.id)
def test_gelu_and_quickgelu(c):
    _check("act", c, _run_act)


# ================================================================================================ the small row kernels
def _run_l2b(c, inp):
    L, check, ptr, stream = _L()
    dx, x, dy = Guarded(c.rows, c.D, F32), _d(inp["x"]), _d(inp["dy"])
    check(L.sc_l2norm_bwd(ptr(x), ptr(dy), ptr(dx.out()), c.rows, c.D, stream()), c.id)
    return dict(dx=dx.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["l2bwd"].cases(), ids=lambda c: c.id)
def test_l2norm_bwd(c):
    _check("l2bwd", c, _run_l2b)


def _run_add(c, inp):
    L, check, ptr, stream = _L()
    out, a, b = Guarded(c.rows, c.D, F32), _d(inp["a"]), _d(inp["b"])
    check(L.sc_add_rows_f32(ptr(a), ptr(b), ptr(out.out()), c.rows, c.D, inp["b"].shape[0], T.ADD_ALPHA, stream()), c.id)
    return dict(out=out.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["addrows"].cases(), ids=lambda c: c.id)
def test_add_rows(c):
    _check("addrows", c, _run_add)


def _run_mix(c, inp):
    L, check, ptr, stream = _L()
    dw, w, da = _filled(1, c.D, inp["dw0"]), _d(inp["w"]), _d(inp["da"])
    check(L.sc_mix_softmax_bwd(ptr(w), ptr(da), c.rows, c.D, ptr(dw.out()), stream()), c.id)
    return dict(dw=dw.check(c.id).reshape(-1))


@pytest.mark.parametrize("c", T.GROUPS["mixbwd"].cases(), ids=lambda c: c.id)
def test_mix_softmax_bwd(c):
    _check("mixbwd", c, _run_mix)


def _run_cos(c, inp):
    L, check, ptr, stream = _L()
    da, a, G, rd = Guarded(c.rows, c.D, F32), _d(inp["a"]), _d(inp["G"]), _d(inp["rd"])
    check(L.sc_cosine_bwd_finish(ptr(a), ptr(G), ptr(rd), ptr(da.out()), c.rows, c.D, T.COS_EPS, stream()), c.id)
    return dict(da=da.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["cosfin"].cases(), ids=lambda c: c.id)
def test_cosine_bwd_finish(c):
    assert float(T.GROUPS["cosfin"].inputs(c)["a"][-1].norm()) < T.COS_EPS          # the clamped row is in every case
    _check("cosfin", c, _run_cos)


def _run_hilo(c, inp):
    L, check, ptr, stream = _L()
    nblk, lda = c.opt
    K = c.D
    buf = torch.full((c.rows, lda), T.PAST_VALUE, dtype=F32, device="cuda")
    buf[:, :K] = _d(inp["a"])
    out = Guarded(c.rows, nblk * K, BF)
    check(L.sc_split_hilo_bf16(ptr(buf), lda, ptr(out.out()), c.rows, K, nblk, stream()), c.id)
    o = out.check(c.id)
    if nblk == 3:
        assert torch.equal(o[:, 2 * K:], o[:, :K]), (c.id, "block 3 is not hi")
    return dict(hi=o[:, :K], sum=o[:, :K] + o[:, K:2 * K])


@pytest.mark.parametrize("c", T.GROUPS["hilo"].cases(), ids=lambda c: c.id)
def test_split_hilo(c):
    got, ref, inp = _check("hilo", c, _run_hilo)
    a = inp["a"]
    assert torch.equal(got["hi"].to(F32).to(BF).view(torch.int16), a.to(F32).to(BF).view(torch.int16)), (c.id, "hi is not bf16(a) bit for bit")
    assert bool(((got["sum"] - a).abs() <= T.HILO_STATED * a.abs()).all()), (c.id, "hi + lo outside 2^-16 1.001 |a|")


# ================================================================================================ sc_sgemm / sc_sgemm_batched
def _run_gemm(c, inp):
    L, check, ptr, stream = _L()
    off = 1 if c.layout == "off1" else 0
    A, B = _placed(inp["A"], off), _placed(inp["B"], off)
    lda, ldb = inp["A"].shape[-1], inp["B"].shape[-1]
    sA, sB = inp["A"].shape[1] * lda, inp["B"].shape[1] * ldb
    assert (A.data_ptr() % 16 == 0) == (off == 0) and (lda % 4 == 0) == (c.layout != "ldodd")
    ldc = c.N + 3 if c.ldc_pad else c.N
    C = _filled(c.batch * c.M, ldc, inp["C0"].reshape(c.batch * c.M, c.N), width=c.N)
    bias = _d(inp["bias"]) if c.bias else None
    if c.batch == 1:
        check(L.sc_sgemm(int(c.ta), int(c.tb), c.M, c.N, c.K, c.alpha, ptr(A), lda, ptr(B), ldb, c.beta, ptr(C.out()), ldc, ptr(bias), stream()), c.id)
    else:
        check(L.sc_sgemm_batched(int(c.ta), int(c.tb), c.M, c.N, c.K, c.alpha, ptr(A), lda, sA, ptr(B), ldb, sB, c.beta, ptr(C.out()), ldc, c.M * ldc, ptr(bias),
                                 c.N if c.bias else 0, c.batch, stream()), c.id)
    return dict(C=C.check(c.id).view(c.batch, c.M, c.N))


@pytest.mark.parametrize("c", T.GROUPS["sgemm"].cases(), ids=lambda c: c.id)
def test_sgemm_every_transpose_layout_and_split(c):
    _check("sgemm", c, _run_gemm)


# ================================================================================================ sc_kw_bn_train_fwd / sc_kw_bn_bwd
def _run_kb(c, inp):
    L, check, ptr, stream = _L()
    C = c.K * c.E
    x, dy, gamma, beta, m32, rs32 = (_d(inp[k]) for k in ("x", "dy", "gamma", "beta", "mean32", "rstd32"))
    y, mean, rstd = Guarded(c.B, C, F32), Guarded(1, C, F32), Guarded(1, C, F32)
    rm, rv = (_filled(1, C, inp["rm0"]), _filled(1, C, inp["rv0"])) if c.running else (None, None)
    check(L.sc_kw_bn_train_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y.out()), ptr(mean.out()), ptr(rstd.out()), ptr(rm.out()) if rm else 0, ptr(rv.out()) if rv else 0,
                               c.B, c.K, c.E, T.KB_MOM, T.KB_EPS, stream()), c.id)
    dx, dg, db = Guarded(c.B, C, F32), Guarded(1, C, F32), Guarded(1, C, F32)
    check(L.sc_kw_bn_bwd(ptr(x), ptr(dy), ptr(gamma), ptr(m32), ptr(rs32), ptr(dx.out()), ptr(dg.out()), ptr(db.out()), c.B, c.K, c.E, stream()), c.id)
    out = dict(y=y.check(c.id), mean=mean.check(c.id), rstd=rstd.check(c.id), dx=dx.check(c.id), dgamma=dg.check(c.id), dbeta=db.check(c.id))
    if c.running:
        out["run_mean"], out["run_var"] = rm.check(c.id), rv.check(c.id)
    return out


@pytest.mark.parametrize("c", T.GROUPS["kwbn"].cases(), ids=lambda c: c.id)
def test_kw_batchnorm_train_fwd_and_bwd(c):
    _check("kwbn", c, _run_kb)


# ================================================================================================ sc_vq_st_bwd
def _run_vq(c, inp):
    import ctypes
    L, check, ptr, stream = _L()
    cos = _d(inp["cos"])
    g = _filled(c.R, c.V, inp["g"])
    rowdot = Guarded(1, c.R, F32)
    ids = T.vq_mask_ids(c)
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    check(L.sc_vq_st_bwd(ptr(cos), ptr(g.out()), ptr(rowdot.out()), c.R, c.V, c.temp, ctypes.cast(arr, ctypes.c_void_p), len(ids), stream()), c.id)
    return dict(dcos=g.check(c.id), rowdot=rowdot.check(c.id).reshape(-1))


@pytest.mark.parametrize("c", T.GROUPS["vqst"].cases(), ids=lambda c: c.id)
def test_vq_straight_through_bwd(c):
    ids = T.vq_mask_ids(c)
    assert len(ids) == c.nmask and (c.nmask == 0 or {0, c.V - 1} <= set(ids))
    _check("vqst", c, _run_vq)


# ================================================================================================ sc_attn_small_bwd
def _run_at(c, inp):
    L, check, ptr, stream = _L()
    W = c.H * 64
    qkv, dout = inp["qkv"].to(F32).to(BF).cuda().contiguous(), _d(inp["dout"])
    dqkv = Guarded(c.B * c.L, 3 * W, F32)
    check(L.sc_attn_small_bwd(ptr(qkv), ptr(dout), ptr(dqkv.out()), c.B, c.L, c.H, 64, int(c.causal), stream()), c.id)
    return dict(dqkv=dqkv.check(c.id))


@pytest.mark.parametrize("c", T.GROUPS["attnbwd"].cases(), ids=lambda c: c.id)
def test_attn_small_bwd(c):
    _check("attnbwd", c, _run_at)


# ================================================================================================ sc_infonce_fwd + sc_infonce_bwd, and dfeat through ops.infonce_fwd_bwd
def _run_nce(c, inp):
    from speechclip_amd import ops
    L, check, ptr, stream = _L()
    a, b = _d(inp["a"]), _d(inp["b"])
    ids = inp["ids"].cuda() if "ids" in inp else None                     # the backward runs with ids = NULL in every "none" case
    ws = torch.empty(L.sc_infonce_workspace_bytes(c.Bg), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(L.sc_infonce_bwd_workspace_bytes(c.Bg), dtype=torch.uint8, device="cuda")
    out3, G, dinv = Guarded(1, 3, F32), Guarded(c.Bg, c.Bg, F32), Guarded(1, 1, F32)
    args = (c.Bg, c.E, c.inv_t, c.margin, int(c.dcl), int(c.a2b), int(c.b2a), stream())
    check(L.sc_infonce_fwd(ptr(a), ptr(b), ptr(ids), ptr(ws), ptr(out3.out()), *args), c.id)
    check(L.sc_infonce_bwd(ptr(a), ptr(b), ptr(ids), ptr(ws), ptr(ws2), ptr(G.out()), ptr(dinv.out()), *args), c.id)
    o3, da, dv, db = ops.infonce_fwd_bwd(a, b, ids, c.inv_t, c.margin, c.dcl, c.a2b, c.b2a, want_dfeat_b=True)
    got = dict(out3=out3.check(c.id).reshape(-1), G=G.check(c.id), dinv=dinv.check(c.id).reshape(-1), dfeat_a=da.cpu().to(F64), dfeat_b=db.cpu().to(F64))
    assert torch.equal(o3.cpu().to(F64), got["out3"]) and torch.equal(dv.cpu().to(F64), got["dinv"]), (c.id, "ops.infonce_fwd_bwd and the C ABI disagree")
    return got


@pytest.mark.parametrize("c", T.GROUPS["infonce"].cases(), ids=lambda c: c.id)
def test_infonce_loss_G_dinv_and_dfeat(c):
    inp = T.nce_inputs(c)
    assert c.inv_t * float((inp["a"] @ inp["b"].t()).max()) < 80
    _check("infonce", c, _run_nce)

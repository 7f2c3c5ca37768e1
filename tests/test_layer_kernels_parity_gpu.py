"""GPU: the bf16 kernels of the layer-training path (csrc/train_hubert.hip apart from its attention kernels) and train_hubert.wgrad against the plain fp64 statements of
tests/layer_kernels_ref.py, element by element, under the bounds DERIVED there from the arithmetic (no element is excluded; tools/layer_kernel_bounds.py is the CPU
self-check of statements, bounds and mutants).  Every kernel is called through the C ABI of speechclip_amd._lib -- lib() directly wherever the ops wrapper hides an
argument (ld, ld_dz, accumulate, a caller-owned part / ws) -- every output lands in a sentinel-filled buffer, and everything outside the written region must still
hold the sentinel bit for bit.  Each case prints its worst err / bound and where it occurred (-s); profiles/layer_kernels_parity.txt keeps that table.

Which case reaches which code (the case ids carry the path):
    sc_layernorm_bwd_bf16   ln_bwd_bf16_kernel (D % 256 != 0: nd 1 / 3 / 15) and ln_bwd_bf16_vec_kernel (ng 1 / 3 / 4); 4 rows per block below 4096 rows and 32 from
                            there on; a chunk with fewer rows than waves, a last chunk of one row, a last chunk that is not full; x and dy are followed by a row of
                            PAST_VALUE, part holds exactly sc_layernorm_bwd_bf16_partials(rows) rows; dx, the raw partial rows, dgamma and dbeta (ops.colsum of the
                            partials, as the wrapper forms them) are judged each on its own, dx also by its slope per row
    sc_gelu_bwd_bf16        all 65280 finite bf16 values of u; the 16-byte lanes and the pairwise tail of 2, 4 and 6 elements at the first and the second block
    sc_colsum_bf16          64 and 128 rows per block (65536 rows), stage 2's eightfold loop and its tail, rows % 4, ld > cols, accumulate 0 / 1, a guarded workspace of
                            exactly sc_colsum_bf16_workspace_bytes; two calls give equal bits
    sc_axpy_bf16            one and several blocks, the last block partly filled, four values of alpha; x unchanged; slope
    sc_cls_pool_dz          NQ 1 / 2, R 1 .. 8, D below and above a block's 256 threads, lens 0 / T / between, ld_dz > D
    sc_transpose_bf16       bit for bit: both sides of the 64-tile edge, three paddings, batches; the 8-byte form and each of its conditions failing alone; the
                            overlapping-row view; ld_out > rows_padded and the side-by-side placement
    train_hubert.wgrad      bit for bit on integer operands on both sides of every clause of the split rule; one real-valued case per path under a derived bound
The argument rules of include/speechclip_hip.h are tested as refusals (only arguments the entry's code refuses before any launch, never a pointer outside an
allocation), and calls of size zero must return 0 and touch nothing."""
import pytest
import torch

import layer_kernels_ref as R
from row_kernels_ref import GUARD, Guarded, judge as _judge

pytestmark = pytest.mark.gpu
F64, F32, BF = R.F64, R.F32, R.BF


def _L():
    from speechclip_amd._lib import check, lib, ptr, stream
    return lib(), check, ptr, stream


def _bf(t):
    return t.to(F32).to(BF).cuda().contiguous()


def _f(t):
    return t.to(F32).cuda().contiguous()


def _with_past_row(t):
    """a bf16 [rows, ld] operand followed by one row of PAST_VALUE: reading row `rows` is loud"""
    buf = torch.full((t.shape[0] + 1, t.shape[1]), R.PAST_VALUE, dtype=BF, device="cuda")
    buf[:t.shape[0]] = _bf(t)
    return buf


def _filled(rows, ld, data, dt, width=None):
    go = Guarded(rows, ld, dt, width)
    go.out().copy_(data.to(F32).to(dt).cuda().reshape(go.out().shape))
    return go


def _judge_all(c, G, got, inp):
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(got) == set(ref), (c.id, sorted(got), sorted(ref))
    for name, r in ref.items():
        _judge(f"{c.id} {name}", got[name], r, bd[name].bound)
    return ref, bd


def _slope(what, got, ref, pre):
    ratio, row, allow = R.slope_check(got, ref, pre)
    print(f"{what + ' slope':72s} worst slope difference / allowance {ratio:8.4f} (row {row}; smallest allowance {allow:.3g})")
    assert ratio <= 1.0, (what, "slope difference / allowance", ratio, "row", row)


def _refused(rc, name):
    L = _L()[0]
    msg = L.sc_last_error().decode()
    assert rc != 0 and name in msg, (name, rc, msg)


# ================================================================================================ sc_layernorm_bwd_bf16
def _run_lnb(c, inp):
    from speechclip_amd import ops
    L, check, ptr, stream = _L()
    nparts = int(L.sc_layernorm_bwd_bf16_partials(c.rows))
    assert nparts == R.lnb_partials(c.rows)[0]
    x, dy, gamma = _with_past_row(inp["x"]), _with_past_row(inp["dy"]), _f(inp["gamma"])
    dx, part = Guarded(c.rows, c.D, BF), Guarded(nparts, 2 * c.D, F32)
    check(L.sc_layernorm_bwd_bf16(ptr(x), ptr(dy), ptr(gamma), ptr(dx.out()), ptr(part.out()), c.rows, c.D, R.LN_EPS, stream()), c.id)
    sums = ops.colsum(part.out()).cpu().to(F64)                 # as ops.layernorm_bwd_bf16 forms dgamma and dbeta
    return dict(dx=dx.check(c.id), part=part.check(c.id).view(nparts, 2, c.D), dgamma=sums[:c.D], dbeta=sums[c.D:])


@pytest.mark.parametrize("c", R.lnb_cases(), ids=lambda c: c.id)
def test_layernorm_bwd_bf16(c):
    assert c.kern == ("vec" if c.D % 256 == 0 else "scalar") and c.rpb == (32 if c.rows >= 4096 else 4)
    inp = R.lnb_inputs(c)
    assert bool((inp["gamma"] == 0).sum() == 1) and bool((inp["gamma"] < 0).any()) and bool((inp["gamma"] > 0).any())
    got = _run_lnb(c, inp)
    ref, _ = _judge_all(c, R.GROUPS["ln_bwd"], got, inp)
    if c.rows >= 4:
        _slope(c.id + " dx", got["dx"], ref["dx"], R.lnb_pre(c, inp)["dx"])


# ================================================================================================ sc_gelu_bwd_bf16
def _run_gb(c, inp):
    L, check, ptr, stream = _L()
    u, dh, du = _bf(inp["u"]), _bf(inp["dh"]), Guarded(1, c.n, BF)
    check(L.sc_gelu_bwd_bf16(ptr(u), ptr(dh), ptr(du.out()), c.n, stream()), c.id)
    return dict(du=du.check(c.id).reshape(-1))


@pytest.mark.parametrize("c", R.gb_cases(), ids=lambda c: c.id)
def test_gelu_bwd_bf16(c):
    inp = R.gb_inputs(c)
    if c.kind == "allbits":
        bits = inp["u"].to(F32).to(BF).view(torch.int16).to(torch.int32) & 0xffff
        assert c.n == 65280 and bits.unique().numel() == 65280 and bool(torch.isfinite(inp["u"]).all())
    got = _run_gb(c, inp)
    ref, _ = _judge_all(c, R.GROUPS["gelu_bwd"], got, inp)          # (the judge asserts that every output is finite)
    if c.kind == "slope":
        assert float(inp["u"].abs().max()) <= 4
        _slope(c.id + " du", got["du"], ref["du"], R.gb_pre(c, inp))


def test_gelu_bwd_bf16_argument_rules():
    L, check, ptr, stream = _L()
    buf = torch.zeros(3, 64, dtype=BF, device="cuda")
    _refused(L.sc_gelu_bwd_bf16(ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), 7, stream()), "sc_gelu_bwd_bf16")
    for k in range(3):          # each operand in turn 4 bytes into its row: not 16-byte aligned
        ops_ = [buf[j][2:] if j == k else buf[j] for j in range(3)]
        _refused(L.sc_gelu_bwd_bf16(ptr(ops_[0]), ptr(ops_[1]), ptr(ops_[2]), 8, stream()), "sc_gelu_bwd_bf16")
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


# ================================================================================================ sc_colsum_bf16
def _run_cb(c, inp):
    L, check, ptr, stream = _L()
    nbytes = int(L.sc_colsum_bf16_workspace_bytes(c.rows, c.cols))
    assert nbytes == R.cb_workspace_bytes(c.rows, c.cols)
    x = _with_past_row(inp["x"])
    outs = []
    for _ in range(2):
        ws, out = Guarded(1, nbytes // 4, F32), _filled(1, c.cols, inp["out0"], F32)
        check(L.sc_colsum_bf16(ptr(x), c.ld, c.rows, c.cols, ptr(ws.out()), ptr(out.out()), c.acc, stream()), c.id)
        ws.check(c.id + " ws")
        outs.append(out.check(c.id).reshape(-1))
    assert torch.equal(outs[0], outs[1]), (c.id, "two calls differ: the entry is stated deterministic")
    return dict(out=outs[0])


@pytest.mark.parametrize("rows", R.CB_ROWS_SMALL + R.CB_ROWS_LARGE)
def test_colsum_bf16(rows):
    cases = [c for c in R.cb_cases() if c.rows == rows]
    assert {c.acc for c in cases} == {0, 1} and {c.ld > c.cols for c in cases} == {False, True}
    for c in cases:
        inp = R.cb_inputs(c)
        _judge_all(c, R.GROUPS["colsum16"], _run_cb(c, inp), inp)


# ================================================================================================ sc_axpy_bf16
def _run_ax(c, inp):
    L, check, ptr, stream = _L()
    x, y = _bf(inp["x"]), _filled(1, c.n, inp["y"], BF)
    x0 = x.clone()
    check(L.sc_axpy_bf16(ptr(y.out()), ptr(x), c.alpha, c.n, stream()), c.id)
    out = y.check(c.id).reshape(-1)
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16)), (c.id, "x changed")
    return dict(y=out)


@pytest.mark.parametrize("c", R.ax_cases(), ids=lambda c: c.id)
def test_axpy_bf16(c):
    inp = R.ax_inputs(c)
    got = _run_ax(c, inp)
    ref, bd = _judge_all(c, R.GROUPS["axpy"], got, inp)
    if c.alpha == 0.0:
        assert torch.equal(got["y"], inp["y"]), (c.id, "alpha = 0 changed y")
    if c.n >= 510:
        _slope(c.id + " y", got["y"], ref["y"], bd["y"].bound - bd["y"].store)


# ================================================================================================ sc_cls_pool_dz
def _run_pz(c, inp):
    L, check, ptr, stream = _L()
    pp, ds, dzbar, u = (_f(inp[k]) for k in ("pp", "ds", "dzbar", "u"))
    lens = torch.tensor(c.lens, dtype=torch.int32, device="cuda")
    dz = Guarded(c.B * c.T, c.ld_dz, BF, width=c.D)
    check(L.sc_cls_pool_dz(ptr(pp), ptr(ds), ptr(dzbar), ptr(u), ptr(lens), ptr(dz.out()), c.B, c.T, c.NQ, c.R, c.D, c.ld_dz, stream()), c.id)
    return dict(dz=dz.check(c.id))


@pytest.mark.parametrize("c", R.pz_cases(), ids=lambda c: c.id)
def test_cls_pool_dz(c):
    inp = R.pz_inputs(c)
    assert bool((inp["pp"][:, :, :c.NQ] == R.PAST_VALUE).all()) and bool((inp["ds"][:, :, :c.NQ] == R.PAST_VALUE).all())
    got = _run_pz(c, inp)
    _judge_all(c, R.GROUPS["cls_pool_dz"], got, inp)
    dz = got["dz"].view(c.B, c.T, c.D)
    for b, n in enumerate(c.lens):
        assert bool((dz[b, n:] == 0).all()), (c.id, "a row at t >= lens[b] is not exactly zero", b)


def test_cls_pool_dz_case_list_holds_the_lengths():
    lens = {(n, c.T) for c in R.pz_cases() for n in c.lens}
    assert any(n == 0 for n, _ in lens) and any(n == T for n, T in lens) and any(0 < n < T for n, T in lens)
    assert {(c.B, c.T, c.NQ, c.R, c.D) for c in R.pz_cases()} == set(R.PZ_SHAPES) and {c.ld_dz - c.D for c in R.pz_cases()} == {0, 8}


# ================================================================================================ sc_transpose_bf16
def _run_tr(c):
    """-> None; asserts the whole output allocation bit for bit: the transposed matrices, exact zeros in the pad columns, the sentinel everywhere else"""
    L, check, ptr, stream = _L()
    flat = R.tr_input(c)
    src = flat.cuda().view(BF)
    n_out = c.out_off + (c.batch - 1) * c.stride_out + (c.C - 1) * c.ld_out + c.Rp
    sent = int(torch.tensor(R.SENT16, dtype=BF).view(torch.int16))
    want = torch.full((2 * GUARD + n_out,), sent, dtype=torch.int16)
    ref = R.tr_ref(c, flat)
    col, r = torch.arange(c.C).view(-1, 1), torch.arange(c.Rp).view(1, -1)
    for z in range(c.batch):
        want[GUARD + c.out_off + z * c.stride_out + col * c.ld_out + r] = ref[z]
    buf = torch.full((2 * GUARD + n_out,), R.SENT16, dtype=BF, device="cuda")
    i_ptr, o_ptr = ptr(src) + 2 * c.in_off, ptr(buf) + 2 * (GUARD + c.out_off)
    assert (i_ptr % 8 == 0) == (c.in_off % 4 == 0) and (o_ptr % 8 == 0) == (c.out_off % 4 == 0)
    check(L.sc_transpose_bf16(i_ptr, c.ld_in, c.stride_in, o_ptr, c.ld_out, c.stride_out, c.R, c.C, c.Rp, c.batch, stream()), c.id)
    got = buf.cpu().view(torch.int16)
    bad = (got != want).nonzero()
    print(f"{c.id:72s} bit for bit: {int(bad.numel())} of {got.numel()} elements differ")
    assert bad.numel() == 0, (c.id, "first difference at flat element", int(bad[0]) - GUARD, "got", int(got[bad[0]]), "want", int(want[bad[0]]))


@pytest.mark.parametrize("Rr", R.TR_RC)
def test_transpose_bf16_tile_edges_paddings_batches(Rr):
    cases = [c for c in R.tr_grid_cases() if c.R == Rr]
    assert {c.C for c in cases} == set(R.TR_RC) and {c.batch for c in cases} == {1, 3} and {c.Rp for c in cases} == set(R.tr_pads(Rr))
    for c in cases:
        _run_tr(c)


@pytest.mark.parametrize("c", R.tr_vector_cases(), ids=lambda c: c.id)
def test_transpose_bf16_vector_form_and_each_condition_failing(c):
    _run_tr(c)


# ================================================================================================ train_hubert.wgrad
@pytest.mark.parametrize("M,N,K", R.wg_exact_shapes(), ids=lambda v: str(v))
def test_wgrad_exact_integers(M, N, K):
    from speechclip_amd.train_hubert import wgrad
    dy, x = R.wg_int_inputs(M, N, K)
    got = wgrad(dy.cuda().to(BF), x.cuda().to(BF)).cpu()
    ref = dy.to(F32).t() @ x.to(F32)                      # integers below 2^24: exact in fp32 in any order
    assert float(ref.abs().max()) < 2 ** 24 and 9 * M < 2 ** 24
    bad = int((got != ref).sum())
    print(f"{R.wg_id(M, N, K, 'exact'):72s} bit for bit: {bad} of {ref.numel()} elements differ")
    assert got.dtype == F32 and got.shape == (N, K) and bad == 0


@pytest.mark.parametrize("c", R.wg_cases(), ids=lambda c: c.id)
def test_wgrad_real_values(c):
    from speechclip_amd.train_hubert import wgrad
    inp = R.wg_inputs(c)
    got = wgrad(_bf(inp["dy"]), _bf(inp["x"])).cpu().to(F64)
    _judge_all(c, R.GROUPS["wgrad"], dict(dW=got), inp)


def test_wgrad_case_list_reaches_every_clause():
    shapes = R.wg_exact_shapes()
    clauses = {R.wg_clause(*s) for s in shapes}
    assert clauses >= {"below4096", "rows", "tiles"} and any(R.wg_split(*s)[0] == 32 for s in shapes)
    assert R.wg_split(*R.WG_BINDING)[0] == 3 and R.WG_BINDING[0] // 2048 == 4
    assert any(R.wg_split(*s)[2] != s[0] and R.wg_split(*s)[0] > 1 for s in shapes)                      # zero padding of the last chunk, several splits
    assert {R.wg_split(*s)[3] for s in shapes} == {128, 256} and {R.wg_split(c.M, c.N, c.K)[0] > 1 for c in R.wg_cases()} == {False, True}


# ================================================================================================ argument rules and calls of size zero
def test_layernorm_bwd_bf16_argument_rules():
    L, check, ptr, stream = _L()
    D = 256
    x, dy, dx = (torch.zeros(4 * D + 8, dtype=BF, device="cuda") for _ in range(3))
    gamma, part = torch.ones(D, device="cuda"), torch.zeros(2 * D, device="cuda")
    args = [x, dy, gamma, dx, part]
    _refused(L.sc_layernorm_bwd_bf16(ptr(x), ptr(dy), ptr(gamma), ptr(dx), ptr(part), 4, 96, 1e-5, stream()), "sc_layernorm_bwd_bf16")      # D % 64
    _refused(L.sc_layernorm_bwd_bf16(ptr(x), ptr(dy), ptr(gamma), ptr(dx), ptr(part), 4, 1088, 1e-5, stream()), "sc_layernorm_bwd_bf16")    # D > 1024
    for k in range(5):                                                                                          # each operand null in turn
        p = [0 if j == k else ptr(a) for j, a in enumerate(args)]
        _refused(L.sc_layernorm_bwd_bf16(p[0], p[1], p[2], p[3], p[4], 4, D, 1e-5, stream()), "sc_layernorm_bwd_bf16")
    for k in (0, 1, 3):                                                                                         # x, dy, dx 4 bytes off an 8-byte boundary, D % 256 == 0
        p = [ptr(a[2:]) if j == k else ptr(a) for j, a in enumerate(args)]
        _refused(L.sc_layernorm_bwd_bf16(p[0], p[1], p[2], p[3], p[4], 4, D, 1e-5, stream()), "sc_layernorm_bwd_bf16")
    torch.cuda.synchronize()
    assert bool((dx == 0).all()) and bool((part == 0).all())


def test_layernorm_bwd_bf16_scalar_kernel_takes_a_4_byte_aligned_view():
    """the alignment rule belongs to the 8-byte kernel alone: D = 192 runs from views 2 elements into their allocations, same values"""
    L, check, ptr, stream = _L()
    c = [k for k in R.lnb_cases() if k.D == 192 and k.rows == 5][0]
    inp = R.lnb_inputs(c)
    nparts = R.lnb_partials(c.rows)[0]
    x, dy = (torch.cat([torch.full((2,), R.PAST_VALUE, dtype=BF, device="cuda"), _bf(inp[k]).reshape(-1)]) for k in ("x", "dy"))
    dx, part = Guarded(c.rows, c.D + 2, BF), Guarded(nparts, 2 * c.D, F32)
    o = dx.buf[GUARD + 2:GUARD + 2 + c.rows * c.D]
    gamma = _f(inp["gamma"])
    assert ptr(x[2:]) % 8 == 4 and ptr(o) % 8 == 4
    check(L.sc_layernorm_bwd_bf16(ptr(x[2:]), ptr(dy[2:]), ptr(gamma), ptr(o), ptr(part.out()), c.rows, c.D, R.LN_EPS, stream()), c.id)
    ref, bd = R.lnb_ref(c, inp), R.lnb_bound(c, inp)
    _judge(f"{c.id} dx (views 4 bytes off)", o.cpu().to(F64).view(c.rows, c.D), ref["dx"], bd["dx"].bound)
    _judge(f"{c.id} part (views 4 bytes off)", part.check(c.id).view(nparts, 2, c.D), ref["part"], bd["part"].bound)


def test_colsum_bf16_and_axpy_bf16_argument_rules():
    L, check, ptr, stream = _L()
    x = torch.zeros(8, 16, dtype=BF, device="cuda")
    ws, out = torch.zeros(64, device="cuda"), torch.zeros(16, device="cuda")
    _refused(L.sc_colsum_bf16(0, 16, 8, 16, ptr(ws), ptr(out), 0, stream()), "sc_colsum_bf16")
    _refused(L.sc_colsum_bf16(ptr(x), 16, 8, 16, 0, ptr(out), 0, stream()), "sc_colsum_bf16")
    _refused(L.sc_colsum_bf16(ptr(x), 16, 8, 16, ptr(ws), 0, 0, stream()), "sc_colsum_bf16")
    _refused(L.sc_colsum_bf16(ptr(x), 15, 8, 16, ptr(ws), ptr(out), 0, stream()), "sc_colsum_bf16")                 # ld < cols
    _refused(L.sc_colsum_bf16(ptr(x), 2 ** 31 - 1, 1, 65535 * 256 + 1, ptr(ws), ptr(out), 0, stream()), "sc_colsum_bf16")   # more column blocks than a grid holds
    y = torch.zeros(64, dtype=BF, device="cuda")
    xv = torch.ones(64, dtype=BF, device="cuda")
    _refused(L.sc_axpy_bf16(ptr(y), ptr(xv), 1.0, 7, stream()), "sc_axpy_bf16")                                     # odd n
    _refused(L.sc_axpy_bf16(0, ptr(xv), 1.0, 8, stream()), "sc_axpy_bf16")
    _refused(L.sc_axpy_bf16(ptr(y), 0, 1.0, 8, stream()), "sc_axpy_bf16")
    _refused(L.sc_axpy_bf16(ptr(y[1:]), ptr(xv), 1.0, 8, stream()), "sc_axpy_bf16")                                 # 2 bytes off a 4-byte boundary
    _refused(L.sc_axpy_bf16(ptr(y), ptr(xv[1:]), 1.0, 8, stream()), "sc_axpy_bf16")
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((ws == 0).all()) and bool((y == 0).all())


def test_zero_size_calls_return_0_and_touch_nothing():
    L, check, ptr, stream = _L()
    x = torch.ones(4, 64, dtype=BF, device="cuda")
    g = torch.ones(64, device="cuda")
    dx, part, ws, out, y, du = Guarded(4, 64, BF), Guarded(1, 128, F32), Guarded(1, 64, F32), Guarded(1, 64, F32), Guarded(1, 64, BF), Guarded(1, 64, BF)
    assert L.sc_layernorm_bwd_bf16(ptr(x), ptr(x), ptr(g), ptr(dx.out()), ptr(part.out()), 0, 64, 1e-5, stream()) == 0
    assert L.sc_colsum_bf16(ptr(x), 64, 0, 64, ptr(ws.out()), ptr(out.out()), 0, stream()) == 0
    assert L.sc_colsum_bf16(ptr(x), 64, 4, 0, ptr(ws.out()), ptr(out.out()), 1, stream()) == 0
    assert L.sc_axpy_bf16(ptr(y.out()), ptr(x), 2.0, 0, stream()) == 0
    assert L.sc_gelu_bwd_bf16(ptr(x), ptr(x), ptr(du.out()), 0, stream()) == 0
    for name, go in (("dx", dx), ("part", part), ("ws", ws), ("out", out), ("y", y), ("du", du)):
        assert bool((go.check(name) == go.sent).all()), (name, "a call of size zero wrote its output")

"""GPU: the forward kernels of the cascaded branch (csrc/cascaded.hip) and the two analysis kernels (csrc/analysis.hip) through their C entries, and the host chain
ops.cosine_scores(exact=False), against the plain fp64 statements of tests/cascaded_fwd_ref.py: bit for bit where the statement is a copy, an integer or exact arithmetic,
element by element under bounds DERIVED there everywhere else (no element is excluded; tools/cascaded_fwd_bounds.py is the CPU self-check of statements, emulations, bounds
and mutants).  Operands sit between NaN runs (score rows with ld > m: PAST_VALUE behind the row; padded keys: NaN), outputs and workspaces in sentinel-filled guarded
windows, and everything outside the written region must still hold the sentinel.  Each test prints, per case, the worst err / bound and where it occurred, or the bitwise
verdict (-s).  The first-generation tests (tests/test_cascaded_gpu.py, tests/test_analysis_gpu.py) stay where they are.

Which case reaches which code:
    sc_kw_affine            kw_affine_kernel          kwaffine/total1 / 255 / 256 / 257 / 703: one thread, a part-filled block, a full one, one thread of a second block, three
                            blocks; K 1 and 8, rows % K != 0 (15 and 19 rows), D 1 / 17 / 37 / 64 / 257
    sc_cosine_scores        row_inv_norm_kernel + cosine_tile_kernel   cosine/real-* and cosine/int-*: R and V at 1 / 63 / 64 / 65 / 130 (one tile, a part-filled one, the
                            tail of a second and of a third in both grid axes), E 4 / 20 (the part-filled KC chunk) / 64 / 516; a zero row, a row below eps and rows at
                            2^-20 / 2^20 on each side; int: every operation exact, bit for bit.  The (R + V) float workspace is a guarded window.
    sc_cosine_refine[_masked]   cosine_refine_kernel  refine/*: E 4 / 64 / 260 / 512 (the 256-strided loops with 1, 1, 2 and 2 trips; the tail of the second), V 5 / 256 / 257 /
                            1031; 1, 2, 127, 128 candidates: the one-sweep path; 129, 300 and every column: the in-order chunk walk (V 256: one chunk, 257: a one-column second
                            chunk, 1031: five); delta = 0; R = 0: no launch; mask0 / mask023 / mask8 (-lead: a masked column 0.05 ahead of every row): the unmasked maximum;
                            an id >= V.  Two runs from the same input are compared bit for bit.
    ops.cosine_scores(exact=False) / auto   sc_l2norm_fwd -> sc_split_hilo_bf16 -> sc_gemm_bf16 -> sc_cosine_refine_masked: chain/R1-V4 (the smallest GEMM), R5-V8 and
                            R65-V260 with the quantizer's mask and a leading masked column, R3-V1028-E128, and chain/auto-R4096-V1028 (R V just above 2^22: the dispatch rule
                            itself picks the path); chain/sparse-*: operands with three non-zeros of 9 .. 12 significant bits, on which the three-term split errs by six to
                            seven refine bounds (a skipped or mask-blind refine fails them on real values); sc_vq_fwd on the result must pick fp64's sub-word on every row
    sc_vq_fwd               vq_row / vq_col / vq_col_finish / vq_final   vq/*: V 1 / 7 / 255 / 256 / 257 / 1031 / 49408, R 1 / 63 / 64 / 65 (a short last split) / 257 / 1024
                            (nsplit 1 / 8 / 32), K 1 / 8 / 257 (the second trip of vq_final's loop), no mask / three ids / eight ids with 0 and V - 1 / an id >= V; rows with
                            a masked maximum, exact ties, a one-hot peak, a -inf column.  The workspace is a guarded window of sc_vq_workspace_bytes.  Two runs bit for bit.
                            test_vq_row_without_a_comparable_entry: one NaN row among normal rows -> target 0, the other rows' targets unaffected (vq_row_kernel's guard)
    sc_gather_rows          gather_rows_kernel        gather/E1 / 255 / 256 / 257 (the second trip), repeated and last-row indices, R = 0
    sc_retrieval_ranks      retrieval_rank_kernel     ranks/*: m 1 / 63 / 64 / 65 / 300, n 1 / 3 / 4 / 5 (a part-filled block, a second block), ld > m with PAST_VALUE behind
    sc_topk_rows_f32        topk_rows_kernel          topk/*: V 1 / 255 / 256 / 257 / 1031, K 1 / 10 / V, ld > V, the maximum planted on both sides of wave and block borders,
                            -inf tails, NaN tails (index -1)
    sc_attention_probs_fwd  attention_probs_kernel    probs/*: hd 8 / 96 / 1024, L 1 / 63 / 64 / 65 / 130, n_rows 0 / 1 / 5 / L, ld_qkv > 3 H hd, no mask / ragged / a fully
                            padded batch row, peaked rows"""
import ctypes

import pytest
import torch

import cascaded_fwd_ref as C
import row_kernels_ref as R

pytestmark = pytest.mark.gpu
F64, F32, BF = R.F64, R.F32, R.BF
Guarded, _judge = R.Guarded, R.judge
PAD = 64
NAN = float("nan")
ISENT = -7777


def _cases(name):
    return pytest.mark.parametrize("c", C.GROUPS[name].cases(), ids=lambda c: c.id)


def _op(t64, dt=F32, fill=NAN):
    """an operand of the kernel's type between two runs of PAD NaN elements (16-byte aligned)"""
    n = t64.numel()
    buf = torch.full((2 * PAD + n,), fill, dtype=dt, device="cuda")
    buf[PAD:PAD + n] = t64.reshape(-1).to(F32).to(dt).cuda()
    return buf[PAD:PAD + n].view(t64.shape)


def _iop(t, dt, fill=0):
    """an integer operand between two runs of PAD elements of `fill` (row indices: 0, a row that exists; ids: a value no id has; pad flags: padded)"""
    n = t.numel()
    buf = torch.full((2 * PAD + n,), fill, dtype=dt, device="cuda")
    buf[PAD:PAD + n] = t.reshape(-1).to(dt).cuda()
    return buf[PAD:PAD + n].view(t.shape)


class IGuarded:
    """Guarded for an integer output [n]"""

    def __init__(self, n, dt):
        self.n = n
        self.buf = torch.full((2 * PAD + n,), ISENT, dtype=dt, device="cuda")

    def out(self):
        return self.buf[PAD:PAD + self.n]

    def check(self, what):
        flat = self.buf.cpu()
        assert bool((flat[:PAD] == ISENT).all() and (flat[PAD + self.n:] == ISENT).all()), (what, "wrote outside its output region")
        return flat[PAD:PAD + self.n].to(F64)


def _bitwise(what, got, want):
    got = got.reshape(want.shape)
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    n = int(bad.sum())
    print(f"{what:60s} bitwise {'equal' if n == 0 else f'{n} of {want.numel()} elements differ'}")
    if n:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError((what, "differs at", i, "got", float(got[i]), "want", float(want[i]), "elements wrong", n))


def _judge_all(c, G, got, inp):
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    for name, r in ref.items():
        if bool((bd[name].bound == 0).all()):
            _bitwise(f"{c.id} {name}", got[name], r)
        else:
            _judge(f"{c.id} {name}", got[name], r, bd[name].bound)
    return ref, bd


def _mask_arg(mask):
    ids = (ctypes.c_int32 * max(1, len(mask)))(*[int(i) for i in mask])
    return ids, ctypes.cast(ids, ctypes.c_void_p), len(mask)


# ================================================================================================ sc_kw_affine
@_cases("kwaffine")
def test_kw_affine(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.ka_inputs(c)
    go = Guarded(c.rows, c.D, F32)
    x, scale, shift = _op(inp["x"]), _op(inp["scale"]), _op(inp["shift"])
    check(lib().sc_kw_affine(ptr(x), ptr(scale), ptr(shift), ptr(go.out()), c.rows, c.K, c.D, stream()), c.id)
    _judge_all(c, C.GROUPS["kwaffine"], dict(out=go.check(c.id)), inp)


# ================================================================================================ sc_cosine_scores
@_cases("cosine")
def test_cosine_scores(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.cs_inputs(c)
    assert lib().sc_cosine_workspace_bytes(c.R, c.V) == (c.R + c.V) * 4
    go, ws = Guarded(c.R, c.V, F32), Guarded(1, c.R + c.V, F32)
    a, e = _op(inp["a"]), _op(inp["e"])
    check(lib().sc_cosine_scores(ptr(a), ptr(e), ptr(ws.out()), ptr(go.out()), c.R, c.V, c.E, C.EPS, stream()), c.id)
    ws.check(c.id + " workspace")
    _judge_all(c, C.GROUPS["cosine"], dict(out=go.check(c.id)), inp)


# ================================================================================================ sc_cosine_refine[_masked]
def _refine(c, inp):
    from speechclip_amd._lib import lib, check, ptr, stream
    go = Guarded(c.R, c.V, F32)
    if c.R:
        go.out().copy_(inp["scores"].to(F32).cuda())
    a, e = _op(inp["a"]), _op(inp["e"])
    if c.mask:
        keep, ids, n = _mask_arg(c.mask)
        check(lib().sc_cosine_refine_masked(ptr(go.out()), ptr(a), ptr(e), c.R, c.V, c.E, c.delta, C.EPS, ids, n, stream()), c.id)
    else:
        check(lib().sc_cosine_refine(ptr(go.out()), ptr(a), ptr(e), c.R, c.V, c.E, c.delta, C.EPS, stream()), c.id)
    return go.check(c.id)


@_cases("refine")
def test_cosine_refine(c):
    inp = C.rf_inputs(c)
    C.rf_wellposed(c, inp)
    got = _refine(c, inp)
    _, bd = _judge_all(c, C.GROUPS["refine"], dict(out=got), inp)
    untouched = bd["out"].bound == 0
    _bitwise(f"{c.id} entries outside the refined set", got[untouched], inp["scores"][untouched])
    _bitwise(f"{c.id} second run", _refine(c, inp), got)


# ================================================================================================ ops.cosine_scores(exact=False) and the auto dispatch
@_cases("chain")
def test_cosine_scores_mfma_chain(c):
    from speechclip_amd import ops
    inp = C.ch_inputs(c)
    C.ch_wellposed(c, inp)
    a, emb = _op(inp["a"]), _op(inp["e"])
    got = ops.cosine_scores(a, emb, exact=c.exact, mask_ids=c.mask)
    again = ops.cosine_scores(a, emb, exact=c.exact, mask_ids=c.mask)
    targets = ops.vq_fwd(got, 1, c.mask)[0]
    got64 = got.cpu().to(F64)
    _judge_all(c, C.GROUPS["chain"], dict(out=got64, argmax=targets.cpu().to(F64)), inp)
    _bitwise(f"{c.id} second run", again.cpu().to(F64), got64)


# ================================================================================================ sc_vq_fwd
def _vq(c, inp):
    from speechclip_amd._lib import lib, check, ptr, stream
    nws = C.vq_workspace_floats(c.R, c.V)
    assert lib().sc_vq_workspace_bytes(c.R, c.V) == 4 * nws
    tg, st, en, ws = IGuarded(c.R, torch.int64), Guarded(1, 2, F32), Guarded(1, c.K, F32), Guarded(1, nws, F32)
    keep, ids, n = _mask_arg(c.mask)
    x = _op(inp["x"])
    check(lib().sc_vq_fwd(ptr(x), ptr(tg.out()), ptr(st.out()), ptr(en.out()), ptr(ws.out()), c.R, c.K, c.V, ids, n, stream()), c.id)
    ws.check(c.id + " workspace")
    return dict(targets=tg.check(c.id), stats=st.check(c.id).view(2), ent=en.check(c.id).view(c.K))


@_cases("vq")
def test_vq_fwd(c):
    inp = C.vq_inputs(c)
    got = _vq(c, inp)
    _judge_all(c, C.GROUPS["vq"], got, inp)
    again = _vq(c, inp)
    for name in got:
        _bitwise(f"{c.id} {name} second run", again[name], got[name])


def test_vq_row_without_a_comparable_entry():
    """one all-NaN row among normal rows: target 0 and a histogram index inside [0, V); the other rows' targets are those of the statement"""
    from speechclip_amd._lib import lib, check, ptr, stream
    c = C.VQCase("vq/V257-R5-K1-nanrow", 257, 5, 1, (0, 2, 3))
    inp = C.vq_inputs(c)
    want = C.vq_ref(c, inp)["targets"]
    inp["x"][2] = NAN
    want[2] = 0
    nws = C.vq_workspace_floats(c.R, c.V)
    tg, st, en, ws = IGuarded(c.R, torch.int64), Guarded(1, 2, F32), Guarded(1, c.K, F32), Guarded(1, nws, F32)
    keep, ids, n = _mask_arg(c.mask)
    x = _op(inp["x"])
    check(lib().sc_vq_fwd(ptr(x), ptr(tg.out()), ptr(st.out()), ptr(en.out()), ptr(ws.out()), c.R, c.K, c.V, ids, n, stream()), c.id)
    torch.cuda.synchronize()
    ws.check(c.id + " workspace")
    _bitwise(f"{c.id} targets", tg.check(c.id), want)


# ================================================================================================ sc_gather_rows
@_cases("gather")
def test_gather_rows(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.gt_inputs(c)
    go = Guarded(c.R, c.E, F32)
    src, idx = _op(inp["src"]), _iop(inp["idx"], torch.int64)
    check(lib().sc_gather_rows(ptr(src), ptr(idx), ptr(go.out()), c.R, c.E, stream()), c.id)
    _judge_all(c, C.GROUPS["gather"], dict(out=go.check(c.id)), inp)


# ================================================================================================ sc_retrieval_ranks
@_cases("ranks")
def test_retrieval_ranks(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.rk_inputs(c)
    score = torch.full((c.n, c.ld), R.PAST_VALUE, dtype=F64)
    score[:, :c.m] = inp["score"]
    go = IGuarded(c.n, torch.int32)
    sc, own, cand = _op(score), _iop(inp["own"], torch.int64, -1), _iop(inp["cand"], torch.int64, -2)
    check(lib().sc_retrieval_ranks(ptr(sc), c.ld, ptr(own), ptr(cand), ptr(go.out()), c.n, c.m, stream()), c.id)
    _judge_all(c, C.GROUPS["ranks"], dict(rank=go.check(c.id)), inp)


# ================================================================================================ sc_topk_rows_f32
@_cases("topk")
def test_topk_rows(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.tk_inputs(c)
    x = torch.full((c.rows, c.ld), R.PAST_VALUE, dtype=F64)
    x[:, :c.V] = inp["x"]
    gv, gi = Guarded(c.rows, c.K, F32), IGuarded(c.rows * c.K, torch.int32)
    xd = _op(x)
    check(lib().sc_topk_rows_f32(ptr(xd), c.ld, c.rows, c.V, c.K, ptr(gv.out()), ptr(gi.out()), stream()), c.id)
    _judge_all(c, C.GROUPS["topk"], dict(vals=gv.check(c.id), idx=gi.check(c.id)), inp)


# ================================================================================================ sc_attention_probs_fwd
@_cases("probs")
def test_attention_probs(c):
    from speechclip_amd._lib import lib, check, ptr, stream
    inp = C.pb_inputs(c)
    D = c.H * c.hd
    ld = 3 * D + c.ld_extra
    qkv = torch.full((c.B, c.L, ld), NAN, dtype=F64)
    qkv[:, :c.n_rows, :D] = inp["q"][:, :c.n_rows].reshape(c.B, c.n_rows, D)
    k = inp["k"].reshape(c.B, c.L, D).clone()
    if inp["pad"] is not None:
        k[inp["pad"]] = NAN                                                       # a padded key is never read
    qkv[:, :, D:2 * D] = k
    dev = _op(qkv.view(c.B * c.L, ld), BF)
    pad = None if inp["pad"] is None else _iop(inp["pad"], torch.uint8, 1)
    go = Guarded(c.B * c.H * c.n_rows, c.L, F32)
    out_ptr = go.buf.data_ptr() + 4 * R.GUARD                                       # (an empty window -- n_rows = 0 -- has no data_ptr of its own)
    check(lib().sc_attention_probs_fwd(dev.data_ptr(), dev.data_ptr() + 2 * D, out_ptr, ptr(pad), c.B, c.H, c.L, c.hd, c.n_rows, ld, inp["scale"], stream()), c.id)
    got = go.check(c.id).view(c.B, c.H, c.n_rows, c.L)
    _judge_all(c, C.GROUPS["probs"], dict(probs=got, rowsum=got.sum(-1)), inp)
    if inp["pad"] is not None and c.n_rows:
        assert bool((got[inp["pad"][:, None, None, :].expand_as(got)] == 0).all()), (c.id, "a padded key has a non-zero probability")

"""GPU: the quantizer-mode kernels (csrc/vq_modes.hip) against the plain fp64 statements of tests/vq_modes_parity_ref.py -- bit for bit where the statement is exact,
element by element under the bounds DERIVED there everywhere else (no element is excluded; tools/vq_mode_bounds.py is the CPU self-check of statements, bounds and
mutants).  Every kernel is called through the C ABI (speechclip_amd._lib), every output pointer -- keywords, row_max, row_den, the split workspace, the dense
probabilities, dprob_inout, both rowdots, the targets, the noise image, the table -- is a window inside a sentinel-filled buffer, and everything outside the written
region must still hold the sentinel.  Each case prints its worst err / bound and where it occurred (-s); SC_VQ_PARITY_OUT=<file> appends those lines
(profiles/vq_modes_parity.txt is such a file).

Which case reaches which code:
    table/*      vq_soft_table_kernel: V below, at and above one 32-row block, the zero rows past V written over a NaN fill, E / 16 = 4 and 12 column tiles
    onehot/twohot vq_soft_embed_kernel<NE, false> for NE 1 2 3 4 6 8 and grid.y 1 2 5 (E 64 .. 768), wave rows 0 and 1, a second and a partly filled row tile
                 (R 1 .. 256), every chunk boundary of nsplit 1 / 2 / 5 / auto / 64 (clamped to the 11 steps; at 5 the last chunk is empty), vq_soft_finish_kernel
    argmax/*     vq_noisy_argmax_kernel<false>: ties inside a thread, across lanes, across waves with the lowest index in the LATER wave; 0 / 3 / 8 masked ids
    allmasked/*  the p_den > 0 branch of vq_soft_embed_kernel, vq_probs_kernel, vq_mode_bwd_kernel, the arg-max's empty row
    noise/*      vq_gumbel_noise_kernel, the smallest and the largest uniform the draw can give
    probs/*      vq_probs_kernel<NOISE> and vq_row_stats_kernel<NOISE>: V below, at and above the block's 256 threads, V = 5 with two live columns
    soft/*       vq_soft_embed_kernel<NE, NOISE> on the grid above with V = 333 and 1031, and once on the workload's 49408-row table
    modebwd/*    vq_mode_bwd_kernel<true>; stbwd/*: vq_mode_bwd_kernel<false> against vq_st_bwd_kernel, bit for bit"""
import ctypes
import functools
import os

import pytest
import torch

import vq_modes_parity_ref as P
from row_kernels_ref import GUARD, Guarded, worst

pytestmark = pytest.mark.gpu
F64, F32 = P.F64, P.F32
I16_SENT, I64_SENT = 0x5a5a, -7777


def _note(line):
    print(line)
    path = os.environ.get("SC_VQ_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _judge(what, got, ref, bound):
    """row_kernels_ref.judge, with the line also appended to SC_VQ_PARITY_OUT"""
    got = got.reshape(ref.shape)
    r, i = worst((got - ref).abs(), bound)
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.numel() else ()
    _note(f"{what:60s} worst err/bound {r:8.4f} at {idx}")
    assert torch.isfinite(got).all(), what
    assert r <= 1.0, (what, "err / bound", r, "at", idx, "got", float(got[idx]), "ref", float(ref[idx]), "bound", float(bound[idx]))
    return r


def _L():
    from speechclip_amd._lib import check, lib, ptr, stream
    return lib(), check, ptr, stream


def _d(t):
    return t.to(F32).cuda().contiguous()


def _filled(rows, ld, data):
    go = Guarded(rows, ld, F32)
    go.out().copy_(data.to(F32).cuda().reshape(rows, ld))
    return go


class _Mask:
    def __init__(self, ids):
        self.arr = (ctypes.c_int * max(1, len(ids)))(*ids)
        self.p, self.n = ctypes.cast(self.arr, ctypes.c_void_p), len(ids)


def _untouched(go, what):
    assert bool((go.buf == go.sent).all()), (what, "an output was written")


def _ends_intact(go, what):
    assert bool((go.buf[:GUARD] == go.sent).all()) and bool((go.buf[-GUARD:] == go.sent).all()), (what, "wrote outside its output region")


class _RawGuard:
    """a flat window of n integers inside a sentinel-filled buffer (the table as bf16 bit patterns, the int64 targets)"""

    def __init__(self, n, dt, sent, fill=None):
        self.n, self.sent = n, sent
        self.buf = torch.full((2 * GUARD + n,), sent, dtype=dt, device="cuda")
        self.win = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.win.fill_(fill)

    def check(self, what):
        flat = self.buf.cpu()
        assert bool((flat[:GUARD] == self.sent).all()) and bool((flat[GUARD + self.n:] == self.sent).all()), (what, "wrote outside its output region")
        return flat[GUARD:GUARD + self.n].clone()


def _build_table(emb, what):
    """sc_vq_soft_table into a NaN-filled window of sc_vq_soft_table_bytes bytes -> (_RawGuard, bit patterns on the host)"""
    L, check, ptr, stream = _L()
    V, E = emb.shape
    nbytes = L.sc_vq_soft_table_bytes(V, E)
    assert nbytes == 2 * P.table_elems(V, E)
    tab = _RawGuard(nbytes // 2, torch.int16, I16_SENT, P.TABLE_FILL)
    e = _d(emb)
    check(L.sc_vq_soft_table(ptr(e), ptr(tab.win), V, E, stream()), what)
    return tab, tab.check(what)


@functools.lru_cache(maxsize=3)
def _table_for(kind, V, E):
    emb = P.hot_table(V, E) if kind == "hot" else P._emb(V, E)
    return _build_table(emb, f"table {kind} {V}x{E}")[0]


def _soft_embed(x_d, tab, Rr, V, E, temp, seed, on, mk, nsplit, what):
    """sc_vq_soft_embed with every output pointer guarded -> (keywords, row_max, row_den on the host, the chunk count it launched)"""
    L, check, ptr, stream = _L()
    ws_bytes = L.sc_vq_soft_embed_workspace_bytes(Rr, V, E, nsplit)
    ns = ws_bytes // (Rr * E * 4) if ws_bytes else 1
    assert ws_bytes == (ns * Rr * E * 4 if ns > 1 else 0) and 1 <= ns <= P.nsteps(V)
    kw, rmax, rden, ws = Guarded(Rr, E, F32), Guarded(1, Rr, F32), Guarded(1, Rr, F32), Guarded(1, max(ns, 2) * Rr * E, F32)
    check(L.sc_vq_soft_embed(ptr(x_d), ptr(tab.win), ptr(kw.out()), ptr(rmax.out()), ptr(rden.out()), ptr(ws.out()), Rr, V, E, temp, seed, on, mk.p, mk.n, nsplit,
                             stream()), what)
    if ns > 1:
        _ends_intact(ws, what)
        assert bool((ws.buf[GUARD + ns * Rr * E:] == ws.sent).all()), (what, "wrote past its chunks of the workspace")
    else:
        _untouched(ws, what)
    return kw.check(what), rmax.check(what).reshape(-1), rden.check(what).reshape(-1), ns


# ================================================================================================ 1. exact
@pytest.mark.parametrize("E", P.TABLE_E)
@pytest.mark.parametrize("V", P.TABLE_V)
def test_soft_table_bit_for_bit(V, E):
    """every one of the 2 * ceil(V / 32) * 32 * E elements equals the host restatement of the layout, the zero rows past V included (written over a NaN fill)"""
    emb = P.table_emb(V, E)
    _, got = _build_table(emb, f"table/{V}x{E}")
    want = P.table_bits(emb)
    assert got.numel() == want.numel() == P.table_elems(V, E)
    bad = (got != want).nonzero().reshape(-1)
    _note(f"{f'table/{V}x{E}':60s} {got.numel()} elements, {bad.numel()} differ; guards intact")
    assert bad.numel() == 0, (V, E, "first difference at flat element", int(bad[0]), hex(int(got[bad[0]]) & 0xffff), hex(int(want[bad[0]]) & 0xffff))


@pytest.mark.parametrize("c", P.hot_cases(), ids=lambda c: c.id)
def test_one_hot_and_two_hot_products_bit_for_bit(c):
    """keywords = emb[w(r)], or (emb[a] + emb[b]) / 2, exactly; row_max and row_den exactly; for every nsplit"""
    inp = P.hot_inputs(c)
    ref = P.hot_ref(c, inp)
    tab, x_d, mk = _table_for("hot", P.HOT_V, c.E), _d(inp["x"]), _Mask(P.R.MASK)
    launched = []
    for nsplit in P.GRID_NSPLIT:
        what = f"{c.id} nsplit {nsplit}"
        kw, rmax, rden, ns = _soft_embed(x_d, tab, c.R, P.HOT_V, c.E, c.temp, 0, 0, mk, nsplit, what)
        launched.append(ns)
        assert torch.equal(rmax, ref["row_max"]) and torch.equal(rden, ref["row_den"]), what
        bad = (kw != ref["kw"]).nonzero()
        assert bad.numel() == 0, (what, "chunks", ns, "first difference at", bad[0].tolist(), float(kw[tuple(bad[0])]), float(ref["kw"][tuple(bad[0])]))
    assert launched[:3] == [1, 2, 5] and launched[4] == P.nsteps(P.HOT_V)                      # the clamp
    _note(f"{c.id.replace('hot-', 'hot/'):60s} bitwise equal for nsplit {P.GRID_NSPLIT} (chunks launched {tuple(launched)}); NE {P.soft_ne(c.E)} grid.y {P.grid_y(c.E)}")


def _argmax(x, ids, what, seed=0, on=0):
    L, check, ptr, stream = _L()
    Rr, V = x.shape
    t = _RawGuard(Rr, torch.int64, I64_SENT)
    mk = _Mask(ids)
    x_d = _d(x)
    check(L.sc_vq_noisy_argmax(ptr(x_d), ptr(t.win), Rr, V, seed, on, mk.p, mk.n, stream()), what)
    return t.check(what)


@pytest.mark.parametrize("c", P.arg_cases(), ids=lambda c: c.id)
def test_argmax_planted_ties_and_masks(c):
    inp = P.arg_inputs(c)
    want = P.arg_ref(c, inp)["targets"].to(torch.int64)
    got = _argmax(inp["x"], c.ids, c.id)
    _note(f"{c.id.replace('argmax-', 'argmax/'):60s} targets {got.tolist()} want {want.tolist()}")
    assert torch.equal(got, want)


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("V,ids", P.ALLMASKED, ids=[f"V{v}" for v, _ in P.ALLMASKED])
def test_row_with_every_column_masked(V, ids, noise):
    """sc_vq_probs: a row of zeros; sc_vq_soft_embed: a zero keyword row for every nsplit, row_max = -inf, row_den = 0; sc_vq_mode_bwd: dcos = 0 and both rowdots 0;
    sc_vq_noisy_argmax: target 0 (include/speechclip_hip.h states all four)"""
    L, check, ptr, stream = _L()
    Rr, E, what = 3, 64, f"allmasked/V{V}-{'noise' if noise else 'plain'}"
    g_ = P.gen("allmasked", V)
    x = P.rnd(P.scores_like(g_, Rr, V), F32)
    x_d, mk, on = _d(x), _Mask(ids), int(noise)
    zero = torch.zeros(Rr, V, dtype=F64)
    for temp in (1.0, 0.1):
        out = Guarded(Rr, V, F32)
        check(L.sc_vq_probs(ptr(x_d), ptr(out.out()), Rr, V, temp, P.SEED, on, mk.p, mk.n, stream()), what)
        assert torch.equal(out.check(what), zero), what
        tab = _build_table(P._emb(333, E)[:V], what)[0]
        for nsplit in P.GRID_NSPLIT:
            kw, rmax, rden, ns = _soft_embed(x_d, tab, Rr, V, E, temp, P.SEED, on, mk, nsplit, what)
            assert ns == 1 and torch.equal(kw, torch.zeros(Rr, E, dtype=F64)), (what, nsplit)
            assert torch.equal(rmax, torch.full((Rr,), float("-inf"), dtype=F64)) and torch.equal(rden, torch.zeros(Rr, dtype=F64)), (what, nsplit)
        dp = _filled(Rr, V, P.rnd(torch.randn(Rr, V, generator=g_, dtype=F64), F32))
        rc_, rz_ = Guarded(1, Rr, F32), Guarded(1, Rr, F32)
        check(L.sc_vq_mode_bwd(ptr(x_d), ptr(dp.out()), ptr(rc_.out()), ptr(rz_.out()), Rr, V, temp, P.SEED, on, mk.p, mk.n, stream()), what)
        assert torch.equal(dp.check(what), zero) and torch.equal(rc_.check(what), torch.zeros(1, Rr, dtype=F64)) and torch.equal(rz_.check(what), torch.zeros(1, Rr, dtype=F64))
    assert _argmax(x, ids, what, P.SEED, on).tolist() == [0] * Rr
    _note(f"{what:60s} probs, keywords (every nsplit), row_max = -inf, row_den, dcos, rowdots, targets: all exact")


@pytest.mark.parametrize("nmask", P.BWD_NMASK)
@pytest.mark.parametrize("Rr,V,temp", [(7, 257, 1.0), (48, 1000, 0.1)])
def test_mode_bwd_without_noise_is_the_straight_through_kernel_bitwise(Rr, V, temp, nmask):
    L, check, ptr, stream = _L()
    c = P.BwdCase(f"stbwd/{Rr}x{V}-T{temp:g}-mask{nmask}", Rr, V, temp, nmask, ())
    inp = P.bwd_inputs(c)
    mk, cos = _Mask(P.vq_mask_ids(c)), _d(inp["cos"])
    d1, d2 = _filled(Rr, V, inp["dprob"]), _filled(Rr, V, inp["dprob"])
    r1, r2, z2 = Guarded(1, Rr, F32), Guarded(1, Rr, F32), Guarded(1, Rr, F32)
    check(L.sc_vq_st_bwd(ptr(cos), ptr(d1.out()), ptr(r1.out()), Rr, V, temp, mk.p, mk.n, stream()), c.id)
    check(L.sc_vq_mode_bwd(ptr(cos), ptr(d2.out()), ptr(r2.out()), ptr(z2.out()), Rr, V, temp, 12345, 0, mk.p, mk.n, stream()), c.id)
    a, b = d1.check(c.id), d2.check(c.id)
    assert torch.equal(a.to(F32).view(torch.int32), b.to(F32).view(torch.int32))
    ra, rb, zb = (t.check(c.id).to(F32).view(torch.int32) for t in (r1, r2, z2))
    assert torch.equal(ra, rb) and torch.equal(rb, zb)
    assert bool((b != 0).any()) and (nmask == 0 or bool((b[:, P.vq_mask_ids(c)] == 0).all()))
    _note(f"{c.id:60s} dcos, rowdot_cos, rowdot_z: the bits of sc_vq_st_bwd")


def test_argument_checks_return_their_code_and_write_nothing():
    L, check, ptr, stream = _L()
    Rr, V, E = 3, 333, 64
    x = _d(P._soft_scores(65, V)[:Rr])
    tab = _table_for("soft", V, E)
    mk, none = _Mask(P.R.MASK), _Mask(())
    outs = dict(kw=Guarded(Rr, E, F32), rmax=Guarded(1, Rr, F32), rden=Guarded(1, Rr, F32), ws=Guarded(1, P.nsteps(V) * Rr * E, F32), dense=Guarded(Rr, V, F32),
                rc=Guarded(1, Rr, F32), rz=Guarded(1, Rr, F32))
    tg = _RawGuard(Rr, torch.int64, I64_SENT)
    o = {k: ptr(v.out()) for k, v in outs.items()}

    def soft(Rr_=Rr, V_=V, E_=E, temp=1.0, m=mk, n=None, nsplit=0):
        return L.sc_vq_soft_embed(ptr(x), ptr(tab.win), o["kw"], o["rmax"], o["rden"], o["ws"], Rr_, V_, E_, temp, 1, 1, m.p, m.n if n is None else n, nsplit, stream())

    def probs(Rr_=Rr, V_=V, temp=1.0, n=None):
        return L.sc_vq_probs(ptr(x), o["dense"], Rr_, V_, temp, 1, 1, mk.p, mk.n if n is None else n, stream())

    def bwd(Rr_=Rr, V_=V, temp=1.0, n=None):
        return L.sc_vq_mode_bwd(ptr(x), o["dense"], o["rc"], o["rz"], Rr_, V_, temp, 1, 1, mk.p, mk.n if n is None else n, stream())

    def amax(Rr_=Rr, V_=V, n=None):
        return L.sc_vq_noisy_argmax(ptr(x), ptr(tg.win), Rr_, V_, 1, 1, mk.p, mk.n if n is None else n, stream())

    def noise(Rr_=Rr, V_=V):
        return L.sc_vq_gumbel_noise(o["dense"], Rr_, V_, 1, stream())

    for temp in (0.0, -1.0):
        assert soft(temp=temp) < 0 and probs(temp=temp) < 0 and bwd(temp=temp) < 0, temp
    for n in (9, -1):
        assert soft(n=n) < 0 and probs(n=n) < 0 and bwd(n=n) < 0 and amax(n=n) < 0, n
    assert soft(nsplit=-1) < 0
    big = 65536                                                              # R * V = 2^32
    assert soft(big, big) < 0 and probs(big, big) < 0 and bwd(big, big) < 0 and amax(big, big) < 0 and noise(big, big) < 0
    assert soft(E_=48) == 1 and soft(V_=4) == 1                              # "not covered": the caller composes sc_vq_probs and a GEMM
    assert L.sc_vq_soft_embed(None, None, None, None, None, None, Rr, V, 48, 1.0, 1, 1, None, 0, 0, None) == 1
    assert soft(0) == 0 and probs(0) == 0 and bwd(0) == 0 and amax(0) == 0 and noise(0) == 0          # R = 0: nothing to do
    torch.cuda.synchronize()
    for k, v in outs.items():
        _untouched(v, k)
    assert bool((tg.buf == I64_SENT).all())
    assert soft() == 0 and probs() == 0 and bwd() == 0 and amax() == 0 and noise() == 0                # (the same calls with valid arguments do run)
    torch.cuda.synchronize()
    assert not bool((outs["kw"].out() == outs["kw"].sent).any()) and not bool((tg.win == I64_SENT).any())
    _note(f"{'args/refusals':60s} temp <= 0, n_mask 9 / -1, nsplit < 0, R * V = 2^32: error code; E = 48, V = 4: 1; R = 0: 0; no output written")


# ================================================================================================ 2. per-element parity
def _check(group, c, got):
    G = P.GROUPS[group]
    inp = G.inputs(c)
    ref, bd = G.ref(c, inp), G.bound(c, inp)
    assert set(got) == set(ref), (c.id, sorted(got), sorted(ref))
    for name, r in ref.items():
        _judge(f"{c.id.replace('-', '/', 1)} {name}", got[name], r, bd[name].bound)
    return ref, bd


@pytest.mark.parametrize("c", P.noise_cases(), ids=lambda c: c.id)
def test_gumbel_noise_per_element(c):
    L, check, ptr, stream = _L()
    out = Guarded(c.R, c.V, F32)
    check(L.sc_vq_gumbel_noise(ptr(out.out()), c.R, c.V, c.seed, stream()), c.id)
    got = out.check(c.id)
    ref, bd = _check("noise", c, dict(g=got))
    which = "derived TR (1 + |g|)" if P.NOISE_FALLBACK is None else f"FALLBACK to the suite's flat {P.NOISE_FALLBACK:g}"
    flat = float((got - ref["g"]).abs().max())
    _note(f"{c.id.replace('-', '/', 1) + ' bound':60s} {which}; max |err| {flat:.3e} (the flat 1e-5 of tests/test_vq_modes_gpu.py: {'met' if flat <= 1e-5 else 'MISSED'})")
    if c.extreme is not None:
        idx, kind = c.extreme
        g_ext = float(ref["g"].reshape(-1)[idx])
        assert abs(g_ext - (-2.82 if kind == "low" else 16.64)) < 0.01
        e_ext = abs(float(got.reshape(-1)[idx]) - g_ext)
        _note(f"{c.id.replace('-', '/', 1) + ' extreme':60s} g = {g_ext:.4f} err / bound {e_ext / float(bd['g'].bound.reshape(-1)[idx]):8.4f}")


@pytest.mark.parametrize("c", P.prob_cases(), ids=lambda c: c.id)
def test_probs_row_max_row_den_per_element(c):
    """p from sc_vq_probs; row_max and row_den from sc_vq_soft_embed's pre-pass (E = 64) on the same scores"""
    L, check, ptr, stream = _L()
    inp = P.prob_inputs(c)
    ids = P.vq_mask_ids(c)
    mk, x_d = _Mask(ids), _d(inp["x"])
    out = Guarded(c.R, c.V, F32)
    check(L.sc_vq_probs(ptr(x_d), ptr(out.out()), c.R, c.V, c.temp, P.SEED, int(c.noise), mk.p, mk.n, stream()), c.id)
    p = out.check(c.id)
    tab = _table_for("soft", 1031, 64) if c.V == 1031 else _build_table(P._emb(333, 64)[:c.V], c.id)[0]
    _, rmax, rden, _ = _soft_embed(x_d, tab, c.R, c.V, 64, c.temp, P.SEED, int(c.noise), mk, 1, c.id)
    if ids:
        assert bool((p[:, ids] == 0).all()), c.id                                          # masked columns: exactly 0
    _check("probs", c, dict(p=p, row_max=rmax, row_den=rden))


@pytest.mark.parametrize("c", P.soft_cases(), ids=lambda c: c.id)
def test_soft_embed_keywords_per_element(c):
    """every nsplit of the case against the same reference; at R = 200 every nsplit also run twice, bit for bit"""
    G = P.GROUPS["soft"]
    inp = G.inputs(c)
    ref = G.ref(c, inp)["kw"]
    tab, x_d, mk = _table_for("soft", c.V, c.E), _d(inp["x"]), _Mask(P.R.MASK)
    res = []
    for nsplit in c.nsplits:
        what = f"{c.id} nsplit {nsplit}"
        kw, rmax, rden, ns = _soft_embed(x_d, tab, c.R, c.V, c.E, c.temp, P.SEED, int(c.noise), mk, nsplit, what)
        assert bool(torch.isfinite(kw).all()), what
        if c.R == 200:
            again = _soft_embed(x_d, tab, c.R, c.V, c.E, c.temp, P.SEED, int(c.noise), mk, nsplit, what)
            assert torch.equal(again[0], kw) and torch.equal(again[1], rmax) and torch.equal(again[2], rden), (what, "not bitwise run to run")
        res.append((nsplit, ns, kw))
    one, per_chunk, _ = P.soft_bound_terms(c, inp)
    top = None
    for nsplit, ns, kw in res:
        r, i = worst((kw - ref).abs(), one + (ns - 1) * per_chunk)
        if top is None or r > top[0]:
            top = (r, i, nsplit, ns, kw)
    r, i, nsplit, ns, kw = top
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    _note(f"{c.id.replace('-', '/', 1) + ' kw':60s} worst err/bound {r:8.4f} at {idx} nsplit {nsplit} (chunks launched {tuple(t[1] for t in res)})")
    assert r <= 1.0, (c.id, "nsplit", nsplit, "chunks", ns, "err / bound", r, "at", idx, "got", float(kw[idx]), "ref", float(ref[idx]))


@pytest.mark.parametrize("c", P.bwd_cases(), ids=lambda c: c.id)
def test_mode_bwd_with_noise_per_element(c):
    L, check, ptr, stream = _L()
    inp = P.bwd_inputs(c)
    ids = P.vq_mask_ids(c)
    mk, cos = _Mask(ids), _d(inp["cos"])
    dp, rc, rz = _filled(c.R, c.V, inp["dprob"]), Guarded(1, c.R, F32), Guarded(1, c.R, F32)
    check(L.sc_vq_mode_bwd(ptr(cos), ptr(dp.out()), ptr(rc.out()), ptr(rz.out()), c.R, c.V, c.temp, P.SEED, 1, mk.p, mk.n, stream()), c.id)
    d = dp.check(c.id)
    if ids:
        assert bool((d[:, ids] == 0).all()), c.id
    _check("modebwd", c, dict(dcos=d, rowdot_cos=rc.check(c.id).reshape(-1), rowdot_z=rz.check(c.id).reshape(-1)))

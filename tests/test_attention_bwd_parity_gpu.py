"""Per-element fp64 parity of the fused attention backward (csrc/attention_bwd.hip) on every path of its two entries: sc_attention_bwd_packed (ragged row_off
and the uniform layout, wide leading dimensions) and sc_attention_hd_bwd (head_dim 64 / 96 / 128; Tq == Tk interleaved and into three separately strided
buffers; Tq == 1), plain and with dropout, O from the CPU and from the project's forward kernel.

Statements, inputs, bounds and the slope check: tests/attention_bwd_ref.py (self-checked on the CPU by tools/attention_bwd_bounds.py); derivations: DESIGN.md,
"Attention backward: parity".  Every case runs through the C ABI into sentinel-guarded buffers and is checked five ways:
  1. every element of dq, dk, dv against its derived bound; rows that take no part exactly 0; guards and the gaps of strided rows untouched; the count asserted;
  2. the statistics workspace after the call -- lse (log2 units) and delta at the layout of unit_of(), 0 for queries >= klen -- per element against fp64.  This is
     a WHITE-BOX check: it moves with unit_of() and with the workspace layout of csrc/attention_bwd.hip;
  3. the slope check (a systematic error below a bf16 half-ulp) on every operand with at least 4096 participating elements;
  4. a second call, and a third with NaN on every row that takes no part (q, k, v, dO, O; the halo rows of packed utterances), return the same bits;
  5. the stored-O paths a second time against the TRUTH (delta = sum Pd dP) under the same bound plus the exactly computed propagation of
     Delta_i = dO_i . (O_i - o_true,i); the share of that term in the bound is printed.
The image chain of the padded layout (sc_attn_bwd_probs, sc_attn_softmax_bwd / _dropout / _heads, train_hubert.attention_bwd) is judged per element of its P and dS
images, padding included, and end to end; it computes every query row of an utterance, so check 4's NaN run does not apply to it.
117 tests, 6 - 8 s on the MI355X (profiles/attention_bwd_parity.txt)."""
import ctypes
import time

import pytest
import torch

import attention_bwd_ref as A
from row_kernels_ref import BF, F32, F64, Guarded, worst

pytestmark = pytest.mark.gpu
FILL = 7.0          # what the columns between q | k | v of a wide row hold (never read)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _rows(c, ins, i, O=None, nan=False):
    """[sum rows, H * hd] of operand i (0 q, 1 k, 2 v, 3 dO; O: the list itself) over all utterances, bf16; nan: the rows that take no part hold NaN"""
    out = []
    for b in range(c.B):
        t = (O[b] if O is not None else ins[b][i]).clone()
        if nan:
            t[(c.kl(b) if O is None and i in (1, 2) else c.nq(b)):] = float("nan")
        out.append(t.reshape(t.shape[0], -1))
    return torch.cat(out).to(BF)


def _place(total, ld, parts, fill=FILL):
    buf = torch.full((total, ld), fill, dtype=BF)
    for col, t in parts:
        buf[:, col:col + t.shape[1]] = t
    return buf.cuda()


class Run:
    """one call of a case's entry: device buffers, the call, the outputs per utterance"""

    def __init__(self, c, ins, O, nan=False, row_off=None, entry=None):
        from speechclip_amd import _lib, ops
        L_ = _lib.lib()
        self.c, H, hd, D = c, c.H, c.hd, c.H * c.hd
        entry = entry or ("packed" if c.group in ("packed", "uniform") else "hd")
        q, k, v, dO = (_rows(c, ins, i, nan=nan) for i in range(4))
        Ob = _rows(c, ins, 0, O=O, nan=nan)
        total, nqr = k.shape[0], q.shape[0]
        klens = None if c.null_klens else _i32(c.klens)
        kp = 0 if klens is None else klens.data_ptr()
        p, seed = float(c.p), c.seed & 0xffffffff
        if entry == "packed":
            w = c.wide
            ld, qo, ko, vo = (3 * D + 24, 8, D + 16, 2 * D + 24) if w else (3 * D, 0, D, 2 * D)
            ldo, do_ = (2 * D + 16, D + 8) if w else (2 * D, D)
            qkv, oo = _place(total, ld, ((qo, q), (ko, k), (vo, v))), _place(total, ldo, ((0, Ob), (do_, dO)))
            self.outs = [Guarded(total, 3 * D + 8 if w else 3 * D, BF, 3 * D)]
            g = self.outs[0]
            off = A.offsets(c.rows) if c.group == "packed" or row_off else None
            offd = None if off is None else _i32(off)
            nws = 2 * total * H
            assert L_.sc_attention_bwd_packed_workspace_bytes(total, H) == 4 * nws
            self.ws = Guarded(1, nws, F32)
            base, ob = qkv.data_ptr(), g.win.data_ptr()
            rc = L_.sc_attention_bwd_packed(base + 2 * qo, base + 2 * ko, base + 2 * vo, ld, oo.data_ptr(), oo.data_ptr() + 2 * do_, ldo, kp,
                                            0 if offd is None else offd.data_ptr(), c.B, H, c.T, total, hd, ctypes.c_float(c.scale), ctypes.c_float(p), seed,
                                            ob, ob + 2 * D, ob + 4 * D, g.ld, self.ws.win.data_ptr(), ops.stream())
            self.where = {"dq": (0, 0), "dk": (0, D), "dv": (0, 2 * D)}
        else:
            T, Tq = c.T, c.tq(0)
            ldo = 2 * D
            oo = _place(nqr, ldo, ((0, Ob), (D, dO)))
            if c.group == "hdq1":
                qb, kv = q.cuda(), _place(total, 2 * D, ((0, k), (D, v)))
                qs, kvs, qp, kpn, vp = (D, D), (T * 2 * D, 2 * D), qb.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * D
                self.outs = [Guarded(c.B, D, BF), Guarded(total, 2 * D, BF)]
                self.where = {"dq": (0, 0), "dk": (1, 0), "dv": (1, D)}
            elif c.wide:          # q from its own buffer, k | v from another, dq, dk and dv into three buffers (dk and dv share their strides by the ABI)
                qb, kv = _place(total, D + 8, ((0, q),)), _place(total, 2 * D + 16, ((0, k), (D + 8, v)))
                qs, kvs, qp, kpn, vp = (T * (D + 8), D + 8), (T * (2 * D + 16), 2 * D + 16), qb.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * (D + 8)
                self.outs = [Guarded(total, D + 8, BF, D), Guarded(total, D + 24, BF, D), Guarded(total, D + 24, BF, D)]
                self.where = {"dq": (0, 0), "dk": (1, 0), "dv": (2, 0)}
            else:                 # the interleaved [B*L, 3D] form of ops.attention_hd_qkv_bwd
                qb = kv = _place(total, 3 * D, ((0, q), (D, k), (2 * D, v)))
                qs = kvs = (T * 3 * D, 3 * D)
                qp, kpn, vp = qb.data_ptr(), qb.data_ptr() + 2 * D, qb.data_ptr() + 4 * D
                self.outs = [Guarded(total, 3 * D, BF)]
                self.where = {"dq": (0, 0), "dk": (0, D), "dv": (0, 2 * D)}
            gq, gk, gv = (self.outs[self.where[op][0]] for op in A.OPS)
            nws = 2 * c.B * H * Tq
            assert L_.sc_attention_hd_bwd_workspace_bytes(c.B, H, Tq) == 4 * nws
            self.ws = Guarded(1, nws, F32)
            rc = L_.sc_attention_hd_bwd(qp, kpn, vp, oo.data_ptr(), oo.data_ptr() + 2 * D, kp, c.B, H, Tq, T, hd, qs[0], qs[1], kvs[0], kvs[1], Tq * ldo, ldo,
                                        gq.win.data_ptr() + 2 * self.where["dq"][1], Tq * gq.ld, gq.ld, gk.win.data_ptr() + 2 * self.where["dk"][1],
                                        gv.win.data_ptr() + 2 * self.where["dv"][1], T * gk.ld, gk.ld, ctypes.c_float(c.scale), ctypes.c_float(p), seed,
                                        self.ws.win.data_ptr(), ops.stream())
        assert rc == 0, L_.sc_last_error()
        torch.cuda.synchronize()
        self.keep = (qb, kv, oo) if entry != "packed" else (qkv, oo)

    def results(self, what):
        """guards checked; -> {op: list over utterances [rows, H, hd]}, lse and delta lists [H, Tq] (the layout of unit_of(): unit (b, h) at
        (query rows before the utterance) * H + h * Tq, delta behind all of lse)"""
        c, D = self.c, self.c.H * self.c.hd
        mats = [g.check(what) for g in self.outs]
        out = {}
        for op in A.OPS:
            gi, col = self.where[op]
            m = mats[gi][:, col:col + D]
            off = A.offsets([c.tq(b) if op == "dq" else c.rows[b] for b in range(c.B)])
            out[op] = [m[off[b]:off[b + 1]].reshape(-1, c.H, c.hd) for b in range(c.B)]
        ws = self.ws.check(what + " workspace").reshape(2, -1)
        off = A.offsets([c.tq(b) for b in range(c.B)])
        for i, name in enumerate(("lse", "delta")):
            out[name] = [ws[i, off[b] * c.H:off[b + 1] * c.H].view(c.H, c.tq(b)) for b in range(c.B)]
        return out

    def bits(self):
        return [g.buf.clone() for g in self.outs]


def forward_O(c, ins):
    """O from the project's forward kernel on the case's operands -> per utterance [Tq, H, hd] fp64"""
    from speechclip_amd import ops
    D = c.H * c.hd
    q, k, v = (_rows(c, ins, i) for i in range(3))
    kl = _i32(c.klens)
    if c.group == "hdq1":
        kv = torch.cat([k, v], 1).contiguous().cuda()
        o = ops.attention_hd(q.cuda(), kv, kv[:, D:], c.B, c.H, 1, c.T, c.hd, (D, D), (c.T * 2 * D, 2 * D), kl, drop_p=c.p, seed=c.seed).view(c.B, D)
    else:
        qkv = torch.cat([q, k, v], 1).contiguous().cuda()
        if c.group == "packed":
            o = ops.attention_packed(qkv, c.B, c.T, c.H, kl, _i32(A.offsets(c.rows)), drop_p=c.p, seed=c.seed)
        elif c.group == "uniform":
            o = ops.attention(qkv, c.B, c.T, c.H, kl, drop=(c.p, c.seed) if c.p else None)
        else:
            assert abs(c.scale - c.hd ** -0.5) < 1e-12
            o = ops.attention_hd_qkv(qkv, c.B, c.T, c.H, kl, drop_p=c.p, seed=c.seed)
    o = o.cpu().to(F64)
    off = A.offsets([c.tq(b) for b in range(c.B)])
    return [o[off[b]:off[b + 1]].reshape(-1, c.H, c.hd) for b in range(c.B)]


def check_case(c):
    t0 = time.time()
    ins = A.case_inputs(c.id)
    O = forward_O(c, ins) if c.o_src == "fwd" else A.cpu_O(c, ins)
    R = A.case_reference(c, O, ins)
    run = Run(c, ins, O)
    got = run.results(c.id)
    line = [c.id]
    for op in A.OPS:
        w, n, _, at = A.judge_op(f"{c.id} {op}", got[op], R.ref[op], R.b32[op], R.bbf[op])
        assert n == A.n_elements(c, op), (c.id, op, n)
        assert w <= 1.0, (c.id, op, "err / bound", w, "(flat index, got, ref, bound)", at)
        line.append(f"{op} {w:.3f}")
        if A.participating(c, op) >= A.SLOPE_MIN:
            d, thr = A.slope_check(got[op], R.ref[op], R.b32[op], R.vsum[op])
            print(f"{c.id} {op}: |slope - 1| {d:.3e} threshold {thr:.3e}")
            assert d <= thr, (c.id, op, "slope", d, thr)
            line.append(f"slope {d / thr:.3f}")
        else:
            line.append("slope -")
        if c.form == "stored":
            w2, _, share, at = A.judge_op(f"{c.id} {op} vs the truth", got[op], R.truth[op], R.b32[op], R.bbf[op], R.extra[op])
            assert w2 <= 1.0, (c.id, op, "err / (bound + Delta term) against the truth", w2, at)
            line.append(f"truth {w2:.3f} Delta-share {share:.3f}")
    n_stat = sum(c.tq(b) for b in range(c.B)) * c.H
    for name, ref, e in (("lse", R.lse, R.e_lse), ("delta", R.delta, R.e_delta)):
        g, r, bd = A.cat(got[name]), A.cat(ref), A.cat(e)
        w, i = worst((g - r).abs(), bd)
        print(f"{c.id} workspace {name}: worst err/bound {w:.4f} over {g.numel()} values")
        assert g.numel() == n_stat and w <= 1.0, (c.id, name, w, i, float(g[i]), float(r[i]), float(bd[i]))
        line.append(f"{name} {w:.3f}")
    A.single_key_check(c, R)
    first = run.bits()
    for what, other in (("second call", Run(c, ins, O)), ("NaN on the rows that take no part", Run(c, ins, O, nan=True))):
        other.results(c.id + " " + what)
        assert all(torch.equal(x, y) for x, y in zip(first, other.bits())), (c.id, what, "not the same bits")
    print("PARITY| " + " | ".join(line) + f" | {time.time() - t0:.2f} s")


@pytest.mark.parametrize("cid", A.ids_of("packed"))
def test_packed_ragged_every_element_vs_fp64(cid):
    check_case(A.case(cid))


@pytest.mark.parametrize("cid", A.ids_of("uniform"))
def test_packed_uniform_every_element_vs_fp64(cid):
    check_case(A.case(cid))


@pytest.mark.parametrize("cid", A.ids_of("hd"))
def test_hd_full_rows_every_element_vs_fp64(cid):
    check_case(A.case(cid))


@pytest.mark.parametrize("cid", A.ids_of("hdq1"))
def test_hd_single_query_every_element_vs_fp64(cid):
    check_case(A.case(cid))


def test_case_counts():
    assert {g: len(A.ids_of(g)) for g in A.N_CASES} == A.N_CASES
    assert A.PACKED_KLENS.count(1) == 2 and A.case("packed-p0.1-cpu").p > 0          # two utterances with one valid key under dropout


@pytest.mark.parametrize("cid", [i for i in A.ids_of("uniform") if A.case(i).p == 0.0])
def test_row_off_and_uniform_addressing_and_both_entries_are_bitwise_equal(cid):
    """Without dropout: equal-length rows addressed through row_off = (0, T, 2T, ..) and as the uniform layout return the same bits, and so does head_dim 64
    through sc_attention_hd_bwd (one kernel set behind both entries; the same statistics kernel when nothing drops)."""
    c = A.case(cid)
    ins = A.case_inputs(cid)
    O = A.cpu_O(c, ins)
    uni, off = Run(c, ins, O), Run(c, ins, O, row_off=True)
    assert all(torch.equal(x, y) for x, y in zip(uni.bits(), off.bits())) and torch.equal(uni.ws.buf, off.ws.buf)
    a, b = uni.results(cid), Run(c, ins, O, entry="hd").results(cid + " hd entry")
    for op in A.OPS + ("lse", "delta"):
        assert all(torch.equal(x, y) for x, y in zip(a[op], b[op])), (cid, op)
    assert float(A.cat(a["dv"]).abs().sum()) > 0


# ---- the image chain of the padded layout: sc_attn_bwd_probs, sc_attn_softmax_bwd / _dropout / _heads, train_hubert.attention_bwd
def _judge_images(what, c, got, R):
    """got: {P, dS} -> [B, H, Lp, Lp]; every element of both images, the padding rows and columns up to Lp included (their bound is 0: exactly 0)"""
    out = []
    for n in ("P", "dS"):
        g = got[n].reshape(-1)
        r, bd = A.cat([im[n][0] for im in R.img]), A.cat([im[n][1] + im[n][2] for im in R.img])
        assert g.numel() == c.B * c.H * c.Lp * c.Lp == r.numel() and bool(torch.isfinite(g).all()), (what, n)
        w, i = worst((g - r).abs(), bd)
        print(f"{what} {n} image: worst err/bound {w:.4f} over {g.numel()} elements")
        assert w <= 1.0, (what, n, w, i, float(g[i]), float(r[i]), float(bd[i]))
        out.append(f"{n} {w:.3f}")
    return out


@pytest.mark.parametrize("cid", A.ids_of("image"))
def test_image_chain_every_element_vs_fp64(cid):
    """sc_attn_bwd_probs: the P and dS images per element.  The three sc_attn_softmax_bwd entries on GIVEN fp32 S / dP images (NaN wherever they may not read):
    _heads per element, the per-head entries bitwise equal to it.  At T >= 64 the whole chain, train_hubert.attention_bwd, per element of dq | dk | dv."""
    from speechclip_amd import _lib, ops
    from speechclip_amd.train_hubert import attention_bwd
    L_ = _lib.lib()
    t0 = time.time()
    c = A.case(cid)
    ins = A.case_inputs(cid)
    O = A.cpu_O(c, ins)
    R, Rg = A.case_reference(c, O, ins), A.case_reference(c, O, ins, given=True)
    B, H, L, Lp, D = c.B, c.H, c.T, c.Lp, c.H * 64
    q, k, v, dO = (_rows(c, ins, i) for i in range(4))
    qkv = torch.zeros(B * L + Lp - L, 3 * D, dtype=BF)          # with the slack rows train_hubert.attention_bwd requires
    qkv[:B * L] = torch.cat([q, k, v], 1)
    qkv, att, datt, kl = qkv.cuda(), _rows(c, ins, 0, O=O).cuda(), dO.cuda(), _i32(c.klens)
    p, seed, scale = float(c.p), c.seed & 0xffffffff, ctypes.c_float(c.scale)

    def images(call):
        gs = [Guarded(B * H * Lp, Lp, BF), Guarded(B * H * Lp, Lp, BF)]
        call(gs[0].win.data_ptr(), gs[1].win.data_ptr())
        torch.cuda.synchronize()
        return {n: g.check(cid + " " + n).view(B, H, Lp, Lp) for n, g in zip(("P", "dS"), gs)}

    def probs(P, dS):
        assert L_.sc_attn_bwd_probs(qkv.data_ptr(), qkv.data_ptr() + 2 * D, qkv.data_ptr() + 4 * D, 3 * D, datt.data_ptr(), att.data_ptr(), D, kl.data_ptr(), P, dS,
                                    B, H, L, Lp, scale, ctypes.c_float(p), seed, ops.stream()) == 0, L_.sc_last_error()
    got = images(probs)
    line = [cid] + _judge_images(cid + " sc_attn_bwd_probs", c, got, R)
    again = images(probs)
    assert all(torch.equal(got[n], again[n]) for n in got)
    # the given fp32 images: fp64 products of the bf16 operands, rounded to fp32; NaN on the keys >= klen and on the padding
    S, dP = torch.full((B, H, Lp, Lp), float("nan")), torch.full((B, H, Lp, Lp), float("nan"))
    for b in range(B):
        if c.nq(b):
            qh, kh, vh, dh = A.slices(c, b, ins)
            S[b, :, :L, :c.kl(b)], dP[b, :, :L, :c.kl(b)] = (qh @ kh.transpose(-1, -2)).float(), (dh @ vh.transpose(-1, -2)).float()
    S, dP = S.cuda(), dP.cuda()
    img = Lp * Lp

    def heads(P, dS):
        assert L_.sc_attn_softmax_bwd_heads(S.data_ptr(), dP.data_ptr(), Lp, img, datt.data_ptr(), D, att.data_ptr(), D, L, kl.data_ptr(), P, dS, L, Lp, B, H, scale,
                                            ctypes.c_float(p), seed, ops.stream()) == 0, L_.sc_last_error()

    def per_head(P, dS):
        for h in range(H):
            a = (S.data_ptr() + 4 * h * img, dP.data_ptr() + 4 * h * img, Lp, H * img, datt.data_ptr() + 128 * h, D, att.data_ptr() + 128 * h, D, L, kl.data_ptr(),
                 P + 2 * h * img, dS + 2 * h * img, L, Lp, B, scale)
            rc = L_.sc_attn_softmax_bwd_dropout(*a, ctypes.c_float(p), seed, H, h, ops.stream()) if p else L_.sc_attn_softmax_bwd(*a, ops.stream())
            assert rc == 0, L_.sc_last_error()
    gh = images(heads)
    line += ["given:"] + _judge_images(cid + " sc_attn_softmax_bwd_heads", c, gh, Rg)
    # utterances without a valid key: the per-head entries share the kernel, so the comparison is bit for bit everywhere
    ph = images(per_head)
    assert all(torch.equal(gh[n], ph[n]) for n in gh), (cid, "per-head entries differ from _heads")
    if L >= 64:
        dqkv = attention_bwd(qkv, att, datt, B, L, H, kl, (p, c.seed) if p else None).cpu().to(F64)
        assert dqkv.shape == (B * L, 3 * D)
        for j, op in enumerate(A.OPS):
            g = [dqkv[b * L:(b + 1) * L, j * D:(j + 1) * D].reshape(L, H, 64) for b in range(B)]
            w, n, _, at = A.judge_op(f"{cid} chain {op}", g, R.ref[op], R.b32[op], R.bbf[op])
            assert n == B * L * D and w <= 1.0, (cid, op, w, at)
            d, thr = A.slope_check(g, R.ref[op], R.b32[op], R.vsum[op])
            assert d <= thr, (cid, op, "slope", d, thr)
            line.append(f"chain {op} {w:.3f} slope {d / thr:.3f}")
    print("PARITY| " + " | ".join(line) + f" | {time.time() - t0:.2f} s")

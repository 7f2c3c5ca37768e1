"""CPU only: the MODEL errors behind the bounds of tests/test_attention_fwd_parity_gpu.py, the well-posedness of its references, and the sensitivity of its
bounds to the bugs an attention forward can have.  The twin of tools/packed_frontend_bounds.py; no kernel runs here.

For every case of the test (same builders, imported from the test module):
  * MODEL = per-row max|err| / max|ref| of a CPU model of a correct kernel (the fp64 reference with the kernel's documented roundings: probabilities rounded to the
    operand format after the dropout mask and rescale, one rounding of the output), maximum over all rows.  The test's bound is 4 x that + 1e-3.
  * the reference alone must be well-posed: finite, no row with max|ref| < 1e-2 (the 1e-3 floor never carries a row), the sentinel keys holding 5 % .. 95 % of the
    probability on the rows the mask mutants are judged on (the plain heads h % 4 < 2; the staircase heads concentrate a row on its last tile by construction).
  * MUTANT references must fall outside the case's bound: key length + 1 / - 1 (at least 90 % of the rows that see the key, on the plain heads; half of them under dropout), causal diagonal + 1 / - 1 (at
    least half of all rows, and every row next to a 64-key tile / 128- / 256-row block edge on the plain heads), causal key-tile count one short for the last query
    block (only the rows that see the last tile can move: a handful, one at T = 64 k + 1; one row outside the bound is what is required), the rescale skipped on a tile where the lazy online softmax moves its reference maximum, heads h and h ^ 1 swapped on V, dropped probabilities not
    rescaled, row sum over the dropped probabilities, pair stride T / 2 instead of ceil(T / 2) (odd T), the 16-bit halves of the hash swapped, and for the packed
    mask: the utterance's own length instead of Tmax, b * Tmax instead of row_off[b].

    python tools/attention_bounds.py            the table; exits non-zero if a check fails or a constant of the test is not reproduced
    python tools/attention_bounds.py --emit     the MODEL dict of the test, to paste"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_attention_fwd_parity_gpu as T   # noqa: E402
from test_dropout_gpu import _keep_rows      # noqa: E402

F64 = torch.float64
LOG2E = 1.4426950408889634


def metric_rows(a, b):
    """list over utterances of [T_b, H] row metrics"""
    return [T.row_metric(x, y) for x, y in zip(a, b)]


def online_ref(q, k, v, kl, scale, skip_tile=None, lazy_log2=8.0):
    """The kernel's recurrence for ONE head, non-causal: 64-key tiles, reference maximum moved only when the running maximum rose by more than `lazy_log2`.
    skip_tile: MUTANT -- on the first tile >= skip_tile that moves the maximum, O and the row sum are not rescaled (alpha = 1).
    -> (out [Tq, hd], tiles >= 1 on which some row rescaled, share of the rows that rescaled per tile >= 1; the kernel decides per row)"""
    qd, kd, vd = q.double(), k.double(), v.double()
    Tq = qd.shape[0]
    m_run = torch.full((Tq, 1), float("-inf"), dtype=F64)
    l = torch.zeros(Tq, 1, dtype=F64)
    o = torch.zeros(Tq, vd.shape[1], dtype=F64)
    moved, still, skipped = [], [], False
    for t in range((kl + 63) // 64):
        s = scale * (qd @ kd[t * 64: min(t * 64 + 64, kl)].t())
        m_cand = torch.maximum(m_run, s.amax(-1, keepdim=True))
        move = (m_cand - m_run) * LOG2E > lazy_log2
        alpha = torch.where(move, torch.exp(m_run - m_cand), torch.ones_like(m_run))
        m_run = torch.where(move, m_cand, m_run)
        if t > 0:
            still.append(move.double().mean().item())
        if t > 0 and move.any():
            moved.append(t)
            if skip_tile is not None and t >= skip_tile and not skipped:
                alpha, skipped = torch.ones_like(alpha), True
        P = torch.exp(s - m_run)
        l = l * alpha + P.sum(-1, keepdim=True)
        o = o * alpha + P @ vd[t * 64: min(t * 64 + 64, kl)]
    return o / l, moved, still


def keep_rows(seed, row_ids, n_keys, stride, p, swap=False):
    """test_dropout_gpu._keep_rows; swap: MUTANT -- the two 16-bit halves of every hash exchanged, i.e. the mask columns exchanged pairwise (generated over an even
    number of keys so that an odd last key has its partner)."""
    if not swap:
        return _keep_rows(seed, row_ids, n_keys, stride, p)
    m = _keep_rows(seed, row_ids, n_keys + (n_keys & 1), stride, p)
    return m.view(m.shape[0], -1, 2).flip(-1).reshape(m.shape[0], -1)[:, :n_keys].contiguous()


def probs(q, k, kl, scale, causal):
    """normalised probabilities [H, Tq, Tk] of one utterance (fp64)"""
    qd, kd = q.double().permute(1, 0, 2), k.double().permute(1, 0, 2)
    s = scale * (qd @ kd.transpose(-1, -2))
    j, i = torch.arange(k.shape[0])[None, :], torch.arange(q.shape[0])[:, None]
    valid = (j < kl).expand(q.shape[0], k.shape[0])
    if causal:
        valid = valid & (j <= i)
    return torch.softmax(s.masked_fill(~valid[None], float("-inf")), -1)


def edge_rows(Tn):
    """rows next to a 64-key tile edge (128- and 256-row block edges are among them), and the last row"""
    r = torch.arange(Tn)
    return ((r % 64 >= 62) | (r % 64 <= 1) | (r == Tn - 1)) & (r >= 2)


def plain_heads(c):
    return [h for h in range(c.H) if h % 4 < 2 or c.p > 0.0]


class Report:
    def __init__(self, quiet=False):
        self.fail, self.quiet = [], quiet

    def line(self, s):
        if not self.quiet:
            print(s)

    def need(self, ok, what):
        if not ok:
            self.fail.append(what)
            self.line("   FAILED: " + what)


def exceed(c, mut, ref, bound):
    """list over utterances of bool [T_b, H]: rows the mutant moves out of the bound"""
    return [m > bound for m in metric_rows(mut, ref)]


def frac(mask_list, sel=None):
    n = sum(int(m.numel() if sel is None else m[sel[i]].numel()) for i, m in enumerate(mask_list))
    k = sum(int(m.sum() if sel is None else m[sel[i]].sum()) for i, m in enumerate(mask_list))
    return k, n


def check_case(c, rep, mutants=True):
    """-> the case's MODEL value"""
    ins = T.case_inputs(c.id)
    ref = T.case_reference(c)
    mod = T.case_reference(c, model=True)
    model = max(m.max().item() for m in metric_rows(mod, ref))
    bound = T.bound_of(model)
    amax = torch.cat([r.abs().amax(-1).flatten() for r in ref])
    n_zero = int((amax == 0).sum())              # dropout: a row whose every valid key was dropped is exactly zero in the reference (the kernel must give exact zeros)
    rmin = amax[amax > 0].min().item()
    rep.need(n_zero == 0 or c.p > 0, f"{c.id}: {n_zero} all-zero reference rows without dropout")
    rep.need(all(torch.isfinite(r).all() for r in ref), f"{c.id}: non-finite reference")
    rep.need(rmin >= 1e-2, f"{c.id}: a reference row has max|ref| = {rmin:.2e} < 1e-2")
    const = T.MODEL.get(c.id)
    rep.need(const is not None and abs(const - model) <= 0.02 * model, f"{c.id}: MODEL constant in the test {const} is not the value computed here {model:.3e}")
    notes = []
    if not mutants:
        rep.line(f"{c.id:28s} model {model:.3e} bound {bound:.3e} min max|ref| {rmin:.2e}")
        return model
    ph = plain_heads(c)
    nq = [r.shape[0] for r in ref]

    # ---- sentinel shares on the plain heads
    lo, hi = 1.0, 0.0
    for b, (q, k, v) in enumerate(ins):
        kl = min(c.klens[b], c.rows[b])
        P = probs(q[:nq[b]], k, kl, c.scale, c.causal)[ph]
        if c.causal:
            rows = torch.nonzero(edge_rows(c.rows[b]) & (torch.arange(c.rows[b]) < kl)).flatten()
            sh = P[:, rows, rows] if len(rows) else None
        else:
            sh = P[:, :, kl - 1] if kl >= 2 else None
        if sh is not None and sh.numel():
            lo, hi = min(lo, sh.min().item()), max(hi, sh.max().item())
    if hi > 0:
        rep.need(0.05 <= lo and hi <= 0.95, f"{c.id}: sentinel share {lo:.3f} .. {hi:.3f} outside 5 % .. 95 %")
        notes.append(f"share {lo:.2f}..{hi:.2f}")

    def judge(name, mut, need_all=None, need_frac=None, part=1.0):
        ex = exceed(c, mut, ref, bound)
        k, n = frac(ex)
        ok = k >= 1
        txt = f"{name} {k}/{n}"
        if need_frac is not None:
            ok = ok and k >= need_frac * n
        if need_all is not None:                    # list over utterances of (row mask or None); heads: the plain ones
            ka = na = 0
            for b, rows in enumerate(need_all):
                if rows is None:
                    continue
                sub = ex[b][rows][:, ph]
                ka, na = ka + int(sub.sum()), na + sub.numel()
            ok = ok and ka >= part * na
            txt += f" (judged rows {ka}/{na})"
        rep.need(ok, f"{c.id}: mutant '{name}' stays inside the bound: {txt}")
        notes.append(txt)

    every = lambda b: torch.ones(nq[b], dtype=torch.bool)
    # ---- key length +1 / -1
    if c.group != "causal" or c.klens != c.rows:
        plus = tuple(min(kl + 1, r) for kl, r in zip(c.klens, c.rows))
        minus = tuple(kl - 1 for kl in c.klens)
        part = 0.9 if c.p == 0.0 else 0.5           # of the rows that see the key; with dropout the sentinel key itself is dropped on a share p of the rows
        vis = lambda b, kl: (torch.arange(nq[b]) >= kl - 1) if c.causal else every(b)      # causal: rows that see the key in question
        if plus != tuple(c.klens):
            judge("klen+1", T.case_reference(c, klens=plus), need_all=[vis(b, c.klens[b] + 1) if plus[b] != c.klens[b] else None for b in range(c.B)], part=part)
        judge("klen-1", T.case_reference(c, klens=minus), need_all=[vis(b, c.klens[b]) for b in range(c.B)], part=part)
    # ---- causal diagonal and tile count
    if c.causal:
        if c.T > 1:
            for d in (1, -1):
                # + 1 admits key i + 1 (rows below the last valid key); - 1 drops key i (row 0 would be empty: it keeps its key)
                mut = T.case_reference(c, diag=d)
                if d == -1:
                    mut = [torch.cat([r[:1], m[1:]]) for r, m in zip(ref, mut)]
                rows = [edge_rows(c.rows[b]) & (torch.arange(c.rows[b]) < min(c.klens[b], c.rows[b]) - (1 if d == 1 else 0)) for b in range(c.B)]
                judge(f"diag{d:+d}", mut, need_all=rows, need_frac=0.5 if c.klens == c.rows else None)
        rows_blk = 128 if c.T <= 128 else 256
        q0 = (c.T - 1) // rows_blk * rows_blk
        lim, any_lim = [], False
        for b in range(c.B):
            nkv = min((min(c.klens[b], c.T) + 63) // 64, (c.T + 63) // 64)
            l_ = torch.full((c.T,), c.T + 1)
            if nkv >= 2:
                l_[q0:] = (nkv - 1) * 64
                any_lim = True
            lim.append(l_)
        if any_lim:
            judge("tiles-1", T.case_reference(c, key_limit=lim))
    # ---- V heads swapped
    if c.H >= 2:
        perm = [h ^ 1 if (h ^ 1) < c.H else h for h in range(c.H)]
        judge("v-heads", T.case_reference(c, ins=[(q, k, v[:, perm]) for q, k, v in ins]))
    # ---- lazy rescale: the recurrence restates the softmax; a skipped rescale does not
    if not c.causal and c.p == 0.0:
        worst_same, hit, found = 0.0, 0, 0
        for b, (q, k, v) in enumerate(ins):
            kl = min(c.klens[b], c.rows[b])
            for h in range(c.H):
                if h % 4 < 2 or kl <= 64:
                    continue
                same, moved, still = online_ref(q[:nq[b], h], k[:, h], v[:, h], kl, c.scale)
                if h % 4 == 2 and kl > 128:      # staircase head, three tiles or more: the step under the threshold leaves tile 1 without a rescale, the step over it rescales on every tile
                    ok = min(still) <= 0.5 and max(still) == 1.0 if b % 2 == 0 else min(still) >= 0.8      # under: some tile keeps the lagging maximum on half the rows or more; over: every tile rescales on 80 % of the rows or more
                    rep.need(ok, f"{c.id}: staircase head {h} of utterance {b} ({'under' if b % 2 == 0 else 'over'}): share of rows that rescale per tile {still}")
                worst_same = max(worst_same, (same - ref[b][:, h]).abs().max().item())
                if moved:
                    found += 1
                    mut, _, _ = online_ref(q[:nq[b], h], k[:, h], v[:, h], kl, c.scale, skip_tile=moved[-1])
                    hit += int((T.row_metric(mut, ref[b][:, h]) > bound).all())
        if found:
            rep.need(worst_same < 1e-9, f"{c.id}: the lazy recurrence differs from the softmax by {worst_same:.1e}")
            rep.need(hit == found, f"{c.id}: mutant 'alpha=1' inside the bound on {found - hit} of {found} (utterance, head) pairs")
            notes.append(f"alpha=1 {hit}/{found} heads (recurrence == softmax to {worst_same:.0e})")
    # ---- dropout
    if c.p > 0.0:
        judge("no-rescale", T.case_reference(c, drop_rescale=False), need_frac=0.5)
        judge("sum-dropped", T.case_reference(c, sum_dropped=True), need_frac=0.5)
        off = T.offsets(c.rows)
        if c.group == "packed":
            ids = lambda b, base: ((base + np.arange(c.rows[b]))[None, :] * c.H + np.arange(c.H)[:, None]).reshape(-1)
            mk = lambda b, base, stride, swap=False: keep_rows(c.seed, ids(b, base), c.rows[b], stride, c.p, swap).view(c.H, c.rows[b], c.rows[b])
            st = (c.T + 1) // 2
            judge("swap-halves", T.case_reference(c, keeps=[mk(b, off[b], st, True) for b in range(c.B)]), need_frac=0.25)
            judge("own-length", T.case_reference(c, keeps=[mk(b, off[b], (c.rows[b] + 1) // 2) for b in range(c.B)]))
            judge("b*Tmax", T.case_reference(c, keeps=[mk(b, b * c.T, st) for b in range(c.B)]))
        else:
            mk = lambda stride, swap=False: list(keep_rows(c.seed, np.arange(c.B * c.H * c.T), c.T, stride, c.p, swap).view(c.B, c.H, c.T, c.T))
            judge("swap-halves", T.case_reference(c, keeps=mk((c.T + 1) // 2, True)), need_frac=0.25)
            if c.T % 2:
                judge("stride-T/2", T.case_reference(c, keeps=mk(c.T // 2)), need_frac=0.25)
    rep.line(f"{c.id:28s} model {model:.3e} bound {bound:.3e} min max|ref| {rmin:.2e} | " + "; ".join(notes))
    return model


REDUCED = ("fwd-bf16-T129", "fwd-f16-T257", "causal-bf16-T129", "causal-klens-f16-T257", "causal-klens-bf16-T65", "drop-p0.1-T131", "drop-causal-p0.25-T65",
           "hd96-L129", "hdq1-hd96")


def run(ids=None, quiet=False, mutants=True):
    rep = Report(quiet)
    models = {}
    for c in T.all_cases():
        if ids is None or c.id in ids:
            models[c.id] = check_case(c, rep, mutants)
    return models, rep.fail


def main():
    torch.manual_seed(0)
    if "--emit" in sys.argv:
        models, _ = run(quiet=True, mutants=False)
        line = "MODEL = {"
        for k, v in models.items():
            item = f'"{k}": {v:.2e}, '
            if len(line) + len(item) > 160:
                print(line.rstrip())
                line = "    "
            line += item
        print(line.rstrip() + "\n}")
        return 0
    models, fail = run(REDUCED if "--reduced" in sys.argv else None)
    groups = {}
    for k, v in models.items():
        g = T.case(k).group + "/" + T.case(k).dtype
        groups.setdefault(g, []).append(v)
    for g, vals in groups.items():
        print(f"== {g}: {len(vals)} cases, model {min(vals):.2e} .. {max(vals):.2e} -> bounds {T.bound_of(min(vals)):.2e} .. {T.bound_of(max(vals)):.2e}")
    print("FAILED: %d checks" % len(fail) if fail else "all checks passed")
    return 1 if fail else 0


if __name__ == "__main__":
    sys.exit(main())

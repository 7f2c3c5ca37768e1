"""Search by threshold on the MI355X (sc_search_range_count / _fill and their bf16 forms, ops.search_range*, EmbeddingIndex.search_range,
KWClipBase.search_range) against the host statement of tests/search_range_ref.py.  Every comparison is bitwise: lims, positions and the bits of the scores.
Score bits come from tests/search_ref.py (fp32: exact integers through scores64, real rows through the exact chain restatement) and, for bf16 rows, from
ops.search_topk_bf16 over windows of <= 128 rows (search_range_ref.window_scores_bf16) -- never from the entries under test.

Measured on the MI355X: every test below holds; the whole file takes 4 s.  Timings of the entries: profiles/search_range_bench.txt."""
import dataclasses

import numpy as np
import pytest
import torch

import search_bf16_ref as RB
import search_range_ref as RR
import search_ref as R

pytestmark = pytest.mark.gpu

FORMATS = ["fp32", "bf16"]


def int_rows(rng, n, E):
    return rng.integers(-8, 9, size=(n, E)).astype(np.float32)


def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def dev(a, fmt):
    """host fp32 rows -> device rows in the storage type (bf16: the rows must already be bf16 numbers)."""
    if fmt == "fp32":
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return torch.from_numpy(RB.bf16_bits(a)).view(torch.bfloat16).cuda()


def entry(fmt):
    from speechclip_amd import ops
    return ops.search_range if fmt == "fp32" else ops.search_range_bf16


def run(fmt, q, g, thresh, **kw):
    """host rows and thresholds -> host (lims, vals, idx)"""
    qd = q if torch.is_tensor(q) else dev(q, fmt)
    gd = g if torch.is_tensor(g) else dev(g, fmt)
    for name in ("g_item", "q_skip"):
        if kw.get(name) is not None:
            kw[name] = torch.from_numpy(np.asarray(kw[name], np.int32)).cuda()
    out = entry(fmt)(qd, gd, torch.from_numpy(np.asarray(thresh, np.float32)).cuda(), **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def int_scores(q, g):
    """Integer operands whose sums stay below 2^24: the fmaf chain and the bf16 MFMA sum are both exact, so both formats form these bits."""
    s = R.scores64(q, g)
    assert np.abs(q).astype(np.float64).sum(1).max(initial=0) * 8 < 2 ** 24
    return (s + 0.0).astype(np.float32)


def own_thresholds(score, rng):
    """One threshold per query FROM ITS OWN SCORE VALUES, so that ties sit on it: the score of gallery row 0 (the row the caller repeats across the tile and
    range edges) for every third query, else the score at a rank that moves through the row with i."""
    Q, N = score.shape
    t = np.empty(Q, np.float32)
    for i in range(Q):
        srt = np.sort(score[i][~np.isnan(score[i])])[::-1]
        t[i] = score[i, 0] if i % 3 == 0 else srt[(37 * i + 10) % len(srt)]
    return t


# ---------------------------------------------------------------------------------------- 1. exact-integer arm
# (Q, N, E fp32, E bf16, n_split): every value of every parameter at least once, on both tile widths (Q <= 64 / Q > 64); (1, 1, .., 7) and (3, 5, .., 7) have
# trailing ranges that are empty; n_split = 0 at N = 4097 gives 16 ranges.
INT_CASES = [(1, 1, 4, 16, 7), (1, 4097, 64, 64, 0), (63, 127, 8, 16, 1), (64, 128, 64, 64, 2), (65, 129, 100, 80, 7), (129, 257, 512, 512, 0),
             (129, 4097, 8, 16, 0), (5, 4097, 100, 80, 7), (64, 257, 4, 16, 2), (3, 5, 8, 16, 7)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q,N,E32,E16,n_split", INT_CASES)
def test_exact_integers_equal_the_host_statement_in_every_bit(fmt, Q, N, E32, E16, n_split):
    rng = np.random.default_rng(1000 * Q + N)
    E = E32 if fmt == "fp32" else E16
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    S = n_split or R.search_splits(Q, N, 1)
    per = -(-N // S)
    for edge in set(range(128, N + 1, 128)) | {s * per for s in range(1, S)}:     # one row on both sides of every tile and range edge
        for p in (edge - 1, edge, edge + 1):
            if 0 < p < N:
                g[p] = g[0]
    score = int_scores(q, g)
    thresh = own_thresholds(score, rng)
    want = RR.search_range(score, thresh, idx_base=7)
    got = run(fmt, q, g, thresh, n_split=n_split, idx_base=7)
    print(f"{fmt} Q={Q} N={N} E={E} n_split={n_split} (S={S}): {want[0][-1]} hits, got {got[0][-1]}")
    assert RR.same(got, want)
    assert want[0][-1] > 0 and (N < 128 or (np.diff(want[0]) > 1).any())


# ---------------------------------------------------------------------------------------- 2. dense rows, empty rows, and independence of the other queries
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q", [6, 70])
def test_dense_and_empty_rows_mixed_with_selective_ones_equal_their_runs_alone(fmt, Q):
    rng = np.random.default_rng(7)
    N, E = 300, 64
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    score = int_scores(q, g)
    thresh = own_thresholds(score, rng)
    thresh[0::6], thresh[2::6], thresh[3::6] = -np.inf, np.inf, np.nan
    for n_split in (1, 3):
        want = RR.search_range(score, thresh)
        got = run(fmt, q, g, thresh, n_split=n_split)
        assert RR.same(got, want), n_split
        counts = np.diff(got[0])
        assert (counts[0::6] == N).all() and (counts[2::6] == 0).all() and (counts[3::6] == 0).all() and 0 < counts[1] < N
        for i in list(range(6)) + [Q - 1]:                                        # the slice of query i does not depend on the call around it
            alone = run(fmt, q[i:i + 1], g, thresh[i:i + 1], n_split=(n_split % 3) + 1)
            lo, hi = got[0][i], got[0][i + 1]
            assert RR.same(alone, (np.array([0, hi - lo]), want[1][lo:hi], want[2][lo:hi])), (n_split, i)


# ---------------------------------------------------------------------------------------- 3. real arm
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N,E32,E16", [(300, 512, 512), (4097, 100, 80), (4097, 512, 512), (300, 100, 80)])
def test_real_rows_at_the_tenth_score_return_the_top_k_entrys_first_ten(fmt, N, E32, E16):
    from speechclip_amd import ops
    E = E32 if fmt == "fp32" else E16                                             # bf16 rows take multiples of 16 only: 80 stands where fp32 has 100
    rng = np.random.default_rng(N + E)
    Q, K = 5, 10
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    if fmt == "bf16":
        q, g = RB.round_bf16(q), RB.round_bf16(g)
    g[11] = g[3]                                                                  # an exact tie inside the gallery
    qd, gd = dev(q, fmt), dev(g, fmt)
    topk = ops.search_topk if fmt == "fp32" else ops.search_topk_bf16
    tv, ti = (t.cpu().numpy() for t in topk(qd, gd, K + 6))
    thresh = tv[:, K - 1].copy()
    assert (tv[:, -1] < thresh).all()                                             # the list reaches past every tie of the 10th score
    lims, vals, idx = run(fmt, qd, gd, thresh)
    if fmt == "bf16":                                                             # every pair, hits and misses, against the bits of the bf16 top-K entry
        assert RR.same((lims, vals, idx), RR.search_range(RR.window_scores_bf16(ops, qd, gd), thresh))
    for i in range(Q):
        keep = tv[i] >= thresh[i]
        o = np.argsort(ti[i][keep])
        lo, hi = lims[i], lims[i + 1]
        assert hi - lo == keep.sum() >= K
        assert np.array_equal(idx[lo:hi], ti[i][keep][o]) and np.array_equal(vals[lo:hi].view(np.uint32), tv[i][keep][o].view(np.uint32)), i
        if fmt == "fp32":                                                         # the whole hit list against the exact chain restatement
            chain = np.array([R.fmaf_chain(q[i], g[j]) for j in idx[lo:hi]], np.float32)
            assert np.array_equal(vals[lo:hi].view(np.uint32), chain.view(np.uint32)), i


# ---------------------------------------------------------------------------------------- 4. guards
@pytest.mark.parametrize("fmt", FORMATS)
def test_strides_nan_rows_sentinels_and_empty_calls(fmt):
    from speechclip_amd import ops
    rng = np.random.default_rng(4)
    Q, N, E, ld = 9, 300, 80, 96
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    g[[5, 128, 299]] = np.nan                                                     # NaN gallery rows: never a hit, not even at -inf
    score = int_scores(q, np.nan_to_num(g))
    score[:, [5, 128, 299]] = np.nan
    thresh = own_thresholds(score, rng)
    thresh[4] = -np.inf
    want = RR.search_range(score, thresh, idx_base=3)
    assert not np.isin(want[2] - 3, [5, 128, 299]).any() and want[0][5] - want[0][4] == N - 3
    dtype = torch.float32 if fmt == "fp32" else torch.bfloat16

    def guarded(a):                                                               # rows between NaN guard rows, NaN in the gap behind column E
        buf = torch.full((a.shape[0] + 2, ld), float("nan"), device="cuda", dtype=dtype)
        buf[1:-1, :E] = dev(a, fmt)
        return buf[1:-1, :E]
    qd, gd, td = guarded(q), guarded(g), torch.from_numpy(thresh).cuda()
    assert qd.stride(0) == ld and gd.stride(0) == ld
    for n_split in (1, 3):
        assert RR.same(run(fmt, qd, gd, thresh, n_split=n_split, idx_base=3), want)
        # the two passes by hand: a counts table wider than the split count, outputs of exactly T entries between sentinels, all pre-filled with garbage
        table = torch.full((Q, n_split + 4), -77, device="cuda", dtype=torch.int32)
        ops.search_range_count(qd, gd, td, n_split, out=table[:, 2:2 + n_split])
        assert (table[:, :2] == -77).all() and (table[:, 2 + n_split:] == -77).all()
        lims, offs, T = ops.search_range_offsets(table[:, 2:2 + n_split].contiguous())
        assert T == want[0][-1] and np.array_equal(lims.cpu().numpy(), want[0])
        wide = torch.full((Q, n_split + 3), -1, device="cuda", dtype=torch.int64)  # offsets with a row stride above the split count
        wide[:, 1:1 + n_split] = offs
        vbuf = torch.full((T + 8,), float("nan"), device="cuda")
        ibuf = torch.full((T + 8,), -99, device="cuda", dtype=torch.int64)
        ops.search_range_fill(qd, gd, td, wide[:, 1:1 + n_split], vbuf[4:4 + T], ibuf[4:4 + T], n_split, 3)
        torch.cuda.synchronize()
        assert torch.isnan(vbuf[:4]).all() and torch.isnan(vbuf[4 + T:]).all() and (ibuf[:4] == -99).all() and (ibuf[4 + T:] == -99).all()
        assert RR.same((lims.cpu().numpy(), vbuf[4:4 + T].cpu().numpy(), ibuf[4:4 + T].cpu().numpy()), want)
    # Q == 0: nothing is launched; T == 0: nothing is filled
    lims, vals, idx = entry(fmt)(qd[:0], gd, td[:0])
    assert lims.tolist() == [0] and vals.numel() == 0 and idx.numel() == 0 and lims.dtype == idx.dtype == torch.int64 and vals.dtype == torch.float32
    lims, vals, idx = entry(fmt)(qd, gd, torch.full((Q,), float("inf"), device="cuda"))
    assert lims.tolist() == [0] * (Q + 1) and vals.numel() == 0 and idx.numel() == 0
    with pytest.raises(ValueError, match=rf"{want[0][-1]} hits exceed max_results={want[0][-1] - 1}"):
        entry(fmt)(qd, gd, td, max_results=int(want[0][-1]) - 1)


# ---------------------------------------------------------------------------------------- 5. skip codes
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("Q", [7, 66])
def test_skip_codes_leave_out_the_own_item_and_nothing_else(fmt, Q):
    rng = np.random.default_rng(5)
    N, E = 301, 64
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    items = (np.arange(N) // 5).astype(np.int32)                                  # five rows per item
    skip = np.array([[i % (N // 5), -1, 10 ** 6][i % 3] for i in range(Q)], np.int32)
    score = int_scores(q, g)
    thresh = own_thresholds(score, rng)
    for i in range(0, Q, 3):                                                      # the own item's rows would be hits: the threshold is at their lowest score
        thresh[i] = score[i, items == skip[i]].min()
    thresh[1] = -np.inf
    for n_split in (0, 1, 3):
        want = RR.search_range(score, thresh, 7, items, skip)
        got = run(fmt, q, g, thresh, n_split=n_split, idx_base=7, g_item=items, q_skip=skip)
        assert RR.same(got, want), n_split
        assert not (items[got[2][got[0][0]:got[0][1]] - 7] == skip[0]).any()
        plain = RR.search_range(score, thresh, 7)
        assert want[0][-1] <= plain[0][-1] - 5 * len(range(0, Q, 3))
        assert RR.same(run(fmt, q, g, thresh, n_split=n_split, idx_base=7, g_item=items), plain)          # a null q_skip: the plain result
        assert RR.same(run(fmt, q, g, thresh, n_split=n_split, idx_base=7), plain)


# ---------------------------------------------------------------------------------------- 6. index and model
@pytest.mark.parametrize("kind", ["fp32", "bf16", "shadow"])
def test_index_three_adds_equal_one_add_with_ids_exclude_and_per_query_scores(kind):
    from speechclip_amd.module import EmbeddingIndex
    rng = np.random.default_rng(6)
    E, N, Q = 64, 700, 70
    feats = torch.from_numpy(rng.standard_normal((N, E)).astype(np.float32)).cuda()
    feats[300] = feats[20]
    queries = torch.from_numpy(rng.standard_normal((Q, E)).astype(np.float32)).cuda()
    names = [f"item{n // 5}" for n in range(N)]
    make = lambda: EmbeddingIndex(E, storage="bf16" if kind == "bf16" else "fp32", shadow=kind == "shadow")
    one = make().add(feats, names)
    three = make().add(feats[:300], names[:300]).add(feats[300:301], names[300:301]).add(feats[301:], names[301:])
    assert len(one) == len(three) == N and len(three.segments) == 3
    top_v, top_p, _ = one.search(queries, 12)
    min_score = top_v[torch.arange(Q), 7 + torch.arange(Q) % 4]                   # one value per query: its 8th to 11th score
    a = one.search_range(queries, min_score)
    b = three.search_range(queries, min_score)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu())
    assert a[3] == b[3] == [names[p] for p in a[2].cpu().tolist()]
    lims, scores, pos = (t.cpu().numpy() for t in a[:3])
    tv, tp = top_v.cpu().numpy(), top_p.cpu().numpy()
    for i in range(Q):                                                            # the hits are `search`'s first rows, in ascending position, bit for bit
        keep = tv[i] >= min_score[i].item()
        o = np.argsort(tp[i][keep])
        assert keep.sum() < 12 and np.array_equal(pos[lims[i]:lims[i + 1]], tp[i][keep][o])
        assert np.array_equal(scores[lims[i]:lims[i + 1]].view(np.uint32), tv[i][keep][o].view(np.uint32))
    assert (np.diff(lims) >= 8).all()
    # one float for all queries, a host sequence, and exclude
    t = float(np.sort(tv[:, 9])[Q // 2])
    c = three.search_range(queries, t)
    d = three.search_range(queries, [t] * Q)
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(c[:3], d[:3])) and c[3] == d[3]
    own = [names[p] for p in tp[:, 0]]
    e = three.search_range(queries, t, exclude=own)
    el, cl, cp = e[0].cpu().numpy(), c[0].cpu().numpy(), c[2].cpu().numpy()
    assert own[0] not in e[3][el[0]:el[1]] and e[0][-1] < c[0][-1]
    for i in range(Q):
        kept = [p for p in cp[cl[i]:cl[i + 1]] if names[p] != own[i]]
        assert e[2][el[i]:el[i + 1]].cpu().tolist() == kept
    assert torch.equal(three.search_range(queries, t, exclude=[None] * Q)[2], c[2])
    with pytest.raises(ValueError, match="hits exceed max_results=3"):
        three.search_range(queries, t, max_results=3)
    with pytest.raises(ValueError, match="min_score must be"):
        three.search_range(queries, [t, t])
    none = three.search_range(queries, 2.0)
    assert none[0].tolist() == [0] * (Q + 1) and none[1].numel() == 0 and none[3] == []


@pytest.fixture(scope="module")
def model():
    from helpers import make_config
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.hubert import HubertConfig
    torch.manual_seed(3)
    return KWClip_GeneralTransformer(make_config(d_model=128, branch_heads=4, hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())),
                                                 clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))).cuda().eval()


def test_model_search_range_by_speech_agrees_with_thresholding_the_full_search(model):
    g = torch.Generator().manual_seed(72)
    images = torch.randn(12, 3, 64, 64, generator=g).cuda()
    wavs = [0.3 * torch.randn(n, generator=g).cuda() for n in (8000, 6000, 3000, 5000)]
    names = [f"img{n}.jpg" for n in range(12)]
    index = model.build_index(images=images, ids=names, batch_size=5)
    full_v, full_p, _ = model.search(index, len(index), wav=wavs)                 # 12 rows: every score of every query
    min_score = full_v[:, 4].clone()                                              # the fifth score of every query: at least five hits each
    lims, scores, pos, ids = model.search_range(index, min_score, wav=wavs)
    assert not model.training and lims.tolist()[0] == 0 and (torch.diff(lims) >= 5).all() and lims[-1].item() < 4 * 12
    fv, fp = full_v.cpu().numpy(), full_p.cpu().numpy()
    lims, scores, pos = lims.cpu().numpy(), scores.cpu().numpy(), pos.cpu().numpy()
    for i in range(4):
        keep = fv[i] >= min_score[i].item()
        o = np.argsort(fp[i][keep])
        assert np.array_equal(pos[lims[i]:lims[i + 1]], fp[i][keep][o])
        assert np.array_equal(scores[lims[i]:lims[i + 1]].view(np.uint32), fv[i][keep][o].view(np.uint32))
    assert ids == [names[p] for p in pos]
    with pytest.raises(ValueError):
        model.search_range(index, 0.0, images=images, wav=wavs)

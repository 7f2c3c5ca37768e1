"""Gallery search inside a subset on the MI355X (sc_search_select / sc_search_select_bf16 / sc_pack_row_mask, EmbeddingIndex.search(allow=, allow_ids=,
within=, row_groups=, query_groups=), KWClipBase.search) against the host statement of tests/search_select_ref.py.  Everything but the bf16 real-operand
check is equality of bits: the scores are exact integers, or the scores of sc_search_items on the gathered eligible rows; what is judged is the selection.

Every call of the entries goes through `call`: outputs between sentinel guards, the workspace of exactly the stated size between guards and pre-filled
(0xFF bytes: NaN values and -1 indices; 0x00 bytes: score 0.0 at position 0, which a list left unwritten would leak into the merge)."""
import dataclasses

import numpy as np
import pytest
import torch

import search_bf16_ref as R16
import search_items_ref as RI
import search_ref as R
import search_select_ref as RS

pytestmark = pytest.mark.gpu

FORMATS = ("fp32", "bf16")


def dev(a, fmt):
    """Host fp32 array (bf16 numbers for fmt == "bf16") or a device tensor -> device rows of the format."""
    if torch.is_tensor(a):
        return a
    if fmt == "bf16":
        return torch.from_numpy(np.ascontiguousarray(R16.bf16_bits(a))).view(torch.bfloat16).cuda()
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def i32(a):
    """int32 host array, or uint32 mask words (handed over by their bits), or a device tensor, or None -> device tensor or None."""
    if a is None or torch.is_tensor(a):
        return a
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32)).cuda()


def call(fmt, q, g, k, items, words=None, g_group=None, q_group=None, skip=None, distinct=False, n_split=0, idx_base=0, fill=0xFF):
    """-> device (vals [Q, k], idx [Q, k], items [Q, k]) of sc_search_select[_bf16]."""
    from speechclip_amd._lib import lib, stream
    L = lib()
    q, g, items, words, g_group, q_group, skip = dev(q, fmt), dev(g, fmt), i32(items), i32(words), i32(g_group), i32(q_group), i32(skip)
    (Q, E), N = q.shape, g.shape[0]
    assert words is None or words.numel() == (N + 31) // 32
    nbytes = L.sc_search_items_workspace_bytes(Q, N, k, n_split)
    assert nbytes == RI.workspace_bytes(Q, N, k, n_split)
    ws = torch.full((nbytes + 128,), 0xA5, device="cuda", dtype=torch.uint8)
    ws[64:64 + nbytes] = fill
    vals = torch.full((Q * k + 32,), 12345.0, device="cuda")
    idx = torch.full((Q * k + 32,), -777, device="cuda", dtype=torch.int64)
    its = torch.full((Q * k + 32,), -555, device="cuda", dtype=torch.int32)
    p = lambda t: None if t is None else t.data_ptr()
    entry = L.sc_search_select_bf16 if fmt == "bf16" else L.sc_search_select
    rc = entry(q.data_ptr(), q.stride(0), g.data_ptr(), g.stride(0), Q, N, E, k, n_split, idx_base, p(words), p(g_group), p(q_group), items.data_ptr(), p(skip),
               int(distinct), vals[16:].data_ptr(), idx[16:].data_ptr(), its[16:].data_ptr(), ws[64:].data_ptr() if nbytes else None, stream())
    assert rc == 0, L.sc_last_error()
    torch.cuda.synchronize()
    assert (ws[:64] == 0xA5).all() and (ws[-64:] == 0xA5).all()
    for buf, guard in ((vals, 12345.0), (idx, -777), (its, -555)):
        assert (buf[:16] == guard).all() and (buf[-16:] == guard).all()
    return tuple(b[16:-16].view(Q, k) for b in (vals, idx, its))


def host(t):
    return tuple(x.cpu().numpy() for x in t)


def same(a, b):
    """Bit equality of (vals, idx[, items]) triples or pairs, device tensors or host arrays."""
    a = [x.cpu().numpy() if torch.is_tensor(x) else x for x in a]
    b = [x.cpu().numpy() if torch.is_tensor(x) else x for x in b]
    return len(a) == len(b) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def unit_rows(rng, n, E, fmt="fp32"):
    x = rng.standard_normal((n, E))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return R16.round_bf16(x) if fmt == "bf16" else x


# ---------------------------------------------------------------------------------------- (a) (e) (f) the case list on exact-integer operands
@pytest.mark.parametrize("N", RS.NS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_integer_operands_match_the_host_statement_bit_for_bit_at_every_split(fmt, N):
    """Every mask of the list at this N, with the Q, K, E and group variant the list gives it: the result equals the statement at 1, 3 and 7 splits (ranges
    that cut words and tiles), whatever the workspace held, and a second run returns the same bits."""
    for case in (c for c in RS.CASES if c.N == N):
        o = RS.operands(case, fmt)
        s = R.scores64(o["q"], o["g"])
        assert np.array_equal(s, np.rint(s)) and np.abs(s).max() <= 4 * RS.ES[fmt][case.e]
        want = RS.search(s, o["items"], case.K, o["words"], o["g_group"], o["q_group"], o["skip"], o["distinct"], idx_base=5)
        qd, gd = dev(o["q"], fmt), dev(o["g"], fmt)
        for S in RS.SPLITS:
            runs = [call(fmt, qd, gd, case.K, o["items"], o["words"], o["g_group"], o["q_group"], o["skip"], o["distinct"], S, 5, fill) for fill in (0xFF, 0x00)]
            assert same(runs[0], want), (case, S)
            assert same(runs[1], runs[0]), (case, S)
        if case.mask == "zeros":
            assert (want[1] == -1).all() and (want[2] == -1).all() and np.isneginf(want[0]).all()


# ---------------------------------------------------------------------------------------- (b) real operands
def real_case(fmt, E):
    """4133 rows, the first tile and a run of tiles in the middle dead, 30 % of the other rows allowed; two interleaved groups; five queries: no
    restriction, either group, a code no row carries, and a group with a skipped item."""
    rng = np.random.default_rng(7 + E)
    N, Q = 4133, 5
    q, g = unit_rows(rng, Q, E, fmt), unit_rows(rng, N, E, fmt)
    mask = rng.random(N) < 0.3
    mask[:150] = False
    mask[1000:1700] = False
    g[[400, 700]] = g[2000]                                                   # exact ties
    mask[[400, 700, 2000]] = True
    items = RI.grouped_items(rng, N, big=300)
    g_group = (np.arange(N) % 2).astype(np.int32)
    q_group = np.array([-1, 0, 1, 9, 0], np.int32)
    skip = np.array([-1, -1, int(items[401]), -1, int(items[2000])], np.int32)
    return q, g, mask, RS.pack_row_mask(mask), items, g_group, q_group, skip


def test_fp32_real_operands_equal_search_items_on_the_gathered_eligible_rows():
    from speechclip_amd import ops
    q, g, mask, words, items, g_group, q_group, skip = real_case("fp32", 68)
    qd, gd = dev(q, "fp32"), dev(g, "fp32")
    for distinct in (False, True):
        for K in (17, 128):
            want = []
            for i in range(len(q)):                                           # the comparator a user has today: gather the rows, search them, map positions back
                rows = np.flatnonzero(RS.eligible_rows(len(g), words, g_group, int(q_group[i])))
                v, p, c = np.full(K, -np.inf, np.float32), np.full(K, -1, np.int64), np.full(K, -1, np.int32)
                if len(rows):
                    kk = min(K, len(rows))
                    gv, gp, gc = host(ops.search_items(qd[i:i + 1], gd[torch.from_numpy(rows).cuda()].contiguous(), kk, i32(items[rows]), i32(skip[i:i + 1]), distinct))
                    v[:kk], c[:kk] = gv[0], gc[0]
                    p[:kk] = np.where(gp[0] >= 0, rows[np.clip(gp[0], 0, None)] + 3, -1)
                want.append((v, p, c))
            want = tuple(np.stack(x) for x in zip(*want))
            assert (want[1][3] == -1).all() and (want[1][[0, 1, 2, 4]][:, :17] >= 0).all()
            for S in RS.SPLITS + (0,):
                assert same(call("fp32", qd, gd, K, items, words, g_group, q_group, skip, distinct, S, 3), want), (distinct, K, S)


def test_bf16_real_operands_are_judged_on_the_eligible_rows():
    q, g, mask, words, items, g_group, q_group, skip = real_case("bf16", 80)
    qd, gd = dev(q, "bf16"), dev(g, "bf16")
    K = 17
    for S in RS.SPLITS + (0,):
        v, p, c = host(call("bf16", qd, gd, K, items, words, g_group, q_group, None, False, S, 3))
        for i in range(len(q)):
            rows = np.flatnonzero(RS.eligible_rows(len(g), words, g_group, int(q_group[i])))
            if not len(rows):
                assert (p[i] == -1).all() and (c[i] == -1).all() and np.isneginf(v[i]).all()
                continue
            at = np.searchsorted(rows, p[i] - 3)
            assert (at < len(rows)).all() and np.array_equal(rows[at], p[i] - 3), (S, i)      # only eligible rows come back
            assert np.array_equal(c[i], items[p[i] - 3])
            ok, worst = R16.judge_real(v[i:i + 1], at[None, :], q[i:i + 1], g[rows], K)
            assert ok, (S, i, worst)


# ---------------------------------------------------------------------------------------- (c) the identity
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_null_selectors_equal_search_items_bit_for_bit(fmt):
    from speechclip_amd import ops
    plain = ops.search_items_bf16 if fmt == "bf16" else ops.search_items
    rng = np.random.default_rng(11)
    for Q, N, E, K in ((1, 33, 16, 17), (65, 257, 80, 16), (130, 4133, 48, 64), (5, 4133, 112, 128), (64, 129, 16, 1)):
        q, g = unit_rows(rng, Q, E, fmt), unit_rows(rng, N, E, fmt)
        g[N // 2] = g[0]
        items = i32(RI.grouped_items(rng, N, big=N // 4))
        skip = i32(rng.integers(-1, 5, Q))
        qd, gd = dev(q, fmt), dev(g, fmt)
        for distinct in (False, True):
            for S in (1, 3, 7, 0):
                want = plain(qd, gd, K, items, q_skip=skip, distinct=distinct, n_split=S, idx_base=9)
                assert same(call(fmt, qd, gd, K, items, None, None, None, skip, distinct, S, 9), want), (Q, N, E, K, distinct, S)


# ---------------------------------------------------------------------------------------- (d) rows nobody selected may hold anything
@pytest.mark.parametrize("fmt", FORMATS)
def test_nan_and_inf_in_dead_tiles_and_deselected_rows_change_nothing(fmt):
    for case in (c for c in RS.CASES if c.N in (257, 4133) and c.mask not in ("ones",)):
        o = RS.operands(case, fmt)
        N = case.N
        nobody = np.ones(N, bool)
        for i in range(case.Q):
            nobody &= ~RS.eligible_rows(N, o["words"], o["g_group"], None if o["q_group"] is None else int(o["q_group"][i]))
        assert nobody.any()
        g = o["g"].copy()
        g[nobody] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), int(nobody.sum()))[:, None]
        for S in (1, 7):
            clean = call(fmt, o["q"], o["g"], case.K, o["items"], o["words"], o["g_group"], o["q_group"], o["skip"], o["distinct"], S)
            dirty = call(fmt, o["q"], g, case.K, o["items"], o["words"], o["g_group"], o["q_group"], o["skip"], o["distinct"], S)
            assert same(dirty, clean), (case, S)


# ---------------------------------------------------------------------------------------- sc_pack_row_mask
def test_pack_row_mask_equals_its_restatement_and_writes_nothing_else():
    from speechclip_amd._lib import lib, stream
    from speechclip_amd import ops
    rng = np.random.default_rng(5)
    for N in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4133, 100003):
        mask = (rng.random(N) < 0.4).astype(np.uint8) * rng.integers(1, 256, N).astype(np.uint8)      # any non-zero byte counts
        md = torch.from_numpy(mask).cuda()
        W = (N + 31) // 32
        buf = torch.full((W + 32,), -777, device="cuda", dtype=torch.int32)
        assert lib().sc_pack_row_mask(md.data_ptr(), N, buf[16:].data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        assert (buf[:16] == -777).all() and (buf[-16:] == -777).all()
        assert np.array_equal(buf[16:-16].cpu().numpy().view(np.uint32), RS.pack_row_mask(mask)), N
        for m in (md, md != 0):
            words = ops.pack_row_mask(m)
            assert words.dtype == torch.uint32 and words.shape == (W,) and np.array_equal(words.cpu().numpy(), RS.pack_row_mask(mask))
    assert ops.pack_row_mask(torch.zeros(0, dtype=torch.bool, device="cuda")).shape == (0,)


# ---------------------------------------------------------------------------------------- (g) EmbeddingIndex
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_index_of_three_adds_equals_one_add_under_every_subset_argument(storage):
    from speechclip_amd.module import EmbeddingIndex
    gen = torch.Generator().manual_seed(80)
    feats, queries = torch.randn(178, 64, generator=gen), torch.randn(7, 64, generator=gen)
    feats[50], feats[177] = feats[0], feats[1]                                # exact ties across segments
    paths = [f"images/{(n * 7) % 46:04d}.jpg" for n in range(178)]            # 46 images, about four rows each, interleaved
    one = EmbeddingIndex(64, storage=storage).add(feats, paths)
    three = EmbeddingIndex(64, storage=storage)
    for a, b in ((0, 45), (45, 145), (145, 178)):                             # segment edges inside mask words
        three.add(feats[a:b], paths[a:b])
    rng = np.random.default_rng(81)
    allow = torch.from_numpy(rng.random(178) < 0.3)
    allow[100:145] = False                                                    # the tail of the second segment and ...
    allow_ids = [paths[3], paths[4], "images/none.jpg", paths[150]]
    within = [paths[0], None, "images/none.jpg", paths[5], paths[1], paths[177], paths[77]]
    row_groups = torch.from_numpy(rng.integers(0, 3, 178))
    query_groups = [0, 1, 2, -1, 5, 0, 1]
    variants = (dict(allow=allow), dict(allow=allow.numpy()), dict(allow_ids=allow_ids), dict(within=within), dict(row_groups=row_groups, query_groups=query_groups),
                dict(allow=allow, row_groups=row_groups.cuda(), query_groups=torch.tensor(query_groups)), dict(allow_ids=set(allow_ids), within=within, distinct=True),
                dict(allow=allow, within=within, exclude=[paths[9]] * 7))
    for kw in variants:
        for k in (1, 10, 45):
            s1, p1, i1 = one.search(queries, k, **kw)
            s3, p3, i3 = three.search(queries.cuda(), k, **kw)
            assert same((s1, p1), (s3, p3)) and i1 == i3, (sorted(kw), k)
            assert s1.shape == p1.shape == (7, k) and i1 == [[paths[p] if p >= 0 else None for p in row] for row in p1.cpu().tolist()]
            pos = p1.cpu().numpy()
            if "allow" in kw:
                assert allow.numpy()[pos[pos >= 0]].all()
            if "allow_ids" in kw:
                assert all(x is None or x in allow_ids for row in i1 for x in row)
            if "within" in kw:
                assert all(x is None or x == w for row, w in zip(i1, within) for x in row) and all(x is None for r in (1, 2) for x in i1[r])
            if "row_groups" in kw:
                assert all(g < 0 or (row_groups.numpy()[r[r >= 0]] == g).all() for r, g in zip(pos, query_groups)) and (pos[4] == -1).all()
    # the subset is exact, not an over-fetch: against the plain ranking of all 178 rows (k = 128 reaches every allowed row here)
    sp, pp, _ = one.search(queries, 128)
    sa, pa, _ = one.search(queries, 10, allow=allow)
    for r in range(7):
        keep = allow[pp[r].cpu()].nonzero().flatten()[:10]
        assert len(keep) == 10 and torch.equal(pa[r].cpu(), pp[r].cpu()[keep]) and torch.equal(sa[r].cpu(), sp[r].cpu()[keep])
    assert same(one.search(queries, 10, within=within, exclude=within)[:1], (np.full((7, 10), -np.inf, np.float32),))      # an id and its converse: nothing
    assert same(three.search(queries, 10)[:2], one.search(queries, 10)[:2])   # none of the arguments: the plain entry, as before
    # a selector: reused, equal to the argument it was made from, refused after a later add and by another index
    for index in (one, three):
        sel, sel_ids = index.selector(allow=allow), index.selector(allow_ids=allow_ids)
        assert len(sel.words) == len(index.segments) and all(w.dtype == torch.uint32 and w.is_cuda for w in sel.words)
        for _ in range(2):
            assert same(index.search(queries, 10, allow=sel)[:2], one.search(queries, 10, allow=allow)[:2])
            assert same(index.search(queries, 10, allow=sel_ids, within=within)[:2], one.search(queries, 10, allow_ids=allow_ids, within=within)[:2])
    with pytest.raises(ValueError, match="another index"):
        one.search(queries, 10, allow=three.selector(allow=allow))
    sel = three.selector(allow=allow)
    three.add(feats[:2], ["images/new.jpg", paths[0]])
    with pytest.raises(ValueError, match="held 178 rows; it holds 180 now"):
        three.search(queries, 10, allow=sel)
    grown = three.search(queries, 3, within=["images/new.jpg"] * 7)            # the item codes follow the add
    assert grown[1][:, 0].tolist() == [178] * 7 and (grown[1][:, 1:] == -1).all()
    bare = EmbeddingIndex(64, storage=storage).add(feats)                     # without ids the id of a row is its position
    assert bare.search(queries, 2, within=[5, 6, 7, 8, 9, 10, 999])[1].tolist() == [[5, -1], [6, -1], [7, -1], [8, -1], [9, -1], [10, -1], [-1, -1]]
    assert set(bare.search(queries, 3, allow_ids=[5, 6, 999])[1].flatten().tolist()) == {5, 6, -1}
    shadow = EmbeddingIndex(64, shadow=True).add(feats, paths) if storage == "fp32" else None
    if shadow is not None:
        with pytest.raises(ValueError, match="certificate speaks about the whole gallery"):
            shadow.search(queries, 5, rerank=16, allow=allow)


# ---------------------------------------------------------------------------------------- (h) the model surface
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


def test_model_search_within_returns_every_querys_own_rows(model):
    gen = torch.Generator().manual_seed(72)
    names = [f"img{n}.jpg" for n in range(5)]
    wavs = [0.3 * torch.randn(3000 + 500 * (n % 4), generator=gen).cuda() for n in range(15)]
    ids = [names[n % 5] for n in range(15)]                                   # three utterances per image, interleaved
    images = torch.randn(4, 3, 64, 64, generator=gen).cuda()
    index = model.build_index(wav=wavs, ids=ids, batch_size=7)
    assert len(index) == 15 and [s.shape[0] for s in index.segments] == [7, 7, 1]
    sv, sp, _ = model.search(index, len(index), images=images)                # every score of every query, from the plain path
    s = np.empty((4, 15), np.float32)
    s[np.arange(4)[:, None], sp.cpu().numpy()] = sv.cpu().numpy()
    codes = np.array([names.index(x) for x in ids], np.int32)
    within = [names[2], None, "elsewhere.jpg", names[0]]
    q_group = np.array([2, 5, 5, 0], np.int32)                                # None and an id the index lacks: a code no row carries
    for k in (1, 3, 4):
        want = RS.search(s, codes, k, None, codes, q_group)
        scores, pos, got_ids = model.search(index, k, images=images, within=within)
        assert same((scores, pos), want[:2])
        assert got_ids == [[ids[p] if p >= 0 else None for p in row] for row in want[1].tolist()]
    assert sorted(pos[0].tolist()) == [-1, 2, 7, 12] and (pos[1:3] == -1).all()
    allow = torch.tensor([n % 2 == 0 for n in range(15)])
    want = RS.search(s, codes, 5, RS.pack_row_mask(allow.numpy()), None, None, np.array([2, -1, -1, 0], np.int32), True)
    got = model.search(index, 5, images=images, allow=allow, distinct=True, exclude=within)
    assert same(got[:2], want[:2])

"""Gallery search by item on the MI355X (sc_search_items / sc_search_items_bf16 / sc_topk_merge_items, EmbeddingIndex.search(distinct=, exclude=),
KWClipBase.search) against the host statement of tests/search_items_ref.py.  Everything here is equality of bits: the scores are the plain entries' (the
identities), exact integers, the restated fp32 chain, or the device's own plain scores; what is judged is the selection.

Measured on the MI355X: all 32 cases hold, 6 s for the file ("Search by item"; timings in profiles/search_items_bench.txt).

Every call of the entries goes through `call`: outputs between sentinel guards, the workspace of exactly the stated size between guards and pre-filled."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import search_bf16_ref as R16
import search_items_ref as RI
import search_ref as R

pytestmark = pytest.mark.gpu

FORMATS = ("fp32", "bf16")
SPLITS = (1, 2, 7, 0)


def dev(a, fmt):
    """Host fp32 array (bf16 numbers for fmt == "bf16") or a device tensor -> device rows of the format."""
    if torch.is_tensor(a):
        return a
    if fmt == "bf16":
        return torch.from_numpy(np.ascontiguousarray(R16.bf16_bits(a))).view(torch.bfloat16).cuda()
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def i32(a):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda())


def call(fmt, q, g, k, items, skip=None, distinct=False, n_split=0, idx_base=0, fill=0xFF):
    """-> device (vals [Q, k], idx [Q, k], items [Q, k]).  fill: what the workspace holds before the call (0xFF bytes are NaN values and -1 indices)."""
    from speechclip_amd._lib import lib, stream
    L = lib()
    q, g, items, skip = dev(q, fmt), dev(g, fmt), i32(items), i32(skip)
    (Q, E), N = q.shape, g.shape[0]
    nbytes = L.sc_search_items_workspace_bytes(Q, N, k, n_split)
    assert nbytes == RI.workspace_bytes(Q, N, k, n_split)
    ws = torch.full((nbytes + 128,), 0xA5, device="cuda", dtype=torch.uint8)
    ws[64:64 + nbytes] = fill
    vals = torch.full((Q * k + 32,), 12345.0, device="cuda")
    idx = torch.full((Q * k + 32,), -777, device="cuda", dtype=torch.int64)
    its = torch.full((Q * k + 32,), -555, device="cuda", dtype=torch.int32)
    entry = L.sc_search_items_bf16 if fmt == "bf16" else L.sc_search_items
    rc = entry(q.data_ptr(), q.stride(0), g.data_ptr(), g.stride(0), Q, N, E, k, n_split, idx_base, items.data_ptr(), None if skip is None else skip.data_ptr(),
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


# ---------------------------------------------------------------------------------------- 1. identities
@pytest.mark.parametrize("Q", [1, 65, 129])
@pytest.mark.parametrize("fmt", FORMATS)
def test_identities_with_the_plain_entries_bit_for_bit(fmt, Q):
    """distinct == 0 without a skip, and distinct != 0 with all codes different (a permutation, so that code order is not row order), return the plain
    entry's vals and idx -- over every list capacity, both tile widths, one / several / auto splits, whole and ragged stages of E."""
    from speechclip_amd import ops
    plain = ops.search_topk_bf16 if fmt == "bf16" else ops.search_topk
    rng = np.random.default_rng(100 + Q)
    for N in (1, 127, 129, 1000):
        codes = i32(rng.permutation(N))
        for E in ((16, 64, 112) if fmt == "bf16" else (4, 64, 100)):
            q, g = unit_rows(rng, Q, E, fmt), unit_rows(rng, N, E, fmt)
            for p in (1, 63, 64, 65, 127, 128, 333, 334, 500, 999):            # exact ties across tile and split edges
                if p < N:
                    g[p] = g[0]
            qd, gd = dev(q, fmt), dev(g, fmt)
            for K in (1, 10, 16, 17, 64, 65, 128):
                if K > N:
                    continue
                for n_split in (1, 3, 0):
                    want = plain(qd, gd, K, n_split=n_split, idx_base=11)
                    for distinct in (False, True):
                        got = call(fmt, qd, gd, K, codes, None, distinct, n_split, idx_base=11)
                        assert same(got[:2], want), (N, E, K, n_split, distinct)
                        assert torch.equal(got[2], codes[(got[1] - 11).clamp(min=0)].where(got[1] >= 0, torch.tensor(-1, device="cuda", dtype=torch.int32)))


# ---------------------------------------------------------------------------------------- 2. integer operands with heavy ties
N_INT, E_INT, Q_INT = 1000, 16, 67
EDGES = (128, 256, 384, 143, 286, 429, 572, 715, 858, 334, 668, 500)          # tile edges; split edges of 7, 3 (the auto rule here) and 2 splits


@functools.lru_cache(maxsize=None)
def int_case():
    """Operands in [-2, 2] (bf16 numbers; scores are integers of at most 64: exact in both formats, some seventy rows per value), item groups of 1..7 rows
    shuffled over the gallery plus one item of 300 rows, the same item and the same row contents on both sides of every tile and split edge, NaN gallery
    rows, one NaN query, and per-query skips: none, the big item, a code the gallery does not hold, a small item."""
    rng = np.random.default_rng(2)
    q = rng.integers(-2, 3, (Q_INT, E_INT)).astype(np.float32)
    g = rng.integers(-2, 3, (N_INT, E_INT)).astype(np.float32)
    items = RI.grouped_items(rng, N_INT, big=300)
    big = int(np.bincount(items).argmax())
    for e in EDGES:
        g[e - 1:e + 2] = g[0]
        items[e - 1:e + 2] = items[e - 1]
    items[[127, 128, 499, 500]] = big                                         # the big item on both sides of a tile edge and of a split edge
    g[[5, 130, 999]] = np.nan
    q[3] = np.nan
    skip = np.array([(-1, big, 10 ** 6, int(items[7]))[i % 4] for i in range(Q_INT)], np.int32)
    assert R.search_splits(Q_INT, N_INT, 10) == 3 and np.bincount(items).max() >= 300 and set(np.bincount(items).tolist()) >= set(range(1, 8))
    return q, g, items, skip, R.scores64(q, g)


@functools.lru_cache(maxsize=None)
def int_want(variant, K, distinct):
    q, g, items, skip, s = int_case()
    if variant == "few":                                                      # 40 items: K above the number of items, padding slots
        items = items % 40
    if variant == "one":                                                      # a single item, excluded for every other query: all-empty rows
        items, skip = np.zeros(N_INT, np.int32), np.array([0, -1] * Q_INT, np.int32)[:Q_INT]
    return items, skip, RI.search(s, items, K, skip, distinct, idx_base=5)


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("fmt", FORMATS)
def test_integer_operands_with_item_groups_skips_and_nan_match_the_host_rule(fmt, distinct):
    q, g, _, _, _ = int_case()
    qd, gd = dev(q, fmt), dev(g, fmt)
    for variant, Ks in (("groups", (10, 64, 128)), ("few", (10, 64, 128)), ("one", (10, 17))):
        for K in Ks:
            items, skip, want = int_want(variant, K, distinct)
            for n_split in SPLITS:
                got = call(fmt, qd, gd, K, items, skip, distinct, n_split, idx_base=5)
                assert same(got, want), (variant, K, n_split)
            narrow = call(fmt, qd[:5], gd, K, items, skip[:5], distinct, 0, idx_base=5)      # at most 64 queries: the narrow tile's instantiations
            assert same(narrow, tuple(w[:5] for w in want)), (variant, K)
    if distinct:
        _, _, want = int_want("few", 64, True)
        assert ((want[1] >= 0).sum(1).max() == 40) and (want[1][:, 40:] == -1).all() and np.isneginf(want[0][3]).all()
        _, _, want = int_want("one", 10, True)
        assert (want[1][0::2] == -1).all() and ((want[1][1::2] >= 0).sum(1)[[0, 2]] == 1).all()


# ---------------------------------------------------------------------------------------- 3. real-valued operands
def test_fp32_unit_norm_rows_match_the_host_chain_bit_for_bit():
    rng = np.random.default_rng(30)
    Q, N, E = 2, 1000, 8
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    g[[400, 700]] = g[100]
    items = RI.grouped_items(rng, N, big=300)
    skip = np.array([int(items[100]), -1], np.int32)
    s = R.chain_scores(q, g)
    for distinct in (False, True):
        for K in (10, 128):
            want = RI.search(s, items, K, skip, distinct)
            for n_split in (0, 2):
                assert same(call("fp32", q, g, K, items, skip, distinct, n_split), want), (distinct, K, n_split)


@pytest.mark.parametrize("N,E", [(128, 64), (77, 16)])
def test_bf16_real_rows_match_the_host_rule_on_the_devices_own_scores(N, E):
    """ops.search_topk_bf16(q, g, N) returns ALL of the device's scores; purity makes them the bits the items entry selects from."""
    from speechclip_amd import ops
    rng = np.random.default_rng(31 + N)
    Q = 5
    q, g = unit_rows(rng, Q, E, "bf16"), unit_rows(rng, N, E, "bf16")
    g[[40, 70]] = g[10]
    qd, gd = dev(q, "bf16"), dev(g, "bf16")
    v, i = host(ops.search_topk_bf16(qd, gd, N))
    assert np.array_equal(np.sort(i, 1), np.tile(np.arange(N), (Q, 1)))
    s = np.empty((Q, N), np.float32)
    s[np.arange(Q)[:, None], i] = v
    items = RI.grouped_items(rng, N, big=30)
    skip = np.array([int(items[10]), -1, 10 ** 6, int(items[0]), int(items[40])], np.int32)
    for distinct in (False, True):
        for K in (1, 10, 17, N):
            want = RI.search(s, items, K, skip, distinct)
            for n_split in SPLITS:
                assert same(call("bf16", qd, gd, K, items, skip, distinct, n_split), want), (distinct, K, n_split)


# ---------------------------------------------------------------------------------------- 4. purity
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_rows_result_does_not_depend_on_the_call_around_it(fmt):
    rng = np.random.default_rng(40)
    E, N, K = 32, 300, 33
    q, g = unit_rows(rng, 5, E, fmt), unit_rows(rng, N, E, fmt)
    g[[77, 200]] = g[3]
    g[[9, 128]] = np.nan                                                      # NaN gallery rows take no part
    items = RI.grouped_items(rng, N, big=100)
    skip = np.array([-1, int(items[3]), 10 ** 6, int(items[0]), int(items[150])], np.int32)
    gd = dev(g, fmt)
    for distinct in (False, True):
        alone = tuple(np.concatenate(c) for c in zip(*[host(call(fmt, q[i:i + 1], gd, K, items, skip[i:i + 1], distinct, 1)) for i in range(5)]))
        assert not np.isin(alone[1], [9, 128]).any() and (alone[1] >= 0).all()
        if distinct:
            assert all(len(set(row.tolist())) == K for row in alone[2])
        assert not (alone[2] == skip[:, None]).any()
        # inside a batch, at other positions of other query tiles, next to a NaN query (an all-empty row)
        batch = unit_rows(rng, 131, E, fmt)
        bskip = rng.integers(-1, 50, 131).astype(np.int32)
        at = [0, 31, 64, 129, 130]
        batch[at], bskip[at] = q, skip
        batch[65] = np.nan
        for n_split in SPLITS:
            for fill in (0xFF, 0x00):
                bv, bi, bc = host(call(fmt, batch, gd, K, items, bskip, distinct, n_split, fill=fill))
                assert same((bv[at], bi[at], bc[at]), alone), (distinct, n_split, fill)
                assert (bi[65] == -1).all() and (bc[65] == -1).all() and np.isneginf(bv[65]).all()
        for k in (1, 10, 17):
            for n_split in (0, 3):
                assert same(call(fmt, q, gd, k, items, skip, distinct, n_split), tuple(a[:, :k] for a in alone)), (distinct, k, n_split)


# ---------------------------------------------------------------------------------------- 5. sc_topk_merge_items
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("K,L", [(1, 1), (1, 7), (10, 10), (10, 70), (128, 128), (128, 896), (10, 20000)])
def test_merge_against_the_host_rule(K, L, distinct):
    """Heavy ties, duplicate items, idx < 0, NaN values, a row with no candidate, a row of one item; L = 20 000 reaches the second word of a thread's share
    of the dead bitmap."""
    from speechclip_amd import ops
    rng = np.random.default_rng(60 + K + L)
    Q = 5
    vals = rng.integers(-3, 4, (Q, L)).astype(np.float32)
    idx = np.stack([rng.permutation(10 * L)[:L] for _ in range(Q)]).astype(np.int64)
    items = rng.integers(0, max(2, L // 3), (Q, L)).astype(np.int32)
    idx[rng.random((Q, L)) < 0.2] = -1
    vals[rng.random((Q, L)) < 0.1] = np.nan
    vals[0, 0] = -np.inf
    idx[1] = -1
    items[2] = 4
    want = RI.merge(vals, idx, items, K, distinct)
    t = lambda a: torch.from_numpy(a).cuda()
    got = ops.topk_merge_items(t(vals), t(idx), t(items), K, distinct)
    assert same(got, want)
    if not distinct:
        assert same(ops.topk_merge(t(vals), t(idx), K), want[:2])


# ---------------------------------------------------------------------------------------- 6. EmbeddingIndex
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_index_of_three_adds_equals_one_add_under_distinct_and_exclude(storage):
    from speechclip_amd.module import EmbeddingIndex
    gen = torch.Generator().manual_seed(70)
    feats, queries = torch.randn(136, 64, generator=gen), torch.randn(7, 64, generator=gen)
    feats[50], feats[135] = feats[0], feats[1]                                # exact ties across segments
    paths = [f"images/{(n * 7) % 46:04d}.jpg" for n in range(136)]            # 46 images, about three rows each, interleaved
    one = EmbeddingIndex(64, storage=storage).add(feats, paths)
    three = EmbeddingIndex(64, storage=storage)
    for a, b in ((0, 1), (1, 131), (131, 136)):
        three.add(feats[a:b], paths[a:b])
    exclude = [paths[0], None, "images/none.jpg", paths[5], paths[1], paths[135], paths[77]]
    plain = one.search(queries, 10)
    assert same(three.search(queries, 10, distinct=False, exclude=None)[:2], plain[:2])
    back = EmbeddingIndex.from_state_dict(three.state_dict(), "cuda")
    assert [s.shape[0] for s in back.segments] == [1, 130, 5]
    for distinct, excl in ((True, None), (False, exclude), (True, exclude)):
        for k in (1, 10, 46 if distinct else 128):
            s1, p1, i1 = one.search(queries, k, distinct=distinct, exclude=excl)
            for other in (three, back):
                s3, p3, i3 = other.search(queries.cuda(), k, distinct=distinct, exclude=excl)
                assert same((s1, p1), (s3, p3)) and i1 == i3, (distinct, k)
            assert s1.shape == p1.shape == (7, k) and s1.dtype == torch.float32 and p1.dtype == torch.int64
            assert i1 == [[paths[p] if p >= 0 else None for p in row] for row in p1.cpu().tolist()]
            for row, ex in zip(i1, excl or [None] * 7):
                found = [x for x in row if x is not None]
                assert ex not in found
                if distinct:
                    assert len(set(found)) == len(found) == (k if k < 46 or ex not in paths else 45)
    # neither argument changes what a row scores: the distinct list is the plain list with the later rows of an id left out
    s1, p1, i1 = one.search(queries, 46, distinct=True)
    sp, pp, ip = one.search(queries, 128)
    for r in range(7):
        first = [n for n, x in enumerate(ip[r]) if x not in ip[r][:n]]
        assert i1[r][:len(first)] == [ip[r][n] for n in first] and torch.equal(s1[r, :len(first)], sp[r, first])
    ints = EmbeddingIndex(64, storage=storage).add(feats, torch.arange(136) // 3)
    assert all(len(set(row)) == 10 for row in ints.search(queries, 10, distinct=True)[2])
    assert not any(4 in row for row in ints.search(queries, 10, exclude=torch.full((7,), 4))[2])
    bare = EmbeddingIndex(64, storage=storage).add(feats)
    assert same(bare.search(queries, 10, distinct=True)[:2], plain[:2])       # without ids every row is its own item
    top = plain[1][:, 0].cpu().tolist()
    assert [row[0] for row in bare.search(queries, 10, exclude=top)[2]] == plain[1][:, 1].cpu().tolist()
    with pytest.raises(ValueError, match="47 .*46 different ids"):
        one.search(queries, 47, distinct=True)
    with pytest.raises(ValueError, match="6 exclude ids for 7 queries"):
        one.search(queries, 3, exclude=exclude[:6])
    n_before = len(three._item_codes()[0])
    three.add(feats[:2], ["images/new.jpg", paths[0]])
    assert n_before == 3 and len(three._item_codes()[0]) == 4 and three._item_codes()[2] == 47


# ---------------------------------------------------------------------------------------- 7. the model surface
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


def test_model_search_by_image_over_spoken_captions_returns_distinct_images(model):
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
    exclude = [names[2], None, "elsewhere.jpg", names[0]]
    skip = np.array([2, -1, -1, 0], np.int32)
    for distinct, k in ((True, 4), (True, 5), (False, 10)):
        if distinct and k == 5:                                               # five images, one excluded for two of the queries: their last slot is empty
            want = RI.search(s, codes, k, skip, True)
            assert (want[1][[0, 3], 4] == -1).all() and (want[1][[1, 2]] >= 0).all()
        want = RI.search(s, codes, k, skip, distinct)
        scores, pos, got_ids = model.search(index, k, images=images, distinct=distinct, exclude=exclude)
        assert same((scores, pos), want[:2])
        assert got_ids == [[ids[p] if p >= 0 else None for p in row] for row in want[1].tolist()]
    assert same(model.search(index, 3, images=images)[:2], (sv[:, :3], sp[:, :3]))

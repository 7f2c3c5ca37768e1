"""Gallery search on the MI355X (sc_search_topk / sc_topk_merge, EmbeddingIndex, KWClipBase.build_index / search) against the host statements of
tests/search_ref.py: exact bits where the arithmetic is exact or restated exactly, the derived bound gamma_E * sum |q g| elsewhere.

Measured on the MI355X (see profiles/search_parity.txt): every bitwise test below holds; in the real arm the largest |vals - s64| / b is recorded there."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import search_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(q, g, k, n_split=0, idx_base=0):
    from speechclip_amd import ops
    v, i = ops.search_topk(dev(q), dev(g), k, n_split=n_split, idx_base=idx_base)
    return v.cpu().numpy(), i.cpu().numpy()


def int_rows(rng, n, E):
    return rng.integers(-8, 9, size=(n, E)).astype(np.float32)


# ---------------------------------------------------------------------------------------- 1. exact-integer arm
# (Q, N, E, K, n_split): every value of every parameter of the issue's table at least once, the edge values together; the last two rows add a K in
# (16, 64] on both query-tile widths, which take other kernel instantiations, an E with a whole 64-element stage plus a tail that ends in half a group
# (100 = 64 + 32 + 4), and the largest E (entries in [-8, 8]: sums up to 1024 * 64, still exact).
INT_CASES = [
    (1, 10, 4, 10, 0), (2, 63, 8, 1, 1), (31, 64, 64, 10, 2), (32, 65, 512, 10, 3), (33, 127, 4, 1, 7), (127, 128, 8, 128, 7), (128, 129, 64, 128, 2),
    (129, 255, 512, 10, 3), (257, 256, 8, 10, 0), (129, 257, 64, 128, 7), (257, 4097, 512, 10, 0), (33, 4097, 512, 128, 7), (1, 4097, 64, 1, 3),
    (129, 257, 64, 33, 2), (3, 300, 8, 40, 0), (65, 300, 100, 10, 2), (2, 300, 1024, 10, 0),
]


@pytest.mark.parametrize("Q,N,E,K,n_split", INT_CASES)
def test_integer_operands_give_the_host_order_bit_for_bit(Q, N, E, K, n_split):
    """Entries in [-8, 8]: every partial sum is an integer of at most 512 * 64, exact in fp32, so the chain equals the fp64 score and the whole result is
    decided by the order alone.  Small E gives heavy ties; on top, one row is repeated at both sides of every tile (128) and split edge."""
    rng = np.random.default_rng(1000 * Q + N + E + K)
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    S = n_split or R.search_splits(Q, N, K)
    per = -(-N // S)
    for edge in {64, 128, 256, 4096} | {s * per for s in range(1, S)}:
        for p in (edge - 1, edge, edge + 1):
            if 0 < p < N:
                g[p] = g[0]
    want_v, want_i = R.topk(R.scores64(q, g), K, idx_base=7)
    got_v, got_i = run(q, g, K, n_split, idx_base=7)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))


# ---------------------------------------------------------------------------------------- 2. real arm
def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_unit_norm_rows_within_the_derived_bound_and_the_right_members():
    Q, N, E, K = 129, 4097, 512, 10
    rng = np.random.default_rng(22)      # chosen on the host: seeds 20 .. 31 give 1 .. 12 ambiguous entries over the 129 rows (b ~ 2e-5), this one gives 1
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    s64, b = R.scores64(q, g), R.bound(q, g)
    kth = -np.sort(-s64, axis=1)[:, K - 1:K]
    # not vacuous: an "ambiguous" entry lies within 2b of the K-th fp64 score (the K-th itself apart); at most one per row, none on >= 90 % of the rows
    ambiguous = (np.abs(s64 - kth) <= 2 * b).sum(1) - 1
    print(f"ambiguous entries: {int(ambiguous.sum())} over {Q} rows; max b = {b.max():.3e}")
    assert ambiguous.max() <= 1 and (ambiguous == 0).mean() >= 0.9
    vals, idx = run(q, g, K)
    rows = np.arange(Q)[:, None]
    assert ((idx >= 0) & (idx < N)).all()
    err = np.abs(vals.astype(np.float64) - s64[rows, idx])
    print(f"max |vals - s64| / b = {(err / b[rows, idx]).max():.4f}, max |vals - s64| = {err.max():.3e}")
    assert (err <= b[rows, idx]).all()
    member = np.zeros((Q, N), bool)
    member[rows, idx] = True
    assert member.sum(1).tolist() == [K] * Q                                  # K distinct rows
    assert member[s64 > kth + 2 * b].all()                                    # everything clearly above the K-th score is returned
    assert (s64[rows, idx] >= kth - 2 * b[rows, idx]).all()                   # nothing clearly below it is
    dv, di = np.diff(vals.astype(np.float64), axis=1), np.diff(idx, axis=1)
    assert ((dv < 0) | ((dv == 0) & (di > 0))).all()                          # (value descending, idx ascending)


# ---------------------------------------------------------------------------------------- 3. the chain
@pytest.mark.parametrize("E", [4, 8, 64, 100])
def test_scores_equal_the_exact_fmaf_chain_bit_for_bit(E):
    """8 x 16 pairs of mixed magnitude (2^-10 .. 2^10, both signs): N = K returns every pair's score; the host chain is rational arithmetic with one
    correct rounding to fp32 per step."""
    rng = np.random.default_rng(30 + E)
    def mixed(n):
        return (rng.choice([-1.0, 1.0], (n, E)) * np.exp2(rng.integers(-10, 11, (n, E))) * (1 + rng.random((n, E)))).astype(np.float32)
    q, g = mixed(8), mixed(16)
    vals, idx = run(q, g, 16)
    got = np.empty((8, 16), np.float32)
    got[np.arange(8)[:, None], idx] = vals
    want = R.chain_scores(q, g)
    assert np.array_equal(np.sort(idx, 1), np.tile(np.arange(16), (8, 1)))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got.astype(np.float64) - want).max()


# ---------------------------------------------------------------------------------------- 4. independence
def test_a_pairs_score_and_a_rows_result_do_not_depend_on_the_call_around_them():
    rng = np.random.default_rng(40)
    E, N = 512, 128
    q, g = unit_rows(rng, 5, E), unit_rows(rng, N, E)
    g[77] = g[3]                                                              # one exact tie per row
    def table(vals, idx):
        t = np.empty(vals.shape, np.float32)
        t[np.arange(vals.shape[0])[:, None], idx] = vals
        return t.view(np.uint32)
    alone_v, alone_i = map(np.concatenate, zip(*[run(q[i:i + 1], g, N) for i in range(5)]))
    want = table(alone_v, alone_i)
    # inside a batch, at other positions of other query tiles
    batch = unit_rows(rng, 131, E)
    at = [0, 31, 64, 129, 130]
    batch[at] = q
    bv, bi = run(batch, g, N)
    assert np.array_equal(bv[at].view(np.uint32), alone_v.view(np.uint32)) and np.array_equal(bi[at], alone_i)
    # gallery permuted: the same bits per pair, and the same order up to the tie rule
    perm = rng.permutation(N)
    pv, pi = run(q, g[perm], N)
    assert np.array_equal(table(pv, perm[pi]), want)
    # other splits, a wider gallery around the same rows, smaller K: prefixes
    for n_split in (1, 2, 3, 7):
        sv, si = run(q, g, N, n_split)
        assert np.array_equal(sv.view(np.uint32), alone_v.view(np.uint32)) and np.array_equal(si, alone_i), n_split
    for k in (1, 10, 33):
        for n_split in (0, 3):
            kv, ki = run(q, g, k, n_split)
            assert np.array_equal(kv.view(np.uint32), alone_v[:, :k].view(np.uint32)) and np.array_equal(ki, alone_i[:, :k]), (k, n_split)


# ---------------------------------------------------------------------------------------- 5. hygiene
def test_guards_gaps_workspace_contents_nan_rows_short_lists_and_the_empty_call():
    from speechclip_amd._lib import lib, stream
    L = lib()
    rng = np.random.default_rng(50)
    Q, N, E, K, S, ld = 33, 300, 8, 10, 3, 12
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    g[[5, 128, 299]] = np.nan                                                 # NaN gallery rows: never returned
    want_v, want_i = R.topk(R.scores64(q, g), K)
    assert not np.isin(want_i, [5, 128, 299]).any()
    def guarded(a):                                                           # rows between NaN guard rows, NaN in the gap behind column E
        buf = torch.full((a.shape[0] + 2, ld), float("nan"), device="cuda")
        buf[1:-1, :E] = dev(a)
        return buf
    qb, gb = guarded(q), guarded(g)
    nbytes = L.sc_search_workspace_bytes(Q, N, K, S)
    assert nbytes == R.workspace_bytes(Q, N, K, S) == Q * S * K * 12
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes + 128,), 0xFF, device="cuda", dtype=torch.uint8)
        ws[64:-64] = fill
        vals = torch.full((Q * K + 32,), 12345.0, device="cuda")
        idx = torch.full((Q * K + 32,), -777, device="cuda", dtype=torch.int64)
        rc = L.sc_search_topk(qb[1:].data_ptr(), ld, gb[1:].data_ptr(), ld, Q, N, E, K, S, 0, vals[16:].data_ptr(), idx[16:].data_ptr(), ws[64:].data_ptr(), stream())
        assert rc == 0, L.sc_last_error()
        torch.cuda.synchronize()
        assert (ws[:64] == 0xFF).all() and (ws[-64:] == 0xFF).all()
        assert (vals[:16] == 12345.0).all() and (vals[-16:] == 12345.0).all() and (idx[:16] == -777).all() and (idx[-16:] == -777).all()
        outs.append((vals[16:-16].cpu().numpy().reshape(Q, K), idx[16:-16].cpu().numpy().reshape(Q, K)))
    for v, i in outs:
        assert np.array_equal(i, want_i) and np.array_equal(v.view(np.uint32), want_v.view(np.uint32))
    # fewer than K comparable scores: -inf / -1 in the remaining slots, with one split and with several
    g2 = int_rows(rng, 10, E)
    g2[[2, 3, 9]] = np.nan
    for n_split in (1, 3):
        v, i = run(q, g2, 10, n_split)
        w_v, w_i = R.topk(R.scores64(q, g2), 10)
        assert np.array_equal(i, w_i) and np.array_equal(v.view(np.uint32), w_v.view(np.uint32))
        assert (i[:, 7:] == -1).all() and np.isneginf(v[:, 7:]).all() and (i[:, :7] >= 0).all()
    # Q == 0: nothing is launched, nothing is written
    vals = torch.full((16,), 12345.0, device="cuda")
    idx = torch.full((16,), -777, device="cuda", dtype=torch.int64)
    assert L.sc_search_topk(qb.data_ptr(), ld, gb.data_ptr(), ld, 0, N, E, K, S, 0, vals.data_ptr(), idx.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert (vals == 12345.0).all() and (idx == -777).all()


# ---------------------------------------------------------------------------------------- 6. sc_topk_merge
@pytest.mark.parametrize("K,mult", [(1, 1), (10, 1), (10, 7), (128, 1), (128, 7), (10, 0)])
def test_merge_against_the_host_order(K, mult):
    from speechclip_amd import ops
    rng = np.random.default_rng(60 + K + mult)
    L, Q = (K * mult if mult else K + 1), 5
    vals = rng.integers(-3, 4, (Q, L)).astype(np.float32)                     # heavy ties
    idx = np.stack([rng.permutation(10 * L)[:L] for _ in range(Q)]).astype(np.int64)
    idx[rng.random((Q, L)) < 0.2] = -1
    vals[rng.random((Q, L)) < 0.1] = np.nan
    vals[0, 0] = -np.inf
    idx[1] = -1                                                               # a row with no candidate at all
    want_v, want_i = R.merge(vals, idx, K)
    v, i = ops.topk_merge(dev(vals), dev(idx), K)
    assert np.array_equal(i.cpu().numpy(), want_i) and np.array_equal(v.cpu().numpy().view(np.uint32), want_v.view(np.uint32))


def test_two_segments_merged_equal_one_segment():
    from speechclip_amd import ops
    rng = np.random.default_rng(61)
    q, g = unit_rows(rng, 9, 64), unit_rows(rng, 333, 64)
    g[200] = g[100]
    one_v, one_i = run(q, g, 10)
    a, b = run(q, g[:131], 10, idx_base=0), run(q, g[131:], 10, idx_base=131)
    v, i = ops.topk_merge(dev(np.concatenate([a[0], b[0]], 1)), dev(np.concatenate([a[1], b[1]], 1)), 10)
    assert np.array_equal(i.cpu().numpy(), one_i) and np.array_equal(v.cpu().numpy().view(np.uint32), one_v.view(np.uint32))


# ---------------------------------------------------------------------------------------- 7. EmbeddingIndex and the model surface
def test_index_of_three_adds_equals_index_of_one_add_and_ids_and_state_round_trip():
    from speechclip_amd.module import EmbeddingIndex
    import avssl.module
    assert avssl.module.EmbeddingIndex is EmbeddingIndex
    g = torch.Generator().manual_seed(70)
    feats, queries = torch.randn(136, 64, generator=g), torch.randn(7, 64, generator=g)
    paths = [f"images/{n:04d}.jpg" for n in range(136)]
    one = EmbeddingIndex(64).add(feats, paths)
    three = EmbeddingIndex(64)
    for a, b in ((0, 1), (1, 131), (131, 136)):
        three.add(feats[a:b].double() if a else feats[a:b].cuda(), paths[a:b])    # host or device, any float dtype
    assert len(one) == len(three) == 136 and len(three.segments) == 3 and len(one.segments) == 1
    first = three.segments[0].data_ptr()
    s1, p1, i1 = one.search(queries, 10)
    s3, p3, i3 = three.search(queries.cuda(), 10)
    assert three.segments[0].data_ptr() == first
    assert torch.equal(s1, s3) and torch.equal(p1, p3) and i1 == i3
    assert s1.dtype == torch.float32 and p1.dtype == torch.int64 and s1.shape == p1.shape == (7, 10)
    assert i1 == [[paths[p] for p in row] for row in p1.cpu().tolist()]
    ints = EmbeddingIndex(64).add(feats, torch.arange(136) * 3 + 1)
    assert ints.search(queries, 4)[2] == (p1[:, :4].cpu() * 3 + 1).tolist()
    assert EmbeddingIndex(64).add(feats).search(queries, 4)[2] == p1[:, :4].cpu().tolist()
    sd = three.state_dict()
    assert all(isinstance(v, (int, bool, list, type(None))) or (torch.is_tensor(v) and not v.is_cuda) for v in sd.values())
    back = EmbeddingIndex.from_state_dict(sd, "cuda")
    sb, pb, ib = back.search(queries, 10)
    assert len(back) == 136 and [s.shape[0] for s in back.segments] == [1, 130, 5]
    assert torch.equal(sb, s3) and torch.equal(pb, p3) and ib == i3
    with pytest.raises(ValueError):
        one.search(queries, 137)


def test_membership_in_the_search_result_is_rank_below_k_of_the_dense_path():
    from speechclip_amd import ops
    from speechclip_amd.module import EmbeddingIndex
    rng = np.random.default_rng(71)
    Q, N, E, k = 40, 500, 64, 10
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    index = EmbeddingIndex(E, normalize=False)
    for a, b in ((0, 200), (200, 203), (203, 500)):
        index.add(torch.from_numpy(g[a:b]), torch.arange(a, b))
    _, pos, ids = index.search(torch.from_numpy(q), k)
    own = torch.from_numpy(rng.integers(0, N, Q))
    own[:8] = pos[:8, [0, 0, 4, 4, 9, 9, 9, 0]].diagonal().cpu()              # some certain hits, the k-th place among them
    rank = ops.retrieval_ranks(ops.sgemm(dev(q), dev(g), transb=True), own, torch.arange(N))
    member = (pos.cpu() == own[:, None]).any(1)
    assert torch.equal(rank.cpu() < k, member) and member[:8].all() and not member.all()
    assert ids == pos.cpu().tolist()


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


def test_model_build_index_of_images_and_search_by_speech_agree_with_the_dense_path(model):
    from speechclip_amd import ops
    g = torch.Generator().manual_seed(72)
    images = torch.randn(12, 3, 64, 64, generator=g).cuda()
    wavs = [0.3 * torch.randn(n, generator=g).cuda() for n in (8000, 6000, 3000, 5000)]
    names = [f"img{n}.jpg" for n in range(12)]
    k = 3
    index = model.build_index(images=images, ids=names, batch_size=5)
    assert len(index) == 12 and [s.shape[0] for s in index.segments] == [5, 5, 2] and not model.training
    scores, pos, ids = model.search(index, k, wav=wavs)
    assert scores.shape == pos.shape == (4, k) and ids == [[names[p] for p in row] for row in pos.cpu().tolist()]
    with torch.no_grad():
        feats = model.encode_speech(wavs)
    audio = feats["cascaded_audio_feat"] if model.config.retrieval.audio_feat_src == "cascaded" else feats["parallel_audio_feat"]
    qn, gal = ops.l2norm(audio.float().contiguous()), torch.cat(index.segments, 0)
    dense_v, dense_i = ops.topk_rows(ops.sgemm(qn, gal, transb=True), k)
    qh, gh = qn.cpu().numpy(), gal.cpu().numpy()
    s64, b = R.scores64(qh, gh), R.bound(qh, gh)
    srt = -np.sort(-s64, axis=1)
    clear = (srt[:, :k] - srt[:, 1:k + 1] > 2 * b.max(1, keepdims=True)).all(1)   # the first k + 1 fp64 scores further apart than both paths' error
    assert clear.any()
    want = np.argsort(-s64, axis=1, kind="stable")[:, :k]
    assert np.array_equal(pos.cpu().numpy()[clear], want[clear]) and np.array_equal(dense_i.cpu().numpy()[clear], want[clear])
    assert (np.abs(scores.cpu().numpy() - s64[np.arange(4)[:, None], pos.cpu().numpy()]) <= b[np.arange(4)[:, None], pos.cpu().numpy()]).all()
    with pytest.raises(ValueError):
        model.build_index(images=images, wav=wavs)

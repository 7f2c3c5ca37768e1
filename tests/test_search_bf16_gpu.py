"""bf16 gallery search on the MI355X (sc_search_topk_bf16, EmbeddingIndex(storage="bf16"), KWClipBase.build_index(storage="bf16")) against the host
statements of tests/search_bf16_ref.py: exact bits where the arithmetic is exact (integers, purity, segments), the derived accumulation bound elsewhere.

Measured on the MI355X (profiles/search_bf16_parity.txt): every bitwise test below holds; the real arm's worst |vals - s64| / bound is recorded there."""
import dataclasses

import numpy as np
import pytest
import torch

import search_bf16_ref as R
import search_ref as R32

pytestmark = pytest.mark.gpu

SPLITS = (0, 1, 2, 7)


def dev16(a):
    """fp32 host array of bf16 numbers -> bf16 device tensor with exactly those bits."""
    return torch.from_numpy(np.ascontiguousarray(R.bf16_bits(a))).view(torch.bfloat16).cuda()


def run(q, g, k, n_split=0, idx_base=0, workspace=None):
    from speechclip_amd import ops
    q = q if torch.is_tensor(q) else dev16(q)
    g = g if torch.is_tensor(g) else dev16(g)
    v, i = ops.search_topk_bf16(q, g, k, n_split=n_split, idx_base=idx_base, workspace=workspace)
    return v.cpu().numpy(), i.cpu().numpy()


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def int_rows(rng, n, E):
    return rng.integers(-8, 9, size=(n, E)).astype(np.float32)


def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E))
    return R.round_bf16((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


# ---------------------------------------------------------------------------------------- 1. exact-integer arm
# one row, one tile minus one, one tile plus one with a second query tile, a K above 16 (other instantiations), two wide query tiles plus one row over eight
# gallery tiles at K = 64, the largest E with K above 64 (the 128-entry list), the largest K
INT_CASES = [(1, 1, 16, 1), (3, 127, 16, 5), (65, 129, 48, 16), (64, 300, 80, 17), (129, 1000, 512, 64), (70, 700, 1024, 65), (5, 513, 64, 128)]


@pytest.mark.parametrize("Q,N,E,K", INT_CASES)
def test_integer_operands_give_the_host_order_bit_for_bit(Q, N, E, K):
    """Entries in [-8, 8] are bf16 numbers and every partial sum stays below 1024 * 64 < 2^24: the scores are exact in any order of addition, ties are
    plentiful, and the whole result is decided by the order alone -- under every split count."""
    rng = np.random.default_rng(1000 * Q + N + E + K)
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    qd, gd = dev16(q), dev16(g)
    for n_split in SPLITS:
        v, i = run(qd, gd, K, n_split, idx_base=7)
        assert R.judge_exact(v, i, q, g, K, idx_base=7), n_split


# ---------------------------------------------------------------------------------------- 2. real arm
@pytest.mark.parametrize("Q,N,E,K", [(65, 129, 48, 16), (129, 1000, 512, 64), (70, 700, 1024, 65)])
def test_unit_norm_rows_within_the_derived_bound_and_the_right_members(Q, N, E, K):
    rng = np.random.default_rng(Q + N + E)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    v, i = run(q, g, K)
    ok, worst = R.judge_real(v, i, q, g, K)
    print(f"(Q, N, E, K) = {(Q, N, E, K)}: worst |vals - s64| / bound = {worst:.4f}, max bound = {R.bound(q, g).max():.3e}")
    assert ok


# ---------------------------------------------------------------------------------------- 3. purity
def test_a_rows_result_does_not_depend_on_the_call_around_it():
    rng = np.random.default_rng(40)
    E, N, K = 64, 300, 33
    q, g = unit_rows(rng, 5, E), unit_rows(rng, N, E)
    g[277] = g[3]                                                             # one exact tie per row
    gd = dev16(g)
    alone = tuple(map(np.concatenate, zip(*[run(q[r:r + 1], gd, K) for r in range(5)])))
    assert R.judge_real(alone[0], alone[1], q, g, K)[0]
    # inside a batch of 129, at other positions of other query tiles
    batch = unit_rows(rng, 129, E)
    at = [0, 31, 64, 127, 128]
    batch[at] = q
    bv, bi = run(batch, gd, K)
    assert same((bv[at], bi[at]), alone)
    batch[[5, 70, 100, 1, 30]] = q                                            # ... and at yet another position
    bv, bi = run(batch, gd, K)
    assert same((bv[[5, 70, 100, 1, 30]], bi[[5, 70, 100, 1, 30]]), alone)
    # every split count; a smaller K is a prefix
    for n_split in SPLITS + (3,):
        assert same(run(q, gd, K, n_split), alone), n_split
    for k in (1, 10, 17):
        for n_split in (0, 3):
            kv, ki = run(q, gd, k, n_split)
            assert same((kv, ki), (alone[0][:, :k], alone[1][:, :k])), (k, n_split)
    # rows of stride ld > E with NaN behind column E
    def padded(a, ld):
        buf = torch.full((a.shape[0], ld), float("nan"), device="cuda", dtype=torch.bfloat16)
        buf[:, :E] = dev16(a)
        return buf[:, :E]
    for n_split in (0, 2):
        assert same(run(padded(q, E + 8), padded(g, E + 24), K, n_split), alone), n_split
    # whatever the workspace held before
    from speechclip_amd._lib import lib
    nbytes = lib().sc_search_workspace_bytes(5, N, K, 7)
    assert nbytes == 5 * 7 * K * 12
    for fill in (0xFF, 0x00, 0x7F):
        ws = torch.full((nbytes,), fill, device="cuda", dtype=torch.uint8)
        assert same(run(q, gd, K, 7, workspace=ws), alone), fill


# ---------------------------------------------------------------------------------------- 4. edges
def test_guards_sentinels_nan_rows_short_lists_and_the_empty_call():
    from speechclip_amd._lib import lib, stream
    L = lib()
    rng = np.random.default_rng(50)
    Q, N, E, K, S, ld = 33, 300, 16, 10, 3, 24
    q, g = int_rows(rng, Q, E), int_rows(rng, N, E)
    g[[5, 128, 299]] = np.nan                                                 # NaN gallery rows: never returned
    want_v, want_i = R.topk(R.scores64(q, g), K)
    assert not np.isin(want_i, [5, 128, 299]).any()
    def guarded(a):                                                           # rows between NaN guard rows, NaN in the gap behind column E
        buf = torch.full((a.shape[0] + 2, ld), float("nan"), device="cuda", dtype=torch.bfloat16)
        buf[1:-1, :E] = dev16(a)
        return buf
    qb, gb = guarded(q), guarded(g)
    nbytes = L.sc_search_workspace_bytes(Q, N, K, S)
    for fill in (0xFF, 0x00):
        ws = torch.full((nbytes + 128,), 0xFF, device="cuda", dtype=torch.uint8)
        ws[64:-64] = fill
        vals = torch.full((Q * K + 32,), 12345.0, device="cuda")
        idx = torch.full((Q * K + 32,), -777, device="cuda", dtype=torch.int64)
        rc = L.sc_search_topk_bf16(qb[1:].data_ptr(), ld, gb[1:].data_ptr(), ld, Q, N, E, K, S, 0, vals[16:].data_ptr(), idx[16:].data_ptr(), ws[64:].data_ptr(),
                                   stream())
        assert rc == 0, L.sc_last_error()
        torch.cuda.synchronize()
        assert (ws[:64] == 0xFF).all() and (ws[-64:] == 0xFF).all()
        assert (vals[:16] == 12345.0).all() and (vals[-16:] == 12345.0).all() and (idx[:16] == -777).all() and (idx[-16:] == -777).all()
        got = (vals[16:-16].cpu().numpy().reshape(Q, K), idx[16:-16].cpu().numpy().reshape(Q, K))
        assert same(got, (want_v, want_i)), fill                              # every output slot written, with the host's bits
    # one split writes vals / idx directly: the same sentinels, no workspace at all
    vals = torch.full((Q * K + 32,), 12345.0, device="cuda")
    idx = torch.full((Q * K + 32,), -777, device="cuda", dtype=torch.int64)
    assert L.sc_search_topk_bf16(qb[1:].data_ptr(), ld, gb[1:].data_ptr(), ld, Q, N, E, K, 1, 0, vals[16:].data_ptr(), idx[16:].data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert (vals[:16] == 12345.0).all() and (vals[-16:] == 12345.0).all() and (idx[:16] == -777).all() and (idx[-16:] == -777).all()
    assert same((vals[16:-16].cpu().numpy().reshape(Q, K), idx[16:-16].cpu().numpy().reshape(Q, K)), (want_v, want_i))
    # fewer than K comparable scores: -inf / -1 in the remaining slots, with one split and with several
    g2 = int_rows(rng, 10, E)
    g2[[2, 3, 9]] = np.nan
    for n_split in (1, 3):
        v, i = run(q, g2, 10, n_split)
        assert same((v, i), R.topk(R.scores64(q, g2), 10))
        assert (i[:, 7:] == -1).all() and np.isneginf(v[:, 7:]).all() and (i[:, :7] >= 0).all()
    # Q == 0: nothing is launched, nothing is written
    vals = torch.full((16,), 12345.0, device="cuda")
    idx = torch.full((16,), -777, device="cuda", dtype=torch.int64)
    assert L.sc_search_topk_bf16(qb.data_ptr(), ld, gb.data_ptr(), ld, 0, N, E, K, S, 0, vals.data_ptr(), idx.data_ptr(), None, stream()) == 0
    torch.cuda.synchronize()
    assert (vals == 12345.0).all() and (idx == -777).all()


# ---------------------------------------------------------------------------------------- 5. EmbeddingIndex and the model surface
@pytest.fixture(scope="module")
def feats():
    g = torch.Generator().manual_seed(70)
    return torch.randn(136, 64, generator=g), torch.randn(7, 64, generator=g), [f"images/{n:04d}.jpg" for n in range(136)]


def test_bf16_index_of_three_adds_equals_one_add_astype_and_state_round_trip(feats):
    from speechclip_amd import ops
    from speechclip_amd.module import EmbeddingIndex
    rows, queries, paths = feats
    one = EmbeddingIndex(64, storage="bf16").add(rows, paths)
    three = EmbeddingIndex(64, storage="bf16")
    for a, b in ((0, 1), (1, 131), (131, 136)):
        three.add(rows[a:b].double() if a else rows[a:b].cuda(), paths[a:b])
    assert [s.shape[0] for s in three.segments] == [1, 130, 5] and all(s.dtype == torch.bfloat16 for s in three.segments + one.segments)
    s1, p1, i1 = one.search(queries, 10)
    s3, p3, i3 = three.search(queries.cuda(), 10)
    assert torch.equal(s1, s3) and torch.equal(p1, p3) and i1 == i3
    assert s1.dtype == torch.float32 and p1.dtype == torch.int64 and i1 == [[paths[p] for p in row] for row in p1.cpu().tolist()]
    # the stored rows are the fp32-normalised rows rounded to nearest even, and the result is the entry's on them
    want = ops.l2norm(rows.cuda()).to(torch.bfloat16)
    assert torch.equal(one.segments[0], want)
    v, p = ops.search_topk_bf16(ops.l2norm(queries.cuda()).to(torch.bfloat16), want, 10)
    assert torch.equal(v, s1) and torch.equal(p, p1)
    # astype: fp32 -> bf16 rounds the same rows, bf16 -> fp32 widens exactly; boundaries and ids stay
    fp32 = EmbeddingIndex(64)
    for a, b in ((0, 1), (1, 131), (131, 136)):
        fp32.add(rows[a:b], paths[a:b])
    down = fp32.astype("bf16")
    assert down.storage == "bf16" and fp32.storage == "fp32" and fp32.segments[1].dtype == torch.float32 and len(down) == 136 and down.ids == fp32.ids
    assert all(torch.equal(a, b) for a, b in zip(down.segments, three.segments)) and len(down.segments) == 3
    sd_, pd_, id_ = down.search(queries, 10)
    assert torch.equal(sd_, s3) and torch.equal(pd_, p3) and id_ == i3
    up = three.astype("fp32")
    assert up.storage == "fp32" and [s.shape[0] for s in up.segments] == [1, 130, 5] and up.ids == three.ids
    assert all(u.dtype == torch.float32 and torch.equal(u, s.float()) for u, s in zip(up.segments, three.segments))
    assert up.segments[0].data_ptr() != three.segments[0].data_ptr() and three.astype("bf16").segments[1].data_ptr() != three.segments[1].data_ptr()
    su, pu, _ = up.astype("bf16").search(queries, 10)
    assert torch.equal(su, s3) and torch.equal(pu, p3)
    # state_dict: host values, the rows as a bf16 tensor, the same results after the round trip
    sd = three.state_dict()
    assert all(isinstance(v, (int, bool, list, type(None))) or (torch.is_tensor(v) and not v.is_cuda) for v in sd.values())
    assert sd["storage"] == 16 and sd["feats"].dtype == torch.bfloat16 and sd["feats"].shape == (136, 64)
    assert sd["feats"].numel() * sd["feats"].element_size() * 2 == fp32.state_dict()["feats"].numel() * 4
    back = EmbeddingIndex.from_state_dict(sd, "cuda")
    sb, pb, ib = back.search(queries, 10)
    assert back.storage == "bf16" and [s.shape[0] for s in back.segments] == [1, 130, 5]
    assert torch.equal(sb, s3) and torch.equal(pb, p3) and ib == i3
    # a dict written before there was a storage key is an fp32 index
    old = fp32.state_dict()
    assert old.pop("storage") == 32
    legacy = EmbeddingIndex.from_state_dict(old, "cuda")
    assert legacy.storage == "fp32" and legacy.segments[1].dtype == torch.float32
    sl, pl, il = legacy.search(queries, 10)
    sf, pf, if_ = fp32.search(queries, 10)
    assert torch.equal(sl, sf) and torch.equal(pl, pf) and il == if_
    with pytest.raises(ValueError):
        EmbeddingIndex.from_state_dict(dict(sd, storage=8), "cuda")


@pytest.mark.parametrize("E", [32, 64, 512])
def test_planted_neighbours_of_the_fp32_index_are_in_the_bf16_result(E):
    """Three rows of cosine ~ 0.94 per query among random unit rows.  Rounding a unit row to bf16 moves it by at most 2^-9 of its length, so by
    Cauchy-Schwarz a score moves by at most 2^-9 + 2^-9 + 2^-18 < 1.01 * 2^-8; delta adds both accumulation bounds (sum |q g| <= 1.01 for unit rows).  An
    fp32 result more than 2 delta above the fp32 (K + 1)-th score cannot be displaced by any row outside the fp32 top K."""
    from speechclip_amd.module import EmbeddingIndex
    rng = np.random.default_rng(80 + E)
    Q, N, K = 8, 400, 10
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)             # noqa: E731
    q, g = unit(rng.standard_normal((Q, E))), unit(rng.standard_normal((N, E)))
    planted = rng.permutation(N)[:3 * Q].reshape(Q, 3)
    for r in range(Q):
        noise = rng.standard_normal((3, E))
        noise = unit(noise - (noise @ q[r])[:, None] * q[r])
        g[planted[r]] = 0.94 * q[r] + np.sqrt(1 - 0.94 ** 2) * noise
    gt, qt = torch.from_numpy(g.astype(np.float32)), torch.from_numpy(q.astype(np.float32))
    s32, p32, _ = EmbeddingIndex(E).add(gt).search(qt, K + 1)
    s16, p16, _ = EmbeddingIndex(E, storage="bf16").add(gt).search(qt, K)
    delta = 1.01 * 2.0 ** -8 + 1.01 * (R.c_of(E) * R.U + R32.gamma(E))
    s32, p32, p16 = s32.cpu().numpy().astype(np.float64), p32.cpu().numpy(), p16.cpu().numpy()
    sure = s32[:, :K] - s32[:, K:] > 2 * delta
    counts = sure.sum(1)
    print(f"E = {E}: delta = {delta:.3e}; fp32 results more than 2 delta above the (K + 1)-th score per query: {counts.tolist()}")
    assert (counts >= 3).all()
    for r in range(Q):
        assert np.isin(p32[r, :K][sure[r]], p16[r]).all(), r
        assert np.isin(planted[r], p32[r, :K][sure[r]]).all(), r                  # the planted rows are among them


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


def test_model_build_index_with_bf16_storage_returns_planted_duplicates_first(model):
    g = torch.Generator().manual_seed(72)
    images = torch.randn(12, 3, 64, 64, generator=g).cuda()
    names = [f"img{n}.jpg" for n in range(12)]
    index = model.build_index(images=images, ids=names, batch_size=5, storage="bf16")
    assert index.storage == "bf16" and len(index) == 12 and [s.shape[0] for s in index.segments] == [5, 5, 2]
    assert all(s.dtype == torch.bfloat16 for s in index.segments) and not model.training
    assert model.build_index(images=images[:2]).storage == "fp32"               # the default is unchanged
    dup = [7, 2, 11, 0]
    scores, pos, ids = model.search(index, 3, images=images[dup])
    top = scores.cpu().numpy()
    print(f"duplicate's score and its margin over the runner-up: {top[:, 0].tolist()} {(top[:, 0] - top[:, 1]).tolist()}")
    assert pos[:, 0].cpu().tolist() == dup and [row[0] for row in ids] == [names[p] for p in dup]
    assert scores.dtype == torch.float32 and (np.abs(top[:, 0] - 1.0) < 2.0 ** -7).all()      # |q_bf16|^2: within two roundings of 1
    with pytest.raises(ValueError):
        model.build_index(images=images, storage="fp16")

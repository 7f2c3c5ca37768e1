"""EmbeddingIndex.search(q, k, rerank=R) end to end: it must equal index.search(q, k) bit for bit in scores and positions, with equal ids -- where the
certificate carries the result (a share is asserted, so the fallback cannot carry the test), where nothing is certified, and where both happen in one call.
The galleries and the flags' restatement are tests/search_rerank_ref.py's; tests/test_search_rerank_host.py shows that every flag asserted here lies far
from the certificate's edge."""
import dataclasses

import numpy as np
import pytest
import torch

import search_rerank_ref as RR

pytestmark = pytest.mark.gpu


def index_of(g, cuts=None, ids=None, shadow=True):
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(g.shape[1], shadow=shadow)
    cuts = cuts or [(0, len(g))]
    for a, b in cuts:
        index.add(torch.from_numpy(g[a:b]), None if ids is None else ids[a:b])
    return index


def both(index, q, k, R, **kw):
    """fp32 search against two-stage search -> the certified flags (bool [Q], host)."""
    q = torch.from_numpy(q) if isinstance(q, np.ndarray) else q
    ws, wp, wi = index.search(q, k, **kw)
    out = index.search(q, k, rerank=R, return_certified=True, **kw)
    assert len(out) == 4 and len(index.search(q, k, rerank=R, **kw)) == 3
    s, p, i, c = out
    assert s.dtype == torch.float32 and p.dtype == torch.int64 and c.dtype == torch.bool and not c.is_cuda and c.shape == (q.shape[0],)
    assert torch.equal(s.view(torch.int32), ws.view(torch.int32)) and torch.equal(p, wp) and i == wi
    return c


@pytest.mark.parametrize("N,E,K,R,seed", [(4096, 64, 4, 32, 0), (2048, 128, 10, 128, 3)])
def test_random_unit_rows_are_certified_and_equal_the_fp32_search(N, E, K, R, seed):
    q, g = RR.gallery_a(N, E, seed=seed)
    c = both(index_of(g), q, K, R)
    print(f"certified share {c.float().mean().item():.3f}")
    assert c.float().mean().item() >= 0.9


def test_near_duplicates_fall_back_and_still_equal_the_fp32_search():
    q, g = RR.gallery_b()
    index = index_of(g)
    c = both(index, q, 5, 40)
    assert not c.any()
    # control: this gallery is one the bf16 search alone gets wrong
    qt = torch.from_numpy(q)
    assert (index.astype("bf16").search(qt, 5)[1] != index.search(qt, 5)[1]).any(1).any()


def test_mixed_gallery_certifies_exactly_the_queries_away_from_the_duplicates():
    q, g = RR.gallery_c()
    c = both(index_of(g), q, RR.C_K, RR.C_R)
    half = len(q) // 2
    assert not c[:half].any() and c[half:].all()


def test_three_segments_one_shorter_than_R_and_with_shadow_of_an_existing_index():
    q, g = RR.gallery_a(1520, 64, Q=33, seed=5)
    cuts = [(0, 1000), (1000, 1020), (1020, 1520)]
    index = index_of(g, cuts)
    assert [s.shape[0] for s in index.shadow_segments] == [1000, 20, 500] and all(s.dtype == torch.bfloat16 for s in index.shadow_segments)
    c = both(index, q, 5, 32)
    assert c.float().mean().item() >= 0.9
    plain = index_of(g, cuts, shadow=False)
    later = plain.with_shadow()
    assert not plain.shadow and later.shadow and later.segments[0].data_ptr() == plain.segments[0].data_ptr()
    for a, b, r in zip(later.shadow_segments, plain.astype("bf16").segments, index.shadow_segments):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(a.view(torch.int16), r.view(torch.int16))
    assert torch.equal(both(later, q, 5, 32), c)
    both(index, q, 25, 25)                                                    # k above the short segment's length: padded lists, R == k


def test_exclude_with_rerank_equals_search_with_exclude():
    """Five rows per item (item + 0.3 noise); every query is a row of the gallery and leaves its own item out."""
    rng = np.random.default_rng(6)
    items, E = 120, 64
    centre = RR.unit_rows(rng, items, E)
    g = np.repeat(centre, 5, 0) + 0.3 * RR.unit_rows(rng, 5 * items, E)
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    ids = [f"item{n // 5}" for n in range(5 * items)]
    index = index_of(g, [(0, 333), (333, 600)], ids)
    rows = rng.permutation(5 * items)[:40]
    exclude = [ids[r] for r in rows]
    exclude[3] = None
    exclude[4] = "not in the index"
    c = both(index, g[rows], 10, 64, exclude=exclude)
    _, _, got = index.search(torch.from_numpy(g[rows]), 10, exclude=exclude, rerank=64)
    assert all(e not in row for e, row in zip(exclude[5:], got[5:]))
    assert c.any()


def test_state_dict_round_trip_keeps_the_shadow_option_and_rebuilds_the_rows():
    from speechclip_amd.module import EmbeddingIndex
    q, g = RR.gallery_a(700, 64, Q=9, seed=7)
    index = index_of(g, [(0, 300), (300, 700)], list(range(100, 800)))
    sd = index.state_dict()
    assert sd["shadow"] is True and not any("shadow" in k and k != "shadow" for k in sd)
    assert all(isinstance(v, (int, bool, list, type(None))) or (torch.is_tensor(v) and not v.is_cuda) for v in sd.values())
    back = EmbeddingIndex.from_state_dict(sd, "cuda")
    assert back.shadow and len(back.shadow_segments) == 2
    for a, b in zip(back.shadow_segments, index.shadow_segments):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(both(back, q, 6, 48), both(index, q, 6, 48))
    sd.pop("shadow")
    assert not EmbeddingIndex.from_state_dict(sd, "cuda").shadow                # a dict without the key loads as before
    with pytest.raises(ValueError):
        EmbeddingIndex.from_state_dict(sd, "cuda").search(torch.from_numpy(q), 6, rerank=48)


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


def test_model_search_with_rerank_equals_model_search(model):
    g = torch.Generator().manual_seed(72)
    images = torch.randn(12, 3, 64, 64, generator=g).cuda()
    wavs = [0.3 * torch.randn(n, generator=g).cuda() for n in (8000, 6000, 3000, 5000)]
    names = [f"img{n}.jpg" for n in range(12)]
    index = model.build_index(images=images, ids=names, batch_size=5, shadow=True)
    assert index.shadow and [s.shape[0] for s in index.shadow_segments] == [5, 5, 2]
    want = model.search(index, 3, wav=wavs)
    got = model.search(index, 3, wav=wavs, rerank=8)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1]) and got[2] == want[2]
    assert not model.build_index(images=images, ids=names, batch_size=5).shadow

"""CPU-only checks of the gallery-search surface: the header's contract and the exported entries, the two pure host functions against their Python
restatements, every argument rule (refused before any launch), the no-GPU behaviour of EmbeddingIndex and the exact chain restatement itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sc_search_splits", "sc_search_workspace_bytes", "sc_search_topk", "sc_topk_merge"]


def test_entries_are_declared_documented_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is (ctypes.c_int64 if n.endswith("_bytes") else ctypes.c_int)
    block = text[text.index("Gallery search"):]
    assert "ARITHMETIC CONTRACT" in block and "fmaf(q[i*ld_q + e], g[j*ld_g + e], acc)" in block and "v_mfma_f32_32x32x2_f32" in block
    assert "score descending, then j ascending" in block and "-inf / -1" in block
    assert L.sc_abi_version() == 1


def test_split_rule_and_workspace_size_equal_their_restatements():
    from speechclip_amd._lib import lib
    L = lib()
    for Q in (0, 1, 2, 63, 64, 65, 128, 129, 256, 1000, 4096, 100000):
        for N in (1, 10, 255, 256, 257, 511, 512, 5000, 123287, 1000000, 2 ** 31 - 1):
            for K in (1, 10, 16, 17, 64, 65, 128):
                assert L.sc_search_splits(Q, N, K) == R.search_splits(Q, N, K), (Q, N, K)
                for n_split in (0, 1, 2, 7, 1024):
                    want = R.workspace_bytes(Q, N, K, n_split) if Q > 0 else 0
                    assert L.sc_search_workspace_bytes(Q, N, K, n_split) == want, (Q, N, K, n_split)
    assert L.sc_search_splits(1, 10 ** 6, 10) == 512 and L.sc_search_splits(256, 10 ** 6, 10) == 256 and L.sc_search_splits(1000, 5000, 10) == 19
    assert L.sc_search_workspace_bytes(1000, 10 ** 6, 10, 0) == 1000 * 64 * 10 * 12 < 1000 * 10 ** 6 * 4 // 8
    assert L.sc_search_workspace_bytes(1000, 10 ** 6, 10, 1024) < 1000 * 10 ** 6 * 4 // 8          # O(Q n_split K) at the largest split count too


def test_every_argument_rule_is_a_code_with_a_message_before_any_launch():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused
    def topk(q=A, ld_q=64, g=A, ld_g=64, Q=4, N=100, E=64, K=10, n_split=1, vals=A, idx=A, ws=None):
        return L.sc_search_topk(q, ld_q, g, ld_g, Q, N, E, K, n_split, 0, vals, idx, ws, None)
    for kw, msg in [(dict(E=6, ld_q=8, ld_g=8), b"E=6"), (dict(E=0), b"E=0"), (dict(E=1028, ld_q=1028, ld_g=1028), b"E=1028"), (dict(ld_q=60), b"ld_q=60"),
                    (dict(ld_g=66), b"ld_g=66"), (dict(q=A + 4), b"16-byte"), (dict(g=A + 8), b"16-byte"), (dict(K=0), b"K=0"), (dict(K=129, N=500), b"K=129"),
                    (dict(K=10, N=9), b"exceeds N=9"), (dict(N=2 ** 31), b"2^31"), (dict(n_split=-1), b"n_split=-1"), (dict(n_split=1025), b"n_split=1025"),
                    (dict(Q=-1), b"Q=-1"), (dict(q=None), b"null operand"), (dict(vals=None), b"null operand"), (dict(n_split=2), b"workspace")]:
        assert topk(**kw) != 0 and msg in L.sc_last_error(), (kw, L.sc_last_error())
    assert topk(Q=0) == 0 and topk(Q=0, q=None, g=None, vals=None, idx=None) == 0           # the empty call is a no-op
    def merge(Q=4, L_=20, K=10, vin=A, iin=A, vals=A, idx=A):
        return L.sc_topk_merge(vin, iin, Q, L_, K, vals, idx, None)
    for kw, msg in [(dict(K=0), b"K=0"), (dict(K=129, L_=500), b"K=129"), (dict(K=10, L_=9), b"exceeds L=9"), (dict(Q=-1), b"Q=-1"), (dict(vin=None), b"null operand")]:
        assert merge(**kw) != 0 and msg in L.sc_last_error(), (kw, L.sc_last_error())
    assert merge(Q=0) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_embedding_index_without_a_gpu_raises_instead_of_falling_back():
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(8)
    assert len(index) == 0
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.add(torch.zeros(3, 8))
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 8), 1)
    from speechclip_amd import ops
    with pytest.raises(SpeechClipHipError):
        ops.search_topk(torch.zeros(1, 8), torch.zeros(4, 8), 1)
    with pytest.raises(SpeechClipHipError):
        ops.topk_merge(torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int64), 1)


def test_exact_chain_restatement():
    """On integers the chain is exact, so it must equal numpy's product; on mixed magnitudes it must differ from the fp64 sum by no more than the bound,
    equal a float64 emulation wherever that one is itself exact, and round ties to even."""
    rng = np.random.default_rng(5)
    q, g = rng.integers(-8, 9, (6, 64)).astype(np.float32), rng.integers(-8, 9, (7, 64)).astype(np.float32)
    assert np.array_equal(R.chain_scores(q, g), (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32))
    from fractions import Fraction
    assert R.round_f32(Fraction(2 ** 24 + 1)) == np.float32(2 ** 24) and R.round_f32(Fraction(2 ** 24 + 3)) == np.float32(2 ** 24 + 4)
    assert R.round_f32(Fraction(-(2 ** 24 + 1))) == np.float32(-(2 ** 24)) and R.round_f32(Fraction(1, 3)) == np.float32(1 / 3)
    assert R.round_f32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148) and R.round_f32(Fraction(1, 2 ** 150)) == 0       # subnormal grid: 2^-149
    q = (rng.choice([-1.0, 1.0], (4, 8)) * np.exp2(rng.integers(-10, 11, (4, 8))) * (1 + rng.random((4, 8)))).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], (5, 8)) * np.exp2(rng.integers(-10, 11, (5, 8))) * (1 + rng.random((5, 8)))).astype(np.float32)
    s = R.chain_scores(q, g)
    assert (np.abs(s.astype(np.float64) - R.scores64(q, g)) <= R.bound(q, g)).all()
    one = R.fmaf_chain(q[0, :1], g[0, :1])                                    # a single step is the correctly rounded product
    assert one == np.float32(np.float64(q[0, 0]) * np.float64(g[0, 0]))


def test_topk_and_merge_restatements_agree_on_ties_nan_and_short_rows():
    s = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 1.0]])
    v, i = R.topk(s, 6, idx_base=10)
    assert i.tolist() == [[11, 13, 10, 15, 14, -1]] and v[0, :5].tolist() == [3.0, 3.0, 1.0, 1.0, -np.inf] and np.isneginf(v[0, 5])
    mv, mi = R.merge(np.array([[1.0, 3.0, 3.0, 7.0, np.nan]], np.float32), np.array([[4, 9, 2, -1, 5]]), 4)
    assert mi.tolist() == [[2, 9, 4, -1]] and mv[0, :3].tolist() == [3.0, 3.0, 1.0]

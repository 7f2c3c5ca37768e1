"""CPU-only checks of the search by threshold: the header's contract and the four exported entries, every argument rule (refused before any launch), the
no-GPU behaviour of ops.search_range*, EmbeddingIndex.search_range and KWClipBase.search_range, the scan that joins the two passes, and the host statement
(tests/search_range_ref.py) against a brute-force loop."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import search_range_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, FILL = ["sc_search_range_count", "sc_search_range_count_bf16"], ["sc_search_range_fill", "sc_search_range_fill_bf16"]


def test_entries_are_declared_documented_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n, arity in [(n, 14) for n in COUNT] + [(n, 17) for n in FILL]:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]) == arity, n
        assert getattr(L, n).restype is ctypes.c_int
    assert text.index("Gallery search by threshold") > text.index("int sc_search_rescore(")            # a block of its own after the others
    block = text[text.index("Gallery search by threshold"):]
    for phrase in ("RANGE CONTRACT", "s(i, j) >= thresh[i]", "NaN threshold hits nothing", "ASCENDING j", "NO ATOMICS", "sc_search_splits(Q, N, 1)",
                   "ld_counts > n_split", "pure", "refused"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "speechclip_amd", "csrc", "search_range.hip")).read()
    assert sorted(re.findall(r'extern "C"\s+\w+\s+(\w+)\s*\(', src)) == sorted(COUNT + FILL)
    assert "atomicAdd" not in src and "__hip_atomic" not in src and "search_kernel" not in src
    for name in ("search_range", "search_range_bf16", "search_range_count", "search_range_fill", "search_range_offsets"):
        from speechclip_amd import ops
        assert callable(getattr(ops, name)), name


def test_every_argument_rule_is_a_code_with_a_message_before_any_launch():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused
    def call(name, fill, q=A, ld_q=64, g=A, ld_g=64, Q=4, N=1000, E=64, thresh=A, n_split=1, g_item=None, q_skip=None, tab=A, ld_tab=1, vals=A, idx=A):
        if fill:
            return getattr(L, name)(q, ld_q, g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip, 0, tab, ld_tab, vals, idx, None)
        return getattr(L, name)(q, ld_q, g, ld_g, Q, N, E, thresh, n_split, g_item, q_skip, tab, ld_tab, None)
    for names, fill in ((COUNT, False), (FILL, True)):
        for name in names:
            bf16 = name.endswith("_bf16")
            rules = [(dict(E=0), b"E=0"), (dict(E=1040, ld_q=1040, ld_g=1040), b"E=1040"), (dict(ld_q=56), b"ld_q=56"), (dict(ld_g=66), b"ld_g=66"),
                     (dict(q=A + 4), b"16-byte"), (dict(g=A + 8), b"16-byte"), (dict(N=2 ** 31), b"2^31"), (dict(n_split=-1), b"n_split=-1"),
                     (dict(n_split=1025, ld_tab=2000), b"n_split=1025"), (dict(Q=-1), b"Q=-1"), (dict(q=None), b"null operand"), (dict(g=None), b"null operand"),
                     (dict(tab=None), b"null operand"), (dict(thresh=None), b"null thresh"), (dict(q_skip=A), b"q_skip without g_item"),
                     (dict(n_split=3, ld_tab=2), b"ld_offs=2" if fill else b"ld_counts=2"),
                     (dict(n_split=0, N=10 ** 6, ld_tab=511), b"below the 512 splits")]      # the automatic split count is sc_search_splits(Q, N, 1)
            rules += [(dict(E=72, ld_q=72, ld_g=72), b"E=72"), (dict(ld_q=68), b"ld_q=68")] if bf16 else [(dict(E=6, ld_q=8, ld_g=8), b"E=6"), (dict(ld_q=66), b"ld_q=66")]
            rules += [(dict(vals=None), b"null operand"), (dict(idx=None), b"null operand")] if fill else []
            for kw, msg in rules:
                assert call(name, fill, **kw) != 0 and name.encode() + b":" in L.sc_last_error() and msg in L.sc_last_error(), (name, kw, L.sc_last_error())
            assert call(name, fill, Q=0) == 0 and call(name, fill, Q=0, q=None, g=None, thresh=None, tab=None, vals=None, idx=None) == 0   # the empty call


def test_offsets_are_the_exclusive_scan_and_the_limit_is_checked_before_anything_is_allocated():
    from speechclip_amd import ops
    counts = torch.tensor([[2, 0, 1], [0, 0, 0], [4, 5, 0]], dtype=torch.int32)
    lims, offs, total = ops.search_range_offsets(counts)
    assert lims.tolist() == [0, 3, 3, 12] and offs.tolist() == [[0, 2, 2], [3, 3, 3], [3, 7, 12]] and total == 12
    assert lims.dtype == offs.dtype == torch.int64
    assert ops.search_range_offsets(counts, max_results=12)[2] == 12
    with pytest.raises(ValueError, match="12 hits exceed max_results=11"):
        ops.search_range_offsets(counts, max_results=11)
    lims, offs, total = ops.search_range_offsets(torch.zeros(0, 4, dtype=torch.int32))
    assert lims.tolist() == [0] and offs.shape == (0, 4) and total == 0
    big = torch.full((3, 2), 2 ** 30, dtype=torch.int32)                          # the scan runs in 64 bits
    with pytest.raises(ValueError, match=f"{6 * 2 ** 30} hits exceed max_results={ops.RANGE_MAX_RESULTS}"):
        ops.search_range_offsets(big)
    assert ops.RANGE_MAX_RESULTS * 12 <= 2 ** 30 < (ops.RANGE_MAX_RESULTS + 1) * 12


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_without_a_gpu_every_layer_raises_instead_of_falling_back():
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.model.kwClip import KWClipBase
    from speechclip_amd.module import EmbeddingIndex
    t = torch.zeros(1)
    with pytest.raises(SpeechClipHipError):
        ops.search_range(torch.zeros(1, 8), torch.zeros(4, 8), t)
    with pytest.raises(SpeechClipHipError):
        ops.search_range_bf16(torch.zeros(1, 16, dtype=torch.bfloat16), torch.zeros(4, 16, dtype=torch.bfloat16), t)
    with pytest.raises(SpeechClipHipError):
        ops.search_range_count(torch.zeros(1, 8), torch.zeros(4, 8), t)
    with pytest.raises(SpeechClipHipError):
        ops.search_range_fill(torch.zeros(1, 8), torch.zeros(4, 8), t, torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1), torch.zeros(1, dtype=torch.int64))
    for index in (EmbeddingIndex(16), EmbeddingIndex(16, storage="bf16"), EmbeddingIndex(16, shadow=True)):
        with pytest.raises(SpeechClipHipError, match="no host fallback"):
            index.search_range(torch.zeros(1, 16), 0.5)
        with pytest.raises(SpeechClipHipError, match="no host fallback"):
            index.search_range(torch.zeros(2, 16), [0.5, 0.25], exclude=[1, 2], max_results=10)
    stub = types.SimpleNamespace(_embed=lambda images=None, sents=None, wav=None: torch.zeros(len(wav), 16))
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        KWClipBase.search_range(stub, EmbeddingIndex(16), 0.5, wav=[None, None])


def test_model_entry_point_stands_beside_search_and_passes_its_options_through():
    from speechclip_amd.model.kwClip import KWClipBase
    params = inspect.signature(KWClipBase.search_range).parameters
    assert list(params) == ["self", "index", "min_score", "images", "sents", "wav", "exclude", "max_results"]
    assert params["exclude"].default is None and params["max_results"].default is None
    seen = {}
    index = types.SimpleNamespace(search_range=lambda rows, min_score, exclude=None, max_results=None: seen.update(rows=rows, t=min_score, e=exclude, m=max_results))
    stub = types.SimpleNamespace(_embed=lambda images=None, sents=None, wav=None: ("rows of", sents))
    KWClipBase.search_range(stub, index, 0.25, sents=["a"], exclude=["x"], max_results=5)
    assert seen == dict(rows=("rows of", ["a"]), t=0.25, e=["x"], m=5)
    from speechclip_amd.module import EmbeddingIndex
    assert list(inspect.signature(EmbeddingIndex.search_range).parameters) == ["self", "queries", "min_score", "exclude", "max_results"]


def test_host_statement_equals_a_brute_force_loop():
    rng = np.random.default_rng(11)
    score = rng.integers(-3, 4, (7, 23)).astype(np.float32)                       # few values: many ties on every threshold
    score[2, 5] = score[4, :] = np.nan
    score[3, 7], score[3, 8] = np.inf, -np.inf
    thresh = np.array([0.0, -np.inf, 1.0, np.inf, -np.inf, np.nan, 3.0], np.float32)
    items = (np.arange(23) // 5).astype(np.int32)
    skip = np.array([1, -1, 10 ** 6, 0, 2, 3, 4])
    for kw in (dict(), dict(idx_base=7), dict(idx_base=7, items=items, skip=skip), dict(items=items, skip=None)):
        got, want = RR.search_range(score, thresh, **kw), RR.brute_force(score, thresh, **kw)
        assert RR.same(got, want), kw
        assert got[0].dtype == got[2].dtype == np.int64 and got[1].dtype == np.float32
    lims, vals, idx = RR.search_range(score, thresh)
    assert np.diff(lims).tolist() == [int((score[0] >= 0).sum()), 23, int((score[2] >= 1).sum()), 1, 0, 0, int((score[6] >= 3).sum())]
    assert idx[lims[3]:lims[4]].tolist() == [7] and (np.diff(idx[lims[1]:lims[2]]) == 1).all()          # +inf reaches +inf only; -inf takes every row, -inf included
    assert all((np.diff(idx[lims[i]:lims[i + 1]]) > 0).all() for i in range(7))                          # ascending j
    assert RR.hits([1.0, np.nan, 2.0], 1.0).tolist() == [0, 2] and RR.hits([1.0, 2.0], np.nan).tolist() == []
    assert RR.hits([1.0, 2.0, 3.0], 1.0, [4, 5, 4], 4).tolist() == [1] and RR.hits([1.0, 2.0, 3.0], 1.0, [4, 5, 4], -1).tolist() == [0, 1, 2]
    assert not RR.same((lims, vals, idx + 1), (lims, vals, idx)) and not RR.same((lims, -vals, idx), (lims, vals, idx))

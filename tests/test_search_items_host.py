"""CPU-only checks of the id-aware gallery search: the header's contract and the exported entries, the workspace size against its restatement, every
argument rule (refused before any launch), the host statement's own properties on tie-heavy integer scores (tests/search_items_ref.py), and the host-side
argument rules of EmbeddingIndex.search(distinct=, exclude=)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_items_ref as RI
import search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sc_search_items_workspace_bytes", "sc_search_items", "sc_search_items_bf16", "sc_topk_merge_items"]


def test_entries_are_declared_documented_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib, ops
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is (ctypes.c_int64 if n.endswith("_bytes") else ctypes.c_int)
    assert len(L.sc_search_items.argtypes) == len(L.sc_search_items_bf16.argtypes) == len(L.sc_search_topk.argtypes) + 4 == 18
    assert text.index("Gallery search by item") > text.index("int sc_search_topk_bf16(")              # a block of its own AFTER the bf16 one
    block = text[text.index("Gallery search by item"):]
    for phrase in ("SELECTION CONTRACT", "eligible(i, j)", "g_item[j] != q_skip[i]", "REPRESENTATIVE", "first K representatives", "-inf / -1 / -1",
                   "prefix", "bit for bit", "16 Q n_split K", "sc_topk_merge_items joins them", "a null g_item", "outputs must not alias inputs"):
        assert phrase in block, phrase
    assert L.sc_abi_version() == 1
    src = open(os.path.join(ROOT, "speechclip_amd", "csrc", "search_items.hip")).read()
    assert sorted(re.findall(r'extern "C"\s+\w+\s+(\w+)\s*\(', src)) == sorted(NAMES)
    for name in ("search_items", "search_items_bf16", "topk_merge_items"):
        assert callable(getattr(ops, name))


def test_workspace_size_equals_its_restatement():
    from speechclip_amd._lib import lib
    L = lib()
    for Q in (0, 1, 2, 63, 64, 65, 128, 129, 256, 1000, 4096, 100000):
        for N in (1, 10, 255, 256, 257, 511, 512, 5000, 123287, 1000000, 2 ** 31 - 1):
            for K in (1, 10, 16, 17, 64, 65, 128):
                for n_split in (0, 1, 2, 7, 1024):
                    want = RI.workspace_bytes(Q, N, K, n_split) if Q > 0 else 0
                    assert L.sc_search_items_workspace_bytes(Q, N, K, n_split) == want, (Q, N, K, n_split)
                    assert 3 * want == 4 * L.sc_search_workspace_bytes(Q, N, K, n_split)                # the same splits, 16 bytes against 12
    assert L.sc_search_items_workspace_bytes(1000, 10 ** 6, 10, 0) == 1000 * 64 * 10 * 16
    assert L.sc_search_items_workspace_bytes(4, 100, 10, -1) == 0


@pytest.mark.parametrize("name,E,bad_E,bad_ld", [("sc_search_items", 64, (6, 0, 1028), (60, 66)), ("sc_search_items_bf16", 64, (24, 8, 0, 1040), (48, 68))])
def test_every_argument_rule_is_a_code_with_a_message_before_any_launch(name, E, bad_E, bad_ld):
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused
    def call(q=A, ld_q=64, g=A, ld_g=64, Q=4, N=100, E=E, K=10, n_split=1, g_item=A, q_skip=None, distinct=0, vals=A, idx=A, items=A, ws=None):
        return getattr(L, name)(q, ld_q, g, ld_g, Q, N, E, K, n_split, 0, g_item, q_skip, distinct, vals, idx, items, ws, None)
    cases = [(dict(E=e, ld_q=max(e, 8), ld_g=max(e, 8)), f"E={e}".encode()) for e in bad_E]
    cases += [(dict(ld_q=bad_ld[0]), f"ld_q={bad_ld[0]}".encode()), (dict(ld_g=bad_ld[1]), f"ld_g={bad_ld[1]}".encode())]
    cases += [(dict(q=A + 8), b"16-byte"), (dict(g=A + 8), b"16-byte"), (dict(K=0), b"K=0"), (dict(K=129, N=500), b"K=129"), (dict(K=10, N=9), b"exceeds N=9"),
              (dict(N=2 ** 31), b"2^31"), (dict(n_split=-1), b"n_split=-1"), (dict(n_split=1025), b"n_split=1025"), (dict(Q=-1), b"Q=-1"),
              (dict(q=None), b"null operand"), (dict(g=None), b"null operand"), (dict(vals=None), b"null operand"), (dict(idx=None), b"null operand"),
              (dict(g_item=None), b"null g_item"), (dict(items=None), b"null items"), (dict(n_split=2), b"workspace"),
              (dict(n_split=0, Q=1, N=10 ** 6), b"workspace")]
    for distinct in (0, 1):
        for kw, msg in cases:
            assert call(distinct=distinct, **kw) != 0, kw
            err = L.sc_last_error()
            assert msg in err and err.startswith(name.encode() + b":"), (kw, err)
    assert call(Q=0) == 0 and call(Q=0, q=None, g=None, g_item=None, vals=None, idx=None, items=None) == 0      # the empty call is a no-op


def test_every_merge_argument_rule_is_a_code_with_a_message_before_any_launch():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20
    def merge(Q=4, L_=20, K=10, distinct=0, vin=A, iin=A, cin=A, vals=A, idx=A, items=A):
        return L.sc_topk_merge_items(vin, iin, cin, Q, L_, K, distinct, vals, idx, items, None)
    for kw, msg in [(dict(K=0), b"K=0"), (dict(K=129, L_=500), b"K=129"), (dict(K=10, L_=9), b"exceeds L=9"), (dict(Q=-1), b"Q=-1"), (dict(vin=None), b"null operand"),
                    (dict(cin=None), b"null operand"), (dict(items=None), b"null operand"), (dict(distinct=1, L_=1024 * 128 + 1), b"L=131073")]:
        assert merge(**kw) != 0 and msg in L.sc_last_error() and b"sc_topk_merge_items" in L.sc_last_error(), (kw, L.sc_last_error())
    assert merge(Q=0) == 0 and merge(Q=0, distinct=1) == 0


# ---------------------------------------------------------------------------------------- the host statement's own properties
def tie_heavy(seed, Q=6, N=400):
    """Integer scores in [-3, 3] (every value some sixty times per row), two NaN columns."""
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, (Q, N)).astype(np.float64)
    s[:, [5, N - 1]] = np.nan
    return rng, s


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_reference_distinct_with_all_different_codes_equals_plain_topk_and_no_skip_equals_plain_topk():
    rng, s = tie_heavy(1)
    N = s.shape[1]
    codes = rng.permutation(N).astype(np.int32)
    for k in (1, 10, 128):
        want_v, want_i = R.topk(s, k, idx_base=7)
        for distinct in (False, True):
            v, i, c = RI.search(s, codes, k, None, distinct, idx_base=7)
            assert np.array_equal(v.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(i, want_i) and np.array_equal(c, codes[i - 7])
        v, i, c = RI.search(s, codes, k, np.full(s.shape[0], -1), True, idx_base=7)
        assert np.array_equal(i, want_i)


def test_reference_examples_by_hand():
    s = np.array([3.0, 5.0, 5.0, np.nan, 1.0, 5.0, 3.0])
    items = np.array([0, 1, 2, 2, 0, 1, 3], np.int32)
    v, i, c = RI.select(s, items, 5)
    assert i.tolist() == [1, 2, 5, 0, 6] and c.tolist() == [1, 2, 1, 0, 3]
    v, i, c = RI.select(s, items, 5, distinct=True)
    assert i.tolist() == [1, 2, 0, 6, -1] and c.tolist() == [1, 2, 0, 3, -1] and v[:4].tolist() == [5.0, 5.0, 3.0, 3.0] and np.isneginf(v[4])
    v, i, c = RI.select(s, items, 3, skip=1, distinct=True, idx_base=10)
    assert i.tolist() == [12, 10, 16] and c.tolist() == [2, 0, 3]
    v, i, c = RI.select(s, items, 3, skip=9)                                 # a code the gallery does not hold
    assert i.tolist() == [1, 2, 5]
    v, i, c = RI.select(s, np.zeros(7, np.int32), 2, skip=0, distinct=True)  # everything excluded
    assert i.tolist() == [-1, -1] and c.tolist() == [-1, -1] and np.isneginf(v).all()
    mv, mi, mc = RI.merge(np.array([[1.0, 3.0, 3.0, 7.0, np.nan, 2.0]], np.float32), np.array([[4, 9, 2, -1, 5, 6]]), np.array([[0, 1, 1, 2, 3, 0]], np.int32), 3, True)
    assert mi.tolist() == [[2, 6, -1]] and mc.tolist() == [[1, 0, -1]]
    mv, mi, mc = RI.merge(np.array([[1.0, 3.0, 3.0, 7.0, np.nan, 2.0]], np.float32), np.array([[4, 9, 2, -1, 5, 6]]), np.array([[0, 1, 1, 2, 3, 0]], np.int32), 3, False)
    assert mi.tolist() == [[2, 9, 6]] and mc.tolist() == [[1, 1, 0]]


def test_reference_prefix_property():
    rng, s = tie_heavy(2)
    items = RI.grouped_items(rng, s.shape[1], big=210)
    skip = np.array([-1, int(items[0]), 10 ** 6, int(items[7]), -1, int(items[0])])
    for distinct in (False, True):
        full = RI.search(s, items, 128, skip, distinct)
        for k in (1, 10, 64, 127):
            assert same(RI.search(s, items, k, skip, distinct), tuple(a[:, :k] for a in full)), (distinct, k)


@pytest.mark.parametrize("S", [1, 2, 7])
def test_reference_per_split_lists_merged_equal_the_whole(S):
    """The exactness argument of the header ("splits"), checked where it bites: item groups of 1..7 rows and one item of more than N / 2 rows, so that the same
    item has a representative in every split, under heavy ties."""
    rng, s = tie_heavy(3 + S)
    N = s.shape[1]
    items = RI.grouped_items(rng, N, big=N // 2 + 10)
    assert np.bincount(items).max() > N // 2 and set(np.bincount(items).tolist()) >= set(range(1, 8))
    skip = np.array([-1, int(items[0]), 10 ** 6, int(items[7]), -1, int(np.bincount(items).argmax())])
    for distinct in (False, True):
        for k in (1, 10, 57):
            whole = RI.search(s, items, k, skip, distinct)
            assert same(RI.split_and_merge(s, items, k, skip, distinct, S), whole), (distinct, k)
    n_items = len(set(items.tolist()))
    whole = RI.search(s, items, 128, None, True)                              # k above what a split holds, padding inside the partial lists
    assert same(RI.split_and_merge(s, items, 128, None, True, S), whole) and ((whole[1] >= 0).sum(1) == min(128, n_items)).all()


# ---------------------------------------------------------------------------------------- EmbeddingIndex
def filled(monkeypatch, ids, n):
    """An index with n rows' worth of ids and no rows, on a stand-in device: the argument rules run on the host before anything touches the GPU."""
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(8)
    monkeypatch.setattr(index, "_device", lambda t=None: torch.device("cpu"))
    index.ids, index._n = ids, n
    return index


def test_embedding_index_refuses_a_bad_exclude_length_and_k_above_the_id_count(monkeypatch):
    index = filled(monkeypatch, ["a", "b", "a", "c", "b", "a"], 6)
    q = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="3 exclude ids for 2 queries"):
        index.search(q, 2, exclude=["a", "b", "c"])
    with pytest.raises(ValueError, match="1 exclude ids for 2 queries"):
        index.search(q, 2, distinct=True, exclude=["a"])
    with pytest.raises(ValueError, match=r"k=4 .*3 different ids"):
        index.search(q, 4, distinct=True)
    with pytest.raises(ValueError, match=r"k=7 .*6 stored rows"):
        index.search(q, 7, distinct=True)
    plain = filled(monkeypatch, None, 200)
    with pytest.raises(ValueError, match=r"k=129 "):
        plain.search(q, 129, distinct=True)
    codes, table, n = index._item_codes()
    assert table == {"a": 0, "b": 1, "c": 2} and n == 3 and codes == []      # first-seen order; one tensor per segment, none here
    assert "_codes" not in index.state_dict() and set(index.state_dict()) == {"dim", "normalize", "storage", "feats", "segment_rows", "ids"}


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_embedding_index_new_arguments_without_a_gpu_raise_instead_of_falling_back():
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(8)
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 8), 1, distinct=True)
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 8), 1, exclude=[3])
    z, zi = torch.zeros(1, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(SpeechClipHipError):
        ops.search_items(z, torch.zeros(4, 8), 1, zi)
    with pytest.raises(SpeechClipHipError):
        ops.search_items_bf16(z.bfloat16(), torch.zeros(4, 16, dtype=torch.bfloat16), 1, zi, distinct=True)
    with pytest.raises(SpeechClipHipError):
        ops.topk_merge_items(torch.zeros(1, 8), torch.zeros(1, 8, dtype=torch.int64), torch.zeros(1, 8, dtype=torch.int32), 1, True)

"""CPU-only checks of the search inside a subset: the header's contract and the exported entries, every argument rule of sc_search_select[_bf16] and
sc_pack_row_mask (refused before any launch), the host statement's own properties (tests/search_select_ref.py: packing, dead tiles, the device's scheme
against the contract, and every mutant of the scheme told apart by a case of the list), and the host-side argument rules of EmbeddingIndex.search."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_ref as R
import search_select_ref as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["sc_search_select", "sc_search_select_bf16", "sc_pack_row_mask"]


def test_entries_are_declared_documented_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib, ops
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is ctypes.c_int
    assert len(L.sc_search_select.argtypes) == len(L.sc_search_select_bf16.argtypes) == len(L.sc_search_items.argtypes) + 3 == 21
    assert text.index("Gallery search by item") < text.index("Gallery search by subset") < text.index("Gallery search, fp32 re-score")
    block = text[text.index("Gallery search by subset"):text.index("Gallery search, fp32 re-score")]
    for phrase in ("SUBSET CONTRACT", "eligible(i, j)", "bit (j & 31) of g_allow[j >> 5]", "not\n *              idx_base + j", "Bits at j >= N are ignored",
                   "g_group[j] == q_group[i]", "q_group[i] < 0", "both are given or neither", "bit for bit", "DEAD", "no global loads", "No global atomics",
                   "-inf / -1 / -1", "sc_topk_merge_items", "unused high bits"):
        assert phrase in block, phrase
    src = open(os.path.join(ROOT, "speechclip_amd", "csrc", "search_select.hip")).read()
    assert sorted(re.findall(r'extern "C"\s+\w+\s+(\w+)\s*\(', src)) == sorted(NAMES)
    for name in ("search_select", "search_select_bf16", "pack_row_mask"):
        assert callable(getattr(ops, name))
    make = open(os.path.join(ROOT, "speechclip_amd", "csrc", "Makefile")).read()
    assert re.search(r"^[^#\n]*\$\(OBJDIR\)/search_select\.o[^:\n]*:[^\n]*search_core\.h[^\n]*search_rows\.h", make, re.M)
    assert all(n in open(os.path.join(ROOT, "INTEGRATION.md")).read() for n in NAMES)


@pytest.mark.parametrize("name,E,bad_E,bad_ld", [("sc_search_select", 64, (6, 0, 1028), (60, 66)), ("sc_search_select_bf16", 64, (24, 8, 0, 1040), (48, 68))])
def test_every_argument_rule_is_a_code_with_a_message_before_any_launch(name, E, bad_E, bad_ld):
    """Every refusal of sc_search_items[_bf16] (the list of tests/test_search_items_host.py), under every combination of selectors, plus one-sided groups."""
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused
    def call(q=A, ld_q=64, g=A, ld_g=64, Q=4, N=100, E=E, K=10, n_split=1, allow=None, g_group=None, q_group=None, g_item=A, q_skip=None, distinct=0, vals=A,
             idx=A, items=A, ws=None):
        return getattr(L, name)(q, ld_q, g, ld_g, Q, N, E, K, n_split, 0, allow, g_group, q_group, g_item, q_skip, distinct, vals, idx, items, ws, None)
    cases = [(dict(E=e, ld_q=max(e, 8), ld_g=max(e, 8)), f"E={e}".encode()) for e in bad_E]
    cases += [(dict(ld_q=bad_ld[0]), f"ld_q={bad_ld[0]}".encode()), (dict(ld_g=bad_ld[1]), f"ld_g={bad_ld[1]}".encode())]
    cases += [(dict(q=A + 8), b"16-byte"), (dict(g=A + 8), b"16-byte"), (dict(K=0), b"K=0"), (dict(K=129, N=500), b"K=129"), (dict(K=10, N=9), b"exceeds N=9"),
              (dict(N=2 ** 31), b"2^31"), (dict(n_split=-1), b"n_split=-1"), (dict(n_split=1025), b"n_split=1025"), (dict(Q=-1), b"Q=-1"),
              (dict(q=None), b"null operand"), (dict(g=None), b"null operand"), (dict(vals=None), b"null operand"), (dict(idx=None), b"null operand"),
              (dict(g_item=None), b"null g_item"), (dict(items=None), b"null items"), (dict(n_split=2), b"workspace"),
              (dict(n_split=0, Q=1, N=10 ** 6), b"workspace")]
    for selectors in (dict(), dict(allow=A), dict(g_group=A, q_group=A), dict(allow=A, g_group=A, q_group=A, q_skip=A)):
        for distinct in (0, 1):
            for kw, msg in cases:
                assert call(distinct=distinct, **selectors, **kw) != 0, kw
                err = L.sc_last_error()
                assert msg in err and err.startswith(name.encode() + b":"), (kw, err)
    for kw, missing in ((dict(g_group=A), b"q_group is null"), (dict(q_group=A), b"g_group is null"), (dict(allow=A, g_group=A), b"q_group is null")):
        assert call(**kw) != 0 and missing in L.sc_last_error() and L.sc_last_error().startswith(name.encode() + b":"), (kw, L.sc_last_error())
    assert call(Q=0) == 0 and call(Q=0, q=None, g=None, g_item=None, vals=None, idx=None, items=None) == 0      # the empty call is a no-op


def test_pack_row_mask_argument_rules():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20
    for args, msg in (((A, -1, A), b"N=-1"), ((A, 2 ** 31, A), b"N=2147483648"), ((None, 5, A), b"null operand"), ((A, 5, None), b"null operand")):
        assert L.sc_pack_row_mask(*args, None) != 0 and msg in L.sc_last_error() and L.sc_last_error().startswith(b"sc_pack_row_mask:"), (args, L.sc_last_error())
    assert L.sc_pack_row_mask(None, 0, None, None) == 0                       # N == 0 launches nothing


# ---------------------------------------------------------------------------------------- the host statement's own properties
def test_packing_restatement_by_hand():
    assert RS.pack_row_mask([1, 0, 0, 1]).tolist() == [0b1001]
    m = np.zeros(65, np.uint8)
    m[[0, 31, 32, 64]] = (1, 7, 255, 1)                                       # any non-zero byte is a set bit
    assert RS.pack_row_mask(m).tolist() == [0x80000001, 0x00000001, 0x00000001]
    assert RS.pack_row_mask(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1] and RS.pack_row_mask(np.ones(64, bool)).tolist() == [0xFFFFFFFF] * 2
    assert RS.pack_row_mask([]).shape == (0,)
    for N in RS.NS:
        mask = np.random.default_rng(N).random(N) < 0.5
        words = RS.pack_row_mask(mask)
        assert words.dtype == np.uint32 and words.shape == ((N + 31) // 32,) and np.array_equal(RS.allowed_rows(words, N), mask)
        assert int(words[-1]) >> ((N - 1) % 32 + 1) == 0
        words[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF) if N % 32 else np.uint32(0)
        assert np.array_equal(RS.allowed_rows(words, N), mask)               # bits at j >= N are ignored


def test_dead_tile_classification_by_hand():
    one = lambda N, rows: RS.pack_row_mask(np.isin(np.arange(N), rows))
    assert [d.tolist() for d in RS.dead_tiles(300, 1, None)] == [[False, False, False]]
    assert [d.tolist() for d in RS.dead_tiles(300, 1, one(300, [128]))] == [[True, False, True]]
    assert [d.tolist() for d in RS.dead_tiles(300, 1, one(300, [127, 299]))] == [[False, True, False]]
    # three ranges of 100 rows: row 100 belongs to the second range alone, though it shares word 3 with rows 96 .. 99 of the first
    assert [d.tolist() for d in RS.dead_tiles(300, 3, one(300, [100]))] == [[True], [False], [True]]
    assert [d.tolist() for d in RS.dead_tiles(300, 3, one(300, [99]))] == [[False], [True], [True]]
    assert [d.tolist() for d in RS.dead_tiles(300, 3, one(300, []))] == [[True], [True], [True]]
    # 7 ranges of 591 rows over 4133: tiles of the second range start at row 591, not at a multiple of 128
    dead = RS.dead_tiles(4133, 7, one(4133, [591 + 127, 591 + 128 * 4]))
    assert [d.tolist() for d in dead][1] == [False, True, True, True, False] and all(d.all() for n, d in enumerate(dead) if n != 1)
    garbage = one(33, [])
    garbage[-1] = 0xFFFFFFFE
    assert [d.tolist() for d in RS.dead_tiles(33, 1, garbage)] == [[True]]


def observe(case, S, mutant=None, queries=6):
    """What a (mutated) implementation shows of a case at S splits: the packed mask, the dead tiles and the result bits of the first few queries."""
    o = RS.operands(case, "fp32")
    n = min(queries, case.Q)
    s = R.scores64(o["q"][:n], o["g"])
    cut = lambda a: None if a is None else a[:n]
    v, i, c = RS.device_scheme(s, o["items"], case.K, o["words"], o["g_group"], cut(o["q_group"]), cut(o["skip"]), o["distinct"], S, 5, mutant)
    dead = np.concatenate(RS.dead_tiles(case.N, S, o["words"], mutant))
    return RS.pack_row_mask(o["mask"], mutant).tobytes(), dead.tobytes(), v.tobytes(), i.tobytes(), c.tobytes()


def test_the_case_list_covers_what_it_claims():
    cases = RS.CASES
    assert len(cases) == len(RS.NS) * len(RS.MASKS) and all(c.K <= c.N for c in cases)
    assert {c.Q for c in cases} == set(RS.QS) and {c.K for c in cases} == set(RS.KS) and {c.e for c in cases} == {0, 1, 2}
    assert {(c.Q > 64 and c.K <= 64, c.K <= 16) for c in cases} == {(a, b) for a in (False, True) for b in (False, True)}      # the four instantiations
    assert {c.group for c in cases} == set(RS.GROUPS) and {(c.N, c.mask) for c in cases} == {(N, m) for N in RS.NS for m in RS.MASKS}
    for N in RS.NS:
        mask, words = RS.make_mask("garbage_high_bits", N)
        assert np.array_equal(RS.allowed_rows(words, N), mask) and (N % 32 == 0 or int(words[-1]) >> (N % 32) == 0xFFFFFFFF >> (N % 32))
    assert any(d.all() for d in RS.dead_tiles(4133, 7, RS.make_mask("one_live_tile", 4133)[1])) and RS.dead_tiles(4133, 1, RS.make_mask("first_tile_dead", 4133)[1])[0][0]


def test_the_scheme_of_ranges_live_tiles_and_merge_equals_the_contract_on_every_case():
    for case in RS.CASES:
        o = RS.operands(case, "fp32")
        n = min(6, case.Q)
        s = R.scores64(o["q"][:n], o["g"])
        cut = lambda a: None if a is None else a[:n]
        want = RS.search(s, o["items"], case.K, o["words"], o["g_group"], cut(o["q_group"]), cut(o["skip"]), o["distinct"], 5)
        for S in RS.SPLITS:
            assert observe(case, S)[2:] == tuple(x.tobytes() for x in want), (case, S)


@pytest.mark.parametrize("mutant", RS.MUTANTS)
def test_every_mutant_is_told_apart_by_a_case_of_the_list(mutant):
    """A mutant no case sees means a case is missing."""
    for case in RS.CASES:
        for S in RS.SPLITS:
            if observe(case, S, mutant) != observe(case, S):
                return
    pytest.fail(f"no case of the list tells {mutant} from the statement")


# ---------------------------------------------------------------------------------------- EmbeddingIndex
def filled(monkeypatch, ids, n):
    """An index with n rows' worth of ids and no rows, on a stand-in device: the argument rules run on the host before anything touches the GPU."""
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(8)
    monkeypatch.setattr(index, "_device", lambda t=None: pytest.fail("an argument rule let the call through to the device"))
    index.ids, index._n = ids, n
    return index


def test_embedding_index_argument_rules_are_checked_before_the_device(monkeypatch):
    from speechclip_amd.module.retrieval import RowSelector
    index = filled(monkeypatch, ["a", "b", "a", "c", "b", "a"], 6)
    q = torch.zeros(2, 8)
    ok = torch.ones(6, dtype=torch.bool)
    for kw, msg in ((dict(allow=ok, allow_ids=["a"]), "exclude each other"),
                    (dict(row_groups=torch.zeros(6, dtype=torch.int64)), "together or not at all"),
                    (dict(query_groups=[0, 1]), "together or not at all"),
                    (dict(within=["a", "b"], row_groups=torch.zeros(6, dtype=torch.int64), query_groups=[0, 0]), "within cannot be combined with row_groups"),
                    (dict(within=["a"]), "1 within ids for 2 queries"),
                    (dict(row_groups=torch.zeros(6, dtype=torch.int64), query_groups=[0]), "1 query_groups for 2 queries"),
                    (dict(row_groups=torch.zeros(5, dtype=torch.int64), query_groups=[0, 0]), r"row_groups must be an int per stored row \[6\]"),
                    (dict(row_groups=torch.zeros(6), query_groups=[0, 0]), "row_groups must be an int per stored row"),
                    (dict(row_groups=torch.tensor([0, 1, -1, 0, 0, 0]), query_groups=[0, 0]), r"values in \[0, 2\^31\)"),
                    (dict(row_groups=torch.zeros(6, dtype=torch.int64), query_groups=[0, 0.5]), "one int per query"),
                    (dict(allow=torch.ones(5, dtype=torch.bool)), r"allow must be a bool per stored row \[6\]"),
                    (dict(allow=torch.ones(6)), "allow must be a bool per stored row"),
                    (dict(allow=RowSelector(filled(monkeypatch, None, 6), [], 6)), "another index"),
                    (dict(allow=RowSelector(index, [], 5)), "held 5 rows; it holds 6 now"),
                    (dict(allow=ok, rerank=10), "certificate speaks about the whole gallery"),
                    (dict(allow_ids=["a"], rerank=10), "certificate speaks about the whole gallery"),
                    (dict(within=["a", "b"], rerank=10), "certificate speaks about the whole gallery"),
                    (dict(row_groups=torch.zeros(6, dtype=torch.int64), query_groups=[0, 0], rerank=10), "certificate speaks about the whole gallery")):
        with pytest.raises(ValueError, match=msg):
            index.search(q, 2, **kw)
    with pytest.raises(ValueError, match="one of the two"):
        index.selector()
    with pytest.raises(ValueError, match="one of the two"):
        index.selector(allow=ok, allow_ids=["a"])
    with pytest.raises(ValueError, match="allow must be a bool per stored row"):
        index.selector(allow=torch.ones(7, dtype=torch.bool))
    assert index._allow_mask(None, ["a", "zzz"]).tolist() == [True, False, True, False, False, True]       # ids the index does not hold select nothing
    assert filled(monkeypatch, None, 4)._allow_mask(None, {1, 3, 9}).tolist() == [False, True, False, True]  # without ids the id of a row is its position
    sel = index._select_arguments(q, None, None, ["c", "nowhere"], None, None, None)
    assert sel[2] == [2, 3] and sel[3]                                        # within: the id's item code; an id the index lacks gets the code no row carries
    assert index._select_arguments(q, None, None, [None, "a"], None, None, None)[2] == [3, 0]
    assert index._select_arguments(q, None, None, None, None, None, None) is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_without_a_gpu_the_new_arguments_raise_instead_of_falling_back():
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(8)
    index._n = 4
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 8), 1, allow=torch.ones(4, dtype=torch.bool))
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 8), 1, within=[2])
    z, zi = torch.zeros(1, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(SpeechClipHipError):
        ops.search_select(z, torch.zeros(4, 8), 1, zi)
    with pytest.raises(SpeechClipHipError):
        ops.search_select_bf16(z.bfloat16(), torch.zeros(4, 16, dtype=torch.bfloat16), 1, zi, g_group=zi, q_group=zi[:1])
    with pytest.raises(SpeechClipHipError):
        ops.pack_row_mask(torch.ones(4, dtype=torch.bool))

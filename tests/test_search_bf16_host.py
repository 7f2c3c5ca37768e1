"""CPU-only checks of the bf16 gallery-search surface: the header's contract and the exported entry, every argument rule (refused before any launch),
EmbeddingIndex's storage argument without a GPU, and the host statements themselves -- the judges of tests/search_bf16_ref.py accept an fp32-accumulated
stand-in and reject three mutants of it."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_bf16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sc_search_topk_bf16"


def test_entry_is_declared_documented_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    assert NAME in _lib.exported_symbols() and hasattr(L, NAME)
    params = re.search(rf"^int {NAME}\s*\(([^)]*)\)", text, re.M).group(1)
    fp32 = re.search(r"^int sc_search_topk\s*\(([^)]*)\)", text, re.M).group(1)
    assert len(L.sc_search_topk_bf16.argtypes) == len(params.split(",")) == len(fp32.split(",")) == 14
    assert L.sc_search_topk_bf16.restype is ctypes.c_int
    assert text.index("Gallery search, bf16 storage") > text.index("int sc_topk_merge(")           # a block of its own AFTER the fp32 one
    block = text[text.index("Gallery search, bf16 storage"):]
    for phrase in ("BF16 ARITHMETIC CONTRACT", "v_mfma_f32_32x32x16_bf16", "ascending groups of 16", "c = 2 E / (1 - 2 E 2^-24)",
                   "score descending, then j ascending", "-inf / -1", "Subnormal operands", "E % 16 != 0", "multiples of 8"):
        assert phrase in block, phrase
    assert L.sc_abi_version() == 1
    src = open(os.path.join(ROOT, "speechclip_amd", "csrc", "search_bf16.hip")).read()
    assert re.findall(r'extern "C"\s+\w+\s+(\w+)\s*\(', src) == [NAME]                             # no other host entry: splits, workspace, merge are reused


def test_every_argument_rule_is_a_code_with_a_message_before_any_launch():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused
    def topk(q=A, ld_q=64, g=A, ld_g=64, Q=4, N=100, E=64, K=10, n_split=1, vals=A, idx=A, ws=None):
        return L.sc_search_topk_bf16(q, ld_q, g, ld_g, Q, N, E, K, n_split, 0, vals, idx, ws, None)
    for kw, msg in [(dict(E=24, ld_q=24, ld_g=24), b"E=24"), (dict(E=8, ld_q=8, ld_g=8), b"E=8"), (dict(E=0), b"E=0"), (dict(E=1040, ld_q=1040, ld_g=1040), b"E=1040"),
                    (dict(ld_q=48), b"ld_q=48"), (dict(ld_g=56), b"ld_g=56"), (dict(ld_q=68), b"ld_q=68"), (dict(ld_g=76), b"ld_g=76"), (dict(q=A + 8), b"16-byte"),
                    (dict(g=A + 2), b"16-byte"), (dict(K=0), b"K=0"), (dict(K=129, N=500), b"K=129"), (dict(K=10, N=9), b"exceeds N=9"), (dict(N=2 ** 31), b"2^31"),
                    (dict(n_split=-1), b"n_split=-1"), (dict(n_split=1025), b"n_split=1025"), (dict(Q=-1), b"Q=-1"), (dict(q=None), b"null operand"),
                    (dict(g=None), b"null operand"), (dict(vals=None), b"null operand"), (dict(idx=None), b"null operand"), (dict(n_split=2), b"workspace"),
                    (dict(n_split=0, Q=1, N=10 ** 6), b"workspace")]:
        assert topk(**kw) != 0, kw
        err = L.sc_last_error()
        assert msg in err and NAME.encode() in err, (kw, err)
    assert topk(Q=0) == 0 and topk(Q=0, q=None, g=None, vals=None, idx=None) == 0           # the empty call is a no-op


def test_embedding_index_storage_argument():
    from speechclip_amd.module import EmbeddingIndex
    assert EmbeddingIndex(8).storage == "fp32" and EmbeddingIndex(32, storage="bf16").storage == "bf16"
    for dim in (8, 24, 100):
        with pytest.raises(ValueError, match="dim % 16"):
            EmbeddingIndex(dim, storage="bf16")
    for bad in ("fp16", "int8", "", None, torch.bfloat16):
        with pytest.raises(ValueError, match="storage"):
            EmbeddingIndex(32, storage=bad)
    with pytest.raises(ValueError, match="storage"):
        EmbeddingIndex(32, storage="bf16").astype("fp8")
    # the (empty) state of both storages without a GPU: the rows' type is the storage, and the key names it
    for storage, dt, bits in (("fp32", torch.float32, 32), ("bf16", torch.bfloat16, 16)):
        sd = EmbeddingIndex(32, storage=storage).state_dict()
        assert sd["storage"] == bits and sd["feats"].dtype == dt and sd["feats"].shape == (0, 32)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour WITHOUT a GPU")
def test_bf16_index_without_a_gpu_raises_instead_of_falling_back():
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.module import EmbeddingIndex
    index = EmbeddingIndex(16, storage="bf16")
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.add(torch.zeros(3, 16))
    with pytest.raises(SpeechClipHipError, match="no host fallback"):
        index.search(torch.zeros(1, 16), 1)
    with pytest.raises(SpeechClipHipError):
        index.astype("fp32").add(torch.zeros(3, 16))
    with pytest.raises(SpeechClipHipError):
        ops.search_topk_bf16(torch.zeros(1, 16, dtype=torch.bfloat16), torch.zeros(4, 16, dtype=torch.bfloat16), 1)


def test_bf16_rounding_is_to_nearest_even_and_equals_torchs():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 0.0, -0.0, 3.0e38, np.inf], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0, 3.0e38, np.inf], np.float32)
    want[7] = torch.tensor(3.0e38).to(torch.bfloat16).float().item()
    got = R.round_bf16(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(R.round_bf16(np.array([np.nan], np.float32))).all()
    y = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    t = torch.from_numpy(y).to(torch.bfloat16)
    assert np.array_equal(R.round_bf16(y), t.float().numpy())
    assert np.array_equal(R.bf16_bits(R.round_bf16(y)), t.view(torch.int16).numpy())


def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E))
    return R.round_bf16((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))


REAL_SHAPES = [(65, 1000, 64, 10), (7, 300, 16, 5), (9, 400, 512, 16)]
INT_SHAPE = (5, 300, 32, 12)


def int_case():
    """Small integers: heavy ties; gallery row 1 is planted as query 0's best match, so that no mutant can hide outside every top-K."""
    rng = np.random.default_rng(11)
    Q, N, E, K = INT_SHAPE
    q, g = rng.integers(-2, 3, (Q, E)).astype(np.float32), rng.integers(-1, 2, (N, E)).astype(np.float32)
    g[1] = np.sign(q[0])
    return q, g, K


def real_case(n):
    """Unit-norm rows rounded to bf16; gallery row 1 is query 0 itself."""
    Q, N, E, K = REAL_SHAPES[n]
    rng = np.random.default_rng(20 + n)
    q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
    g[1] = q[0]
    return q, g, K


def test_the_judges_accept_an_fp32_accumulated_stand_in():
    q, g, K = int_case()
    assert np.array_equal(R.round_bf16(q), q) and np.array_equal(R.round_bf16(g), g)           # small integers are bf16 numbers
    v, i = R.standin(q, g, K, idx_base=7)
    assert R.judge_exact(v, i, q, g, K, idx_base=7)
    top = -np.sort(-R.scores64(q, g), axis=1)[:, :K + 1]
    assert (np.diff(top, axis=1) == 0).any(1).all()                           # every query has tied scores among its first K + 1
    for n, (Q, N, E, _) in enumerate(REAL_SHAPES):
        q, g, K = real_case(n)
        v, i = R.standin(q, g, K)
        ok, worst = R.judge_real(v, i, q, g, K)
        print(f"stand-in at {(Q, N, E, K)}: worst error / bound = {worst:.4f}")
        assert ok and worst <= 0.5                           # a round-to-nearest chain sits far inside a bound made for a truncating adder
    assert R.c_of(512) == 1024 / (1 - 1024 * 2.0 ** -24) and R.bound(q, g).max() < 1e-3


@pytest.mark.parametrize("mutant", ["drop_last_group", "shift_row", "reverse_ties"])
def test_the_judges_reject_each_mutant(mutant):
    """drop_last_group and shift_row change scores: the exact arm and the bound both see them.  reverse_ties changes no score: only the exact arm, whose
    galleries are full of ties, sees it."""
    q, g, K = int_case()
    v, i = R.standin(q, g, K, idx_base=7, mutant=mutant)
    assert not R.judge_exact(v, i, q, g, K, idx_base=7)
    q, g, K = real_case(0)
    v, i = R.standin(q, g, K, mutant=mutant)
    ok, _ = R.judge_real(v, i, q, g, K)
    assert ok == (mutant == "reverse_ties")

"""CPU-only checks of the two-stage gallery search: the bound of tests/search_rerank_ref.py on operands built against it, the exactness of the stand-in of
the whole search, the mutants, the margins of the inputs whose flags the GPU tests assert, the host-side argument rules of EmbeddingIndex, and the ABI
entry with every refusal (refused before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import search_bf16_ref as B
import search_ref as SR
import search_rerank_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------- 1. the arithmetic of the statement
def test_the_fast_chain_is_the_rational_fmaf_chain_bit_for_bit():
    """fma32 / chain against search_ref.fmaf_chain (exact rationals) on mixed magnitudes, cancelling sums and subnormal results."""
    rng = np.random.default_rng(0)
    for E, scale in ((16, 1.0), (33, 1.0), (80, 2.0 ** -70), (12, 2.0 ** -66)):
        q = (rng.standard_normal((6, E)) * np.exp2(rng.integers(-10, 11, (6, E))) * scale).astype(np.float32)
        g = (rng.standard_normal((5, E)) * np.exp2(rng.integers(-10, 11, (5, E))) * scale).astype(np.float32)
        got = RR.chain_scores(q, g)
        want = SR.chain_scores(q, g)
        assert np.array_equal(bits(got), bits(want)), (E, scale)
    assert (np.abs(want) < 2.0 ** -126).any() and (want != 0).any()          # the last arm ends in subnormals
    # ties to even in the fp32 rounding, and the double-rounding trap: 1 + 2^-24 + 2^-60 must round UP, 1 + 2^-24 must stay
    one, h = np.float32(1.0), np.float32(2.0 ** -24)
    assert RR.fma32(np.array([h]), np.array([one]), np.array([one]))[0] == one
    assert RR.fma32(np.array([h]), np.array([np.float32(1 + 2.0 ** -20)]), np.array([one]))[0] == np.nextafter(one, np.float32(2))


def test_kappa_is_the_librarys_and_is_about_two_to_the_minus_seven():
    from speechclip_amd.module.retrieval import RERANK_INFLATE, rerank_kappa
    for E in (16, 64, 512, 1024):
        assert rerank_kappa(E) == RR.kappa(E)
        assert 2.0 ** -7 < RR.kappa(E) < 2.0 ** -7 * 1.05
    assert RERANK_INFLATE == RR.INFLATE


# ---------------------------------------------------------------------------------------- 2. the bound
def _gap(q, g):
    """|s~ - s| of every pair: the bf16 stand-in's score of the rounded rows against the fp32 chain of the stored rows."""
    qb, gb = B.round_bf16(q), B.round_bf16(g)
    st, order = B.standin(qb, gb, g.shape[0])                                # K = N: every score, descending, with its row
    s = RR.chain_scores(q, g)
    return np.abs(st.astype(np.float64) - np.take_along_axis(s, order, 1).astype(np.float64))


def test_the_bound_holds_and_is_nearly_reached_on_operands_built_against_it():
    worst = 0.0
    for name, q, g in RR.worst_case_operands():
        eps = RR.eps_of(q, RR.norms64(g).max()).astype(np.float64)
        gap = _gap(q, g)
        assert (gap <= eps[:, None]).all(), name
        worst = max(worst, float((gap / eps[:, None]).max()))
        # the two smaller constants are REFUTED by these operands, not merely unproven
        for mutant in ("eps_no_query", "eps_half_ulp"):
            assert (gap > RR.eps_of(q, RR.norms64(g).max(), mutant).astype(np.float64)[:, None]).all(), (name, mutant)
    print(f"worst |s~ - s| / eps = {worst:.4f}")
    assert worst >= 0.25                                                     # (observed 0.9946: a halved bound shows)
    rng = np.random.default_rng(1)
    for E in (16, 64, 512):                                                  # and on ordinary rows, where it is loose
        q, g = RR.unit_rows(rng, 8, E), RR.unit_rows(rng, 50, E) * np.float32(3.0)
        assert (_gap(q, g) <= RR.eps_of(q, RR.norms64(g).max()).astype(np.float64)[:, None]).all()


# ---------------------------------------------------------------------------------------- 3. the stand-in and the mutants
@pytest.fixture(scope="module")
def standin_cases():
    return [(name, q, g, K, R, RR.exact_topk(q, g, K)) for name, q, g, K, R in RR.standin_cases()]


@pytest.fixture(scope="module")
def kernel_cases():
    return [(c, RR.rescore(c["q"], c["g"], c["cand"], c["short_vals"], c["eps"], c["K"], c["idx_base"])) for c in RR.kernel_cases()]


def test_the_stand_in_of_the_two_stage_search_is_the_fp32_search_bit_for_bit(standin_cases):
    certified = {}
    for name, q, g, K, R, (wv, wi) in standin_cases:
        v, i, c = RR.two_stage(q, g, K, R)
        assert np.array_equal(bits(v), bits(wv)) and np.array_equal(i, wi), name
        certified[name] = c
    # the cases exercise both arms: proofs that carry the result, and fallbacks
    assert certified["random"].all() and not certified["near_duplicates"].any()
    half = len(certified["mixed"]) // 2
    assert not certified["mixed"][:half].any() and certified["mixed"][half:].all()
    assert certified["shorter_than_R"].all() and certified["equal_rows_R_eq_N"].all()


def test_the_statement_gives_the_flags_and_lists_known_beforehand(kernel_cases):
    seen = 0
    for c, (v, i, f) in kernel_cases:
        if "expect_cert" in c:
            assert np.array_equal(f, c["expect_cert"]) and np.array_equal(v, c["expect_vals"]) and np.array_equal(i, c["expect_idx"]), c["name"]
            seen += 1
        if c["name"] == "E16_R_eq_N40_holes":                                # R == N: certified exactly where no slot was emptied
            holes = np.arange(len(f)) % 3 == 0
            assert np.array_equal(f, (~holes).astype(np.int32))
        if c["name"] == "equal_rows_across_rank_K":
            assert i[0].tolist() == [10, 20] and v[0, 0] == v[0, 1]
    assert seen == 1


def test_every_mutant_is_caught_by_at_least_one_case(standin_cases, kernel_cases):
    caught = {m: [] for m in RR.MUTANTS}
    for m in RR.MUTANTS:
        if m.startswith("eps_"):                                             # a mutant of eps: the operands built against the bound refute it
            for name, q, g in RR.worst_case_operands():
                if (_gap(q, g) > RR.eps_of(q, RR.norms64(g).max(), m).astype(np.float64)[:, None]).any():
                    caught[m].append("bound:" + name)
            continue
        for c, (v, i, f) in kernel_cases:
            mv, mi, mf = RR.rescore(c["q"], c["g"], c["cand"], c["short_vals"], c["eps"], c["K"], c["idx_base"], mutant=m)
            if not (np.array_equal(bits(mv), bits(v)) and np.array_equal(mi, i) and np.array_equal(mf, f)):
                caught[m].append("kernel:" + c["name"])
        for name, q, g, K, R, (wv, wi) in standin_cases:
            mv, mi, _ = RR.two_stage(q, g, K, R, mutant=m)
            if not (np.array_equal(bits(mv), bits(wv)) and np.array_equal(mi, wi)):
                caught[m].append("search:" + name)
    print(caught)
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}
    assert "kernel:certificate_edge" in caught["cert_ge"] and "kernel:certificate_edge" in caught["cert_kth"]
    assert "kernel:E16_R_eq_N40_holes" in caught["full_rule_with_empty"]
    assert "kernel:equal_rows_across_rank_K" in caught["ties_desc"] and "search:equal_rows_R_eq_N" in caught["ties_desc"]
    assert any(c.startswith("search:") for c in caught["pairwise"])          # a wrong chain reaches the caller through a certified query


# ---------------------------------------------------------------------------------------- 4. the inputs whose flags the GPU tests assert
@pytest.mark.parametrize("name", ["a1", "a2", "b", "c"])
def test_asserted_flags_lie_ten_accumulation_bounds_from_the_edge(name):
    """The end-to-end GPU tests assert flags on these galleries.  The first stage's scores on the device may differ from the stand-in's by the bf16
    entry's accumulation bound (another order of the additions), so every asserted flag must lie at least ten such bounds from the certificate's edge; and
    the restatement alone must give the asserted pattern."""
    q, g, K, R = {"a1": (*RR.gallery_a(4096, 64), 4, 32), "a2": (*RR.gallery_a(2048, 128, seed=3), 10, 128), "b": (*RR.gallery_b(), 5, 40),
                  "c": (*RR.gallery_c(), RR.C_K, RR.C_R)}[name]
    qb, gb = B.round_bf16(q), B.round_bf16(g)
    sv, si = B.standin(qb, gb, R)
    eps = RR.eps_of(q, RR.norms64(g).max())
    vals, idx, cert = RR.rescore(q, g, si, sv, eps, K)
    edge = vals[:, K - 1].astype(np.float64) - (sv[:, R - 1].astype(np.float64) + eps.astype(np.float64))
    margin = np.abs(edge) / B.bound(qb, gb).max(1)
    print(f"{name}: certified {cert.mean():.3f}, smallest margin {margin.min():.1f} accumulation bounds")
    assert margin.min() >= 10.0
    half = len(cert) // 2
    if name in ("a1", "a2"):
        assert cert.all()
    elif name == "b":
        assert not cert.any()
        fv, fi = RR.exact_topk(q, g, K)
        assert (si[:, :K] != fi).any(1).all()                               # the bf16-only top-K is wrong on every query
    else:
        assert not cert[:half].any() and cert[half:].all()


# ---------------------------------------------------------------------------------------- 5. host-side argument rules of EmbeddingIndex
def test_index_argument_rules_and_state_dict_keys():
    from speechclip_amd.module.retrieval import EmbeddingIndex
    with pytest.raises(ValueError, match="shadow=True needs"):
        EmbeddingIndex(64, storage="bf16", shadow=True)
    with pytest.raises(ValueError, match="shadow=True needs"):
        EmbeddingIndex(40, shadow=True)
    plain, shadowed = EmbeddingIndex(64), EmbeddingIndex(64, shadow=True)
    keys = ["dim", "normalize", "storage", "feats", "segment_rows", "ids"]
    assert list(plain.state_dict()) == keys and list(shadowed.state_dict()) == keys + ["shadow"] and shadowed.state_dict()["shadow"] is True
    assert list(EmbeddingIndex(64, storage="bf16").state_dict()) == keys
    q = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="needs an index with shadow rows"):
        plain.search(q, 3, rerank=8)
    with pytest.raises(ValueError, match="distinct=True is not supported"):
        shadowed.search(q, 3, distinct=True, rerank=8)
    for R in (2, 129):
        with pytest.raises(ValueError, match=f"rerank={R} must be in"):
            shadowed.search(q, 3, rerank=R)
    with pytest.raises(ValueError, match="return_certified=True needs rerank"):
        plain.search(q, 3, return_certified=True)
    with pytest.raises(ValueError, match="shadow=True needs"):
        EmbeddingIndex(64, storage="bf16").with_shadow()


def test_model_entry_points_pass_both_options_through():
    import inspect
    from speechclip_amd.model.kwClip import KWClipBase
    assert inspect.signature(KWClipBase.build_index).parameters["shadow"].default is False
    assert inspect.signature(KWClipBase.search).parameters["rerank"].default is None


# ---------------------------------------------------------------------------------------- 6. the ABI entry and its refusals
def test_entry_is_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib, ops
    L = _lib.lib()
    n = "sc_search_rescore"
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    assert n in _lib.exported_symbols() and hasattr(L, n)
    params = re.search(rf"^int {n}\s*\(([^)]*)\)", text, re.M).group(1)
    assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]) == 17
    assert getattr(L, n).restype is ctypes.c_int
    src = open(os.path.join(ROOT, "speechclip_amd", "csrc", "search_rescore.hip")).read()
    assert re.findall(r'extern "C"\s+\w+\s+(\w+)\s*\(', src) == [n]
    assert "atomic" not in src.replace("No atomics", "") and "asm" not in src
    assert callable(ops.search_rescore)


def test_every_refusal_is_refused_before_any_launch_and_names_the_value():
    from speechclip_amd._lib import lib
    L = lib()
    A = 1 << 20                                                               # an aligned non-null address that is never dereferenced: every call below is refused

    def call(ld_q=64, ld_g=64, Q=4, N=100, E=64, R=16, K=10, q_off=0, g_off=0, null=None):
        p = {name: (None if null == name else A) for name in ("q", "g", "cand", "short", "eps", "vals", "idx", "cert")}
        return L.sc_search_rescore(p["q"] and p["q"] + q_off, ld_q, p["g"] and p["g"] + g_off, ld_g, Q, N, E, p["cand"], p["short"], R, p["eps"], K, 0, p["vals"],
                                   p["idx"], p["cert"], None)
    for kw, msg in RR.refusals():
        assert call(**kw) != 0, kw
        assert msg in L.sc_last_error(), (kw, L.sc_last_error())
    assert call(Q=0) == 0 and call(Q=0, null="q") == 0                       # the empty call launches nothing and reads nothing

"""sc_search_rescore on the device against its host statement (tests/search_rerank_ref.py): every query of every case is judged, certified or not.  Every
call runs GUARDED: q and g lie between NaN rows with NaN in the gap behind column E, the shortlist between rows that name nothing, and the outputs between
sentinels that must survive."""
import numpy as np
import pytest
import torch

import search_rerank_ref as RR

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_rows(a, ld):
    buf = torch.full((a.shape[0] + 2, ld), float("nan"), device="cuda")
    buf[1:-1, :a.shape[1]] = dev(a)
    return buf


def run(q, g, cand, short_vals, eps, K, idx_base=0, ld_g=None, ld_q=None):
    """The raw entry between guards -> (vals, idx, certified) as numpy."""
    from speechclip_amd._lib import lib, stream
    L = lib()
    (Q, E), N, R = q.shape, g.shape[0], cand.shape[1]
    ld_q, ld_g = ld_q or E + 4, ld_g or E
    qb, gb = guarded_rows(q, ld_q), guarded_rows(g, ld_g)
    cb = torch.full((Q + 2, R), 2 ** 40, device="cuda", dtype=torch.int64)
    cb[1:-1] = dev(cand)
    sb = torch.full((Q + 2, R), float("nan"), device="cuda")
    sb[1:-1] = dev(short_vals)
    eb = torch.full((Q + 32,), float("nan"), device="cuda")
    eb[16:-16] = dev(eps)
    vals = torch.full((Q * K + 32,), 12345.0, device="cuda")
    idx = torch.full((Q * K + 32,), -777, device="cuda", dtype=torch.int64)
    cert = torch.full((Q + 32,), -777, device="cuda", dtype=torch.int32)
    rc = L.sc_search_rescore(qb[1:].data_ptr(), ld_q, gb[1:].data_ptr(), ld_g, Q, N, E, cb[1:].data_ptr(), sb[1:].data_ptr(), R, eb[16:].data_ptr(), K, idx_base,
                             vals[16:].data_ptr(), idx[16:].data_ptr(), cert[16:].data_ptr(), stream())
    assert rc == 0, L.sc_last_error()
    torch.cuda.synchronize()
    assert (vals[:16] == 12345.0).all() and (vals[-16:] == 12345.0).all() and (idx[:16] == -777).all() and (idx[-16:] == -777).all()
    assert (cert[:16] == -777).all() and (cert[-16:] == -777).all()
    return vals[16:-16].cpu().numpy().reshape(Q, K), idx[16:-16].cpu().numpy().reshape(Q, K), cert[16:-16].cpu().numpy()


CASES = {c["name"]: c for c in RR.kernel_cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_and_flags_equal_the_host_statement(name):
    c = CASES[name]
    want_v, want_i, want_c = RR.rescore(c["q"], c["g"], c["cand"], c["short_vals"], c["eps"], c["K"], c["idx_base"])
    v, i, f = run(c["q"], c["g"], c["cand"], c["short_vals"], c["eps"], c["K"], c["idx_base"], ld_g=c["ld_g"])
    print(f"{name}: certified {f.mean():.3f} of {len(f)} queries")
    assert np.array_equal(i, want_i) and np.array_equal(bits(v), bits(want_v)) and np.array_equal(f, want_c)
    if "expect_cert" in c:                                                    # the certificate's edge: eps = 4 -> 0, the float just below 4 -> 1
        assert np.array_equal(f, c["expect_cert"]) and np.array_equal(v, c["expect_vals"]) and np.array_equal(i, c["expect_idx"])


@pytest.mark.parametrize("E,scale", [(16, 1.0), (80, 1.0), (528, 1.0), (16, 2.0 ** -68)])
def test_scores_equal_search_topks_on_the_same_pairs_bit_for_bit(E, scale):
    """Mixed magnitudes (2^-10 .. 2^10, both signs); the last arm scales the rows so that the scores are subnormal.  N = 128 = K = R: both entries return
    every pair, so the whole outputs must agree; then N = 3000, where the shortlist is sc_search_topk's own first 128, shuffled."""
    from speechclip_amd import ops
    rng = np.random.default_rng(30 + E)
    for N in (128, 3000):
        q = (rng.standard_normal((65, E)) * np.exp2(rng.integers(-10, 11, (65, E))) * scale).astype(np.float32)
        g = (rng.standard_normal((N, E)) * np.exp2(rng.integers(-10, 11, (N, E))) * scale).astype(np.float32)
        tv, ti = ops.search_topk(dev(q), dev(g), 128)
        tv, ti = tv.cpu().numpy(), ti.cpu().numpy()
        perm = np.stack([rng.permutation(128) for _ in range(65)])
        cand = np.take_along_axis(ti, perm, 1)
        v, i, f = run(q, g, cand, np.zeros((65, 128), np.float32), np.zeros(65, np.float32), 128)
        assert np.array_equal(i, ti) and np.array_equal(bits(v), bits(tv)), (E, N)
        if scale != 1.0 and N == 128:                                         # (every pair is returned: the small scores are among them)
            assert (np.abs(tv) < 2.0 ** -126).any() and (tv != 0).any()       # subnormal scores, kept
        assert f.all() if N == 128 else True                                  # R == N: certified whatever eps says


def test_nan_scores_take_no_part_and_missing_slots_are_empty():
    rng = np.random.default_rng(40)
    q, g = RR.unit_rows(rng, 3, 16), RR.unit_rows(rng, 50, 16)
    g[[4, 7]] = np.nan                                                        # NaN gallery rows that ARE on the shortlist: scored, never returned
    cand = np.tile(np.array([4, 9, 7, 11, 2, -1, 60, 13], np.int64), (3, 1))
    cand[2] = [-1, 4, -1, 7, -1, 99, -1, -1]                                  # nothing comparable at all
    sv = np.zeros((3, 8), np.float32)
    sv[1, 7] = np.nan                                                         # a NaN at short_vals[R-1]: never certified
    eps = np.zeros(3, np.float32)
    want = RR.rescore(q, g, cand, sv, eps, 6)
    v, i, f = run(q, g, cand, sv, eps, 6)
    assert np.array_equal(i, want[1]) and np.array_equal(bits(v), bits(want[0])) and np.array_equal(f, want[2])
    assert (i[0, 4:] == -1).all() and np.isneginf(v[0, 4:]).all() and sorted(i[0, :4].tolist()) == [2, 9, 11, 13]
    assert (i[2] == -1).all() and np.isneginf(v[2]).all() and not f.any()


def test_a_rows_result_does_not_depend_on_the_call_around_it():
    c = CASES["E80_R33_Q65_holes_base_ld"]
    whole = run(c["q"], c["g"], c["cand"], c["short_vals"], c["eps"], c["K"], c["idx_base"], ld_g=c["ld_g"])
    for rows in ([64], [3, 0, 40]):
        part = run(c["q"][rows], c["g"], c["cand"][rows], c["short_vals"][rows], c["eps"][rows], c["K"], c["idx_base"], ld_g=c["ld_g"], ld_q=c["q"].shape[1])
        for a, b in zip(part, whole):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b[rows].view(np.uint32) if b.dtype == np.float32 else b[rows])


def test_every_refusal_and_the_empty_call_on_device_operands():
    from speechclip_amd import ops
    from speechclip_amd._lib import lib, stream
    L = lib()
    t = {"q": torch.zeros(4, 1028 + 8, device="cuda"), "g": torch.zeros(100, 1028 + 8, device="cuda"), "cand": torch.zeros(4, 129, device="cuda", dtype=torch.int64),
         "short": torch.zeros(4, 129, device="cuda"), "eps": torch.zeros(4, device="cuda"), "vals": torch.full((4, 129), 12345.0, device="cuda"),
         "idx": torch.full((4, 129), -777, device="cuda", dtype=torch.int64), "cert": torch.full((4,), -777, device="cuda", dtype=torch.int32)}

    def call(ld_q=64, ld_g=64, Q=4, N=100, E=64, R=16, K=10, q_off=0, g_off=0, null=None):
        p = {name: (None if null == name else x.data_ptr()) for name, x in t.items()}
        return L.sc_search_rescore(p["q"] and p["q"] + q_off, ld_q, p["g"] and p["g"] + g_off, ld_g, Q, N, E, p["cand"], p["short"], R, p["eps"], K, 0, p["vals"],
                                   p["idx"], p["cert"], stream())
    for kw, msg in RR.refusals():
        assert call(**kw) != 0, kw
        assert msg in L.sc_last_error(), (kw, L.sc_last_error())
    assert call(Q=0) == 0
    torch.cuda.synchronize()
    assert (t["vals"] == 12345.0).all() and (t["idx"] == -777).all() and (t["cert"] == -777).all()      # nothing was launched, nothing written
    v, i, f = ops.search_rescore(t["q"][:0, :64], t["g"][:, :64], t["cand"][:0, :16].contiguous(), t["short"][:0, :16].contiguous(), t["eps"][:0], 10)
    assert v.shape == (0, 10) and i.shape == (0, 10) and f.shape == (0,)

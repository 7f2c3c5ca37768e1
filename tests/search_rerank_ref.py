"""Host statements of the two-stage gallery search (include/speechclip_hip.h, "Gallery search, fp32 re-score of a shortlist"; EmbeddingIndex.search with
rerank=R), shared by tests/test_search_rerank_host.py, tests/test_search_rescore_gpu.py and tests/test_search_rerank_gpu.py: the statement of
sc_search_rescore, kappa and eps with their derivation, a stand-in of the whole two-stage search built on search_bf16_ref.standin, the case lists, the
galleries of the end-to-end tests, and the mutants that the cases must catch.  The chain is search_ref.fmaf_chain's, the order search_ref.order's.

THE BOUND.  q, g are the stored fp32 rows, q~ = bf16(q), g~ = bf16(g) (round to nearest even), s~ the bf16 entry's score of (q~, g~) and s the fp32 fmaf chain
of (q, g).  With q~.g~ and q.g the exact sums,
    |s~ - s| <= |s~ - q~.g~| + |q~.g~ - q.g| + |q.g - s|.
  (1) |s~ - q~.g~| <= c 2^-24 sum_e |q~_e g~_e|,  c = 2E / (1 - 2E 2^-24): the bf16 entry's contract (search_bf16_ref).
  (2) bf16 keeps 8 significand bits, so its unit roundoff is 2^-8: |q~_e - q_e| <= 2^-8 |q_e| for every normal q_e, the same for g, hence
      |q~_e g~_e - q_e g_e| <= ((1 + 2^-8)^2 - 1) |q_e g_e| = (2^-7 + 2^-16) |q_e g_e|.   (A unit roundoff of 2^-9 -- a 9-bit significand -- would halve this
      term; it is not what the format has: 1 + 2^-8 - 2^-23 rounds to 1, a relative error of 2^-8 / (1 + 2^-8).  worst_case_operands() reaches 0.99 of the
      bound below, so the halved constant is refuted, not merely not proven: mutant "eps_half_ulp".)
  (3) |q.g - s| <= gamma_E sum_e |q_e g_e|,  gamma_E = E 2^-24 / (1 - E 2^-24): recursive summation with fused products (search_ref.bound).
  In (1), sum |q~ g~| <= (1 + 2^-8)^2 sum |q g|; and sum_e |q_e g_e| <= ||q|| ||g|| (Cauchy-Schwarz).  Together
    |s~ - s| <= kappa(E) ||q||_2 ||g||_2,   kappa(E) = (2^-7 + 2^-16) + c 2^-24 (1 + 2^-8)^2 + gamma_E          (about 2^-7).
  eps_i = kappa(E) ||q_i|| G with G >= every stored row's norm.  The norms are computed in fp64 (relative error below E 2^-53 each), the product has three
  fp64 roundings, eps is rounded to fp32 (2^-24) and the kernel's fp64 sum short + eps rounds once more: all of it is covered by ONE factor 1 + 2^-22.
SOUNDNESS.  A row outside the shortlist has s~ <= short_vals[R-1] (the first stage's order), hence s <= short_vals[R-1] + eps < vals[K-1] when the certificate
holds: it comes strictly after the K-th returned row, so the first K of the shortlist under the exact order are the first K of the gallery, ties included.
Non-finite and subnormal operands are outside the certificate's contract, as they are outside the bf16 entry's."""
import numpy as np

import search_bf16_ref as B
import search_ref as SR

U = 2.0 ** -24                      # unit roundoff of fp32
UB = 2.0 ** -8                      # unit roundoff of bf16 (8 significand bits)
INFLATE = 1.0 + 2.0 ** -22

MUTANTS = ("cert_ge", "cert_kth", "eps_no_query", "eps_half_ulp", "pairwise", "ties_desc", "full_rule_with_empty")


def kappa(E, mutant=None):
    mid = 2.0 * UB + UB * UB
    if mutant == "eps_no_query":        # only the gallery rows counted as rounded
        mid = UB
    if mutant == "eps_half_ulp":        # a unit roundoff of 2^-9
        mid = 2.0 ** -8 + 2.0 ** -18
    return mid + B.c_of(E) * U * (1.0 + UB) ** 2 + SR.gamma(E)


def norms64(x):
    return np.sqrt((x.astype(np.float64) ** 2).sum(1))


def eps_of(q, G, mutant=None):
    """f32 [Q]: kappa(E) ||q_i|| G, inflated once."""
    return (kappa(q.shape[1], mutant) * norms64(q) * float(G) * INFLATE).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the chain, fast and exact
def fma32(a, b, c):
    """fmaf on fp32 arrays, exactly: the product of two fp32 numbers is exact in fp64; the fp64 sum is turned into a round-to-odd sum with the exact error of
    TwoSum, and rounding a round-to-odd fp64 number to fp32 (53 >= 24 + 2 bits) equals rounding the exact sum once, subnormals included.
    test_search_rerank_host.py holds it against search_ref.fmaf_chain (rational arithmetic)."""
    a, b, c = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def chain(q, g):
    """search_ref.fmaf_chain over the last axis of two broadcastable fp32 arrays: acc = +0; for e ascending: acc = fmaf(q[e], g[e], acc)."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    acc = np.zeros(np.broadcast_shapes(q.shape[:-1], g.shape[:-1]), np.float32)
    for e in range(q.shape[-1]):
        acc = fma32(q[..., e], g[..., e], acc)
    return acc


def pairwise(q, g):
    """MUTANT arithmetic: fp32 products summed pairwise."""
    p = (np.asarray(q, np.float32) * np.asarray(g, np.float32)).astype(np.float32)
    while p.shape[-1] > 1:
        if p.shape[-1] % 2:
            p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float32)], -1)
        p = (p[..., 0::2] + p[..., 1::2]).astype(np.float32)
    return p[..., 0]


def chain_scores(q, g):
    """f32 [Q, N]: the fp32 entry's score of every pair."""
    return chain(q[:, None, :], g[None, :, :])


def exact_topk(q, g, K, idx_base=0):
    """What sc_search_topk returns: the first K by (chain score descending, j ascending)."""
    return SR.topk(chain_scores(q, g), K, idx_base)


# ------------------------------------------------------------------------------------------------------------ sc_search_rescore
def rescore(q, g, cand, short_vals, eps, K, idx_base=0, mutant=None):
    """The host statement of sc_search_rescore -> (vals f32 [Q, K], idx i64 [Q, K], certified i32 [Q]).  g holds exactly the N rows [0, N)."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    cand, short_vals, eps = np.asarray(cand, np.int64), np.asarray(short_vals, np.float32), np.asarray(eps, np.float32)
    (Q, R), N = cand.shape, g.shape[0]
    off = cand - idx_base
    ok = (cand != -1) & (off >= 0) & (off < N)
    rows = g[np.where(ok, off, 0)]                                            # [Q, R, E]; slots that name no row are masked below, never scored
    s = (pairwise if mutant == "pairwise" else chain)(q[:, None, :], rows)
    vals = np.full((Q, K), -np.inf, np.float32)
    idx = np.full((Q, K), -1, np.int64)
    cert = np.zeros(Q, np.int32)
    for i in range(Q):
        js = off[i, ok[i]]
        by_j = np.argsort(-js if mutant == "ties_desc" else js, kind="stable")   # order() breaks ties by position: lay the slots out by j
        js, si = js[by_j], s[i, ok[i]][by_j]
        o = SR.order(si)[:K]
        vals[i, :len(o)] = si[o]
        idx[i, :len(o)] = js[o] + idx_base
        last = short_vals[i, R - 1]
        ref = short_vals[i, K - 1] if mutant == "cert_kth" else last
        lhs, rhs = np.float64(vals[i, K - 1]), np.float64(ref) + np.float64(eps[i])
        proven = R == N or (lhs >= rhs if mutant == "cert_ge" else lhs > rhs)
        full = bool(ok[i].all()) or (mutant == "full_rule_with_empty" and R == N)
        cert[i] = 1 if full and not np.isnan(last) and proven else 0
    return vals, idx, cert


# ------------------------------------------------------------------------------------------------------------ the whole two-stage search
def two_stage(q, g, K, R, mutant=None):
    """Stand-in of EmbeddingIndex.search(q, K, rerank=R) on one segment -> (vals, idx, certified): search_bf16_ref.standin on the rounded rows shortlists
    min(R, N) rows, rescore() on the stored rows, and the queries without the proof take the fp32 entry's result."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    rr = min(R, g.shape[0])
    sv, si = B.standin(B.round_bf16(q), B.round_bf16(g), rr)
    eps = eps_of(q, norms64(g).max(), mutant)
    vals, idx, cert = rescore(q, g, si, sv, eps, K, mutant=mutant)
    fv, fi = exact_topk(q, g, K)
    redo = cert == 0
    vals[redo], idx[redo] = fv[redo], fi[redo]
    return vals, idx, cert


def margins(q, g, K, R):
    """Per query: |vals[K-1] - (short_vals[R-1] + eps)| in units of the bf16 entry's accumulation bound of that query's worst pair (the first stage's score
    on the device may differ from the stand-in's by up to two such bounds, a device normalisation by far less).  inf where R >= N (no edge)."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    if R >= g.shape[0]:
        return np.full(q.shape[0], np.inf)
    qb, gb = B.round_bf16(q), B.round_bf16(g)
    sv, si = B.standin(qb, gb, R)
    eps = eps_of(q, norms64(g).max())
    vals, _, _ = rescore(q, g, si, sv, eps, K)
    edge = vals[:, K - 1].astype(np.float64) - (sv[:, R - 1].astype(np.float64) + eps.astype(np.float64))
    return np.abs(edge) / B.bound(qb, gb).max(1)


# ------------------------------------------------------------------------------------------------------------ operands for the bound
def worst_case_operands(E=64):
    """(name, q [1, E], g [1, E]) built so that every element rounds the same way by almost half a bf16 ulp, q parallel to g (Cauchy-Schwarz tight) and every
    product positive: all three terms of the bound push the same way."""
    down = np.float32(1.0 + 2.0 ** -8 - 2.0 ** -23)          # just below the midpoint of 1 and 1 + 2^-7: rounds DOWN to 1
    up = np.float32(1.0 + 2.0 ** -8 + 2.0 ** -23)            # just above it: rounds UP to 1 + 2^-7
    sign = np.where(np.arange(E) % 3 == 0, -1.0, 1.0).astype(np.float32)
    out = []
    for name, m in (("down", down), ("up", up)):
        out.append((name, np.full((1, E), m, np.float32), np.full((1, E), m, np.float32)))
        out.append((name + "_signed_scaled", (sign * m * np.float32(0.25))[None], (sign * m * np.float32(8.0))[None]))
    return out


# ------------------------------------------------------------------------------------------------------------ galleries of the end-to-end tests
def unit_rows(rng, n, E):
    x = rng.standard_normal((n, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def gallery_a(N, E, Q=64, seed=0):
    """(a) random unit rows and queries: wide gaps, every query certified."""
    rng = np.random.default_rng(seed)
    return unit_rows(rng, Q, E), unit_rows(rng, N, E)


def gallery_b(N=1000, E=32, Q=16, seed=1):
    """(b) near-duplicates: every row is base + 1e-4 noise; bf16 cannot tell them apart, and no query is certified."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((1, E))
    base /= np.linalg.norm(base)
    return unit_rows(rng, Q, E), _unit(base + 1e-4 * rng.standard_normal((N, E)))


def gallery_c(N=1024, E=32, dups=128, Q=16, seed=2):
    """(c) mixed: `dups` near-duplicates of one vector v scattered among random rows; the first half of the queries are near v (uncertified: more
    near-duplicates than any shortlist holds), the second half have v's direction projected out (certified)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((1, E))
    v /= np.linalg.norm(v)
    g = rng.standard_normal((N, E))
    at = rng.permutation(N)[:dups]
    g[at] = v + 1e-4 * rng.standard_normal((dups, E))
    near = v + 1e-4 * rng.standard_normal((Q // 2, E))
    far = rng.standard_normal((Q - Q // 2, E))
    far -= (far @ v.T) * v
    return _unit(np.concatenate([near, far], 0)), _unit(g)


C_K, C_R = 5, 64                    # gallery (c) is searched with these


# ------------------------------------------------------------------------------------------------------------ case lists
def standin_cases():
    """(name, q, g, K, R) for the stand-in of the whole search: the three galleries at small sizes, a gallery shorter than R, exact duplicates with R == N."""
    rng = np.random.default_rng(10)
    out = []
    q, g = gallery_a(300, 32, Q=8, seed=11)
    out.append(("random", q, g, 4, 32))
    q, g = gallery_b(200, 32, Q=6, seed=12)
    out.append(("near_duplicates", q, g, 5, 40))
    q, g = gallery_c(256, 32, dups=64, Q=8, seed=13)
    out.append(("mixed", q, g, 5, 32))
    q, g = gallery_a(20, 16, Q=4, seed=14)
    out.append(("shorter_than_R", q, g, 3, 32))
    g = unit_rows(rng, 24, 16)
    g[[5, 9, 17]] = g[2]                                      # four equal rows: with K = 2 the tie straddles rank K
    out.append(("equal_rows_R_eq_N", np.concatenate([g[2:3], unit_rows(rng, 3, 16)], 0), g, 2, 24))
    return out


def _shortlist(q, g, R):
    sv, si = B.standin(B.round_bf16(q), B.round_bf16(g), R)
    return si, sv, eps_of(q, norms64(g).max())


def kernel_cases():
    """Inputs of sc_search_rescore: dicts with q, g, cand, short_vals, eps, K, idx_base, ld_g and, where the flags are known beforehand, expect_cert.
    Together: E in {16, 80, 528}; R in {K, 33, 64, 65, 128} and K = R = 128; R == N = 40; Q in {1, 65}; ld_g > E; idx_base != 0; -1 slots and slots out of
    range; exactly equal rows on both sides of rank K; the certificate's edge hit exactly."""
    rng = np.random.default_rng(20)
    out = []

    def case(name, Q, N, E, K, R, idx_base=0, ld_g=None, holes=False):
        q, g = unit_rows(rng, Q, E), unit_rows(rng, N, E)
        cand, sv, eps = _shortlist(q, g, R)
        cand = cand + idx_base
        if holes:                                             # every third query: an empty slot, one below the range, one above it
            for i in range(0, Q, 3):
                cand[i, rng.integers(R)] = -1
                cand[i, rng.integers(R)] = idx_base - 1 - int(rng.integers(5)) if idx_base else -1
                cand[i, rng.integers(R)] = idx_base + N + int(rng.integers(5))
        out.append(dict(name=name, q=q, g=g, cand=cand, short_vals=sv, eps=eps, K=K, idx_base=idx_base, ld_g=ld_g or E))

    case("E16_R_eq_K_Q1", 1, 300, 16, 5, 5)
    case("E80_R33_Q65_holes_base_ld", 65, 500, 80, 7, 33, idx_base=1000, ld_g=96, holes=True)
    case("E528_R64_Q65", 65, 400, 528, 10, 64)
    case("E80_R65_Q1", 1, 300, 80, 10, 65)
    case("E528_K128_R128", 3, 300, 528, 128, 128, idx_base=7)
    case("E16_R_eq_N40_holes", 65, 40, 16, 4, 40, holes=True)
    # exactly equal rows on both sides of rank K: rows 10, 20, 30, 40 are the query itself; K = 2 keeps 10 and 20
    q = unit_rows(rng, 2, 16)
    g = unit_rows(rng, 64, 16)
    g[[10, 20, 30, 40]] = q[0]
    cand, sv, eps = _shortlist(q, g, 33)
    out.append(dict(name="equal_rows_across_rank_K", q=q, g=g, cand=cand[:, ::-1].copy(), short_vals=sv, eps=eps, K=2, idx_base=0, ld_g=16))
    # the certificate's edge on small integers: scores 12, 10, 7, 6 -> vals[K-1] = 10, short_vals[R-1] = 6
    q = np.zeros((3, 16), np.float32)
    q[:, 0] = 1.0
    g = np.zeros((8, 16), np.float32)
    g[:, 0] = [3, 12, 5, 10, 7, 1, 6, 2]
    g[:, 1:] = rng.integers(-3, 4, (8, 15))
    cand = np.tile(np.array([1, 3, 4, 6], np.int64), (3, 1))
    sv = np.tile(np.array([12, 10, 7, 6], np.float32), (3, 1))
    eps = np.array([4.0, np.nextafter(np.float32(4.0), np.float32(0.0)), 3.0], np.float32)
    out.append(dict(name="certificate_edge", q=q, g=g, cand=cand, short_vals=sv, eps=eps, K=2, idx_base=0, ld_g=16, expect_cert=np.array([0, 1, 1], np.int32),
                    expect_vals=np.tile(np.array([12, 10], np.float32), (3, 1)), expect_idx=np.tile(np.array([1, 3], np.int64), (3, 1))))
    return out


def refusals():
    """(keyword overrides of a valid call, what sc_last_error must name): every refusal of the contract."""
    return [(dict(E=6, ld_q=8, ld_g=8), b"E=6"), (dict(E=0), b"E=0"), (dict(E=1028, ld_q=1028, ld_g=1028), b"E=1028"), (dict(ld_q=60), b"ld_q=60"),
            (dict(ld_g=60), b"ld_g=60"), (dict(ld_q=66), b"ld_q=66"), (dict(ld_g=70), b"ld_g=70"), (dict(q_off=4), b"16-byte aligned"),
            (dict(g_off=8), b"16-byte aligned"), (dict(K=0), b"K=0"), (dict(K=129, R=129), b"K=129"), (dict(K=10, R=9), b"R=9"), (dict(R=129), b"R=129"),
            (dict(N=0), b"N=0"), (dict(N=2 ** 31), b"N=2147483648"), (dict(Q=-1), b"Q=-1")] + \
           [(dict(null=name), b"null operand") for name in ("q", "g", "cand", "short", "eps", "vals", "idx", "cert")]

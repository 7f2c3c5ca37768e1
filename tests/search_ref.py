"""Host statements of the gallery-search contract (include/speechclip_hip.h, "Gallery search"), shared by tests/test_search_gpu.py and
tests/test_search_host.py: the fp64 score matrix, the stable order, the per-pair rounding bound and an EXACT restatement of the fp32 fmaf chain."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32


def gamma(E):
    """Higham's gamma_E for a chain of E roundings (the products are fused, so one rounding per step)."""
    return E * U / (1.0 - E * U)


def scores64(q, g):
    return q.astype(np.float64) @ g.astype(np.float64).T


def bound(q, g):
    """b[i, j] = gamma_E * sum_e |q[i, e] g[j, e]|: |fmaf chain - exact sum| <= b (standard forward error of recursive summation with fused products)."""
    return gamma(q.shape[1]) * (np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T)


def order(row):
    """Positions of `row` in (score descending, position ascending) order, NaN entries left out."""
    j = np.flatnonzero(~np.isnan(row))
    s = row[j]
    return j[np.lexsort((j, -s))]


def topk(score, k, idx_base=0):
    """(vals f32 [Q, k], idx i64 [Q, k]) of a score matrix given in the precision it is to be compared in; short rows end in -inf / -1."""
    Q = score.shape[0]
    vals = np.full((Q, k), -np.inf, np.float32)
    idx = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        o = order(score[i])[:k]
        vals[i, :len(o)] = score[i, o]
        idx[i, :len(o)] = o + idx_base
    return vals, idx


def merge(vals, idx, k):
    """sc_topk_merge on the host: the first k pairs by (value descending, idx ascending); idx < 0 and NaN take no part."""
    Q = vals.shape[0]
    ov = np.full((Q, k), -np.inf, np.float32)
    oi = np.full((Q, k), -1, np.int64)
    for i in range(Q):
        keep = np.flatnonzero((idx[i] >= 0) & ~np.isnan(vals[i]))
        o = keep[np.lexsort((idx[i, keep], -vals[i, keep].astype(np.float64)))][:k]
        ov[i, :len(o)] = vals[i, o]
        oi[i, :len(o)] = idx[i, o]
    return ov, oi


def round_f32(x):
    """The fp32 number nearest to the rational x, ties to even, subnormals included (no overflow handling: the tests stay far from it)."""
    if x == 0:
        return np.float32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                   # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, quantum)
    n = int(n)
    if 2 * rem > quantum or (2 * rem == quantum and n % 2 == 1):
        n += 1
    y = np.float32(float(n * quantum))           # n * quantum has at most 24 significant bits: exact in a double, exact in fp32
    return -y if x < 0 else y


def fmaf_chain(q, g):
    """acc = +0; for e ascending: acc = round_f32(q[e] * g[e] + acc) with the product and the sum EXACT (rationals): what fmaf computes, per step."""
    acc = Fraction(0)
    for a, b in zip(q.tolist(), g.tolist()):     # float32 -> Python float is exact
        acc = Fraction(float(round_f32(Fraction(a) * Fraction(b) + acc)))
    return np.float32(float(acc))


def chain_scores(q, g):
    return np.array([[fmaf_chain(qi, gj) for gj in g] for qi in q], np.float32)


def search_splits(Q, N, K):
    """Python restatement of sc_search_splits."""
    if Q <= 0 or N <= 0 or K <= 0:
        return 1
    bq = 128 if (K <= 64 and Q > 64) else 64
    qtiles = -(-Q // bq)
    return max(1, min(-(-512 // qtiles), N // 256, 1024))


def workspace_bytes(Q, N, K, n_split):
    S = n_split if n_split else search_splits(Q, N, K)
    return 0 if S <= 1 else Q * S * K * 12

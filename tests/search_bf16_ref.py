"""Host statements of the bf16 gallery-search contract (include/speechclip_hip.h, "Gallery search, bf16 storage"), shared by tests/test_search_bf16_gpu.py
and tests/test_search_bf16_host.py: bf16 rounding, the fp64 score of the rounded operands, the accumulation bound with its derivation, and the two judges
(exact integers, real inputs) that the device result -- and, on the host, a stand-in and three mutants of it -- are put before.  Order, top-K and merge are
those of tests/search_ref.py.

THE BOUND.  q and g hold bf16 numbers (8 significand bits), so every product q[i, e] g[j, e] has at most 16 significand bits and is exact in fp32; the only
errors are those of the additions.  One v_mfma_f32_32x32x16_bf16 adds 16 products to the accumulator: 17 operands, 16 additions, in an order the hardware
does not state.  A row of E elements takes E / 16 such instructions on one accumulator, E additions in all, and whatever the order each product passes
through at most E of them.  If every addition rounds to nearest (relative error <= u = 2^-24), any order of summation gives
    |s - exact| <= gamma_E * sum_e |q g|,   gamma_n = n u / (1 - n u)                      (Higham, Accuracy and Stability, section 4.2).
An adder that truncates instead of rounding has relative error <= 2 u per addition, so u is DOUBLED:
    |s - exact| <= c * 2^-24 * sum_e |q g|,   c = 2 E / (1 - 2 E 2^-24).
The comparison value is the fp64 product of the same operands, itself a sum of E exact products with at most E fp64 roundings: E 2^-53 * sum |q g| is added
for it (2^-29 of the bound).  Sums whose partial sums are all integers below 2^24 have no rounding at all, in any order: the exact arm.
Subnormal operands and products are outside the contract; the tests stay far from them."""
import numpy as np

from search_ref import merge, order, search_splits, topk, workspace_bytes  # noqa: F401  (order, top-K, merge, splits: the fp32 entry's, word for word)

U = 2.0 ** -24                      # unit roundoff of fp32 (round to nearest)


def round_bf16(x):
    """fp32 array -> the nearest bf16 numbers, ties to even, returned as fp32 (NaN stays NaN, overflow goes to inf as the conversion instruction does)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    r = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return np.where(np.isnan(x), np.float32(np.nan), r.view(np.float32)).astype(np.float32)


def bf16_bits(x):
    """fp32 array of bf16-representable numbers -> their 16 storage bits (int16, for torch.Tensor.view(torch.bfloat16)); NaN -> 0x7FC0."""
    x = np.ascontiguousarray(x, np.float32)
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)
    bits = np.where(np.isnan(x), np.uint16(0x7FC0), bits)
    assert np.array_equal(np.nan_to_num(x, nan=0.0), np.nan_to_num((bits.astype(np.uint32) << 16).view(np.float32), nan=0.0)), "not bf16 numbers"
    return bits.view(np.int16)


def scores64(q, g):
    """fp64 scores of (already rounded) operands; + 0.0 turns a -0 sum into the +0 an accumulator that starts at +0 holds."""
    return q.astype(np.float64) @ g.astype(np.float64).T + 0.0


def c_of(E):
    return 2.0 * E / (1.0 - 2.0 * E * U)


def bound(q, g):
    """b[i, j] = (c 2^-24 + E 2^-53) * sum_e |q[i, e] g[j, e]| -- see the module docstring."""
    E = q.shape[1]
    return (c_of(E) * U + E * 2.0 ** -53) * (np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T)


# ------------------------------------------------------------------------------------------------------------ the judges
def judge_exact(vals, idx, q, g, k, idx_base=0):
    """Integer operands whose sums stay below 2^24: the result must equal the host top-K of the exact scores, tie rule included, in every bit."""
    s = scores64(q, g)
    assert np.abs(q).astype(np.float64).sum(1).max() * np.abs(g).max() < 2 ** 24 and np.array_equal(s, np.rint(s)), "not an exact case"
    want_v, want_i = topk(s, k, idx_base)
    return np.array_equal(idx, want_i) and np.array_equal(vals.view(np.uint32), want_v.view(np.uint32))


def judge_real(vals, idx, q, g, k):
    """Real operands (bf16 numbers held as fp32).  -> (ok, worst error / bound).  ok iff
      * idx holds k distinct positions of [0, N) per row, ordered by (vals descending, idx ascending);
      * every value is within b of the fp64 score of the position it is returned with;
      * with slack = 2 max(b): no returned position scores below the fp64 K-th score - slack, and no omitted position scores above the fp64 score of the
        returned K-th + slack.  Near-ties may fall either way: the criterion excludes nothing."""
    Q, N = q.shape[0], g.shape[0]
    s, b = scores64(q, g), bound(q, g)
    rows = np.arange(Q)[:, None]
    if idx.shape != (Q, k) or not ((idx >= 0) & (idx < N)).all():
        return False, np.inf
    member = np.zeros((Q, N), bool)
    member[rows, idx] = True
    dv, di = np.diff(vals.astype(np.float64), axis=1), np.diff(idx, axis=1)
    ordered = bool(((dv < 0) | ((dv == 0) & (di > 0))).all())
    ratio = np.abs(vals.astype(np.float64) - s[rows, idx]) / b[rows, idx]
    slack = 2.0 * b.max()
    kth = -np.sort(-s, axis=1)[:, k - 1:k]
    none_below = bool((s[rows, idx] >= kth - slack).all())
    none_above = bool((np.where(member, -np.inf, s) <= s[rows, idx[:, k - 1:k]] + slack).all())
    worst = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else np.inf
    ok = bool((member.sum(1) == k).all()) and ordered and bool((ratio <= 1.0).all()) and none_below and none_above
    return ok, worst


# ------------------------------------------------------------------------------------------------------------ a stand-in and its mutants
def standin(q, g, k, idx_base=0, mutant=None):
    """A host model of the entry: fp32 accumulation of the exact products, one addition per product in ascending e (ONE of the orders the bound covers),
    then the stated order.  mutant: "drop_last_group" (the last group of 16 never added), "shift_row" (gallery row 1 read one row further on),
    "reverse_ties" (equal scores ordered by j descending) -- what the judges must catch."""
    q, g = np.asarray(q, np.float32), np.asarray(g, np.float32)
    if mutant == "shift_row":
        g = g.copy()
        g[1] = g[2 % g.shape[0]]
    E = q.shape[1] - (16 if mutant == "drop_last_group" else 0)
    acc = np.zeros((q.shape[0], g.shape[0]), np.float32)
    for e in range(E):
        acc = acc + q[:, e, None] * g[None, :, e]            # fp32: the product is exact, the addition rounds to nearest
    if mutant == "reverse_ties":
        N = g.shape[0]
        v, i = topk(acc[:, ::-1].astype(np.float64), k)
        return v, np.where(i >= 0, N - 1 - i + idx_base, -1)
    return topk(acc.astype(np.float64), k, idx_base)

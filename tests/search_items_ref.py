"""Host statement of the id-aware selection (include/speechclip_hip.h, "Gallery search by item"), shared by tests/test_search_items_gpu.py and
tests/test_search_items_host.py.  Scores are not restated here: fp32 scores come from search_ref.chain_scores (or, where they are exact integers, from
search_ref.scores64), bf16 scores from the device's own plain entry; the order is search_ref.order."""
import numpy as np

import search_ref as R


def select(score_row, items, k, skip=-1, distinct=False, idx_base=0):
    """One query: score_row [N] in the precision it is to be compared in, items int [N] -> (vals f32 [k], idx i64 [k], items i32 [k]).
    Eligible: not NaN and (skip < 0 or items[j] != skip).  distinct: only the first pair of each item code in (score descending, j ascending) order."""
    items = np.asarray(items)
    o = R.order(score_row)                                     # NaN left out
    if skip is not None and skip >= 0:
        o = o[items[o] != skip]
    if distinct:
        _, first = np.unique(items[o], return_index=True)
        o = o[np.sort(first)]
    o = o[:k]
    vals, idx, its = np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64), np.full(k, -1, np.int32)
    vals[:len(o)], idx[:len(o)], its[:len(o)] = score_row[o], o + idx_base, items[o]
    return vals, idx, its


def search(score, items, k, skip=None, distinct=False, idx_base=0):
    """select for every row of score [Q, N]; skip: int [Q] or None."""
    rows = [select(score[i], items, k, -1 if skip is None else int(skip[i]), distinct, idx_base) for i in range(score.shape[0])]
    return tuple(np.stack(c) for c in zip(*rows))


def merge(vals, idx, items, k, distinct):
    """sc_topk_merge_items on the host: entries with idx < 0 or a NaN value take no part; with distinct only the first pair of each item code in (value
    descending, idx ascending) order survives; then the first k."""
    Q = vals.shape[0]
    ov, oi, oc = np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int64), np.full((Q, k), -1, np.int32)
    for i in range(Q):
        keep = np.flatnonzero((idx[i] >= 0) & ~np.isnan(vals[i]))
        o = keep[np.lexsort((idx[i, keep], -vals[i, keep].astype(np.float64)))]
        if distinct:
            _, first = np.unique(items[i, o], return_index=True)
            o = o[np.sort(first)]
        o = o[:k]
        ov[i, :len(o)], oi[i, :len(o)], oc[i, :len(o)] = vals[i, o], idx[i, o], items[i, o]
    return ov, oi, oc


def split_and_merge(score, items, k, skip, distinct, S):
    """The device's scheme on the host: S ranges of ceil(N / S) rows, select inside each, merge the partial lists."""
    N = score.shape[1]
    per = -(-N // S)
    parts = [search(score[:, a:a + per], items[a:a + per], k, skip, distinct, idx_base=a) if a < N else
             (np.full((score.shape[0], k), -np.inf, np.float32), np.full((score.shape[0], k), -1, np.int64), np.full((score.shape[0], k), -1, np.int32))
             for a in range(0, S * per, per)]
    return merge(*(np.concatenate(c, 1) for c in zip(*parts)), k, distinct)


def workspace_bytes(Q, N, K, n_split):
    """Python restatement of sc_search_items_workspace_bytes: (i64 + f32 + i32) per (query, split, slot), none for one split."""
    S = n_split if n_split else R.search_splits(Q, N, K)
    return 0 if S <= 1 else Q * S * K * 16


def grouped_items(rng, N, big=0):
    """Item codes for N rows: groups of 1..7 rows shuffled over the gallery, plus (big > 0) one item of `big` rows.  Codes are a permutation of 0 .. n-1,
    so code order and position order disagree."""
    sizes = [big] if big else []
    g = 1
    while sum(sizes) < N:
        sizes.append(min(g, N - sum(sizes)))
        g = g % 7 + 1
    codes = rng.permutation(len(sizes))
    items = np.repeat(codes, sizes)
    return items[rng.permutation(N)].astype(np.int32)

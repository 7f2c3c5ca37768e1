"""Host statement of the search by threshold (include/speechclip_hip.h, "Gallery search by threshold"), shared by tests/test_search_range_gpu.py and
tests/test_search_range_host.py: given a score matrix IN THE BITS THE ENTRY FORMS, the hits of every row at its threshold, in ascending j, with the NaN
rules, the skip codes and `lims`.

Where the score bits come from -- never from the code under test:
  fp32 rows   tests/search_ref.py: chain_scores (the exact restatement of the fmaf chain), or, for integer operands whose sums stay below 2^24, scores64.
  bf16 rows   window_scores_bf16 below: ops.search_topk_bf16 with K = the window size over windows of <= 128 gallery rows selected by pointer offset.  The
              purity contract of that entry says a pair's score does not depend on the call around it, so the K-list of a window, scattered back by its
              positions, holds every score of the window in the bits the bf16 kernels form; a row that is missing from the list has a NaN score."""
import numpy as np


def hits(row, t, items=None, skip=-1):
    """Ascending positions j with row[j] >= t in fp32 (a NaN score or threshold: none), minus the rows whose item code is the skip code (>= 0)."""
    row = np.asarray(row, np.float32)
    with np.errstate(invalid="ignore"):
        keep = row >= np.float32(t)
    if items is not None and skip is not None and skip >= 0:
        keep &= np.asarray(items) != skip
    return np.flatnonzero(keep)


def search_range(score, thresh, idx_base=0, items=None, skip=None):
    """score f32 [Q, N], thresh [Q] -> (lims i64 [Q + 1], vals f32 [T], idx i64 [T]): query i's hits at lims[i]:lims[i + 1], ascending j, idx = idx_base + j."""
    score = np.asarray(score, np.float32)
    Q = score.shape[0]
    per = [hits(score[i], thresh[i], items, -1 if skip is None else int(skip[i])) for i in range(Q)]
    lims = np.zeros(Q + 1, np.int64)
    lims[1:] = np.cumsum([len(p) for p in per])
    vals = np.concatenate([score[i, p] for i, p in enumerate(per)] + [np.zeros(0, np.float32)]).astype(np.float32)
    idx = np.concatenate([p + idx_base for p in per] + [np.zeros(0, np.int64)]).astype(np.int64)
    return lims, vals, idx


def brute_force(score, thresh, idx_base=0, items=None, skip=None):
    """The same statement as three nested decisions per pair, for tests/test_search_range_host.py to hold search_range against."""
    lims, vals, idx = [0], [], []
    for i in range(len(score)):
        for j in range(len(score[i])):
            s, t = float(score[i][j]), float(thresh[i])
            if s != s or t != t or not s >= t:
                continue
            if items is not None and skip is not None and skip[i] >= 0 and items[j] == skip[i]:
                continue
            vals.append(score[i][j])
            idx.append(idx_base + j)
        lims.append(len(vals))
    return np.array(lims, np.int64), np.array(vals, np.float32), np.array(idx, np.int64)


def same(got, want):
    """(lims, vals, idx) equal in every bit."""
    gl, gv, gi = (np.asarray(a) for a in got)
    wl, wv, wi = want
    return (np.array_equal(gl, wl) and gv.shape == wv.shape and np.array_equal(gv.astype(np.float32).view(np.uint32), wv.view(np.uint32))
            and np.array_equal(gi, wi))


def window_scores_bf16(ops, qd, gd, window=128):
    """The [Q, N] scores of bf16 device rows in the bits of sc_search_topk_bf16, from its K-lists over windows of <= 128 rows (module docstring)."""
    Q, N = qd.shape[0], gd.shape[0]
    out = np.full((Q, N), np.nan, np.float32)
    rows = np.arange(Q)[:, None]
    for at in range(0, N, window):
        n = min(window, N - at)
        v, i = ops.search_topk_bf16(qd, gd[at:at + n], n, n_split=1)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        ok = i >= 0
        out[np.broadcast_to(rows, i.shape)[ok], at + i[ok]] = v[ok]
    return out

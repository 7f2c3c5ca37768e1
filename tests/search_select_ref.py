"""Host statement of the search inside a subset (include/speechclip_hip.h, "Gallery search by subset"), shared by tests/test_search_select_gpu.py and
tests/test_search_select_host.py: the selection on a score matrix (search_items_ref.select over the ELIGIBLE rows only -- no score is ever overwritten), the
packing of a row mask, the dead-tile classification of a (N, n_split, mask), the device's scheme (ranges, live tiles, per-range lists, merge) with the
mistakes it can make as MUTANTS, and the case list.  Scores are not restated here (search_ref / search_bf16_ref)."""
import collections
import functools

import numpy as np

import search_items_ref as RI

BN = 128                                                                       # gallery rows per tile


# ---------------------------------------------------------------------------------------- the statement
def pack_row_mask(mask, mutant=None):
    """bool / uint8 [N] -> uint32 [ceil(N / 32)]: bit (j & 31) of word j >> 5 = mask[j] != 0, the unused high bits of the last word 0."""
    mask = np.asarray(mask) != 0
    N = len(mask)
    words = np.zeros((N + 31) // 32, np.uint32)
    for j in np.flatnonzero(mask):
        words[j >> 5] |= np.uint32(1 << (j & 31))
    if mutant == "pack_high_bits" and N % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    return words


def allowed_rows(words, N):
    """uint32 words or None -> bool [N]; bits at j >= N are ignored."""
    if words is None:
        return np.ones(N, bool)
    j = np.arange(N)
    return ((np.asarray(words, np.uint32)[j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def eligible_rows(N, words, g_group, q_group_i):
    """The two new conjuncts for one query: the row mask and the group (q_group_i < 0 or None: no restriction)."""
    el = allowed_rows(words, N)
    if g_group is not None and q_group_i is not None and q_group_i >= 0:
        el &= np.asarray(g_group) == q_group_i
    return el


def select(score_row, items, k, el, skip=-1, distinct=False, idx_base=0):
    """search_items_ref.select on the rows of `el` (bool [N]) only, positions mapped back."""
    rows = np.flatnonzero(el)
    v, i, c = RI.select(score_row[rows], np.asarray(items)[rows], k, skip, distinct)
    idx = np.full(k, -1, np.int64)
    idx[i >= 0] = rows[i[i >= 0]] + idx_base
    return v, idx, c


def search(score, items, k, words=None, g_group=None, q_group=None, skip=None, distinct=False, idx_base=0):
    """The contract: for every row of score [Q, N] the first k pairs among the eligible rows -> (vals f32, idx i64, items i32), each [Q, k]."""
    N = score.shape[1]
    rows = [select(score[i], items, k, eligible_rows(N, words, g_group, None if q_group is None else int(q_group[i])), -1 if skip is None else int(skip[i]),
                   distinct, idx_base) for i in range(score.shape[0])]
    return tuple(np.stack(c) for c in zip(*rows))


# ---------------------------------------------------------------------------------------- the device's scheme and its mutants
MUTANTS = ("bit_relative_to_range", "pack_high_bits", "high_bits_honoured", "first_word_unmasked", "last_word_unmasked", "dead_if_only_last_word",
           "dead_if_only_first_word", "group_inverted", "negative_group_is_a_code", "skip_or_group", "dead_range_leaves_stale_workspace")


def ranges(N, S):
    per = -(-N // S)
    return [(min(N, s * per), min(N, s * per + per)) for s in range(S)]


def tile_live(words, a, b, N, mutant=None):
    """Does [a, b) (a < b, at most BN rows) hold an allowed row?  The words of the rows, the first and the last masked to the rows -- as the kernel walks."""
    last = b - 1
    w0, w1 = a >> 5, last >> 5
    live = False
    for w in range(w0, w1 + 1):
        bits = int(words[w])
        if w == w0 and mutant != "first_word_unmasked":
            bits &= (0xFFFFFFFF << (a & 31)) & 0xFFFFFFFF
        if w == w1 and mutant != "last_word_unmasked" and not (mutant == "high_bits_honoured" and b == N):
            bits &= 0xFFFFFFFF >> (31 - (last & 31))
        if (mutant == "dead_if_only_last_word" and w == w1 and w1 > w0) or (mutant == "dead_if_only_first_word" and w == w0 and w1 > w0):
            continue
        live |= bits != 0
    return live


def dead_tiles(N, S, words, mutant=None):
    """-> one bool array per range: tile t of the range (BN rows from the range's first row) is dead.  Without a mask every tile is live."""
    out = []
    for a, b in ranges(N, S):
        tiles = range(a, b, BN)
        out.append(np.array([words is not None and not tile_live(words, t, min(t + BN, b), N, mutant) for t in tiles], bool))
    return out


STALE = (np.float32(0.0), np.int64(0), np.int32(0))                           # what a workspace of zero bytes holds in a slot


def device_scheme(score, items, k, words, g_group, q_group, skip, distinct, S, idx_base=0, mutant=None):
    """The device's way to the same result: per range the rows of its live tiles, the predicate, a k-list (search_items_ref.select on the eligible rows),
    then the merge of the S lists.  With mutant=None this equals `search`; every name of MUTANTS is one mistake of the kernel."""
    Q, N = score.shape
    items = np.asarray(items)
    dead = dead_tiles(N, S, words, mutant)
    parts = []
    for (a, b), d in zip(ranges(N, S), dead):
        if mutant == "dead_range_leaves_stale_workspace" and S > 1 and d.all():
            parts.append(tuple(np.full((Q, k), x) for x in STALE))
            continue
        scanned = np.zeros(N, bool)
        for t, is_dead in enumerate(d):
            if not is_dead:
                scanned[a + t * BN:min(a + (t + 1) * BN, b)] = True
        if words is None:
            bit = np.ones(N, bool)
        else:
            j = np.arange(N)
            at = j - a if mutant == "bit_relative_to_range" else j
            at = np.clip(at, 0, len(words) * 32 - 1)
            bit = ((np.asarray(words, np.uint32)[at >> 5] >> (at & 31).astype(np.uint32)) & 1).astype(bool)
        rows = []
        for i in range(Q):
            grouped = np.ones(N, bool)
            if q_group is not None:
                code = int(q_group[i])
                if code >= 0 or mutant == "negative_group_is_a_code":
                    grouped = (np.asarray(g_group) != code) if mutant == "group_inverted" else (np.asarray(g_group) == code)
            code = -1 if skip is None else int(skip[i])
            unskipped = np.ones(N, bool) if code < 0 else items != code
            both = (unskipped | grouped) if mutant == "skip_or_group" and q_group is not None and skip is not None else (unskipped & grouped)
            rows.append(select(score[i], items, k, scanned & bit & both, -1, distinct, idx_base))
        parts.append(tuple(np.stack(c) for c in zip(*rows)))
    if S == 1:
        return parts[0]
    return RI.merge(*(np.concatenate(c, 1) for c in zip(*parts)), k, distinct)


# ---------------------------------------------------------------------------------------- the case list
NS = (31, 32, 33, 127, 128, 129, 257, 4133)
SPLITS = (1, 3, 7)
QS = (1, 64, 65, 130)
KS = (1, 16, 17, 64, 128)
ES = {"fp32": (4, 20, 68), "bf16": (16, 48, 80)}
MASKS = ("ones", "zeros", "first_row_of_a_range", "last_row_of_a_range", "one_live_tile", "first_tile_dead", "last_tile_dead", "alternating", "bit31",
         "bit0", "garbage_high_bits")
GROUPS = ("none", "free", "absent_code", "interleaved", "interleaved_skip_distinct")
Case = collections.namedtuple("Case", "N Q K e mask group")                    # e: index into ES[fmt]


def make_mask(name, N):
    """-> (bool [N], the words handed to the entry).  The words are pack_row_mask(mask) except for garbage_high_bits, whose last word's unused bits are
    set.  Range edges are those of 3 and of 7 splits."""
    j = np.arange(N)
    edges = sorted({-(-N // S) * s for S in SPLITS for s in range(1, S) if -(-N // S) * s < N})
    if name in ("ones", "garbage_high_bits"):
        mask = np.ones(N, bool) if name == "ones" else np.random.default_rng(N).random(N) < 0.3
    elif name == "zeros":
        mask = np.zeros(N, bool)
    elif name == "first_row_of_a_range":
        mask = np.isin(j, edges[:1] + edges[-1:])
    elif name == "last_row_of_a_range":
        mask = np.isin(j, [e - 1 for e in edges[:1] + edges[-1:]] + [N - 1])
    elif name == "one_live_tile":                                              # the second tile of the whole gallery (one row of it, if there is no second tile)
        mask = (j >= BN) & (j < 2 * BN) if N > BN else j == N // 2
    elif name == "first_tile_dead":
        mask = j >= min(BN, N - 1)
    elif name == "last_tile_dead":
        mask = j < max(1, (N - 1) // BN * BN)
    elif name == "alternating":
        mask = j % 2 == 1
    elif name == "bit31":
        mask = j % 32 == 31
    else:
        assert name == "bit0", name
        mask = j % 32 == 0
    words = pack_row_mask(mask)
    if name == "garbage_high_bits" and N % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    return mask, words


def case_list():
    """Every N with every mask; Q, K (<= N), the E of the format and the group variant rotate at different rates, so that all values of each, all four
    (tile width, list capacity) instantiations and every (mask, group variant) pair occur.  Every case is run at every n_split of SPLITS."""
    out, c = [], 0
    for n, N in enumerate(NS):
        for m, mask in enumerate(MASKS):
            ks = [K for K in KS if K <= N]
            out.append(Case(N, QS[(c + n) % 4], ks[(c // 2 + m) % len(ks)], c % 3, mask, GROUPS[(m + n) % 5]))
            c += 1
    return out


CASES = case_list()


@functools.lru_cache(maxsize=None)
def operands(case, fmt):
    """Exact-integer operands of a case: entries in [-2, 2] (|score| <= 4 E <= 320: exact in both formats, many ties), item codes in groups, and the
    selector arguments -> dict(q, g, items, mask, words, g_group, q_group, skip, distinct)."""
    N, Q, K, e, mask_name, group = case
    E = ES[fmt][e]
    rng = np.random.default_rng(1000 * N + 10 * Q + K + e)
    q = rng.integers(-2, 3, (Q, E)).astype(np.float32)
    g = rng.integers(-2, 3, (N, E)).astype(np.float32)
    items = rng.integers(0, max(2, N // 3), N).astype(np.int32)
    mask, words = make_mask(mask_name, N)
    i, j = np.arange(Q), np.arange(N)
    g_group = q_group = skip = None
    if group == "free":
        g_group, q_group = (j % 3).astype(np.int32), np.full(Q, -1, np.int32)
    elif group == "absent_code":
        g_group, q_group = (j % 3).astype(np.int32), np.where(i % 2 == 0, 7, 1).astype(np.int32)
    elif group != "none":
        g_group, q_group = (j % 2).astype(np.int32), np.where(i % 3 == 2, -1, i % 2).astype(np.int32)
    if group == "interleaved_skip_distinct":
        skip = np.where(i % 2 == 0, items[N // 2], -1).astype(np.int32)
    return dict(q=q, g=g, items=items, mask=mask, words=words, g_group=g_group, q_group=q_group, skip=skip, distinct=group == "interleaved_skip_distinct")

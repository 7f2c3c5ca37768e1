"""mutualRetrieval -- same signature and return triple as avssl/module/retrieval.py:6-121 (recall@K in percent,
A->B, B->A and their mean).  Implemented with a rank test instead of a full argsort + Python row loops:
item i is a hit@K iff fewer than K candidates score above its best candidate carrying its answer id (sc_retrieval_ranks on the device)."""
from typing import Hashable, List, Optional, Sequence, Tuple, Union

import torch


def _recall_one_way(score: torch.Tensor, own_ids: torch.Tensor, cand_ids: torch.Tensor, recall_at: Sequence[int]) -> dict:
    n, m = score.shape
    # There is ONE implementation: sc_retrieval_ranks on the MI355X.  Host score matrices (the reference's validation_epoch_end hands CPU tensors
    # to mutualRetrieval, kwClip.py:487-491) are moved to the device; without a GPU / the library this raises -- no host re-implementation.
    from .. import ops
    from .._lib import SpeechClipHipError
    if not score.is_cuda:
        if not torch.cuda.is_available():
            raise SpeechClipHipError("mutualRetrieval ranks on the MI355X (sc_retrieval_ranks); no GPU is visible and there is no host fallback")
        # the device the answer ids live on if they are device tensors (a multi-rank run's model device), else this process's CURRENT device --
        # never a bare .cuda() (device 0 of whatever is visible)
        dev = next((t.device for t in (own_ids, cand_ids) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
        score = score.to(dev)
    rank = ops.retrieval_ranks(score.float().contiguous(), own_ids, cand_ids)
    out = {}
    for k in recall_at:
        if k > m:
            print("recall@{} is not eligible for #{} samples".format(k, m))
        out["recall@{}".format(k)] = (rank < min(k, m)).float().mean().item() * 100
    return out


def mutualRetrieval(score_per_A: torch.Tensor, score_per_B: torch.Tensor, AB_answers: torch.Tensor, BA_answers: torch.Tensor,
                    recall_at: list, modality_A_title: str = "audio", modality_B_title: str = "image") -> Tuple[dict, dict, dict]:
    assert score_per_A.dim() == 2 and score_per_B.dim() == 2 and AB_answers.dim() == 1 and BA_answers.dim() == 1
    assert score_per_A.shape == (len(AB_answers), len(BA_answers)), (score_per_A.shape, (len(AB_answers), len(BA_answers)))
    assert score_per_B.shape == (len(BA_answers), len(AB_answers)), (score_per_B.shape, (len(BA_answers), len(AB_answers)))
    ab = _recall_one_way(score_per_A, AB_answers, BA_answers, recall_at)
    ba = _recall_one_way(score_per_B, BA_answers, AB_answers, recall_at)
    mean = {k: (ab[k] + ba[k]) / 2.0 for k in ab}
    return ab, ba, mean


RERANK_MERGE_CANDIDATES = 8192         # most candidates per query that the first stage of the two-stage search hands to sc_topk_merge (splits x R)
RERANK_INFLATE = 1.0 + 2.0 ** -22     # covers the fp64 roundings of the norms and of eps, and its rounding to fp32 (2^-24), with room to spare


def rerank_kappa(E: int) -> float:
    """kappa(E) of the two-stage search: |bf16-stage score of the rounded rows - fp32 chain of the stored rows| <= kappa(E) ||q|| ||g|| for finite, normal
    operands.  Three terms (statement and derivation: tests/search_rerank_ref.py): rounding both operands to bf16 (8 significand bits, unit roundoff 2^-8:
    2^-7 + 2^-16), the bf16 entry's accumulation bound c 2^-24 with c = 2E / (1 - 2E 2^-24) carried from the rounded rows back to the stored ones by
    (1 + 2^-8)^2, and gamma_E = E 2^-24 / (1 - E 2^-24) of the fp32 fmaf chain."""
    u = 2.0 ** -24
    return (2.0 ** -7 + 2.0 ** -16) + 2.0 * E * u / (1.0 - 2.0 * E * u) * (1.0 + 2.0 ** -8) ** 2 + E * u / (1.0 - E * u)


class RowSelector:
    """A row subset of one EmbeddingIndex, prepared once (EmbeddingIndex.selector) and passed to search(allow=...): `words` holds, per segment, the packed
    mask (uint32 [ceil(rows / 32)], bit j & 31 of word j >> 5 = row j of THAT segment is allowed); `rows` is what the index held when it was made."""

    def __init__(self, index: "EmbeddingIndex", words: List[torch.Tensor], rows: int):
        self.index, self.words, self.rows = index, words, rows


class EmbeddingIndex:
    """A gallery of embeddings on the device and the answer to "which k stored items are nearest to this query?" (sc_search_topk: fused fp32
    similarity + top-k, no [Q, N] score image).  Rows are kept as fp32 SEGMENTS, one per `add`; adding never reallocates earlier segments.  A search runs
    every segment with its starting position as idx_base and joins the partial lists with sc_topk_merge; because the score is a fixed fmaf chain per
    (query, row) and ties go to the lower position, the result equals, bit for bit, a search of ONE segment holding the concatenation.
    storage="bf16" (dim % 16 == 0) keeps the rows in bf16 instead: rows and queries are normalised in fp32 as before and then rounded to bf16 (round to
    nearest even), and sc_search_topk_bf16 forms the scores -- exact bf16 products summed in fp32, returned as fp32; half the bytes per row, the same
    segments, positions, ids and merge, and the same one-segment equality.  The default stays fp32.
    shadow=True (fp32 storage, dim % 16 == 0) keeps, beside every fp32 segment, the same rows rounded to bf16 -- exactly what astype("bf16") holds -- and the
    running maximum of the stored rows' norms: what search(..., rerank=R) needs to answer with the fp32 result at close to the bf16 search's cost.
    search_range answers the other question -- "which stored items score at least t for this query?" -- with the same scores (sc_search_range_count /
    sc_search_range_fill: two passes, no score image, hits in ascending position), on either storage.
    There is no host implementation: without the library's GPU `add` / `search` / `search_range` raise SpeechClipHipError, like mutualRetrieval."""

    STORAGES = {"fp32": torch.float32, "bf16": torch.bfloat16}
    STORAGE_BITS = {"fp32": 32, "bf16": 16}            # how state_dict names the storage

    def __init__(self, dim: int, device=None, normalize: bool = True, storage: str = "fp32", shadow: bool = False):
        if storage not in self.STORAGES:
            raise ValueError(f"storage={storage!r} must be one of {sorted(self.STORAGES)}")
        if storage == "bf16" and int(dim) % 16 != 0:
            raise ValueError(f"storage='bf16' needs dim % 16 == 0 (sc_search_topk_bf16), got dim={dim}")
        if shadow and (storage != "fp32" or int(dim) % 16 != 0):
            raise ValueError(f"shadow=True needs storage='fp32' and dim % 16 == 0 (sc_search_topk_bf16 on the shadow rows), got storage={storage!r}, dim={dim}")
        self.shadow = bool(shadow)
        self.shadow_segments: List[torch.Tensor] = []  # with a shadow: segment s rounded to bf16
        self._norm_max = None                      # with a shadow: fp64 device scalar, the largest stored row norm so far
        self.dim, self.normalize, self.storage = int(dim), bool(normalize), storage
        self.device = torch.device(device) if device is not None else None
        self.segments: List[torch.Tensor] = []
        self.ids: Optional[list] = None            # None: the ids are the running positions
        self._n = 0
        self._codes = None                         # item codes of the rows (search with distinct / exclude), derived from ids
        self._code_table = None                    # their host half: (codes per row or None, {id: code} or None, number of codes)

    def __len__(self) -> int:
        return self._n

    def _device(self, t: Optional[torch.Tensor] = None) -> torch.device:
        from .._lib import SpeechClipHipError
        if self.device is None:
            if t is not None and t.is_cuda:
                self.device = t.device
            elif torch.cuda.is_available():
                self.device = torch.device("cuda", torch.cuda.current_device())
        if self.device is None or self.device.type != "cuda" or not torch.cuda.is_available():
            raise SpeechClipHipError("EmbeddingIndex searches on the MI355X (sc_search_topk); no GPU is visible and there is no host fallback")
        return self.device

    def _rows(self, feats: torch.Tensor) -> torch.Tensor:
        from .. import ops
        feats = torch.as_tensor(feats)
        if feats.dim() != 2 or feats.shape[1] != self.dim or not feats.is_floating_point():
            raise ValueError(f"expected float rows [n, {self.dim}], got {tuple(feats.shape)} {feats.dtype}")
        rows = feats.detach().to(self._device(feats), torch.float32).contiguous()
        rows = ops.l2norm(rows) if self.normalize and rows.shape[0] else rows
        return rows.to(self.STORAGES[self.storage])          # bf16 storage: rounded to nearest even AFTER the fp32 normalisation

    def add(self, feats: torch.Tensor, ids: Union[None, torch.Tensor, Sequence[Hashable]] = None) -> "EmbeddingIndex":
        rows = self._rows(feats)
        n = rows.shape[0]
        if ids is not None:
            ids = ids.detach().cpu().tolist() if torch.is_tensor(ids) else list(ids)
            if len(ids) != n:
                raise ValueError(f"{len(ids)} ids for {n} rows")
        if (ids is None) != (self.ids is None) and self._n:
            raise ValueError("an index keeps ids for every row or for none")
        if ids is not None:
            self.ids = (self.ids or []) + ids
        if n:
            self.segments.append(rows)
            self._n += n
            if self.shadow:
                self._add_shadow(rows)
        self._codes = self._code_table = None
        return self

    def _add_shadow(self, rows: torch.Tensor) -> None:
        self.shadow_segments.append(rows.to(torch.bfloat16))             # round to nearest even, after the fp32 normalisation
        top = torch.stack([rows[at:at + 65536].double().norm(dim=1).max() for at in range(0, rows.shape[0], 65536)]).max()   # fp64, in bounded pieces
        self._norm_max = top if self._norm_max is None else torch.maximum(self._norm_max, top)

    def with_shadow(self) -> "EmbeddingIndex":
        """A new fp32 index over the same segments (shared, they are never written) and ids, with shadow rows: what search(..., rerank=R) needs."""
        out = EmbeddingIndex(self.dim, device=self.device, normalize=self.normalize, storage=self.storage, shadow=True)
        out.segments = list(self.segments)
        out.ids = None if self.ids is None else list(self.ids)
        out._n = self._n
        for seg in out.segments:
            out._add_shadow(seg)
        return out

    def _item_codes(self):
        """-> (one int32 device tensor of item codes per segment, {id: code} or None, number of codes).  Equal ids share a code, assigned in first-seen
        order; without ids the code is the position.  Derived from `ids`, built on first use and dropped by `add`; never stored."""
        if self._codes is None:
            codes, table, _ = self._item_codes_host()
            codes = list(range(self._n)) if codes is None else codes
            segs, at = [], 0
            for seg in self.segments:
                segs.append(torch.tensor(codes[at:at + seg.shape[0]], dtype=torch.int32, device=seg.device))
                at += seg.shape[0]
            self._codes = (segs, table, self._n if table is None else len(table))
        return self._codes

    def selector(self, allow=None, allow_ids=None) -> "RowSelector":
        """A reusable row subset for search(allow=...): the packed mask words of every segment, on the device.  allow: bool [len(index)] by position;
        allow_ids: a collection of ids, selecting the rows that carry one of them (ids the index does not hold select nothing) -- the lookup over the
        stored ids is paid here, once, not per search.  The selector speaks about the rows the index holds NOW: it refuses to be used after a later add."""
        if (allow is None) == (allow_ids is None):
            raise ValueError("a selector takes allow (a bool per row) or allow_ids (a collection of ids), one of the two")
        mask = self._allow_mask(allow, allow_ids)
        return self._pack_selector(mask)

    def _allow_mask(self, allow, allow_ids) -> torch.Tensor:
        """Host rules of allow / allow_ids -> a bool tensor [len(index)] (wherever the caller's lives; from ids: on the host)."""
        if allow_ids is not None:
            wanted = set(allow_ids.detach().cpu().tolist() if torch.is_tensor(allow_ids) else allow_ids)
            ids = range(self._n) if self.ids is None else self.ids
            return torch.tensor([x in wanted for x in ids], dtype=torch.bool)
        mask = torch.as_tensor(allow)
        if mask.dtype != torch.bool or mask.shape != (self._n,):
            raise ValueError(f"allow must be a bool per stored row [{self._n}], got {tuple(mask.shape)} {mask.dtype}")
        return mask

    def _pack_selector(self, mask: torch.Tensor) -> "RowSelector":
        from .. import ops
        mask = mask.to(self._device())
        words, at = [], 0
        for seg in self.segments:                  # every segment's slice is packed from ITS row 0: a segment is one call of the entry
            words.append(ops.pack_row_mask(mask[at:at + seg.shape[0]].contiguous()))
            at += seg.shape[0]
        return RowSelector(self, words, self._n)

    def _select_arguments(self, queries, allow, allow_ids, within, row_groups, query_groups, rerank):
        """The host rules of the subset arguments of `search`, checked before anything touches the device -> None without any of them, else
        (selector or bool mask or None, row groups (host or device int tensor) or None, the queries' group codes as a host list or None, within?)."""
        if all(x is None for x in (allow, allow_ids, within, row_groups, query_groups)):
            return None
        if rerank is not None:
            raise ValueError("rerank with allow / allow_ids / within / row_groups is not supported: the certificate speaks about the whole gallery, "
                             "not about a subset of it")
        if allow is not None and allow_ids is not None:
            raise ValueError("allow and allow_ids exclude each other: give the subset by position or by id")
        if (row_groups is None) != (query_groups is None):
            raise ValueError("row_groups and query_groups are given together or not at all")
        if within is not None and row_groups is not None:
            raise ValueError("within cannot be combined with row_groups: within IS row_groups = the item codes and query_groups = the id's code")
        Q = len(queries)
        q_codes = None
        if within is not None:
            within = within.detach().cpu().tolist() if torch.is_tensor(within) else list(within)
            if len(within) != Q:
                raise ValueError(f"{len(within)} within ids for {Q} queries")
            _, table, n_ids = self._item_codes_host()
            # an id the index does not hold, or None, matches nothing: the code n_ids, which no row carries (a negative code would lift the restriction)
            if table is None:
                q_codes = [x if isinstance(x, int) and not isinstance(x, bool) and 0 <= x < self._n else n_ids for x in within]
            else:
                q_codes = [n_ids if x is None else table.get(x, n_ids) for x in within]
        if row_groups is not None:
            row_groups = torch.as_tensor(row_groups)
            if row_groups.is_floating_point() or row_groups.dtype == torch.bool or row_groups.shape != (self._n,):
                raise ValueError(f"row_groups must be an int per stored row [{self._n}], got {tuple(row_groups.shape)} {row_groups.dtype}")
            # (the same rule wherever the tensor lives: of a device tensor this reads two numbers back, before any search is launched)
            if row_groups.numel() and not 0 <= int(row_groups.min()) <= int(row_groups.max()) < 2 ** 31:
                raise ValueError("row_groups must hold values in [0, 2^31)")
            q_codes = query_groups.detach().cpu().tolist() if torch.is_tensor(query_groups) else list(query_groups)
            if len(q_codes) != Q:
                raise ValueError(f"{len(q_codes)} query_groups for {Q} queries")
            if any(isinstance(x, bool) or not isinstance(x, int) or not -2 ** 31 <= x < 2 ** 31 for x in q_codes):
                raise ValueError("query_groups must hold one int per query (negative: no restriction)")
        subset = None
        if isinstance(allow, RowSelector):
            if allow.index is not self:
                raise ValueError("this selector was made by another index")
            if allow.rows != self._n:
                raise ValueError(f"this selector was made when the index held {allow.rows} rows; it holds {self._n} now: make a new one after add")
            subset = allow
        elif allow is not None or allow_ids is not None:
            subset = self._allow_mask(allow, allow_ids)
        return subset, row_groups, q_codes, within is not None

    def _item_codes_host(self):
        """The host half of _item_codes -> (the code of every row as a list, or None without ids; {id: code} or None; number of codes): the argument rules
        run before the device is touched.  The one pass over the ids, built on first use, kept until `add`, and what _item_codes puts on the device."""
        if self._code_table is None:
            table = None if self.ids is None else {}
            codes = None if table is None else [table.setdefault(x, len(table)) for x in self.ids]
            self._code_table = (codes, table, self._n if table is None else len(table))
        return self._code_table

    def search(self, queries: torch.Tensor, k: int, distinct: bool = False, exclude: Optional[Sequence[Hashable]] = None, rerank: Optional[int] = None,
               return_certified: bool = False, allow=None, allow_ids=None, within=None, row_groups=None, query_groups=None):
        """-> (scores f32 [Q, k] descending, positions i64 [Q, k], ids): ids[i][r] is the stored id of positions[i, r] (the position itself without ids).
        distinct=True: the k nearest DIFFERENT ids, each by its best row (rows that share an id are one item; k <= the number of different ids).
        exclude: one id per query (a sequence of len(queries)); rows carrying it are left out of that query's result -- None, or an id the index does not
        hold, leaves out nothing.  With both defaults this is the plain search (sc_search_topk); otherwise sc_search_items, same scores and order.
        rerank=R (an index with a shadow, k <= R <= 128, distinct=False): the SAME result, bit for bit, by two stages -- a bf16 search of the shadow rows
        shortlists R rows per query and segment, sc_search_rescore scores them on the fp32 rows and certifies the queries whose shortlist provably holds
        the first k (rerank_kappa), and only the other queries go through the fp32 search.  return_certified=True (with rerank) appends a bool [Q] host
        tensor: which queries the certificate covered.
        A SUBSET of the gallery (sc_search_select: the predicate acts before the top-k filter, and gallery tiles nobody selected are not scanned):
        allow = a bool per stored row, by position, or a prepared index.selector(...); allow_ids = a collection of ids, selecting the rows that carry one
        of them (ids the index does not hold select nothing; allow and allow_ids exclude each other); row_groups (an int >= 0 per stored row) with
        query_groups (an int per query, negative: no restriction): query i sees only the rows of its group; within = one id per query: only the rows
        carrying that id take part -- the converse of exclude, shorthand for row_groups = the item codes (an id the index does not hold, or None, matches
        nothing; not with row_groups).  A query with fewer than k rows left gets -inf / -1 / None in the last slots.  Nothing of this combines with
        rerank.  With none of these arguments exactly the entries above run."""
        from .. import ops
        k = int(k)
        select = self._select_arguments(queries, allow, allow_ids, within, row_groups, query_groups, rerank)
        if rerank is not None:                    # the rules of the two-stage search are host rules: checked before anything touches the device
            if not self.shadow:
                raise ValueError("rerank needs an index with shadow rows: EmbeddingIndex(..., shadow=True) or index.with_shadow()")
            if distinct:
                raise ValueError("rerank with distinct=True is not supported: an item's best bf16 row need not be its best fp32 row")
            if not k <= int(rerank) <= 128:
                raise ValueError(f"rerank={rerank} must be in [k={k}, 128]")
        elif return_certified:
            raise ValueError("return_certified=True needs rerank=R: only the two-stage search certifies anything")
        dev = self._device()
        if not 1 <= k <= min(128, max(self._n, 1)) or self._n == 0:
            raise ValueError(f"k={k} must be in [1, min(128, {self._n} stored rows)]")
        if rerank is not None:
            return self._search_rerank(queries, k, int(rerank), bool(distinct), exclude, bool(return_certified))
        distinct, by_item = bool(distinct), bool(distinct) or exclude is not None or select is not None
        codes, skip = self._item_arguments(queries, k, distinct, exclude) if by_item else ([None] * len(self.segments), None)
        q = self._rows(queries)
        if skip is not None:
            skip = torch.tensor(skip, dtype=torch.int32, device=dev)
        if select is not None:
            select = self._select_on_device(select, codes, dev)
        scores, pos = self._search_prepared(q, k, distinct, by_item, codes, skip, select)
        return scores, pos, self._ids_of(pos)

    def _select_on_device(self, select, codes, dev):
        """What _select_arguments returned -> (mask words per segment, group codes per segment, the queries' group codes), each a device tensor or None."""
        subset, row_groups, q_codes, by_within = select
        none = [None] * len(self.segments)
        words = none if subset is None else (subset if isinstance(subset, RowSelector) else self._pack_selector(subset)).words
        groups, q_group = none, None
        if q_codes is not None:
            q_group = torch.tensor(q_codes, dtype=torch.int32, device=dev)
            if by_within:
                groups = codes                     # within: the rows' groups are their item codes
            else:
                row_groups = row_groups.to(dev, torch.int32)
                groups, at = [], 0
                for seg in self.segments:          # every segment gets its own slice, as it gets its own slice of the mask
                    groups.append(row_groups[at:at + seg.shape[0]].contiguous())
                    at += seg.shape[0]
        return words, groups, q_group

    def _search_prepared(self, q: torch.Tensor, k: int, distinct: bool, by_item: bool, codes, skip, select=None):
        """The one-stage search of prepared query rows (already normalised and in the storage type) -> (scores, positions).  select: the subset arguments
        on the device (_select_on_device) or None; with it every segment goes through sc_search_select[_bf16], else through exactly the entries of before."""
        from .. import ops
        dev = q.device
        bf16 = self.storage == "bf16"
        search_topk, search_items = (ops.search_topk_bf16, ops.search_items_bf16) if bf16 else (ops.search_topk, ops.search_items)
        search_select = ops.search_select_bf16 if bf16 else ops.search_select
        none = [None] * len(self.segments)
        words, groups, q_group = select if select is not None else (none, none, None)
        parts, base = [], 0
        for seg, code, word, group in zip(self.segments, codes, words, groups):
            kk = min(k, seg.shape[0])
            if select is not None:
                part = search_select(q, seg, kk, code, allow=word, g_group=group if q_group is not None else None, q_group=q_group, q_skip=skip,
                                     distinct=distinct, idx_base=base)
            else:
                part = search_items(q, seg, kk, code, q_skip=skip, distinct=distinct, idx_base=base) if by_item else search_topk(q, seg, kk, idx_base=base)
            if kk < k:                             # a segment shorter than k: its list is padded with entries that take no part in the merge
                part = [torch.cat([t, torch.full((q.shape[0], k - kk), fill, device=dev, dtype=t.dtype)], 1) for t, fill in zip(part, (float("-inf"), -1, -1))]
            parts.append(part)
            base += seg.shape[0]
        if len(parts) == 1:
            scores, pos = parts[0][:2]
        else:
            joined = [torch.cat(t, 1) for t in zip(*parts)]
            scores, pos = (ops.topk_merge_items(*joined, k, distinct) if by_item else ops.topk_merge(*joined, k))[:2]
        return scores, pos

    def _search_rerank(self, queries, k: int, R: int, distinct: bool, exclude, return_certified: bool):
        """search(..., rerank=R).  Per segment: stage 1 on the shadow rows with K = min(R, rows) (sc_search_topk_bf16, or sc_search_items_bf16 with the skip
        codes), sc_search_rescore on the fp32 rows, the usual padding; then sc_topk_merge (a segment is a split: exact per-segment lists merge exactly).
        A query is certified iff it is certified in every segment; the flags are read once, and the queries without the proof -- only those -- are run
        through the one-stage fp32 search, whose rows do not depend on the other queries of the call (the entries' purity contract)."""
        from .. import ops
        by_item = exclude is not None
        codes, skip_host = self._item_arguments(queries, k, False, exclude) if by_item else ([None] * len(self.segments), None)
        q = self._rows(queries)
        dev, Q = q.device, q.shape[0]
        skip = None if skip_host is None else torch.tensor(skip_host, dtype=torch.int32, device=dev)
        qb = q.to(torch.bfloat16)
        # eps_i = kappa(E) ||q_i|| G in fp64, inflated once for the roundings of the norms, of this product and of its conversion to fp32
        eps = (q.double().norm(dim=1) * self._norm_max.to(dev) * (rerank_kappa(self.dim) * RERANK_INFLATE)).to(torch.float32)
        parts, base, flags = [], 0, None
        for seg, sh, code in zip(self.segments, self.shadow_segments, codes):
            rr = min(R, seg.shape[0])
            kk = min(k, rr)
            # sc_topk_merge takes K rounds over S K candidates per query: with K = R the automatic split count (chosen for K = 10-like lists) makes the
            # merge, not the scan, the cost of a few queries against a large gallery -- the splits are capped so that a query merges at most 8192 candidates
            S = max(1, min(ops.lib().sc_search_splits(Q, seg.shape[0], rr), RERANK_MERGE_CANDIDATES // rr))
            short = (ops.search_items_bf16(qb, sh, rr, code, q_skip=skip, distinct=False, n_split=S, idx_base=base) if by_item else
                     ops.search_topk_bf16(qb, sh, rr, n_split=S, idx_base=base))
            v, i, c = ops.search_rescore(q, seg, short[1], short[0], eps, kk, idx_base=base)
            if kk < k:
                v, i = (torch.cat([t, torch.full((Q, k - kk), fill, device=dev, dtype=t.dtype)], 1) for t, fill in zip((v, i), (float("-inf"), -1)))
            parts.append((v, i))
            flags = c if flags is None else flags & c
            base += seg.shape[0]
        scores, pos = parts[0] if len(parts) == 1 else ops.topk_merge(*(torch.cat(t, 1) for t in zip(*parts)), k)
        certified = flags.cpu().bool()                                   # the one read of the flags
        redo = torch.nonzero(~certified).flatten()
        if redo.numel():
            rows = redo.to(dev)
            sub_skip = None if skip is None else skip[rows].contiguous()
            s2, p2 = self._search_prepared(q[rows].contiguous(), k, False, by_item, codes, sub_skip)
            scores, pos = scores.index_copy(0, rows, s2), pos.index_copy(0, rows, p2)
        out = (scores, pos, self._ids_of(pos))
        return out + (certified,) if return_certified else out

    def search_range(self, queries: torch.Tensor, min_score, exclude: Optional[Sequence[Hashable]] = None, max_results: Optional[int] = None):
        """Every stored row that scores at least min_score -> (lims i64 [Q + 1], scores f32 [T], positions i64 [T], ids list [T]): query i's hits are
        lims[i]:lims[i + 1], in ascending position, with the scores of `search` bit for bit.  min_score: one float, or one value per query (a sequence or
        a tensor of len(queries)); a NaN hits nothing, -inf hits every row.  exclude: one id per query, as in `search`.  No [Q, N] score image: every
        segment counts its hits into its own columns of one table (sc_search_range_count), ONE scan and ONE read of the total follow, then every segment
        writes its hits with its starting position as idx_base (sc_search_range_fill) -- so the result equals that of one segment holding the
        concatenation, bit for bit and position for position.  More than max_results hits (default: 1 GiB of results) raise ValueError before anything
        is allocated or written.  An index with a shadow searches its fp32 rows."""
        from .. import ops
        dev = self._device()
        codes, skip = self._item_arguments(queries, 1, False, exclude) if exclude is not None else ([None] * len(self.segments), None)
        q = self._rows(queries)
        Q = q.shape[0]
        thresh = torch.as_tensor(min_score, dtype=torch.float32).to(dev)
        if thresh.dim() == 0:
            thresh = thresh.expand(Q)
        if thresh.shape != (Q,):
            raise ValueError(f"min_score must be one number or one per query ({Q}), got shape {tuple(thresh.shape)}")
        thresh = thresh.contiguous()
        if skip is not None:
            skip = torch.tensor(skip, dtype=torch.int32, device=dev)
        splits = [ops.lib().sc_search_splits(Q, seg.shape[0], 1) for seg in self.segments]
        counts = torch.empty(Q, sum(splits), device=dev, dtype=torch.int32)
        at = 0
        for seg, code, S in zip(self.segments, codes, splits):
            ops.search_range_count(q, seg, thresh, S, code, skip, out=counts[:, at:at + S])
            at += S
        lims, offs, total = ops.search_range_offsets(counts, max_results)
        scores = torch.empty(total, device=dev, dtype=torch.float32)
        pos = torch.empty(total, device=dev, dtype=torch.int64)
        at = base = 0
        for seg, code, S in zip(self.segments, codes, splits):
            ops.search_range_fill(q, seg, thresh, offs[:, at:at + S], scores, pos, S, base, code, skip)
            at += S
            base += seg.shape[0]
        host = pos.cpu().tolist()
        return lims, scores, pos, host if self.ids is None else [self.ids[p] for p in host]

    def _ids_of(self, pos: torch.Tensor) -> list:
        host = pos.cpu().tolist()
        return host if self.ids is None else [[self.ids[p] if p >= 0 else None for p in row] for row in host]

    def _item_arguments(self, queries, k: int, distinct: bool, exclude):
        """search with distinct / exclude -> (one tensor of item codes per segment, the queries' skip codes as a host list or None): every segment goes
        through sc_search_items[_bf16] with its item codes, and the partial lists are joined by sc_topk_merge_items (exact: a segment is a split).  The
        arguments are checked on the host before anything runs."""
        if exclude is not None:
            exclude = exclude.detach().cpu().tolist() if torch.is_tensor(exclude) else list(exclude)
            if len(exclude) != len(queries):
                raise ValueError(f"{len(exclude)} exclude ids for {len(queries)} queries")
        codes, table, n_ids = self._item_codes()
        if distinct and k > min(128, n_ids):
            raise ValueError(f"k={k} must be in [1, min(128, {n_ids} different ids)] with distinct=True")
        if exclude is None:
            return codes, None
        if table is None:                          # no ids: the id of a row is its position
            return codes, [x if isinstance(x, int) and 0 <= x < self._n else -1 for x in exclude]
        return codes, [-1 if x is None else table.get(x, -1) for x in exclude]

    def astype(self, storage: str) -> "EmbeddingIndex":
        """A new index with the same segment boundaries and ids in the other storage: fp32 -> bf16 rounds the stored rows (to nearest even), bf16 -> fp32
        widens them exactly."""
        out = EmbeddingIndex(self.dim, device=self.device, normalize=self.normalize, storage=storage)
        out.segments = [s.to(self.STORAGES[storage], copy=True) for s in self.segments]
        out.ids = None if self.ids is None else list(self.ids)
        out._n = self._n
        return out

    def state_dict(self) -> dict:
        """Plain host values only (numbers, lists, None, host tensors).  "feats" holds the rows in their storage type (a bf16 tensor for a bf16 index: half
        the file); "storage" names it by its width in bits, 32 or 16; "shadow": True is there only for an index with shadow rows."""
        feats = torch.cat(self.segments, 0).cpu() if self.segments else torch.zeros(0, self.dim, dtype=self.STORAGES[self.storage])
        sd = {"dim": self.dim, "normalize": self.normalize, "storage": self.STORAGE_BITS[self.storage], "feats": feats, "segment_rows": [s.shape[0] for s in self.segments],
              "ids": None if self.ids is None else list(self.ids)}
        if self.shadow:
            sd["shadow"] = True                    # the shadow rows are not written: from_state_dict rounds them again
        return sd

    @classmethod
    def from_state_dict(cls, sd: dict, device=None) -> "EmbeddingIndex":
        """Rebuilds the same segments from the stored rows (already normalised when the index normalises: they are not normalised again).  A dict without
        a "storage" key was written before bf16 storage existed: fp32; one without a "shadow" key has none."""
        bits = sd.get("storage", 32)
        names = {b: name for name, b in cls.STORAGE_BITS.items()}
        if bits not in names:
            raise ValueError(f"state dict storage={bits!r} must be one of {sorted(names)} (bits per element)")
        index = cls(sd["dim"], device=device, normalize=sd["normalize"], storage=names[bits], shadow=bool(sd.get("shadow", False)))
        dev = index._device()
        at = 0
        for n in sd["segment_rows"]:
            index.segments.append(sd["feats"][at:at + n].to(dev, cls.STORAGES[index.storage]).contiguous())
            if index.shadow:
                index._add_shadow(index.segments[-1])
            at += n
        index._n = at
        index.ids = None if sd["ids"] is None else list(sd["ids"])
        return index

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


class EmbeddingIndex:
    """A gallery of embeddings on the device and the answer to "which k stored items are nearest to this query?" (sc_search_topk: fused fp32
    similarity + top-k, no [Q, N] score image).  Rows are kept as fp32 SEGMENTS, one per `add`; adding never reallocates earlier segments.  A search runs
    every segment with its starting position as idx_base and joins the partial lists with sc_topk_merge; because the score is a fixed fmaf chain per
    (query, row) and ties go to the lower position, the result equals, bit for bit, a search of ONE segment holding the concatenation.
    storage="bf16" (dim % 16 == 0) keeps the rows in bf16 instead: rows and queries are normalised in fp32 as before and then rounded to bf16 (round to
    nearest even), and sc_search_topk_bf16 forms the scores -- exact bf16 products summed in fp32, returned as fp32; half the bytes per row, the same
    segments, positions, ids and merge, and the same one-segment equality.  The default stays fp32.
    There is no host implementation: without the library's GPU `add` / `search` raise SpeechClipHipError, like mutualRetrieval."""

    STORAGES = {"fp32": torch.float32, "bf16": torch.bfloat16}
    STORAGE_BITS = {"fp32": 32, "bf16": 16}            # how state_dict names the storage

    def __init__(self, dim: int, device=None, normalize: bool = True, storage: str = "fp32"):
        if storage not in self.STORAGES:
            raise ValueError(f"storage={storage!r} must be one of {sorted(self.STORAGES)}")
        if storage == "bf16" and int(dim) % 16 != 0:
            raise ValueError(f"storage='bf16' needs dim % 16 == 0 (sc_search_topk_bf16), got dim={dim}")
        self.dim, self.normalize, self.storage = int(dim), bool(normalize), storage
        self.device = torch.device(device) if device is not None else None
        self.segments: List[torch.Tensor] = []
        self.ids: Optional[list] = None            # None: the ids are the running positions
        self._n = 0
        self._codes = None                         # item codes of the rows (search with distinct / exclude), derived from ids

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
        self._codes = None
        return self

    def _item_codes(self):
        """-> (one int32 device tensor of item codes per segment, {id: code} or None, number of codes).  Equal ids share a code, assigned in first-seen
        order; without ids the code is the position.  Derived from `ids`, built on first use and dropped by `add`; never stored."""
        if self._codes is None:
            table = None if self.ids is None else {}
            codes = list(range(self._n)) if table is None else [table.setdefault(x, len(table)) for x in self.ids]
            segs, at = [], 0
            for seg in self.segments:
                segs.append(torch.tensor(codes[at:at + seg.shape[0]], dtype=torch.int32, device=seg.device))
                at += seg.shape[0]
            self._codes = (segs, table, self._n if table is None else len(table))
        return self._codes

    def search(self, queries: torch.Tensor, k: int, distinct: bool = False, exclude: Optional[Sequence[Hashable]] = None):
        """-> (scores f32 [Q, k] descending, positions i64 [Q, k], ids): ids[i][r] is the stored id of positions[i, r] (the position itself without ids).
        distinct=True: the k nearest DIFFERENT ids, each by its best row (rows that share an id are one item; k <= the number of different ids).
        exclude: one id per query (a sequence of len(queries)); rows carrying it are left out of that query's result -- None, or an id the index does not
        hold, leaves out nothing.  With both defaults this is the plain search (sc_search_topk); otherwise sc_search_items, same scores and order."""
        from .. import ops
        k = int(k)
        dev = self._device()
        if not 1 <= k <= min(128, max(self._n, 1)) or self._n == 0:
            raise ValueError(f"k={k} must be in [1, min(128, {self._n} stored rows)]")
        distinct, by_item = bool(distinct), bool(distinct) or exclude is not None
        codes, skip = self._item_arguments(queries, k, distinct, exclude) if by_item else ([None] * len(self.segments), None)
        q = self._rows(queries)
        if skip is not None:
            skip = torch.tensor(skip, dtype=torch.int32, device=dev)
        bf16 = self.storage == "bf16"
        search_topk, search_items = (ops.search_topk_bf16, ops.search_items_bf16) if bf16 else (ops.search_topk, ops.search_items)
        parts, base = [], 0
        for seg, code in zip(self.segments, codes):
            kk = min(k, seg.shape[0])
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
        return scores, pos, self._ids_of(pos)

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
        the file); "storage" names it by its width in bits, 32 or 16."""
        feats = torch.cat(self.segments, 0).cpu() if self.segments else torch.zeros(0, self.dim, dtype=self.STORAGES[self.storage])
        return {"dim": self.dim, "normalize": self.normalize, "storage": self.STORAGE_BITS[self.storage], "feats": feats, "segment_rows": [s.shape[0] for s in self.segments],
                "ids": None if self.ids is None else list(self.ids)}

    @classmethod
    def from_state_dict(cls, sd: dict, device=None) -> "EmbeddingIndex":
        """Rebuilds the same segments from the stored rows (already normalised when the index normalises: they are not normalised again).  A dict without
        a "storage" key was written before bf16 storage existed: fp32."""
        bits = sd.get("storage", 32)
        names = {b: name for name, b in cls.STORAGE_BITS.items()}
        if bits not in names:
            raise ValueError(f"state dict storage={bits!r} must be one of {sorted(names)} (bits per element)")
        index = cls(sd["dim"], device=device, normalize=sd["normalize"], storage=names[bits])
        dev = index._device()
        at = 0
        for n in sd["segment_rows"]:
            index.segments.append(sd["feats"][at:at + n].to(dev, cls.STORAGES[index.storage]).contiguous())
            at += n
        index._n = at
        index.ids = None if sd["ids"] is None else list(sd["ids"])
        return index

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
        return self

    def search(self, queries: torch.Tensor, k: int):
        """-> (scores f32 [Q, k] descending, positions i64 [Q, k], ids): ids[i][r] is the stored id of positions[i, r] (the position itself without ids)."""
        from .. import ops
        k = int(k)
        dev = self._device()
        if not 1 <= k <= min(128, max(self._n, 1)) or self._n == 0:
            raise ValueError(f"k={k} must be in [1, min(128, {self._n} stored rows)]")
        q = self._rows(queries)
        search_topk = ops.search_topk_bf16 if self.storage == "bf16" else ops.search_topk
        parts_v, parts_i, base = [], [], 0
        for seg in self.segments:
            kk = min(k, seg.shape[0])
            v, i = search_topk(q, seg, kk, idx_base=base)
            if kk < k:                             # a segment shorter than k: its list is padded with entries that take no part in the merge
                v = torch.cat([v, torch.full((q.shape[0], k - kk), float("-inf"), device=dev)], 1)
                i = torch.cat([i, torch.full((q.shape[0], k - kk), -1, device=dev, dtype=torch.int64)], 1)
            parts_v.append(v), parts_i.append(i)
            base += seg.shape[0]
        if len(parts_v) == 1:
            scores, pos = parts_v[0], parts_i[0]
        else:
            scores, pos = ops.topk_merge(torch.cat(parts_v, 1), torch.cat(parts_i, 1), k)
        host = pos.cpu().tolist()
        ids = host if self.ids is None else [[self.ids[p] if p >= 0 else None for p in row] for row in host]
        return scores, pos, ids

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

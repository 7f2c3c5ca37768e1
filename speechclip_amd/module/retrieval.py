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
    There is no host implementation: without the library's GPU `add` / `search` raise SpeechClipHipError, like mutualRetrieval."""

    def __init__(self, dim: int, device=None, normalize: bool = True):
        self.dim, self.normalize = int(dim), bool(normalize)
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
        return ops.l2norm(rows) if self.normalize and rows.shape[0] else rows

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
        parts_v, parts_i, base = [], [], 0
        for seg in self.segments:
            kk = min(k, seg.shape[0])
            v, i = ops.search_topk(q, seg, kk, idx_base=base)
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

    def state_dict(self) -> dict:
        feats = torch.cat(self.segments, 0).cpu() if self.segments else torch.zeros(0, self.dim)
        return {"dim": self.dim, "normalize": self.normalize, "feats": feats, "segment_rows": [s.shape[0] for s in self.segments],
                "ids": None if self.ids is None else list(self.ids)}

    @classmethod
    def from_state_dict(cls, sd: dict, device=None) -> "EmbeddingIndex":
        """Rebuilds the same segments from the stored rows (already normalised when the index normalises: they are not normalised again)."""
        index = cls(sd["dim"], device=device, normalize=sd["normalize"])
        dev = index._device()
        at = 0
        for n in sd["segment_rows"]:
            index.segments.append(sd["feats"][at:at + n].to(dev, torch.float32).contiguous())
            at += n
        index._n = at
        index.ids = None if sd["ids"] is None else list(sd["ids"])
        return index

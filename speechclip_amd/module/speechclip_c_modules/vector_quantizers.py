"""SimpleVectorQuantizer (avssl/module/speechclip_c_modules/my_vector_quantizer.py:12-165) on HIP:
special-token masking, arg-max one-hot, code/prob perplexities and per-keyword entropy in one pass over the
[B*K, V] score matrix (sc_vq_fwd).  `subword_prob` is returned lazily (a dense image is only materialised if read).
Train mode knows all four `use_gumbel` x `hard` settings (:124-139); with y = softmax((x + g) / T), g = Gumbel noise or 0:
  hard, no gumbel (shipped)  subword_prob = one-hot(argmax x), gradient through softmax(x / T)   (train_tail.KeywordSTFn)
  soft (hard: false)         subword_prob = y (g = 0), keywords = y @ E                          (train_tail.KeywordVQFn, sc_vq_soft_embed)
  gumbel hard                subword_prob = one-hot(argmax(x + g)), gradient through y
  gumbel soft                subword_prob = y, keywords = y @ E
The statistics are always those of the noise-free x (:82-121); eval returns the hard one-hot in every mode (:138-139).  The noise is a function of
(vq_results["gumbel_seed"], row * V + column) -- the contract is in include/speechclip_hip.h -- so nothing of size [B*K, V] is stored for the backward."""
import ast

import torch
import torch.nn as nn

from ... import ops

__all__ = ["SimpleVectorQuantizer"]


class _LazyOneHot(dict):
    """vq_results dict whose 'subword_prob' ([B,K,V] one-hot) is built on first access."""

    def __missing__(self, key):
        if key == "subword_prob":
            t = self["targets"]
            B, K, _ = t.shape
            v = torch.zeros(B, K, self["num_vars"], device=t.device, dtype=torch.float32).scatter_(-1, t, 1.0)
            self[key] = v
            return v
        raise KeyError(key)


class _LazyModeProb(_LazyOneHot):
    """vq_results of the soft / gumbel train modes: 'subword_prob' is y = softmax((x + g) / T) (sc_vq_probs) for the soft modes and the one-hot of
    the noisy target for gumbel hard, built on first access.  'vq_mode' = (soft, scores [B*K, V], mask ids) is what `embed` and the branch dispatch on."""

    def __missing__(self, key):
        if key == "subword_prob" and self["vq_mode"][0]:
            _, scores, mask_ids = self["vq_mode"]
            B, K, _ = self["targets"].shape
            v = ops.vq_probs(scores, self["temp"], self["gumbel_seed"], mask_ids).view(B, K, self["num_vars"])
            self[key] = v
            return v
        return super().__missing__(key)


class SimpleVectorQuantizer(nn.Module):
    def __init__(self, temp, groundTruthPerplexity=None, time_first=True, use_gumbel=False, hard=True):
        super().__init__()
        if not time_first:
            raise NotImplementedError("time_first=False is not built: the cascaded branch always hands over [B, K, V] scores, so the reference's "
                                      "transpose (my_vector_quantizer.py:66-67) has no meaning in this model")
        self.time_first, self.use_gumbel, self.hard = time_first, bool(use_gumbel), bool(hard)
        if isinstance(temp, str) and temp.startswith("learnable="):
            self.temp_type = "learnable"
            self.curr_temp = nn.parameter.Parameter(torch.FloatTensor([ast.literal_eval(temp.replace("learnable=", ""))]))
        elif isinstance(temp, str) and temp.startswith("fixed="):
            self.temp_type = "fixed"
            self.register_buffer("curr_temp", torch.FloatTensor([ast.literal_eval(temp.replace("fixed=", ""))]))
            self._fixed_temp = float(ast.literal_eval(temp.replace("fixed=", "")))   # host copy: reading the buffer would sync the stream every step
        else:      # "(max, min, decay)": scheduled (my_vector_quantizer.py:45-52); nothing in the reference calls set_num_updates, so it stays at max
            self.temp_type = "scheduled"
            t3 = ast.literal_eval(temp) if isinstance(temp, str) else tuple(temp)
            assert len(t3) == 3, f"{t3}, {len(t3)}"
            self.max_temp, self.min_temp, self.temp_decay = t3
            self.curr_temp = self.max_temp
        self.groundTruthPerplexity = None if groundTruthPerplexity is None else float(groundTruthPerplexity)
        if self.temp_type == "fixed":   # a checkpoint may carry another value in the buffer: refresh the host copy once, at load time
            self.register_load_state_dict_post_hook(lambda mod, keys: setattr(mod, "_fixed_temp", float(mod.curr_temp.detach().cpu().item())))

    def set_num_updates(self, num_updates):
        if self.temp_type == "scheduled":       # my_vector_quantizer.py:58-62
            self.curr_temp = max(self.max_temp * self.temp_decay ** num_updates, self.min_temp)

    def temperature_value(self) -> float:
        if self.temp_type == "fixed":
            return self._fixed_temp
        return float(self.curr_temp) if self.temp_type == "scheduled" else float(self.curr_temp.item())

    def forward(self, x, prob_msk=[0, 2, 3], produce_targets=True):
        # The statistics and, in the shipped mode, the targets come from the noise-free x in one pass (sc_vq_fwd).  Train mode, shipped setting: hard targets, the
        # straight-through gradient softmax(x / temp) (:133-141) is applied where the sub-word embeddings are formed (train_tail.KeywordSTFn via KW_CascadedBranch).
        # Train mode, soft / gumbel settings: noisy targets, a lazy `subword_prob` and res["vq_mode"], on which `embed` and the branch (train_tail.KeywordVQFn)
        # dispatch.  A learnable temperature (`temp: "learnable=..."`) gets its gradient there in every setting.
        B, K, V = x.shape
        targets, stats, ent = ops.vq_fwd(x.reshape(B * K, V), K, prob_msk)
        new_mode = self.training and (self.use_gumbel or not self.hard)
        res = _LazyModeProb() if new_mode else _LazyOneHot()
        res["num_vars"] = V
        res["code_perplexity"] = stats[0]
        res["prob_perplexity"] = stats[1]
        res["ent_per_t"] = ent
        res["temp"] = self.temperature_value()
        if self.groundTruthPerplexity is not None:      # my_vector_quantizer.py:147-154 (MSELoss of two scalars)
            res["diversity_loss"] = (stats[1] - self.groundTruthPerplexity) ** 2 / (V - self.groundTruthPerplexity) ** 2
        else:
            res["diversity_loss"] = (V - stats[1]) / V
        res["gumbel_seed"] = 0
        if new_mode:
            scores = x.reshape(B * K, V)
            scores = scores if (scores.dtype == torch.float32 and scores.is_contiguous()) else scores.float().contiguous()
            if self.use_gumbel:     # drawn as the branch draws its dropout seed (host generator: no stream sync); never 0, which means "no noise"
                res["gumbel_seed"] = int(torch.randint(1, 2 ** 31 - 8, (1,)).item())
                targets = ops.vq_noisy_argmax(scores, res["gumbel_seed"], tuple(prob_msk))
            res["vq_mode"] = (not self.hard, scores, tuple(int(i) for i in prob_msk))
        res["targets"] = targets.view(B, K, 1)
        return res

    @staticmethod
    def embed(vq_results, emb_weight):
        """subword_prob @ E (kwClip.py:909): a gather of the chosen rows for a hard one-hot, the fused softmax @ E (sc_vq_soft_embed) for the soft train modes."""
        t = vq_results["targets"]
        B, K, _ = t.shape
        mode = dict.get(vq_results, "vq_mode")
        if mode is not None and mode[0]:
            return ops.vq_soft_embed(mode[1], emb_weight, vq_results["temp"], vq_results["gumbel_seed"], mode[2]).view(B, K, emb_weight.shape[1])
        return ops.gather_rows(emb_weight, t.reshape(-1)).view(B, K, emb_weight.shape[1])

"""ClipModel -- the reference's CLIP wrapper (avssl/module/clip_official.py:26-294) over the MI355X CLIP engine.

Same constructor arguments and attributes (`model`, `out_dim`, `tokenizer`, `device`, reduced sub-word vocabulary,
`encode_image`, `encode_text`, `encode_keywords`, `update_device`, `trainable_params`).  openai `clip` is not
required: `self.model` is a parameter tree with openai's key names (clip_model.CLIP) whose towers run on HIP kernels.
No network: weights are loaded only from a local state_dict ($SPEECHCLIP_CLIP_CKPT), else random init.
"""
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from .clip_model import CLIP, ClipConfig

logger = logging.getLogger(__name__)
_clip_models = {"RN50", "RN101", "RN50x4", "RN50x16", "RN50x64", "ViT-B/32", "ViT-B/16", "ViT-L/14"}
SOT_ID, EOT_ID = 49406, 49407
# What SC_TEXT_PACK=auto does: True = pack when that removes at least 10 % of the rows.  tools/text_tower_bench.py measured the packed text tower faster than
# the padded one in 3 of 3 interleaved passes (5000 captions of 6 .. 30 rows and one of 77, ViT-B/32: 10.5 ms against 41.5 ms, profiles/text_tower_bench.txt).
# False would keep `auto` on the padded path; SC_TEXT_PACK=1 / 0 decide regardless.
_TEXT_PACK_AUTO = True
# What SC_IMAGE_PREP=auto does for a model on a GPU: True = resize + centre crop on the device (sc_image_prep_u8).  tools/image_prep_bench.py measured the device
# arm faster than the PIL arm in 3 of 3 interleaved passes on both legs (256 images of 500 x 375 / 375 x 500: PNG files 664 ms against 898 ms per call, decoded
# arrays 10.5 ms against 301 ms; profiles/image_prep_bench.txt).  The two arms give equal bits; SC_IMAGE_PREP=host / device decide regardless.
_IMAGE_PREP_AUTO_DEVICE = True


class _IdDecoder(dict):
    """decoder[i] of the id-literal tokenizer: "<i></w>" for every id."""

    def __missing__(self, i):
        return "<{}></w>".format(int(i))


class _TokenizerIds:
    """Stand-in for openai's SimpleTokenizer (clip/simple_tokenizer.py [3P], not installed and its BPE vocabulary file is not
    available offline).  The hot path needs two ids (clip_official.py:95-101,235-240); the analysis surface (kwClip.py:277-466,
    :918-1001) needs `decoder[id]`, `decode(ids)` and `encode(text)`.  Without the vocabulary, sub-word i prints as the literal "<i>":
    decode / encode are exact inverses of each other on id lists, so hit rates and neighbour lists are computed on the true token ids and
    only their printed form differs.  Assign a real SimpleTokenizer-compatible object to `ClipModel.tokenizer` to get words."""

    def __init__(self, vocab_size=49408):
        self.encoder = {"<|startoftext|>": vocab_size - 2, "<|endoftext|>": vocab_size - 1}
        self.decoder = _IdDecoder()

    def decode(self, tokens) -> str:
        return "".join(self.decoder[t] for t in tokens).replace("</w>", " ")

    def encode(self, text: str) -> list:
        return [int(w[1:-1]) for w in text.split() if w.startswith("<") and w.endswith(">") and w[1:-1].isdigit()]


class ClipModel(nn.Module):
    """The reference's ClipModel surface: encode_image / encode_text / encode_keywords / prep_image / prep_text / deTokenize / get_scores.
    NOT built: `encode_subword` -- in the reference (clip_official.py:266-277) it calls `self.encode_subword_prob`, a method that exists nowhere,
    so it cannot run there either and there is nothing to restate."""

    def __init__(self, name: str, device: str = "cpu", image_encoder_trainable: bool = False, text_encoder_trainable: bool = False,
                 reduce_subword_embbedding: str = None, clip_config: ClipConfig = None, **kwargs):
        super().__init__()
        assert name in _clip_models
        if text_encoder_trainable:
            raise NotImplementedError("text_encoder_trainable: fine-tuning the CLIP text tower is not built on the MI355X path (its backward yields the "
                                      "gradient of the input embeddings only); the image tower trains with image_encoder_trainable")
        self.name, self.device = name, device
        if clip_config is not None and not isinstance(clip_config, ClipConfig):
            clip_config = ClipConfig(**dict(clip_config.to_dict() if hasattr(clip_config, "to_dict") else clip_config))
        cfg = clip_config if clip_config is not None else ClipConfig.from_name(name)
        ckpt = os.environ.get("SPEECHCLIP_CLIP_CKPT", "")
        ckpt_sd = None
        if ckpt and os.path.isfile(ckpt):
            # clip_official.py:50 `clip.load(name, device)`: openai's files are TorchScript archives; read without the `clip` package, fp16 -> fp32 as
            # clip.load does on the CPU, architecture derived from the tensor shapes as clip.model.build_model does -- and it must be the NAMED one
            from ..util.checkpoint_io import clip_config_from_state_dict, load_clip_state_dict
            ckpt_sd = load_clip_state_dict(ckpt)
            file_cfg = clip_config_from_state_dict(ckpt_sd)
            if file_cfg != cfg:
                raise ValueError(f"{ckpt} holds {file_cfg}, but clip.name = {name!r} is {cfg}")
        elif ckpt:
            raise FileNotFoundError(f"SPEECHCLIP_CLIP_CKPT={ckpt} does not exist")
        self.model = CLIP(cfg)
        if ckpt_sd is not None:
            from ..util.checkpoint_io import CLIP_NON_WEIGHT_KEYS, strict_load
            strict_load(self.model, ckpt_sd, allow_unexpected=CLIP_NON_WEIGHT_KEYS, what=f"CLIP checkpoint {ckpt}")
        self.image_encoder_trainable, self.text_encoder_trainable = image_encoder_trainable, text_encoder_trainable
        self.out_dim = self.model.transformer.width
        from ..data.image_transforms import clip_preprocess
        self.image_preprocess = clip_preprocess(cfg.image_resolution)        # clip_official.py:50: the `preprocess` clip.load returns
        self.tokenizer = _TokenizerIds(cfg.vocab_size)
        for p in self.model.parameters():
            p.requires_grad = False
        if image_encoder_trainable:          # clip_official.py `freeze_models`: model.visual stays trainable, everything else is frozen
            for p in self.model.visual.parameters():
                p.requires_grad = True
        self.selected_text_emb_ids = None
        if reduce_subword_embbedding is not None:
            if not os.path.exists(reduce_subword_embbedding):
                raise FileNotFoundError(reduce_subword_embbedding)
            data = np.load(reduce_subword_embbedding)
            self.selected_text_emb_ids = data[:, 0]
            dist = data[:, 1]
            self.selected_text_emb_ids_dist = torch.from_numpy(dist / np.sum(dist))
            self.original_text_emb_weight = self.model.token_embedding.weight
            reduced = self.model.token_embedding.weight[torch.as_tensor(self.selected_text_emb_ids, dtype=torch.long)]
            self.model.token_embedding = nn.Embedding.from_pretrained(reduced.detach().clone())
            self.model.token_embedding.weight.requires_grad = False
            self.original2Reduced = {int(o): n for n, o in enumerate(self.selected_text_emb_ids)}
            self.reducedl2Original = {n: int(o) for n, o in enumerate(self.selected_text_emb_ids)}
            self.startOfTxt_reduced = self.original2Reduced[self.tokenizer.encoder["<|startoftext|>"]]
            self.endOfTxt_reduced = self.original2Reduced[self.tokenizer.encoder["<|endoftext|>"]]

    def trainable_params(self) -> list:
        return list(self.model.visual.parameters()) if self.image_encoder_trainable else []

    def update_device(self, device):
        self.device = device

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        self.device = self.model.token_embedding.weight.device
        return self

    def prep_image(self, paths: list) -> torch.Tensor:
        """clip_official.py:151-164: image files -> pre-processed tensor [B, 3, H, W] on self.device.  PIL open + bicubic resize + centre crop on the
        host (data/image_transforms.py), then the batch goes to the device as uint8 and is scaled / normalised there (sc_image_normalize_u8).
        SC_IMAGE_PREP (read at every call) chooses where the geometry runs: `host` = the PIL path above; `device` = decode only on the host
        (load_images_raw), resize + crop + normalise on the device (ops.image_prep) when the model lives on a GPU, the host path for a CPU model; `auto`
        (the default) = `device`, which is what the measurement decided (faster in 3 of 3 passes on files and on decoded arrays: README,
        profiles/image_prep_bench.txt).  The two paths give equal bits, so the choice cannot change a result."""
        from ..data.image_transforms import load_images_raw, load_images_u8, normalize_u8
        n_px = self.model.cfg.image_resolution
        if self._image_prep_on_device():
            return self.prep_image_arrays(load_images_raw(paths, n_px))
        return normalize_u8(load_images_u8(paths, n_px), self.device)

    def _image_prep_on_device(self) -> bool:
        mode = os.environ.get("SC_IMAGE_PREP", "auto")
        if mode not in ("host", "device", "auto"):
            raise ValueError(f"SC_IMAGE_PREP={mode!r}: expected host, device or auto")
        return (mode == "device" or (mode == "auto" and _IMAGE_PREP_AUTO_DEVICE)) and torch.device(self.device).type == "cuda"

    def prep_image_arrays(self, images: list) -> torch.Tensor:
        """Decoded frames (uint8 [h, w, 3] RGB or [h, w] L arrays / host tensors, sizes may differ: a DataLoader worker's arrays, video frames) ->
        pre-processed tensor [B, 3, n_px, n_px] on self.device, equal bit for bit to prep_image of the same pictures.  SC_IMAGE_PREP chooses as in
        prep_image: the geometry on the device (ops.image_prep), or PIL on the arrays and the normalisation on the device."""
        from ..data.image_transforms import as_u8_image, clip_resize_center_crop_u8, normalize_u8
        n_px = self.model.cfg.image_resolution
        if self._image_prep_on_device():
            from .. import ops
            with torch.cuda.device(torch.device(self.device)):          # "cuda" without an index (the reference's constructor form) = the current device
                return ops.image_prep(images, n_px)
        from PIL import Image
        crops = [clip_resize_center_crop_u8(Image.fromarray(as_u8_image(im)), n_px) for im in images]
        return normalize_u8(torch.from_numpy(np.stack(crops)) if crops else torch.empty(0, n_px, n_px, 3, dtype=torch.uint8), self.device)

    def encode_image(self, image: torch.Tensor) -> torch.Tensor:
        if self.image_encoder_trainable and torch.is_grad_enabled():
            return self.model.encode_image_train(image)          # differentiable: train_vit.ImageTowerTrainFn
        return self.model.encode_image(image)

    def _special_ids(self):
        if self.selected_text_emb_ids is None:
            return self.tokenizer.encoder["<|startoftext|>"], self.tokenizer.encoder["<|endoftext|>"]
        return self.startOfTxt_reduced, self.endOfTxt_reduced

    # ---- text surface (clip_official.py:166-198, 279-289) ------------------------------------------------------------------------------
    def _to_reduced(self, i: int) -> int:
        try:
            return self.original2Reduced[int(i)]
        except KeyError:
            raise KeyError(f"token id {int(i)} is not in the reduced vocabulary ({len(self.original2Reduced)} ids)") from None

    def prep_text(self, sents: list) -> torch.Tensor:
        """clip_official.py:166-180 (`clip.tokenize` restated): sentence -> [SOT] + tokenizer.encode(s) + [EOT], zero padded to context_length; int64
        [B, context_length] on the CPU.  A sentence that does not fit raises RuntimeError.  With a reduced vocabulary every id (the padding id 0 too, as
        in the reference) is mapped through original2Reduced ONCE; an id outside it raises KeyError.  Works with any tokenizer object that has `encode`
        and `encoder["<|startoftext|>"]` / `["<|endoftext|>"]`; the built-in one reads id literals ("<320> <1125>")."""
        if isinstance(sents, str):
            sents = [sents]
        sot, eot = self.tokenizer.encoder["<|startoftext|>"], self.tokenizer.encoder["<|endoftext|>"]
        L = self.model.context_length
        reduced = self.selected_text_emb_ids is not None
        out = torch.full((len(sents), L), self._to_reduced(0) if reduced else 0, dtype=torch.long)
        for i, s in enumerate(sents):
            toks = [sot] + [int(t) for t in self.tokenizer.encode(s)] + [eot]
            if len(toks) > L:
                raise RuntimeError(f"Input {s!r} is too long for context length {L}: {len(toks)} tokens with <|startoftext|> and <|endoftext|>")
            if reduced:
                toks = [self._to_reduced(t) for t in toks]
            out[i, :len(toks)] = torch.tensor(toks, dtype=torch.long)
        return out

    def map_to_reduced(self, text: torch.Tensor) -> torch.Tensor:
        """ORIGINAL ids -> reduced ids by one lookup-table gather (what kwClip.py:538-544 does with a Python double loop); a new tensor, same device.
        An id outside the reduced vocabulary raises KeyError naming it."""
        lut = getattr(self, "_orig2reduced_lut", None)
        if lut is None:
            n = max(int(max(self.original2Reduced)) + 1, int(self.original_text_emb_weight.shape[0]))
            lut = torch.full((n,), -1, dtype=torch.long)
            lut[torch.as_tensor(self.selected_text_emb_ids, dtype=torch.long)] = torch.arange(len(self.selected_text_emb_ids))
            self._orig2reduced_lut = lut
        t = text.long()
        inside = (t >= 0) & (t < lut.numel())
        out = lut.to(t.device)[t.clamp(0, lut.numel() - 1)]
        bad = ~inside | (out < 0)
        if bool(bad.any()):
            raise KeyError(f"token id {int(t[bad][0])} is not in the reduced vocabulary ({len(self.original2Reduced)} ids)")
        return out

    def deTokenize(self, sents) -> list:
        """clip_official.py:182-198: id rows -> strings without the start / end markers.  Differences, both deliberate: the caller's list is NOT mapped
        in place (the reference overwrites it with original ids), and a row is cut at its first <|endoftext|> (the reference decodes the zero padding
        behind it too, "!" for every pad position of the real vocabulary)."""
        if isinstance(sents, torch.Tensor):
            sents = sents.view(*sents.shape[:2]).tolist()
        sot, eot = self.tokenizer.encoder["<|startoftext|>"], self.tokenizer.encoder["<|endoftext|>"]
        res = []
        for sent in sents:
            ids = [int(t) for t in sent]
            if self.selected_text_emb_ids is not None:
                ids = [self.reducedl2Original[t] for t in ids]
            if eot in ids:
                ids = ids[:ids.index(eot)]
            ids = [t for t in ids if t != sot]
            res.append(self.tokenizer.decode(ids).replace("<|startoftext|>", "").replace("<|endoftext|>", "").strip())
        return res

    def get_scores(self, image: torch.Tensor, text: torch.Tensor) -> tuple:
        """clip_official.py:279-289 (CLIP.forward): (logits_per_image [B_image, B_text], logits_per_text = its transpose), fp32,
        exp(logit_scale) * l2(encode_image(image)) @ l2(encode_text(text)).T on the device (sc_l2norm_fwd, sc_sgemm)."""
        from .. import ops
        with torch.no_grad():
            img = ops.l2norm(self.encode_image(image).detach().float().contiguous())
            txt = ops.l2norm(self.encode_text(text).detach().float().contiguous())
            logits_per_image = ops.sgemm(img, txt, transb=True, alpha=float(self.model.logit_scale.detach().exp()))
        return logits_per_image, logits_per_image.t()

    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        """text: [B, L <= 77] token ids (reduced ids if the vocabulary is reduced).  EOT = arg-max id position.
        SC_TEXT_PACK = 0: every caption runs at the batch's full length L (the padded path); 1: packed rows (CLIP.encode_text_ids: positions behind a
        caption's EOT are not computed) whenever the text heads have head_dim 64; auto (default): packed when that removes at least 10 % of the rows
        AND the packed path has been measured faster (_TEXT_PACK_AUTO, profiles/text_tower_bench.txt), else padded."""
        mode = os.environ.get("SC_TEXT_PACK", "auto")
        m = self.model
        if mode != "0" and m.cfg.text_width == 64 * m.transformer.heads and m.token_embedding.weight.is_cuda:
            if mode == "1":
                return m.encode_text_ids(text)
            if _TEXT_PACK_AUTO and mode == "auto":
                plan = m.text_pack_plan(text)
                if plan["total"] <= 0.9 * plan["B"] * plan["L"]:
                    return m.encode_text_ids(text, plan)
        emb = self.model.token_embedding(text)
        return self.model.encode_text_embeddings(emb, text.argmax(dim=-1))

    def encode_keywords(self, keywords: torch.Tensor, keyword_num: int) -> torch.Tensor:
        """clip_official.py:220-264: [SOT, kw_1..kw_K, EOT, pad...] through the text tower, feature at position K+1.
        The causal mask makes positions > K+1 irrelevant, so only K+2 positions are evaluated."""
        if not isinstance(keywords, torch.Tensor):
            raise TypeError(f"Unknown keywords type {type(keywords)}")
        B, dev = keywords.size(0), keywords.device
        sot, eot = self._special_ids()
        tok = self.model.token_embedding.weight
        emb = torch.empty(B, keyword_num + 2, tok.shape[1], device=dev, dtype=torch.float32)
        emb[:, 0] = tok[sot]
        emb[:, 1:1 + keyword_num] = keywords
        emb[:, 1 + keyword_num] = tok[eot]
        return self.model.encode_text_embeddings(emb, keyword_num + 1)       # one EOT position for the batch: a host int, no gather / sync

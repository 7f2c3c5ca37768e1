"""No GPU: the text surface (ClipModel.prep_text / deTokenize / map_to_reduced, KWClipBase.forward_text's id handling) and the two C entries of the packed
text tower in header, library and ctypes table, with their argument errors (negative code, message, no launch: this machine has no device to launch on)."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_text_embed_packed", "sc_attention_fwd_text")
V, SOT, EOT = 512, 510, 511          # ClipRefConfig.tiny(): vocab 512, the id-literal tokenizer puts SOT / EOT at V - 2 / V - 1


def tiny_clip(**kw):
    from oracle.clip_ref import ClipRefConfig
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.clip_official import ClipModel
    return ClipModel("ViT-B/32", clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())), **kw)


def reduced_table(tmp_path, ids):
    path = os.path.join(str(tmp_path), "reduced_ids.npy")
    np.save(path, np.stack([np.asarray(ids, dtype=np.int64), np.arange(1, len(ids) + 1, dtype=np.int64)], axis=1))
    return path


def sent(ids):
    return " ".join(f"<{i}>" for i in ids)


# ------------------------------------------------------------------------------------------------ C entries
def test_new_entries_are_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    L = _lib.lib()
    declared = _lib.exported_symbols()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    for n in NAMES:
        assert n in declared and hasattr(L, n), n
        params = re.search(rf"^int(?:64_t)? {n}\s*\(([^)]*)\)", text, re.M).group(1)
        assert len(getattr(L, n).argtypes) == len([p for p in params.split(",") if p.strip()]), n
        assert getattr(L, n).restype is ctypes.c_int
    assert "#define SC_ATTN_TEXT_GENERAL 0x100" in text and _lib.ATTN_TEXT_GENERAL == 0x100
    assert L.sc_abi_version() == 1


def test_argument_errors_are_codes_with_a_message_and_no_launch():
    from speechclip_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) // 16 * 16 + 16          # an aligned, non-null host address: never dereferenced, every call below returns before a launch

    def attn(head_dim=64, flags=0, row_off=p):
        return L.sc_attention_fwd_text(p, p, p, p, row_off, 2, 1, 16, 20, head_dim, 192, 64, 0.125, flags, None)

    def embed(W=64, row_off=p, L_=77, ctx=77, tok=p):
        return L.sc_text_embed_packed(p, 77, tok, p, row_off, p, 2, L_, 512, ctx, W, 20, None)

    for fn, kw, word in ((attn, dict(head_dim=96), "head_dim=96"), (attn, dict(flags=0x2), "unknown flag bits 0x2"),
                         (attn, dict(flags=0x100 | 0x1), "unknown flag bits 0x101"), (attn, dict(row_off=None), "row_off"), (embed, dict(W=66), "W=66"),
                         (embed, dict(row_off=None), "row_off"), (embed, dict(tok=None), "required"), (embed, dict(L_=78), "L=78")):
        assert fn(**kw) < 0, word
        assert word in L.sc_last_error().decode(), (word, L.sc_last_error())


def test_attention_bounds_are_reproduced_and_reject_the_mutants():
    """tools/text_tower_bounds.py on every case of tests/test_text_tower_gpu.py: the MODEL constants are the computed ones, the references are well-posed, and the
    causal-mask, neighbour-key and double-scale mutants leave the bound (tools/attention_bounds.py's own self-check has its test in test_attention_bounds_cpu.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("text_tower_bounds", os.path.join(ROOT, "tools", "text_tower_bounds.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    models, fail = tool.run(quiet=True)
    assert sorted(models) == sorted(tool.T.CASES) and not fail, fail


# ------------------------------------------------------------------------------------------------ prep_text / deTokenize
def test_prep_text_places_sot_eot_and_pads_with_zeros():
    m = tiny_clip()
    t = m.prep_text([sent([320, 112, 5]), sent([7]), ""])
    assert t.dtype == torch.int64 and tuple(t.shape) == (3, 77) and t.device.type == "cpu"
    assert t[0, :5].tolist() == [SOT, 320, 112, 5, EOT] and int(t[0, 5:].abs().sum()) == 0
    assert t[1, :3].tolist() == [SOT, 7, EOT] and int(t[1, 3:].abs().sum()) == 0
    assert t[2, :2].tolist() == [SOT, EOT] and int(t[2, 2:].abs().sum()) == 0
    assert t.argmax(-1).tolist() == [4, 2, 1]
    assert torch.equal(m.prep_text(sent([7])), t[1:2])          # one string = one sentence, as clip.tokenize


def test_prep_text_length_limit():
    m = tiny_clip()
    t = m.prep_text([sent(range(1, 76))])                        # 75 tokens + SOT + EOT = 77
    assert t[0, 0] == SOT and t[0, 76] == EOT and t[0, 1:76].tolist() == list(range(1, 76))
    long = sent(range(1, 77))
    with pytest.raises(RuntimeError, match="too long for context length 77: 78 tokens") as e:
        m.prep_text([sent([3]), long])
    assert "<76>" in str(e.value)                                # names the sentence


def test_prep_text_works_with_any_tokenizer_object():
    class Words:
        encoder = {"<|startoftext|>": 400, "<|endoftext|>": 401}

        def encode(self, s):
            return [len(w) for w in s.split()]

    m = tiny_clip()
    m.tokenizer = Words()
    assert m.prep_text(["a dog runs"])[0, :6].tolist() == [400, 1, 3, 4, 401, 0]


def test_reduced_vocabulary_maps_once_and_refuses_unknown_ids(tmp_path):
    ids = [0, 5, 7, 112, 320, SOT, EOT]
    m = tiny_clip(reduce_subword_embbedding=reduced_table(tmp_path, ids))
    t = m.prep_text([sent([320, 5]), sent([7, 7, 112])])
    assert t[0, :4].tolist() == [5, 4, 1, 6] and t[1, :5].tolist() == [5, 2, 2, 3, 6]          # positions in `ids`: mapped once, not twice
    assert int(t[0, 4:].abs().sum()) == 0 and t.argmax(-1).tolist() == [3, 4]
    with pytest.raises(KeyError, match="113"):
        m.prep_text([sent([320, 113])])
    assert torch.equal(m.map_to_reduced(torch.tensor([[SOT, 320, EOT, 0]])), torch.tensor([[5, 4, 6, 0]]))
    for bad in (113, 600, -1):
        with pytest.raises(KeyError, match=str(bad)):
            m.map_to_reduced(torch.tensor([[SOT, bad, EOT]]))


def test_detokenize_round_trips_and_leaves_the_callers_list_alone(tmp_path):
    sents = [sent([320, 112, 5]), sent([7]), ""]
    for m in (tiny_clip(), tiny_clip(reduce_subword_embbedding=reduced_table(tmp_path, [0, 5, 7, 112, 320, SOT, EOT]))):
        t = m.prep_text(sents)
        assert m.deTokenize(t) == sents
        assert m.deTokenize(t.view(3, 77, 1)) == sents           # the reference's view(*shape[:2])
        rows = t.tolist()
        keep = [list(r) for r in rows]
        assert m.deTokenize(rows) == sents and rows == keep


# ------------------------------------------------------------------------------------------------ forward_text
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from helpers import make_config
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.hubert import HubertConfig
    kw = dict(d_model=128, branch_heads=4, hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())),
              clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))
    table = reduced_table(tmp_path_factory.mktemp("reduced"), [0, 5, 7, 112, 320, SOT, EOT])
    return KWClip_GeneralTransformer(make_config(**kw)), KWClip_GeneralTransformer(make_config(reduce_vocab=table, **kw))


def test_forward_text_refuses_what_the_reference_refuses(models):
    for m in models:
        with pytest.raises(TypeError, match="Unknown text type"):
            m.forward_text("a string")
        with pytest.raises(ValueError, match="Incorrect text tensor shape"):
            m.forward_text(torch.zeros(2, 77, 1, dtype=torch.long))


def test_forward_text_maps_a_tensor_of_original_ids_once_and_does_not_write_it(models):
    full, red = models
    sents = [sent([320, 5]), sent([7, 7, 112]), sent([])]
    orig = full.clip.prep_text(sents)
    assert torch.equal(full.text_ids(sents), orig) and full.text_ids(orig) is orig          # full vocabulary: ids as given
    keep = orig.clone()
    from_tensor = red.text_ids(orig)
    assert torch.equal(orig, keep)                               # the caller's tensor is unchanged
    assert torch.equal(from_tensor, red.text_ids(sents))         # the list form (mapped by prep_text) gives the same ids
    assert from_tensor[1, :5].tolist() == [5, 2, 2, 3, 6]

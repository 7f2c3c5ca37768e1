"""sc_wave_prep / ops.wave_prep on the device: int16 -> f32, mono mix, polyphase resampling to 16 kHz, crop window and zero padding of a ragged batch.

The case list (wave_prep_cases.py) runs ONCE as one ragged batch inside sentinel guards, with the packed input surrounded and gapped by a pattern that reads
as NaN in f32 and 0x7fff in int16; every test below judges that one result or compares another run with it.  Identity-rate elements and padding are EQUALITY
(bits); a resampled element is judged against the float64 execution of the plan under the bound of tools/wave_prep_bounds.py,
1.005 x K x 2^-24 x sum_k |t_k x_k| (the running-sum error of K fp32 multiply-adds; derivation in the tool)."""
import importlib.util
import os
import wave

import numpy as np
import pytest
import torch

from wave_prep_cases import RATES, cases, clip_samples, clips, references

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096          # sentinel elements in front of and behind the output buffer
GAP = 37              # sentinel elements between the rows: the row stride is Lout + GAP (odd: rows are not 16-byte aligned)
PAD = 64              # bytes of the NaN / 0x7fff pattern around every utterance in the packed input
SENTINEL = 12345.0


def _tool():
    spec = importlib.util.spec_from_file_location("wave_prep_bounds", os.path.join(ROOT, "tools", "wave_prep_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_guarded(cl, starts, lens, Lout=None):
    """ops._wave_prep into a caller-owned buffer with sentinels in front, behind and between the rows -> f32 [B, Lout] on the host."""
    from speechclip_amd import ops
    B = len(cl)
    Lout = max(lens) if Lout is None else Lout
    ld = Lout + GAP
    buf = torch.full((2 * GUARD + B * ld,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + B * ld].view(B, ld)
    out = ops._wave_prep(cl, starts, lens, Lout=Lout, out=view, pad_bytes=PAD)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr() and out.shape == (B, Lout) and out.stride(0) == ld
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + B * ld:] == SENTINEL).all()) and bool((view[:, Lout:] == SENTINEL).all())
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    """The whole case list as one ragged batch: (clips, starts, lens, f32 [B, Lout])."""
    cl = [clips()[i] for (i, _, _) in cases()]
    starts, lens = [s for (_, s, _) in cases()], [n for (_, _, n) in cases()]
    got = _run_guarded(cl, starts, lens)
    got.setflags(write=False)
    return cl, starts, lens, got


def test_identity_bits_resampled_elements_under_the_bound_padding_zero(batch):
    tool = _tool()
    cl, starts, lens, got = batch
    assert np.isfinite(got).all()          # neither the NaN pattern around the utterances nor the sentinels show
    worst, judged, seen = {}, 0, set()
    for b, (i, s, n) in enumerate(cases()):
        y, sabs, K = references()[i]
        row = got[b]
        assert not row[n:].view(np.uint32).any(), (b, "padding is not +0.0")
        if K == 0:
            assert np.array_equal(row[:n].view(np.uint32), y[s:s + n].view(np.uint32)), (b, "identity rate differs")
        else:
            bad, ratio = tool.judge(row[:n], y[s:s + n], sabs[s:s + n], K)
            rate = cl[b][1]
            worst[rate] = max(worst.get(rate, 0.0), ratio)
            judged += n
            assert bad == 0, (b, rate, s, n, bad, ratio)
        seen.add((cl[b][1], cl[b][0].dtype.name, cl[b][0].ndim))
    print(f"sc_wave_prep: {len(cases())} utterances in one batch, {judged} resampled elements judged; worst |err| / bound per rate: "
          + ", ".join(f"{r}: {w:.3f}" for r, w in sorted(worst.items())))
    assert seen == {(r, d, c) for r in RATES for d in ("int16", "float32") for c in (1, 2)} and set(worst) == set(RATES) - {16000}
    assert max(n for (_, _, n) in cases()) > 2 * 2048          # more than two of the kernel's largest segments


def test_one_utterance_per_call_gives_the_bits_of_the_ragged_batch(batch):
    from speechclip_amd import ops
    cl, starts, lens, got = batch
    outs = [ops._wave_prep([cl[b]], [starts[b]], [lens[b]], pad_bytes=PAD) for b in range(len(cl))]
    torch.cuda.synchronize()
    for b, o in enumerate(outs):
        assert o.shape == (1, lens[b]) and np.array_equal(o.cpu().numpy()[0].view(np.uint32), got[b, :lens[b]].view(np.uint32)), b


def test_batch_order_permuted_gives_permuted_rows(batch):
    cl, starts, lens, got = batch
    perm = np.random.default_rng(3).permutation(len(cl))
    again = _run_guarded([cl[p] for p in perm], [starts[p] for p in perm], [lens[p] for p in perm])
    assert np.array_equal(again.view(np.uint32), got[perm].view(np.uint32))


def test_public_form_defaults_and_element_forms(tmp_path):
    """ops.wave_prep: whole utterances by default, Lout = the longest, every element form (array, tensor, pair, path), a wider Lout, empty windows."""
    from speechclip_amd import ops
    from speechclip_amd.data import audio_transforms as A
    st = clip_samples(44100, "int16", 2, 1400)
    mono = clip_samples(16000, "int16", 1, 777)
    with wave.open(str(tmp_path / "a.wav"), "wb") as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(44100), f.writeframes(st.tobytes())
    flt = clip_samples(16000, "f32", 1, 301)
    out = ops.wave_prep([(st, 44100), str(tmp_path / "a.wav"), tmp_path / "a.wav", (torch.from_numpy(st.copy()), 44100), mono, torch.from_numpy(flt.copy())])
    assert out.shape == (6, 777) and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    o = out.cpu().numpy()
    assert all(np.array_equal(o[0], o[k]) for k in (1, 2, 3)) and not o[0, 508:].any()
    assert np.array_equal(o[4], np.mean(mono.reshape(-1, 1).astype(np.float32) / 32768, axis=1)) and np.array_equal(o[5, :301], flt) and not o[5, 301:].any()
    y, sabs = A.execute_plan_numpy(st, 44100, return_abs=True)
    assert _tool().judge(o[0, :508], y, sabs, 104)[0] == 0
    wide = ops.wave_prep([(st, 44100), flt], starts=[100, 1], lens=[0, 0], Lout=5)
    assert wide.shape == (2, 5) and not bool(wide.any())
    assert ops.wave_prep([(st, 44100)], lens=[0]).shape == (1, 0) and ops.wave_prep([]).shape == (0, 0)
    with pytest.raises(ValueError, match="Lout"):
        ops.wave_prep([flt], Lout=300)
    with pytest.raises(ValueError, match="16001 Hz"):
        ops.wave_prep([(flt, 16001)])
    with pytest.raises(TypeError):
        ops.wave_prep([torch.from_numpy(flt.copy()).cuda()])


def test_rows_are_addressed_in_64_bits():
    """A row stride past 2^31 elements: row 1 of the output starts 8 GiB into the buffer.  Only the neighbourhood of the two rows is initialised and read."""
    from speechclip_amd import ops
    ld, Lout = 2 ** 31 + 8, 300
    free, _ = torch.cuda.mem_get_info()
    assert free > 4 * (ld + Lout + GUARD) + (1 << 30), "the test needs 9 GiB of free device memory"
    buf = torch.empty(ld + Lout + GUARD, dtype=torch.float32, device="cuda")
    buf[:Lout + GUARD] = SENTINEL
    buf[ld - GUARD:] = SENTINEL
    view = torch.as_strided(buf, (2, Lout), (ld, 1))
    a, b = clip_samples(44100, "int16", 2, 800), clip_samples(16000, "f32", 1, 300)
    out = ops._wave_prep([(a, 44100), b], out=view, Lout=Lout)
    want = ops.wave_prep([(a, 44100), b])
    torch.cuda.synchronize()
    assert out.stride(0) == ld and torch.equal(out[0], want[0]) and torch.equal(out[1], want[1]) and bool(want[1].any())
    assert bool((buf[Lout:Lout + GUARD] == SENTINEL).all()) and bool((buf[ld - GUARD:ld] == SENTINEL).all()) and bool((buf[ld + Lout:] == SENTINEL).all())
    del buf, view, out
    torch.cuda.empty_cache()


def test_argument_rules_give_a_code_and_a_message_without_a_launch():
    """Every rule is checked on the host copies before the launch.  The device arguments are real, generously sized, zero-filled allocations, so a rule that
    stops refusing makes this test FAIL on `rc` (or on the untouched output) instead of launching on bad addresses."""
    from speechclip_amd import _lib
    from speechclip_amd.data import audio_transforms as A
    L = _lib.lib()
    cl = [(clip_samples(44100, "int16", 2, 1400), 44100), clip_samples(16000, "f32", 1, 333), (clip_samples(8000, "int16", 1, 77), 8000)]
    bp = A.plan_wave_batch(cl)
    Lout = 508
    packed_d = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    out_d = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    keep = []

    def dev(a, pad_to=0):
        t = torch.zeros(max(a.size, pad_to), dtype=torch.from_numpy(a).dtype, device="cuda")
        t[:a.size] = torch.from_numpy(a.reshape(-1))
        keep.append(t)
        return t.data_ptr()

    def call(geom=bp.geom, offsets=bp.offsets, tables_len=None, packed_bytes=bp.packed_bytes, lout=Lout, ld=None, no_tables=False, no_out=False):
        g, o, t = np.ascontiguousarray(geom, np.int64), np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(bp.tables, np.float32)
        keep.extend([g, o, t])
        rc = L.sc_wave_prep(packed_d.data_ptr(), packed_bytes, o.ctypes.data, dev(o), g.ctypes.data, dev(g), None if no_tables else t.ctypes.data,
                            None if no_tables else dev(t, 1 << 17), t.size if tables_len is None else tables_len, 3, None if no_out else out_d.data_ptr(),
                            lout if ld is None else ld, lout, _lib.stream())
        return rc, L.sc_last_error().decode()

    def with_geom(b, field, value, *more):
        g = bp.geom.copy()
        g[b, field] = value
        for f, v in zip(more[::2], more[1::2]):
            g[b, f] = v
        return g

    refused = [          # (what the message must name, the call)
        ("C=3", call(geom=with_geom(0, A.G_C, 3))),
        ("fmt=2", call(geom=with_geom(0, A.G_FMT, 2))),
        ("frames=-1", call(geom=with_geom(1, A.G_FRAMES, -1))),
        ("ratio L/M = 0/441", call(geom=with_geom(0, A.G_L, 0))),
        ("ratio L/M = 2/-1", call(geom=with_geom(2, A.G_M, -1))),
        ("ratio L/M = 320/882", call(geom=with_geom(0, A.G_L, 320, A.G_M, 882))),
        ("window [1, 1 + 508)", call(geom=with_geom(0, A.G_START, 1))),
        ("window [0, 0 + 155)", call(geom=with_geom(2, A.G_LEN, 155))),
        ("window [-1,", call(geom=with_geom(1, A.G_START, -1))),
        ("len=508 exceeds Lout=507", call(lout=507)),
        ("outside packed", call(packed_bytes=int(bp.offsets[2]) + 153)),
        ("misaligned", call(offsets=bp.offsets + np.array([2, 0, 0]))),
        ("table index", call(geom=with_geom(2, A.G_TABLE, bp.tables.size - 75))),
        ("table index", call(tables_len=bp.tables.size - 1)),
        ("K=103", call(geom=with_geom(0, A.G_K, 103))),
        ("identity rate", call(geom=with_geom(1, A.G_TABLE, 0))),
        ("tables is null", call(no_tables=True)),
        ("over the cap", call(geom=with_geom(0, A.G_L, 16000, A.G_M, 16001, A.G_K, 38, A.G_LEN, 10))),
        ("too steeply", call(geom=with_geom(0, A.G_L, 1, A.G_M, 100, A.G_K, 3765, A.G_LEN, 10), tables_len=1 << 16)),
        ("ld=", call(ld=Lout - 1)),
        ("out is null", call(no_out=True)),
    ]
    for what, (rc, msg) in refused:
        assert rc != 0 and what in msg and "sc_wave_prep" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert not bool(out_d.any())                                   # nothing ran
    assert call()[0] == 0                                          # the unmodified arguments are accepted (zero samples in, one launch)
    torch.cuda.synchronize()
    assert not bool(out_d.any())                                   # ... and zeros resample to zeros


# ---- end to end on the tiny HuBERT ------------------------------------------------------------------------------------------------------------------------
def _tiny_model():
    import dataclasses
    from oracle.clip_ref import ClipRefConfig
    from oracle.hubert_ref import HubertRefConfig
    from helpers import make_config
    from speechclip_amd.model import KWClip_GeneralTransformer
    from speechclip_amd.module.clip_model import ClipConfig
    from speechclip_amd.module.hubert import HubertConfig
    torch.manual_seed(0)
    cfg = make_config(d_model=128, branch_heads=4, cascaded=True, hubert_config=HubertConfig(**dataclasses.asdict(HubertRefConfig.tiny())),
                      clip_config=ClipConfig(**dataclasses.asdict(ClipRefConfig.tiny())))
    return KWClip_GeneralTransformer(cfg).eval().cuda()


@pytest.fixture(scope="module")
def model():
    return _tiny_model()


def _same(a: dict, b: dict):
    keys = ("cascaded_audio_feat", "parallel_audio_feat", "keywords")
    return all(a[k] is not None and a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in keys)


def _counting(monkeypatch):
    from speechclip_amd import ops
    calls, real = [], ops.wave_prep
    monkeypatch.setattr(ops, "wave_prep", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_encode_speech_of_int16_and_of_paths_equals_encode_speech_of_the_float_list(model, tmp_path, monkeypatch):
    calls = _counting(monkeypatch)
    monkeypatch.delenv("SC_WAVE_PREP", raising=False)
    pcm = [clip_samples(16000, "int16", 1, n) for n in (5000, 3100, 4321)]
    floats = [torch.from_numpy(p.astype(np.float32) / 32768) for p in pcm]
    paths = []
    for i, p in enumerate(pcm):
        paths.append(str(tmp_path / f"{i}.wav"))
        with wave.open(paths[-1], "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000), f.writeframes(p.tobytes())
    with torch.no_grad():
        monkeypatch.setenv("SC_WAVE_PREP", "host")
        want = model.encode_speech(floats)
        assert not calls
        monkeypatch.delenv("SC_WAVE_PREP")
        got = [model.encode_speech(w) for w in (pcm, [torch.from_numpy(p.copy()) for p in pcm], [(p, 16000) for p in pcm], paths, [paths[0], pcm[1], floats[2]])]
        assert len(calls) == 5
    assert all(_same(g, want) for g in got)
    assert model.processWavs(paths)[1] == [5000, 3100, 4321]
    with pytest.raises(TypeError, match="device tensor"):
        model.encode_speech([floats[0].cuda(), pcm[1].reshape(-1, 1)])
    monkeypatch.setenv("SC_WAVE_PREP", "host")
    with pytest.raises(ValueError, match="SC_WAVE_PREP=host"):
        model.encode_speech(pcm)


def test_encode_speech_of_a_44k_stereo_list_equals_encode_speech_of_what_wave_prep_returns(model, monkeypatch):
    from speechclip_amd import ops
    monkeypatch.delenv("SC_WAVE_PREP", raising=False)
    cl = [(clip_samples(44100, "int16", 2, n), 44100) for n in (12000, 9000)] + [(clip_samples(8000, "f32", 2, 2000), 8000)]
    rows = ops.wave_prep(cl)
    lens = model.processWavs(cl)[1]
    assert lens == [4354, 3266, 4000] and rows.shape == (3, 4354)
    floats = [rows[b, :n].cpu() for b, n in enumerate(lens)]
    with torch.no_grad():
        got = model.encode_speech(cl)
        monkeypatch.setenv("SC_WAVE_PREP", "host")
        want = model.encode_speech(floats)
    assert _same(got, want)
    with torch.no_grad():
        feat_w, hidden_w = model.feature_extractor_s3prl(floats)
        monkeypatch.delenv("SC_WAVE_PREP")
        feat, hidden = model.feature_extractor_s3prl(cl)
    assert len(hidden) == len(hidden_w) and torch.equal(feat, feat_w) and all(torch.equal(a, b) for a, b in zip(hidden, hidden_w))


def test_device_equals_host_on_a_16k_float_list_in_eval_and_in_train_mode(model, monkeypatch):
    """SC_WAVE_PREP=device against host: equal bits in eval mode; in train mode with max_audio_len set and one numpy seed the same crops and the same number
    of draws from the global numpy stream (the layer-drop draws follow the crop draws)."""
    calls = _counting(monkeypatch)
    floats = [torch.from_numpy(clip_samples(16000, "f32", 1, n).copy()) for n in (6000, 3100, 4321, 7000)]
    enc = model.audio_encoder
    with torch.no_grad():
        monkeypatch.setenv("SC_WAVE_PREP", "host")
        want = model.encode_speech(floats)
        monkeypatch.setenv("SC_WAVE_PREP", "device")
        got = model.encode_speech(floats)
        assert len(calls) == 1 and _same(got, want)
        old = enc.max_audio_len
        enc.train()
        try:
            enc.max_audio_len = 4000
            res = {}
            for mode in ("host", "device"):
                monkeypatch.setenv("SC_WAVE_PREP", mode)
                np.random.seed(7)
                torch.manual_seed(7)
                feat, flen = model.forward_audio(floats, [len(f) for f in floats])
                res[mode] = (feat.clone(), flen.clone(), np.random.random())
            assert len(calls) == 2
        finally:
            enc.max_audio_len = old
            enc.eval()
    assert torch.equal(res["host"][0], res["device"][0]) and torch.equal(res["host"][1], res["device"][1]) and res["host"][2] == res["device"][2]
    # the stream advanced by exactly three crop draws (6000, 4321 and 7000 > 4000, in batch order) and the layer-drop draws
    np.random.seed(7)
    for n in (6000, 4321, 7000):
        np.random.randint(n - 4000)
    np.random.random(enc.encoder.cfg.encoder_layers)
    assert res["host"][2] == np.random.random()


def test_get_attention_weights_is_forward_audio_plus_get_attention_map(model, monkeypatch):
    monkeypatch.delenv("SC_WAVE_PREP", raising=False)
    cl = [(clip_samples(22050, "int16", 2, 6000), 22050), clip_samples(16000, "int16", 1, 3500)]
    got_w, got_kw, got_none = model.get_attention_weights(cl)
    wav, wav_len = model.processWavs(cl)
    with torch.no_grad():
        feat, flen = model.forward_audio(wav, wav_len)
    want_w, want_kw, _ = model.cascaded_branch.getAttentionMap(feat, flen)
    assert got_none is None and got_kw == want_kw and len(got_w) == 2 and all(torch.equal(a, b) for a, b in zip(got_w, want_w))

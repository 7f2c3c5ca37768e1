"""Host half of the on-device audio hand-over (data/audio_transforms.py, the sc_wave_prep ABI and its argument rules, tools/wave_prep_bounds.py).

No GPU: the plan is executed in float64 (execute_plan_numpy), the identity rate is demanded bit for bit against the numpy statement of the contract, the
resampler's pass band and stop band are held to -85 dB, every argument rule of the entry refuses on its host copies (the calls pass no output buffer, so a
rule that stopped refusing would be answered by the last rule -- `out is null` -- and fail here on its message instead of launching), and each mis-statement
of the algorithm leaves the bound the GPU test judges under."""
import ctypes
import importlib.util
import os
import re
import wave

import numpy as np
import pytest
import torch

from wave_prep_cases import RATES, clip_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bounds_tool():
    spec = importlib.util.spec_from_file_location("wave_prep_bounds", os.path.join(ROOT, "tools", "wave_prep_bounds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_is_declared_exported_and_bound_with_matching_arity():
    from speechclip_amd import _lib
    from speechclip_amd.data import audio_transforms as A
    L = _lib.lib()
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    assert "sc_wave_prep" in _lib.exported_symbols() and hasattr(L, "sc_wave_prep")
    params = re.search(r"^int sc_wave_prep\s*\(([^)]*)\)", text, re.M).group(1)
    assert len(L.sc_wave_prep.argtypes) == len([p for p in params.split(",") if p.strip()]) == 14
    assert L.sc_wave_prep.restype is ctypes.c_int
    for name, value in (("GEOM", A.GEOM_FIELDS), ("I16", A.FMT_I16), ("F32", A.FMT_F32), ("MAX_TABLE", A.MAX_TABLE_ENTRIES)):
        assert f"#define SC_WAVE_PREP_{name} {value}" in text, name
    assert "ARITHMETIC CONTRACT" in text and L.sc_abi_version() == 1
    assert A.ROLLOFF == A.ROLLOFF_NUM / A.ROLLOFF_DEN == 0.85 and A.ZEROS == 16 and A.BETA == 8.56


def test_table_sizes_of_the_common_rates():
    from speechclip_amd.data import audio_transforms as A
    want = {8000: (2, 1, 38), 48000: (1, 3, 113), 44100: (160, 441, 104), 22050: (320, 441, 52), 11025: (640, 441, 38)}
    for rate, (L, M, K) in want.items():
        l, m, k, taps = A.resample_taps(rate)
        assert (l, m, k) == (L, M, K) and taps.shape == (L, K) and taps.dtype == np.float32
        assert A.resample_taps(rate)[3] is taps          # cached per rate
        # K is the smallest width that covers every phase: some phase uses all K taps, and every row is zero beyond its own count
        counts = [A.phase_support(p, L, M)[1] for p in range(L)]
        assert max(counts) == K and all((taps[p, c:] == 0).all() and taps[p, c - 1] != 0 for p, c in enumerate(counts))
    assert A.resample_taps(16000) == (1, 1, 0, A.resample_taps(16000)[3]) and A.resample_taps(16000)[3].size == 0
    for rate in (12000, 24000, 32000, 96000):
        L, M, K, taps = A.resample_taps(rate)
        assert taps.size <= 1024
    with pytest.raises(ValueError, match="16001 Hz"):
        A.resample_taps(16001)


@pytest.mark.parametrize("rate", RATES)
def test_resampled_length_is_the_integer_formula(rate):
    from speechclip_amd.data import audio_transforms as A
    L, M = A.rate_ratio(rate)
    for frames in (0, 1, M - 1, M, M + 1, 3001, 2 ** 33 + 7):
        if frames < 0:
            continue
        assert A.resampled_length(frames, rate) == (frames * L + M - 1) // M == -((-frames * L) // M)
        if frames <= 3001:
            x = np.zeros(frames, np.float32)
            assert len(A.execute_plan_numpy(x, rate)) == A.resampled_length(frames, rate)
            assert A.plan_wave_batch([(x, rate)]).n_out == [A.resampled_length(frames, rate)]


@pytest.mark.parametrize("C", [1, 2])
def test_identity_plan_equals_the_numpy_statement_on_every_bit(C):
    from speechclip_amd.data import audio_transforms as A
    pcm = clip_samples(16000, "int16", C, 4001).reshape(4001, C)
    pcm[:4] = [[32767] * C, [-32768] * C, [32767, -32768][:C], [-32768, 32767][:C]]
    assert {32767, -32768} <= set(pcm.reshape(-1).tolist())
    want = np.mean(pcm.astype(np.float32) / 32768, axis=1)
    assert want.dtype == np.float32
    got = A.execute_plan_numpy(pcm, 16000)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got1 = A.execute_plan_numpy(pcm if C == 2 else pcm[:, 0], 16000, start=17, length=1000)
    assert np.array_equal(got1.view(np.uint32), want[17:1017].view(np.uint32))
    f = clip_samples(16000, "f32", C, 999)
    wantf = f if C == 1 else (f[:, 0] + f[:, 1]) * np.float32(0.5)
    assert np.array_equal(A.execute_plan_numpy(f, 16000).view(np.uint32), wantf.view(np.uint32))
    tool = _bounds_tool()
    assert np.array_equal(tool.mono(pcm).view(np.uint32), want.view(np.uint32))          # the tool's own mono statement: the numpy expression itself


def _db(v):
    return 20.0 * np.log10(max(float(v), 1e-300))


@pytest.mark.parametrize("rate", [r for r in RATES if r != 16000])
def test_filter_quality(rate):
    """float64 execution on the f32 taps, a quarter-second unit tone, the middle half of the output: pass-band tones (100 Hz, 0.5 Nyq, 0.75 ROLLOFF Nyq,
    Nyq = min(src, dst) / 2) within -85 dB of the ideal sine (worst sample, relative to the amplitude); for the down-sampling rates tones at 1.15 x 8 kHz,
    1.5 x 8 kHz and 0.95 src / 2 below -85 dB.  This design measures -88.1 dB (worst pass-band error, 8000 and 11025 Hz at 0.75 ROLLOFF Nyq) and -90.1 dB
    (worst stop-band tone, 22050 Hz at 9.2 kHz) on exactly these inputs."""
    from speechclip_amd.data import audio_transforms as A
    nyq = min(rate, 16000) / 2
    t = np.arange(rate // 4) / rate

    def run(f):
        y = A.execute_plan_numpy(np.sin(2 * np.pi * f * t + 0.3).astype(np.float32), rate)
        lo, hi = len(y) // 4, len(y) - len(y) // 4
        return y[lo:hi], np.sin(2 * np.pi * f * np.arange(len(y)) / 16000 + 0.3)[lo:hi]

    for f in (100.0, 0.5 * nyq, 0.75 * A.ROLLOFF * nyq):
        y, ideal = run(f)
        err = _db(np.abs(y - ideal).max())
        print(f"{rate} Hz: pass-band tone {f:.1f} Hz: worst error {err:.1f} dB")
        assert err < -85.0, (rate, f, err)
    if rate > 16000:
        for f in (1.15 * 8000, 1.5 * 8000, 0.95 * rate / 2):
            y, _ = run(f)
            lvl = _db(np.abs(y).max())
            print(f"{rate} Hz: stop-band tone {f:.1f} Hz: worst level {lvl:.1f} dB")
            assert lvl < -85.0, (rate, f, lvl)


def test_the_bound_is_reproduced_and_rejects_every_mutant():
    """tools/wave_prep_bounds.py: its own tables and executor equal the module's on every bit, a float32 model of a correct kernel stays inside the bound, and
    each mis-statement (phase off by one, window one sample short, floor length, no zero edge, channels not averaged, neighbouring phase's taps) leaves it on
    every reduced case where it changes anything."""
    tool = _bounds_tool()
    assert tool.main() == 0
    assert tool.MULT == 1.005 and tool.U == 2.0 ** -24
    from speechclip_amd.data import audio_transforms as A
    seen = set()
    for name, x, rate in tool.reduced_cases():
        y, sabs, K = tool.resample(x, rate)
        good = A.execute_plan_numpy(x, rate).astype(np.float32)          # the module's value rounded once to f32: inside the bound
        assert tool.judge(good, y, sabs, K)[0] == 0
        for m in tool.MUTANTS:
            if tool.applicable(m, x, rate):
                bad, _ = tool.judge(tool.resample(x, rate, mutant=m)[0].astype(np.float32), y, sabs, K)
                assert bad > 0, (name, m)
                seen.add(m)
    assert seen == set(tool.MUTANTS)
    # a window of the mutated signal, as the GPU test cuts it: the last sample of a length that does not divide
    x = clip_samples(44100, "int16", 2, 1400)
    n = A.resampled_length(1400, 44100)
    y, sabs, K = tool.resample(x, 44100, start=n - 1, length=1)
    assert tool.judge(tool.resample(x, 44100, start=n - 1, length=1, mutant="floor length")[0].astype(np.float32), y, sabs, K)[0] == 1


def _write_wav(path, pcm, rate, width=2):
    pcm = np.asarray(pcm)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if pcm.ndim == 1 else pcm.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


def test_load_wav_pcm_round_trip_and_refusals(tmp_path):
    from speechclip_amd.data import audio_transforms as A
    for i, (C, frames, rate) in enumerate([(1, 1001, 16000), (2, 1001, 44100), (1, 1, 8000), (2, 3, 22050), (1, 0, 16000), (2, 0, 48000)]):
        pcm = clip_samples(rate, "int16", C, frames).reshape(frames, C)
        _write_wav(tmp_path / f"{i}.wav", pcm, rate)
        got, r = A.load_wav_pcm(tmp_path / f"{i}.wav")
        assert r == rate and got.dtype == np.int16 and got.shape == (frames, C) and np.array_equal(got, pcm) and got.flags.c_contiguous
        got2, _ = A.load_wav_pcm(str(tmp_path / f"{i}.wav"))
        assert np.array_equal(got2, pcm)
    _write_wav(tmp_path / "u8.wav", np.arange(50, dtype=np.uint8), 16000, width=1)
    with pytest.raises(ValueError, match="8-bit PCM with 1 channel"):
        A.load_wav_pcm(tmp_path / "u8.wav")
    _write_wav(tmp_path / "c3.wav", np.zeros((20, 3), np.int16), 16000)
    with pytest.raises(ValueError, match="16-bit PCM with 3 channel"):
        A.load_wav_pcm(tmp_path / "c3.wav")
    (tmp_path / "junk.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match="junk.wav"):
        A.load_wav_pcm(tmp_path / "junk.wav")


def test_batch_plan_layout():
    """Tables once per distinct rate, 16-byte aligned utterances with optional gaps, the window defaults, and what the plan itself refuses."""
    from speechclip_amd.data import audio_transforms as A
    a, b, c, d = (clip_samples(44100, "int16", 2, 1400), clip_samples(16000, "f32", 1, 333), clip_samples(44100, "f32", 1, 50),
                  clip_samples(8000, "int16", 1, 77))
    bp = A.plan_wave_batch([(a, 44100), b, (torch.from_numpy(c), 44100), (d, 8000)], pad_bytes=32)
    assert bp.offsets.tolist() == [32, 32 + 5600 + 32, 32 + 5600 + 32 + 1344 + 32, 32 + 5600 + 32 + 1344 + 32 + 208 + 32]
    assert bp.packed_bytes == bp.offsets[3] + 160 + 32 and all(o % 16 == 0 for o in bp.offsets)
    assert bp.tables.size == 160 * 104 + 2 * 38 and bp.geom[:, A.G_TABLE].tolist() == [0, -1, 0, 160 * 104]
    assert bp.geom[:, A.G_FMT].tolist() == [0, 1, 1, 0] and bp.geom[:, A.G_C].tolist() == [2, 1, 1, 1] and bp.geom[:, A.G_K].tolist() == [104, 0, 104, 38]
    assert bp.geom[:, A.G_START].tolist() == [0] * 4 and bp.geom[:, A.G_LEN].tolist() == bp.n_out == [508, 333, 19, 154]
    bp = A.plan_wave_batch([(a, 44100), b], starts=[8, 0], lens=[500, 0])
    assert bp.geom[:, A.G_START].tolist() == [8, 0] and bp.geom[:, A.G_LEN].tolist() == [500, 0]
    for bad in (dict(starts=[9, 0], lens=[500, 0]), dict(starts=[-1, 0], lens=[5, 0]), dict(starts=[0, 0], lens=[5, 334])):
        with pytest.raises(ValueError, match="window"):
            A.plan_wave_batch([(a, 44100), b], **bad)
    for clip in (np.zeros((5, 3), np.int16), np.zeros(5, np.float64), np.zeros((2, 2, 2), np.float32), (np.zeros(5, np.int16), 0), (np.zeros(5, np.int16), 16000, 1)):
        with pytest.raises(ValueError):
            A.plan_wave_batch([clip])


def test_every_argument_rule_refuses_on_the_host_copies():
    """No GPU is needed: the rules run on the host copies before anything else.  Every call passes a NULL output, which the LAST rule refuses."""
    from speechclip_amd import _lib
    from speechclip_amd.data import audio_transforms as A
    L = _lib.lib()
    clips = [(clip_samples(44100, "int16", 2, 1400), 44100), clip_samples(16000, "f32", 1, 333), (clip_samples(8000, "int16", 1, 77), 8000)]
    bp = A.plan_wave_batch(clips)
    Lout = 508
    keep = []

    def call(geom=bp.geom, offsets=bp.offsets, tables=bp.tables, tables_len=None, packed_bytes=bp.packed_bytes, lout=Lout, ld=None, no_tables=False, B=3):
        g, o, t = np.ascontiguousarray(geom, np.int64), np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(tables, np.float32)
        keep.extend([g, o, t])
        fake = 1 << 20          # never dereferenced: nothing is launched without an output buffer
        rc = L.sc_wave_prep(fake, packed_bytes, o.ctypes.data, fake, g.ctypes.data, fake, None if no_tables else t.ctypes.data, None if no_tables else fake,
                            t.size if tables_len is None else tables_len, B, None, lout if ld is None else ld, lout, None)
        return rc, L.sc_last_error().decode()

    def with_geom(b, field, value, *more):
        g = bp.geom.copy()
        g[b, field] = value
        for f, v in zip(more[::2], more[1::2]):
            g[b, f] = v
        return g

    rc, msg = call()
    assert rc != 0 and "out is null" in msg          # the unmodified arguments pass every other rule
    refused = [
        ("C=3", call(geom=with_geom(0, A.G_C, 3))),
        ("C=0", call(geom=with_geom(1, A.G_C, 0))),
        ("fmt=2", call(geom=with_geom(0, A.G_FMT, 2))),
        ("fmt=-1", call(geom=with_geom(2, A.G_FMT, -1))),
        ("frames=-1", call(geom=with_geom(1, A.G_FRAMES, -1))),
        ("ratio L/M = 0/441", call(geom=with_geom(0, A.G_L, 0))),
        ("ratio L/M = 160/-441", call(geom=with_geom(0, A.G_M, -441))),
        ("ratio L/M = 2/2", call(geom=with_geom(2, A.G_M, 2))),                                   # not coprime
        ("ratio L/M = 320/882", call(geom=with_geom(0, A.G_L, 320, A.G_M, 882))),
        ("window [1, 1 + 508)", call(geom=with_geom(0, A.G_START, 1))),                          # n_out = 508
        ("window [-1,", call(geom=with_geom(1, A.G_START, -1))),
        ("window [0, 0 + -1)", call(geom=with_geom(1, A.G_LEN, -1))),
        ("window [0, 0 + 155)", call(geom=with_geom(2, A.G_LEN, 155))),                          # n_out = 154
        ("window [0, 0 + 508)", call(geom=with_geom(0, A.G_FRAMES, 1397))),                      # three frames less: n_out = 507
        ("len=508 exceeds Lout=507", call(lout=507)),
        ("outside packed", call(packed_bytes=int(bp.offsets[2]) + 153)),                                # the last utterance is 154 bytes
        ("outside packed", call(offsets=bp.offsets + np.array([0, 0, 16]))),
        ("misaligned", call(offsets=bp.offsets + np.array([2, 0, 0]))),                          # a stereo int16 frame is 4 bytes
        ("outside packed", call(offsets=bp.offsets - np.array([0, bp.offsets[1] + 4, 0]))),      # negative
        ("table index", call(geom=with_geom(2, A.G_TABLE, bp.tables.size - 75))),
        ("table index", call(geom=with_geom(0, A.G_TABLE, -1))),
        ("table index", call(tables_len=bp.tables.size - 1)),
        ("K=103", call(geom=with_geom(0, A.G_K, 103))),
        ("K=105", call(geom=with_geom(0, A.G_K, 105))),
        ("2 x 0 entries", call(geom=with_geom(2, A.G_K, 0))),
        ("identity rate", call(geom=with_geom(1, A.G_TABLE, 0))),
        ("identity rate", call(geom=with_geom(1, A.G_K, 38))),
        ("tables is null", call(no_tables=True)),
        ("over the cap", call(geom=np.concatenate([np.array([[1400, 2, 0, 16000, 16001, 38, 0, 0, 10]]), bp.geom[1:]]))),       # 16001 Hz
        ("too steeply", call(geom=np.concatenate([np.array([[1400, 2, 0, 1, 100, 3765, 0, 0, 10]]), bp.geom[1:]]), tables_len=1 << 16)),
        ("B=-1", call(B=-1)),
        ("ld=", call(ld=Lout - 1)),
    ]
    for what, (rc, msg) in refused:
        assert rc != 0 and what in msg and "sc_wave_prep" in msg and "out is null" not in msg, (what, rc, msg)


def test_process_wavs_returns_16k_lengths_for_every_element_form(tmp_path):
    from speechclip_amd.model.kwClip import KWClipBase
    pcm = clip_samples(44100, "int16", 2, 1400)
    _write_wav(tmp_path / "a.wav", pcm, 44100)
    wavs = [torch.zeros(700), np.zeros(301, np.int16), torch.zeros(55, 2), (np.zeros((441, 2), np.float32), 44100), (torch.zeros(100, dtype=torch.int16), 8000),
            str(tmp_path / "a.wav"), tmp_path / "a.wav"]
    out, lens = KWClipBase.processWavs(None, wavs)
    assert lens == [700, 301, 55, 160, 200, 508, 508]
    assert out[0] is wavs[0] and out[3] is wavs[3] and all(isinstance(o, tuple) and o[1] == 44100 and np.array_equal(o[0], pcm) for o in out[5:])
    t = torch.zeros(3, 50)
    assert KWClipBase.processWavs(None, t) == (t, [50, 50, 50])          # a padded tensor is handed on as it is


def test_which_hand_over_a_list_takes(monkeypatch):
    """SC_WAVE_PREP is read per call; `auto` moves 16 kHz float lists to the device only if the measurement said so (the module constant)."""
    from speechclip_amd._lib import SpeechClipHipError
    from speechclip_amd.module import speech_encoder_plus as S
    from speechclip_amd.data import audio_transforms as A
    assert S.random_crop_max_length is A.random_crop_max_length
    pick = S.FairseqSpeechEncoder_Hubert._wave_prep_on_device
    cpu, gpu = torch.device("cpu"), torch.device("cuda", 0)
    floats, f64 = [torch.zeros(40), torch.zeros(30)], [torch.zeros(40, dtype=torch.float64)]
    new = [[np.zeros(40, np.int16)], [torch.zeros(40, dtype=torch.int16)], [torch.zeros(40), (np.zeros(9, np.float32), 8000)], ["a.wav"], [torch.zeros(40, 2)],
           [np.zeros(40, np.float32)]]
    monkeypatch.delenv("SC_WAVE_PREP", raising=False)
    assert pick(floats, gpu) is S._WAVE_PREP_AUTO_DEVICE and pick(floats, cpu) is False and pick(f64, gpu) is False
    for mode, want in (("host", False), ("device", True), ("auto", S._WAVE_PREP_AUTO_DEVICE)):
        monkeypatch.setenv("SC_WAVE_PREP", mode)
        assert pick(floats, gpu) is want and pick(floats, cpu) is False and pick(f64, gpu) is False
        for lst in new:
            if mode == "host":
                with pytest.raises(ValueError, match="SC_WAVE_PREP=host"):
                    pick(lst, gpu)
            else:
                assert pick(lst, gpu) is True
                with pytest.raises(SpeechClipHipError, match="no CPU fallback"):
                    pick(lst, cpu)
    monkeypatch.setenv("SC_WAVE_PREP", "gpu")
    with pytest.raises(ValueError, match="SC_WAVE_PREP"):
        pick(floats, gpu)


def test_ops_wave_prep_has_no_host_fallback(monkeypatch):
    from speechclip_amd import ops
    from speechclip_amd._lib import SpeechClipHipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SpeechClipHipError, match="no CPU fallback"):
        ops.wave_prep([np.zeros(40, np.int16)])

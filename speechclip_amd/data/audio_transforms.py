"""Audio side of the data hand-over: what the host does before sc_wave_prep (csrc/wave_prep.hip) and a float64 restatement of what the device does.

The reference hides decode + mono mix + resampling behind `librosa.load(path, sr=16000)` in its dataset (avssl/data/base_dataset.py:70-87) and crops inside
the encoder forward (avssl/data/audio_transforms.py:5-23, `random_crop_max_length`, kept here under its name).  Here the raw PCM of a ragged batch goes into
one pinned buffer `offsets | geom | tables | samples`, crosses PCIe once, and ONE library call converts int16 -> f32, mixes to mono, resamples by a rational
ratio to 16 kHz, cuts the train-mode crop window and zero-pads to [B, Lout].

THE ARITHMETIC IS THE CONTRACT (include/speechclip_hip.h states the same):
  mono f32 sample   int16: x = (float)(sum_c s_c) * (1.0f / (C * 32768)) -- every step exact in f32 for C in {1, 2}, so at a matching rate the result equals
                    np.mean(pcm.astype(np.float32) / 32768, axis=1) bit for bit;  f32: x = s (C = 1), (s_0 + s_1) * 0.5f (C = 2).
  ratio             L / M = dst / src reduced by their gcd;  n_out = (frames * L + M - 1) // M;  L == M == 1: y[n] = x[n], no table.
  resampler         polyphase Kaiser-windowed sinc, the project's own design (NOT librosa's soxr): in the up-sampled domain (rate src * L)
                    fc = ROLLOFF * 0.5 / max(L, M),  W = ZEROS / (2 fc),
                    h(t) = L * 2 fc * sinc(2 fc t) * I0(BETA * sqrt(1 - (t / W)^2)) / I0(BETA) for |t| <= W, 0 outside.
                    Output n: u = n * M, j0 = u // L, p = u % L;  y[n] = sum_k taps[p][k] * x[j_k] over the inputs j_k with |p + (j0 - j_k) * L| <= W in
                    ascending j (x = 0 outside [0, frames)), accumulated in fp32 in that order.  taps[p][k] = h(p + (j0 - j_k) * L) in float64, rounded
                    once to f32; a row is zero beyond its own tap count; K = the largest tap count of any phase.
  support           ROLLOFF = 17 / 20 exactly, so W = 320 * max(L, M) / 17 and `|t| <= W` is the INTEGER test 17 * |t| <= 320 * max(L, M): host and device
                    agree on every tap of every phase without a floating-point comparison.
  window            out[b, j] = y_b[start_b + j] for j < len_b, exactly 0.0f for len_b <= j < Lout; nothing outside the window is computed.
"""
import math
import os
import wave
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

TARGET_RATE = 16000
ZEROS = 16                 # Z: zero crossings of the sinc on each side of the centre
BETA = 8.56                # Kaiser window shape
ROLLOFF = 0.85             # cut-off as a fraction of the lower Nyquist rate; exactly ROLLOFF_NUM / ROLLOFF_DEN
ROLLOFF_NUM, ROLLOFF_DEN = 17, 20
MAX_TABLE_ENTRIES = 65536  # SC_WAVE_PREP_MAX_TABLE: L * K of one table (256 KiB); 11025 -> 16000 needs 640 x 38 = 24320, 16001 -> 16000 would need 608000
GEOM_FIELDS = 9            # SC_WAVE_PREP_GEOM: frames, C, fmt, L, M, K, table, start, len
FMT_I16, FMT_F32 = 0, 1    # SC_WAVE_PREP_I16 / SC_WAVE_PREP_F32
G_FRAMES, G_C, G_FMT, G_L, G_M, G_K, G_TABLE, G_START, G_LEN = range(GEOM_FIELDS)


def random_crop_max_length(audio: torch.Tensor, max_len: int, orig_len: int = 1000000000) -> torch.Tensor:
    """avssl/data/audio_transforms.py:5-23 (train-mode crop applied inside the encoder forward)."""
    n = min(len(audio), orig_len)
    if max_len < 0 or n <= max_len:
        return audio[:n]
    start = np.random.randint(n - max_len)
    return audio[start:start + max_len]


def rate_ratio(src: int, dst: int = TARGET_RATE) -> Tuple[int, int]:
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError(f"sample rates must be positive, got {src} -> {dst}")
    g = math.gcd(src, dst)
    return dst // g, src // g


def resampled_length(frames: int, src: int, dst: int = TARGET_RATE) -> int:
    L, M = rate_ratio(src, dst)
    return (int(frames) * L + M - 1) // M


def phase_support(p: int, L: int, M: int) -> Tuple[int, int]:
    """(d_hi, count): the taps of phase p read x[j0 - d_hi], ..., x[j0 - d_hi + count - 1]; d = j0 - j runs over 17 * |p + d * L| <= 320 * max(L, M)."""
    wn = 320 * max(L, M)
    d_hi = (wn - ROLLOFF_NUM * p) // (ROLLOFF_NUM * L)
    d_lo = -((wn + ROLLOFF_NUM * p) // (ROLLOFF_NUM * L))
    return d_hi, d_hi - d_lo + 1


def tap_count(L: int, M: int) -> int:
    """K: the smallest row width that covers every phase."""
    p = np.arange(L, dtype=np.int64)
    wn = 320 * max(L, M)
    return int(((wn - ROLLOFF_NUM * p) // (ROLLOFF_NUM * L) + (wn + ROLLOFF_NUM * p) // (ROLLOFF_NUM * L) + 1).max())


def _prototype(t: np.ndarray, L: int, M: int) -> np.ndarray:
    fc = ROLLOFF * 0.5 / max(L, M)
    W = ZEROS / (2.0 * fc)
    r = 1.0 - (t / W) ** 2
    return np.where(r >= 0.0, L * 2.0 * fc * np.sinc(2.0 * fc * t) * np.i0(BETA * np.sqrt(np.maximum(r, 0.0))) / np.i0(BETA), 0.0)


_TAPS = {}


def resample_taps(src: int, dst: int = TARGET_RATE):
    """-> (L, M, K, taps f32 [L, K]) for src -> dst, cached per rate pair.  Identity rate: (1, 1, 0, empty).  A table over MAX_TABLE_ENTRIES is refused with a
    message that names the rate."""
    key = (int(src), int(dst))
    if key not in _TAPS:
        L, M = rate_ratio(*key)
        if L == M == 1:
            _TAPS[key] = (1, 1, 0, np.zeros((1, 0), dtype=np.float32))
        else:
            K = tap_count(L, M)
            if L * K > MAX_TABLE_ENTRIES:
                raise ValueError(f"wave_prep: {key[0]} Hz -> {key[1]} Hz needs a tap table of {L} x {K} entries, over the cap of {MAX_TABLE_ENTRIES}: resample this rate on the host")
            p = np.arange(L, dtype=np.int64)
            wn = 320 * max(L, M)
            d_hi = (wn - ROLLOFF_NUM * p) // (ROLLOFF_NUM * L)
            d_lo = -((wn + ROLLOFF_NUM * p) // (ROLLOFF_NUM * L))
            d = d_hi[:, None] - np.arange(K, dtype=np.int64)[None, :]                  # ascending j = descending d
            h = _prototype((p[:, None] + d * L).astype(np.float64), L, M)
            taps = np.where(d >= d_lo[:, None], h, 0.0).astype(np.float32)
            taps.setflags(write=False)
            _TAPS[key] = (L, M, K, taps)
    return _TAPS[key]


def as_wave_clip(clip, what: str = "wave_prep"):
    """One list element -> (C-contiguous int16 / float32 array [frames, C] with C in {1, 2}, rate).  Accepted: a host array or CPU tensor [n] / [n, C] (taken as
    16 kHz), a (samples, rate) pair, a str / os.PathLike naming a 16-bit PCM .wav file."""
    rate = TARGET_RATE
    if isinstance(clip, (str, os.PathLike)):
        clip, rate = load_wav_pcm(clip)
    elif isinstance(clip, tuple):
        if len(clip) != 2:
            raise ValueError(f"{what}: a tuple element is (samples, rate), got {len(clip)} items")
        clip, rate = clip
    if isinstance(clip, torch.Tensor):
        if clip.is_cuda:
            raise TypeError(f"{what}: device tensors do not take the packed hand-over (the batch crosses PCIe once, as bytes)")
        clip = clip.detach().numpy()
    if not isinstance(clip, np.ndarray) or clip.dtype not in (np.int16, np.float32) or clip.ndim not in (1, 2) or (clip.ndim == 2 and clip.shape[1] not in (1, 2)):
        raise ValueError(f"{what} needs int16 or float32 samples [n] or [n, C] with C in (1, 2), got {getattr(clip, 'dtype', type(clip))} {getattr(clip, 'shape', '')}")
    if int(rate) != rate or rate <= 0:
        raise ValueError(f"{what}: sample rate {rate!r} is not a positive integer")
    return np.ascontiguousarray(clip.reshape(clip.shape[0], 1 if clip.ndim == 1 else clip.shape[1])), int(rate)


class WaveBatchPlan(NamedTuple):
    """The arguments of sc_wave_prep for one ragged batch, as host arrays (include/speechclip_hip.h has the layout)."""
    clips: list                  # (int16 / float32 [frames, C], rate)
    offsets: np.ndarray          # int64 [B]: byte offset of each utterance in the packed buffer (16-byte aligned)
    geom: np.ndarray             # int64 [B, GEOM_FIELDS]
    tables: np.ndarray           # f32 [T]: one [L, K] table per distinct rate
    packed_bytes: int
    n_out: list                  # 16 kHz length of each whole utterance


def plan_wave_batch(clips: Sequence, starts: Sequence[int] = None, lens: Sequence[int] = None, pad_bytes: int = 0, dst: int = TARGET_RATE) -> WaveBatchPlan:
    """Geometry, tables and offsets of one batch.  starts / lens: the crop window of each utterance in OUTPUT samples (default: the whole utterance).
    `pad_bytes` (a multiple of 16) are left free in front of every utterance and behind the last one: the tests fill them with NaN / 0x7fff patterns."""
    if pad_bytes % 16:
        raise ValueError("pad_bytes must be a multiple of 16")
    cl = [as_wave_clip(c) for c in clips]
    B = len(cl)
    offsets = np.zeros(B, dtype=np.int64)
    geom = np.zeros((B, GEOM_FIELDS), dtype=np.int64)
    recs, where, tlen, pos, n_outs = [], {}, 0, 0, []
    for b, (x, rate) in enumerate(cl):
        L, M, K, taps = resample_taps(rate, dst)
        tab = -1
        if K:
            if rate not in where:
                where[rate] = tlen
                recs.append(taps.reshape(-1))
                tlen += taps.size
            tab = where[rate]
        n_out = (x.shape[0] * L + M - 1) // M
        n_outs.append(n_out)
        start = 0 if starts is None else int(starts[b])
        ln = n_out - start if lens is None else int(lens[b])
        if start < 0 or ln < 0 or start + ln > n_out:
            raise ValueError(f"utterance {b}: window [{start}, {start + ln}) outside its {n_out} samples at {dst} Hz")
        pos += pad_bytes
        offsets[b] = pos
        pos += (x.nbytes + 15) // 16 * 16
        geom[b] = (x.shape[0], x.shape[1], FMT_I16 if x.dtype == np.int16 else FMT_F32, L, M, K, tab, start, ln)
    tables = np.concatenate(recs) if recs else np.zeros(0, dtype=np.float32)
    return WaveBatchPlan(cl, offsets, geom, tables, pos + pad_bytes, n_outs)


def mono_f32(x: np.ndarray) -> np.ndarray:
    """[frames, C] int16 / float32 -> the contract's mono f32 signal."""
    C = x.shape[1]
    if x.dtype == np.int16:
        return x.astype(np.int32).sum(axis=1).astype(np.float32) * np.float32(1.0 / (C * 32768))
    return x[:, 0].copy() if C == 1 else (x[:, 0] + x[:, 1]) * np.float32(0.5)


def execute_plan_numpy(x: np.ndarray, rate: int, start: int = 0, length: int = None, dst: int = TARGET_RATE, return_abs: bool = False):
    """The float64 restatement the tests judge against: the window [start, start + length) of the resampled mono signal, the sum taken in float64 over the
    f32-ROUNDED taps and the contract's f32 mono samples.  At identity rate the f32 samples themselves.  return_abs: also sum_k |taps_k * x_k| per element
    (the scale of the fp32 rounding bound, tools/wave_prep_bounds.py)."""
    x, rate = as_wave_clip((x, rate))
    L, M, K, taps = resample_taps(rate, dst)
    frames = x.shape[0]
    n_out = (frames * L + M - 1) // M
    length = n_out - start if length is None else length
    assert 0 <= start and 0 <= length and start + length <= n_out
    m = mono_f32(x)
    if K == 0:
        y = m[start:start + length]
        return (y, np.abs(y).astype(np.float64)) if return_abs else y
    n = np.arange(start, start + length, dtype=np.int64)
    u = n * M
    j0, p = u // L, u % L
    wn = 320 * max(L, M)
    first = j0 - (wn - ROLLOFF_NUM * p) // (ROLLOFF_NUM * L)
    j = first[:, None] + np.arange(K, dtype=np.int64)[None, :]
    xs = np.where((j >= 0) & (j < frames), m.astype(np.float64)[np.clip(j, 0, max(frames - 1, 0))] if frames else 0.0, 0.0)
    prod = taps.astype(np.float64)[p] * xs
    y = prod.sum(axis=1)
    return (y, np.abs(prod).sum(axis=1)) if return_abs else y


def load_wav_pcm(path) -> Tuple[np.ndarray, int]:
    """16-bit PCM .wav -> (int16 [frames, C], rate) with the standard library's `wave` only.  Anything that is not 16-bit PCM with C <= 2 raises a ValueError
    that names the file's format (decode and mix such a file down before the hand-over, as other image modes are left to PIL)."""
    try:
        f = wave.open(os.fspath(path), "rb")
    except wave.Error as e:          # `wave` reads WAVE_FORMAT_PCM only
        raise ValueError(f"{path}: not a PCM .wav file ({e}); 16-bit PCM with 1 or 2 channels is supported") from e
    with f:
        C, width, rate, frames = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if width != 2 or C not in (1, 2):
            raise ValueError(f"{path}: {8 * width}-bit PCM with {C} channel(s); 16-bit PCM with 1 or 2 channels is supported")
        raw = f.readframes(frames)
    pcm = np.frombuffer(raw, dtype="<i2").astype(np.int16, copy=False)
    return np.ascontiguousarray(pcm[:len(pcm) // C * C].reshape(-1, C)), rate


def wave_list_kind(wavs) -> str:
    """How a list of utterances reaches the encoder: "device" (holds a device tensor: the per-utterance loop), "float16k" (1-D float CPU tensors at 16 kHz:
    today's form, either path gives the same bits), "float_other" (1-D float64 / half tensors: the loop, which converts them), "new" (anything only the
    packed hand-over serves).  A device tensor beside a "new" element: TypeError."""
    dev = [isinstance(w, torch.Tensor) and w.is_cuda for w in wavs]
    plain = [isinstance(w, torch.Tensor) and w.dim() == 1 and w.dtype == torch.float32 for w in wavs]
    if any(dev):
        if not all(isinstance(w, torch.Tensor) and w.dim() == 1 for w in wavs):
            raise TypeError("a wav list that holds a device tensor takes 1-D tensors at 16 kHz only: stereo / (samples, rate) / array / path elements "
                            "go through the packed hand-over, which takes host data")
        return "device"
    if all(plain):
        return "float16k"
    if all(isinstance(w, torch.Tensor) and w.dim() == 1 and w.is_floating_point() for w in wavs):
        return "float_other"          # float64 / half lists: the loop converts them, as today
    return "new"


def resolve_wave_list(wavs) -> Tuple[list, List[int]]:
    """-> (the list with every path replaced by its decoded (int16 samples, rate) pair, the 16 kHz length of every element)."""
    out, lens = [], []
    for w in wavs:
        if isinstance(w, (str, os.PathLike)):
            w = load_wav_pcm(w)
        out.append(w)
        lens.append(resampled_length(len(w[0]), w[1]) if isinstance(w, tuple) else len(w))
    return out, lens

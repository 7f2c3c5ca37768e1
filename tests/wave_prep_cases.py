"""Case list shared by test_wave_prep_host.py and test_wave_prep_gpu.py: rates x sample formats x channel counts x frame counts x crop windows.

Frame counts put every edge of the filter's support inside a tested window: 1, 2, K - 1, K, M, M + 1 (K = the rate's tap count, L / M its reduced ratio),
about 3000, and one long enough for three blocks of the kernel's largest segment (2048 outputs).  Windows: the first sample, the last, a middle third, the
whole utterance, and an empty one.  The float64 references are computed once per clip (data.audio_transforms.execute_plan_numpy on the whole utterance) and
sliced per window; nothing changes them afterwards."""
import functools

import numpy as np

RATES = (16000, 8000, 11025, 22050, 44100, 48000)
FORMATS = ("int16", "f32")
LONG_OUT = 4500          # 16 kHz samples of the long clip: more than two segments of 2048 outputs


def clip_samples(rate, fmt, C, frames):
    """Deterministic noise on an offset (neither edge nor channel near zero); int16 clips hold 32767 and -32768."""
    rng = np.random.default_rng([rate, FORMATS.index(fmt), C, frames])
    if fmt == "int16":
        x = np.clip(rng.normal(5000, 9000, (frames, C)), -32768, 32767).astype(np.int16)
        x[::7] = 32767
        x[3::11] = -32768
        if C == 2:
            x[5::13, 1] = 32767
    else:
        x = (0.3 + 0.4 * rng.standard_normal((frames, C))).astype(np.float32)
    return x if C == 2 else x[:, 0]


def frame_counts(rate):
    from speechclip_amd.data.audio_transforms import resample_taps
    L, M, K, _ = resample_taps(rate)
    want = [1, 2, K - 1, K, M, M + 1, 3001, (LONG_OUT * M + L - 1) // L]
    return sorted({f for f in want if f > 0})


def windows(n_out):
    return [(0, min(1, n_out)), (max(n_out - 1, 0), min(1, n_out)), (n_out // 3, (n_out + 2) // 3), (0, n_out), (n_out // 2, 0)]


@functools.lru_cache(maxsize=None)
def clips():
    """[(samples, rate)] -- every rate x format x channel count x frame count."""
    return tuple((clip_samples(rate, fmt, C, f), rate) for rate in RATES for fmt in FORMATS for C in (1, 2) for f in frame_counts(rate))


@functools.lru_cache(maxsize=None)
def references():
    """Per clip: (y float64 or f32 at identity rate, sum|t x| float64, K) for the WHOLE utterance."""
    from speechclip_amd.data.audio_transforms import execute_plan_numpy, resample_taps
    out = []
    for x, rate in clips():
        y, sabs = execute_plan_numpy(x, rate, return_abs=True)
        y.setflags(write=False)
        sabs.setflags(write=False)
        out.append((y, sabs, resample_taps(rate)[2]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    """[(clip index, start, len)] -- every clip x every window."""
    return tuple((i, s, n) for i, (y, _, _) in enumerate(references()) for (s, n) in windows(len(y)))

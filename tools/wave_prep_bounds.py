"""CPU only: the bound tests/test_wave_prep_gpu.py judges sc_wave_prep under, an independent restatement of the entry's arithmetic, and the sensitivity of
the bound to the bugs a polyphase resampler can have.  No kernel runs here.

THE BOUND.  A resampled element is y = sum_k t_k x_k over n <= K taps, accumulated in fp32 in ascending k by one thread, t_k and x_k f32 (the taps rounded
once on the host, the mono sample by the contract's own expression, so both are INPUTS of the sum, not errors of it).  The classical running-sum analysis
(one rounding per product, one per addition, term k passes through at most n of them; with a fused multiply-add fewer) gives
    |fl(y) - y| <= gamma_n sum_k |t_k x_k|,   gamma_n = n u / (1 - n u),   u = 2^-24,
so with n <= K <= SC_WAVE_PREP_MAX_TABLE = 2^16:  gamma_n <= K u / (1 - 2^-8) < 1.004 K u.  The float64 reference carries K 2^-53 sum|t x| of its own,
2^-29 of the bound.  Hence
    bound = MULT * K * 2^-24 * sum_k |t_k x_k|,   MULT = 1.005,
per element, against the float64 value; an element whose sum_k |t_k x_k| is 0 must be exactly 0.  Identity rate and padding: bound 0 (equal bits).

MUTANTS, each run by `resample(...)` below with one switch, each required to leave the bound on every case of a reduced list where it
changes anything (`applicable`: stereo input, more than one phase, a length that does not divide):
    phase+1        u = n M + 1: the output is taken one up-sampled step late
    short window   the last tap of every phase dropped (support one input sample short)
    floor length   n_out = floor(frames L / M): the last output sample is never produced (it reads as padding)
    no zero edge   x outside [0, frames) read as the nearest edge sample instead of 0
    first channel  stereo not averaged: channel 0 alone
    next phase     the taps of phase p + 1 on the inputs of phase p

    python tools/wave_prep_bounds.py            the table; exits non-zero if a check fails
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 2.0 ** -24
MULT = 1.005
Z, BETA, ROLLOFF = 16, 8.56, 0.85
MUTANTS = ("phase+1", "short window", "floor length", "no zero edge", "first channel", "next phase")


def bound(K, sabs):
    return MULT * K * U * np.asarray(sabs, dtype=np.float64)


def judge(got, ref, sabs, K):
    """-> (elements outside the bound, worst |got - ref| / bound over the elements with a positive bound).  got f32, ref / sabs float64."""
    got, ref, sabs = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(sabs, np.float64)
    if got.shape != ref.shape:
        return max(got.size, ref.size), math.inf
    b = bound(K, sabs)
    err = np.abs(got - ref)
    pos = b > 0
    bad = int((err[pos] > b[pos]).sum()) + int((err[~pos] != 0).sum())
    return bad, float((err[pos] / b[pos]).max()) if pos.any() else 0.0


def ratio(src, dst=16000):
    g = math.gcd(src, dst)
    return dst // g, src // g


def taps_of(L, M):
    """This file's own tables: for each phase the offsets d = j0 - j with |p + d L| <= W (exact rational test), descending d = ascending j, h in float64,
    one rounding to f32.  -> (K, taps f32 [L, K], d_hi int64 [L], count int64 [L])"""
    fc = ROLLOFF * 0.5 / max(L, M)
    W = Z / (2.0 * fc)
    i0b = np.i0(BETA)
    rows, dhi = [], []
    for p in range(L):
        d = [k for k in range(-(20 * max(L, M) // L + 2), 20 * max(L, M) // L + 3) if 17 * abs(p + k * L) <= 320 * max(L, M)]
        d = np.array(sorted(d, reverse=True), dtype=np.int64)
        t = (p + d * L).astype(np.float64)
        h = L * 2.0 * fc * np.sinc(2.0 * fc * t) * np.i0(BETA * np.sqrt(np.maximum(1.0 - (t / W) ** 2, 0.0))) / i0b
        rows.append(h.astype(np.float32))
        dhi.append(int(d[0]))
    K = max(len(r) for r in rows)
    taps = np.zeros((L, K), dtype=np.float32)
    for p, r in enumerate(rows):
        taps[p, :len(r)] = r
    return K, taps, np.array(dhi, dtype=np.int64), np.array([len(r) for r in rows], dtype=np.int64)


_T = {}


def mono(x, first_channel=False):
    x = np.asarray(x)
    x = x.reshape(x.shape[0], -1)
    C = x.shape[1]
    if first_channel:
        return (x[:, 0].astype(np.float32) / np.float32(32768)) if x.dtype == np.int16 else x[:, 0].astype(np.float32)
    if x.dtype == np.int16:
        return np.mean(x.astype(np.float32) / np.float32(32768), axis=1, dtype=np.float32)
    return x[:, 0].astype(np.float32) if C == 1 else ((x[:, 0] + x[:, 1]) * np.float32(0.5)).astype(np.float32)


def resample(x, rate, start=0, length=None, mutant=None, f32_model=False, dst=16000):
    """The window [start, start + length) of the contract's output for samples x [frames] / [frames, C] at `rate` -> (y float64, sum|t x| float64, K).
    `mutant` switches one mis-statement on; f32_model: y accumulated in float32 in ascending tap order instead (a CPU model of a correct kernel)."""
    assert mutant is None or mutant in MUTANTS
    L, M = ratio(rate, dst)
    m = mono(x, first_channel=mutant == "first channel")
    frames = m.shape[0]
    n_true = (frames * L + M - 1) // M
    length = n_true - start if length is None else length
    if L == M == 1:
        y = m[start:start + length]
        return y.astype(np.float64), np.abs(y).astype(np.float64), 0
    if (L, M) not in _T:
        _T[(L, M)] = taps_of(L, M)
    K, taps, dhi, cnt = _T[(L, M)]
    n_have = frames * L // M if mutant == "floor length" else n_true
    n = np.arange(start, start + length, dtype=np.int64)
    u = n * M + (1 if mutant == "phase+1" else 0)
    j0, p = u // L, u % L
    j = (j0 - dhi[p])[:, None] + np.arange(K, dtype=np.int64)[None, :]
    live = np.arange(K)[None, :] < (cnt[p] - (1 if mutant == "short window" else 0))[:, None]
    if frames == 0:
        xs = np.zeros(j.shape)
    elif mutant == "no zero edge":
        xs = m.astype(np.float64)[np.clip(j, 0, frames - 1)]
    else:
        xs = np.where((j >= 0) & (j < frames), m.astype(np.float64)[np.clip(j, 0, frames - 1)], 0.0)
    t = taps[(p + 1) % L] if mutant == "next phase" else taps[p]
    prod = np.where(live, t.astype(np.float64) * xs, 0.0)
    if f32_model:
        acc = np.zeros(len(n), dtype=np.float32)
        t32, x32 = np.where(live, t, np.float32(0)), xs.astype(np.float32)
        for k in range(K):
            acc = (acc + t32[:, k] * x32[:, k]).astype(np.float32)
        y = acc.astype(np.float64)
    else:
        y = prod.sum(axis=1)
    y = np.where(n < n_have, y, 0.0)
    return y, np.abs(prod).sum(axis=1), K


def applicable(mutant, x, rate):
    """False where the mis-statement is no change at all: one channel only, a single phase (L = 1), a length that divides (floor = ceil)."""
    L, M = ratio(rate)
    return {"first channel": np.asarray(x).ndim == 2 and np.asarray(x).shape[1] == 2, "next phase": L > 1, "floor length": (len(x) * L) % M != 0}.get(mutant, True)


def reduced_cases():
    """(name, samples, rate): noise on an offset, so that neither edge nor channel is near zero; every table shape (L = 1, L = 2, many phases, up and down)."""
    rng = np.random.default_rng(11)
    out = []
    for rate, frames in ((8000, 301), (11025, 701), (22050, 700), (44100, 1400), (48000, 1201)):
        s = np.clip(rng.normal(9000, 6000, (frames, 2)), -32768, 32767).astype(np.int16)
        s[:, 1] = -s[:, 1] // 2
        out.append((f"{rate} int16 stereo", s, rate))
        out.append((f"{rate} f32 mono", (0.4 + 0.3 * rng.standard_normal(frames)).astype(np.float32), rate))
    return out


def main():
    from speechclip_amd.data import audio_transforms as A
    ok = True
    print(f"bound = {MULT} x K x 2^-24 x sum|t x| per element against the float64 value (gamma_K <= K u / (1 - 2^-8) < 1.004 K u for K <= 2^16; the float64 "
          f"reference adds 2^-29 of that)")
    for name, x, rate in reduced_cases():
        y, sabs, K = resample(x, rate)
        L, M, K2, taps = A.resample_taps(rate)
        same = K == K2 and np.array_equal(taps, _T[(L, M)][1])
        y2, sabs2 = A.execute_plan_numpy(x, rate, return_abs=True)
        same = same and np.array_equal(y, y2) and np.array_equal(sabs, sabs2)
        bad, worst = judge(resample(x, rate, f32_model=True)[0].astype(np.float32), y, sabs, K)
        caught = []
        for mname in MUTANTS:
            if not applicable(mname, x, rate):
                continue
            mb, _ = judge(resample(x, rate, mutant=mname)[0].astype(np.float32), y, sabs, K)
            caught.append(f"{mname} {mb}/{y.size}")
            ok = ok and mb > 0
        ok = ok and same and bad == 0
        print(f"{name:20s} L/M {L}/{M} K {K:3d} | module tables and executor equal: {same} | fp32 model: {bad} outside, worst / bound {worst:.3f} | outside the "
              f"bound: " + "; ".join(caught))
    print("all checks passed" if ok else "A CHECK FAILED")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

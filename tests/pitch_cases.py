"""The rows, ratios and recorded reference figures the pitch tests share: tests/test_gpu_pitch_kernels.py runs them on the GPU,
tests/test_pitch_cpu.py shows on the same rows what the reference does and that the GPU's decision margin catches a halved search."""
import functools

import numpy as np

import pitch_ref as pr

F0 = 207.0  # Hz: the period is a whole number of samples at none of the tests' rates
HARMONICS = (1.0, 0.5, 0.33, 0.25, 0.2)
RATES = (8000, 16000, 44100)
W = {8000: 2048, 16000: 4096, 44100: 8192}  # about a quarter of a second each: 26 to 50 frames at the ratios below
RATIOS = ((3, 2), (2, 3), (635, 504), (640, 639), (1, 2))
SHIFTS = {4.0: (635, 504), -5.0: (221, 295)}  # the property test's shifts and the ratios stn_pitch_ratio gives them


def harmonic(hz, W, f0=F0):
    """five harmonics of f0 with fixed phases, peak below 0.9"""
    t = np.arange(W) / hz
    x = sum(a * np.sin(2 * np.pi * f0 * (k + 1) * t + 0.7 * k) for k, a in enumerate(HARMONICS))
    return (0.9 * x / np.abs(x).max()).astype(np.float32)


def vowel(hz, W, seed=5):
    """seeded noise plus a 130 Hz pulse train through three two-pole resonators (700, 1200, 2600 Hz, scaled into the band at 8 kHz), with
    two silent gaps: exact zeros over [0.30 W, 0.60 W), longer than a target and a hop at every ratio so that some frame's scores all tie,
    and over [0.80 W, 0.84 W)"""
    rng = np.random.default_rng(seed)
    e = 0.3 * rng.standard_normal(W)
    e[::max(1, int(hz / 130.0))] += 4.0
    y = np.zeros(W)
    for f, bw in ((700.0, 90.0), (1200.0, 110.0), (2600.0, 160.0)):
        f = min(f, 0.4 * hz)
        r = np.exp(-np.pi * bw / hz)
        a1, a2 = 2.0 * r * np.cos(2.0 * np.pi * f / hz), -r * r
        s = np.zeros(W)
        s1 = s2 = 0.0
        for i in range(W):
            v = e[i] + a1 * s1 + a2 * s2
            s[i] = v
            s2, s1 = s1, v
        y += s / np.abs(s).max()
    y = 0.8 * y / np.abs(y).max()
    y[int(0.30 * W):int(0.60 * W)] = 0.0
    y[int(0.80 * W):int(0.84 * W)] = 0.0
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows(hz):
    """-> (x float32 [R][W], n [R], names): the harmonic row, the vowel row, an all-zero row, the harmonic row at spans 0, 1, H - 1, N and
    W, and the vowel row cut at 0.7 W with NaN behind the span"""
    w = W[hz]
    H = pr.hop(hz)
    h, v = harmonic(hz, w), vowel(hz, w)
    xs, ns, names = [h, v, np.zeros(w, np.float32)], [w, w, w], ["harmonic", "vowel", "zero"]
    for n in (0, 1, H - 1, 2 * H, w):
        xs.append(h)
        ns.append(n)
        names.append(f"harmonic[:{n}]")
    nan = v.copy()
    n_nan = int(0.7 * w)
    nan[n_nan:] = np.nan
    xs.append(nan)
    ns.append(n_nan)
    names.append("vowel+nan")
    x = np.stack(xs)
    x.setflags(write=False)
    return x, np.asarray(ns, np.int64), tuple(names)


# ---- the wide hops: H = 256, 1024 and 2048 (the rates above have 64, 128 and 512) ----------------------------------------------------------
# H = 256 searches with 448 threads, the one geometry of 7 waves; at 1024 and 2048 the 1537 and 3073 candidates take the 1024 threads 2 and
# 4 trips, the last by thread 0 alone for d = +D, and 2048 fills the prefetch registers and takes 73.9 KB of LDS
WIDE_RATES = (24000, 96000, 192000)
WIDE_W = {hz: 16 * pr.hop(hz) for hz in WIDE_RATES}  # 4096, 16384 and 32768 samples: 11 to 27 frames at the ratios below
# the analysis position moves by H b / a a frame and the continuation by H, so on a row with one good candidate the offset moves by
# H (1 - b / a) a frame until it leaves [-D, D].  8/5: 0, 3 H / 8, 3 H / 4 = +D exactly, then wherever the best of a bad lot lies;
# 4/7: frame 1 lands on -3 H / 4 = -D exactly
WIDE_RATIOS = ((8, 5), (4, 7), (3, 2), (640, 639))


def noise(hz, W):
    """white noise at 0.25 RMS: the only good candidate of a frame is the exact continuation of the grain before, so the ratio steers
    the winners (above), and no slice of the candidates holds a second best that passes for the best"""
    return (0.25 * np.random.default_rng(9).standard_normal(W)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wide_rows(hz):
    """-> (x float32 [R][W], n [R], names) at one of WIDE_RATES: the noise row, the vowel row, the vowel row cut at 0.7 W with NaN behind
    the span, an all-zero row, and the harmonic row at spans H - 1 and 1"""
    w = WIDE_W[hz]
    H = pr.hop(hz)
    h, v = harmonic(hz, w), vowel(hz, w)
    nan = v.copy()
    n_nan = int(0.7 * w)
    nan[n_nan:] = np.nan
    x = np.stack([noise(hz, w), v, nan, np.zeros(w, np.float32), h, h])
    x.setflags(write=False)
    return x, np.asarray([w, w, n_nan, w, H - 1, 1], np.int64), ("noise", "vowel", "vowel+nan", "zero", f"harmonic[:{H - 1}]", "harmonic[:1]")


def search_threads(hz):
    """the workgroup of the search: a thread per candidate up to 1024, in whole waves (kernels_pitch.hip) -> (threads, candidates)"""
    C = 2 * (3 * pr.hop(hz) // 4) + 1
    return min(1024, -(-C // 64) * 64), C


def steady(hz, Wn):
    """the steady part of a row of Wn samples: two grains in from either end, a whole number of 10-ms blocks"""
    N = 2 * pr.hop(hz)
    return 2 * N, Wn - 2 * N


# what a float32 path may add to an envelope figure in dB: per sample the overlap-add is within 4 * 2^-24 max|x| and the resampler's T
# products and sums within (T + 2) * 2^-24 max|x| (T <= 256 for these ratios); against a block RMS of at least 0.2 max|x| (the harmonic
# row's is 0.45) that is a relative error of the RMS below 262 * 2^-24 / 0.2 = 7.8e-5, or 6.8e-4 dB
FP32_ENVELOPE_DB = 20.0 * np.log10(1.0 + 262 * 2.0 ** -24 / 0.2)


@functools.lru_cache(maxsize=None)
def reference_pitch(hz, semitones):
    """the float64 reference's shifted harmonic row at hz for one of SHIFTS (the taps come from the library's host-only design)"""
    from supertonic_amd import binding
    a, b = SHIFTS[semitones]
    k = pr.rate_scale(a, b)
    taps = binding.resample_filter(a * k, b * k)
    y, _ = pr.pitch(harmonic(hz, W[hz]), None, hz, a, b, taps)
    return y


@functools.lru_cache(maxsize=None)
def reference_envelope_db(hz, semitones):
    """the recorded figure: the largest |dB| of the reference's steady-part envelope on the shifted harmonic row"""
    lo, hi = steady(hz, W[hz])
    return max(abs(v) for v in pr.envelope_db(reference_pitch(hz, semitones), hz, lo, hi))

"""The rows, shifts and recorded reference figures the formant tests share: tests/test_gpu_formant_kernels.py runs them on the GPU,
tests/test_formant_cpu.py shows on the same rows what the reference does and that the GPU tests' bounds catch four mutants of it.

The shifted rows are the float64 reference's (tests/pitch_ref.py with the library's own taps) rounded to float32: the device's pitch
stage is no part of the kernel tests, so no near-tie of a WSOLA decision reaches them."""
import functools

import numpy as np

import formant_ref as fr
import pitch_cases as pc
import pitch_ref as pr

RATES = pc.RATES + pc.WIDE_RATES
WIDTH = {**pc.W, **pc.WIDE_W}
SHIFTS = pc.SHIFTS  # +4 and -5 semitones and their ratios
PROPERTY_RATES = (8000, 16000, 44100)


def taps(a, b):
    from supertonic_amd import binding
    k = pr.rate_scale(a, b)
    return binding.resample_filter(a * k, b * k)


def shift(x, n, hz, semitones):
    """the float64 reference's shift of a row, rounded to float32"""
    a, b = SHIFTS[semitones]
    y, _ = pr.pitch(x, n, hz, a, b, taps(a, b))
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rows(hz):
    """-> (x float32 [R][W], n [R], names): the vowel with its silent gaps, the harmonic row, the noise row, an all-zero row, the harmonic
    row at spans 0, 1, H - 1, N and W, and the vowel cut at 0.7 W with NaN behind the span"""
    w = WIDTH[hz]
    H = pr.hop(hz)
    h, v = pc.harmonic(hz, w), pc.vowel(hz, w)
    xs, ns, names = [v, h, pc.noise(hz, w), np.zeros(w, np.float32)], [w, w, w, w], ["vowel", "harmonic", "noise", "zero"]
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


@functools.lru_cache(maxsize=None)
def shifted(hz, semitones):
    """y float32 [R][W] for rows(hz): each row's reference shift over its span, NaN behind the span where x has NaN there"""
    x, n, _ = rows(hz)
    cache = {}
    ys = []
    for r in range(len(x)):
        key = (x[r, :n[r]].tobytes(), int(n[r]))
        if key not in cache:
            cache[key] = shift(np.where(np.isnan(x[r]), 0.0, x[r]).astype(np.float32), int(n[r]), hz, semitones)
        y = cache[key].copy()
        y[np.isnan(x[r])] = np.nan
        ys.append(y)
    y = np.stack(ys)
    y.setflags(write=False)
    return y


def steady_vowel(hz, W, seed=5):
    """pitch_cases.vowel's generator without the gaps: seeded noise plus a 130 Hz pulse train through three two-pole resonators"""
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
    return (0.8 * y / np.abs(y).max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def property_rows(hz, semitones):
    """the steady vowel of 32 hops at hz -> (x, its reference shift y, the reference's correction of y, all [W])"""
    W = 32 * pr.hop(hz)
    x = steady_vowel(hz, W)
    y = shift(x, None, hz, semitones)
    out, _ = fr.formant(x, y, None, hz)
    return x, y, out


def envelope_figures(hz, semitones, corrected=None):
    """(uncorrected, corrected) envelope distance to the original in dB over the steady part; corrected: another corrected row"""
    x, y, out = property_rows(hz, semitones)
    lo, hi = pc.steady(hz, len(x))
    return fr.envelope_distance_db(x, y, hz, lo, hi), fr.envelope_distance_db(x, out if corrected is None else corrected, hz, lo, hi)


# ---- recorded figures -------------------------------------------------------------------------------------------------------------------------
# (uncorrected, corrected) envelope distance in dB of the float64 reference on the steady vowel: envelope_figures(hz, semitones)
ENVELOPE_DB = {
    (8000, -5.0): (11.866, 5.859), (8000, 4.0): (8.136, 3.495),
    (16000, -5.0): (7.052, 1.752), (16000, 4.0): (7.895, 2.275),
    (44100, -5.0): (7.536, 1.702), (44100, 4.0): (8.341, 1.948),
}

# fp32_deviation(hz, semitones, r) for the rows of rows(hz) in their order: the float32 restatement against float64 on the reference's
# tables, per sample.  The harmonic rows' poles lie closest to the unit circle: theirs are the largest.
FP32_DEVIATION = {
    (8000, -5.0): (6.53e-07, 4.03e-06, 7.29e-07, 0, 0, 9.43e-09, 4.57e-07, 3.18e-06, 4.03e-06, 6.53e-07),
    (8000, 4.0): (1.81e-07, 7.63e-06, 1.63e-07, 0, 0, 1.36e-08, 2.88e-07, 1.97e-06, 7.63e-06, 1.31e-07),
    (16000, -5.0): (8.26e-07, 7.48e-06, 1.04e-06, 0, 0, 1.35e-08, 3.37e-07, 3.09e-06, 7.48e-06, 7.99e-07),
    (16000, 4.0): (4.41e-07, 1.08e-05, 2.19e-07, 0, 0, 5.69e-09, 6.36e-07, 3.91e-06, 1.08e-05, 3.34e-07),
    (44100, -5.0): (1.76e-06, 1.75e-05, 9.15e-07, 0, 0, 8.63e-09, 2.48e-06, 7.22e-06, 1.75e-05, 1.57e-06),
    (44100, 4.0): (1.6e-06, 2.05e-05, 4.85e-07, 0, 0, 1.33e-08, 4.35e-06, 1.95e-05, 2.05e-05, 1.74e-06),
    (24000, -5.0): (1.44e-06, 1.36e-05, 1e-06, 0, 0, 4.6e-09, 9.38e-07, 7.61e-06, 1.36e-05, 1.44e-06),
    (24000, 4.0): (9.31e-07, 1.31e-05, 2.75e-07, 0, 0, 1.38e-08, 1.11e-06, 6.63e-06, 1.31e-05, 9.53e-07),
    (96000, -5.0): (5.94e-06, 2.38e-05, 1.28e-06, 0, 0, 1.35e-08, 3.08e-06, 1.07e-05, 2.38e-05, 5.94e-06),
    (96000, 4.0): (4.52e-06, 3.12e-05, 5.29e-07, 0, 0, 5.69e-09, 3.84e-06, 1.8e-05, 3.12e-05, 4.52e-06),
    (192000, -5.0): (8.17e-06, 2.6e-05, 1.21e-06, 0, 0, 9.09e-09, 4.71e-06, 1.46e-05, 2.6e-05, 7.02e-06),
    (192000, 4.0): (1.26e-05, 1.85e-05, 6.5e-07, 0, 0, 9.02e-09, 2.22e-06, 1.29e-05, 1.85e-05, 7.8e-06),
}

# identity_deviation(hz, name): the same for the correction of a row by itself, formant(x, x) against x
IDENTITY_ROWS = ("vowel", "harmonic", "noise")
IDENTITY_DEVIATION = {
    8000: {"vowel": 1.19e-07, "harmonic": 5.3e-06, "noise": 1.19e-07},
    16000: {"vowel": 4.47e-07, "harmonic": 8.73e-06, "noise": 1.79e-07},
    44100: {"vowel": 1.68e-06, "harmonic": 1.63e-05, "noise": 3.58e-07},
    24000: {"vowel": 8.49e-07, "harmonic": 1.27e-05, "noise": 1.79e-07},
    96000: {"vowel": 4.43e-06, "harmonic": 2.59e-05, "noise": 3.58e-07},
    192000: {"vowel": 9.03e-06, "harmonic": 2.38e-05, "noise": 4.17e-07},
}


def identity_deviation(hz, name):
    x, n, names = rows(hz)
    r = names.index(name)
    t = fr.tables(x[r], x[r], n[r], hz)
    d = fr.apply_tables(x[r], n[r], hz, t["ax"], t["cy"], np.float32).astype(np.float64) - x[r].astype(np.float64)
    return float(np.max(np.abs(d)))


def fp32_deviation(hz, semitones, r):
    """the largest per-sample deviation of the float32 restatement (ascending k, every product and sum rounded) from float64 on the
    reference's tables of row r: what the GPU tests' filter bound is 4 x of"""
    x, n, _ = rows(hz)
    y = shifted(hz, semitones)
    t = fr.tables(x[r], y[r], n[r], hz)
    d = fr.apply_tables(y[r], n[r], hz, t["ax"], t["cy"], np.float32).astype(np.float64) - fr.apply_tables(y[r], n[r], hz, t["ax"], t["cy"])
    return float(np.max(np.abs(d), initial=0.0))

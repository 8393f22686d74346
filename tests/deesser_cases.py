"""The inputs, settings, widths and bounds the de-esser's tests share (tests/test_deesser_cpu.py checks the model on them,
tests/test_gpu_deesser_kernels.py the GPU).  Every bound comes from the float32 sequential restatement's deviation from the float64
reference on the same input (tests/deesser_ref.py), times 4: DESIGN.md section 18's convention.  None comes from a kernel.

Per setting the bound of an array is 4 x the restatement's largest deviation over the eight rows.  The band's states, h and y are taken
relative to the row's peak of |x| (the rounding of a biquad scales with what goes in, not with what is left of it); the detector's
states and yL are in dB, absolutely.  A row on which the restatement's detector does not deviate at all (its band stays under the knee,
so every detector state is exactly 0 in both precisions) gets no allowance there: its detector states must be exactly 0, in split mode
its y must be x bit for bit, and in wide mode its y may lie 4 fp32 spacings of the peak away (the division, the power of ten at 2 ulp
and the product a sample goes through)."""
import functools
from types import SimpleNamespace

import numpy as np

import deesser_ref as dr

TILE = dr.SCAN * dr.CHUNK          # samples per scan tile
SPAN = dr.WG * dr.CHUNK            # samples a workgroup of the chunk passes owns
W_MAX = 3 * TILE + 40
NAMES = ["ess", "noise", "knee", "vowel", "zero", "speechlike", "clicks", "ramp"]
ESS, NOISE, KNEE, VOWEL, ZERO, SPEECHLIKE, CLICKS, RAMP = range(8)
LOUD = (ESS, NOISE)                # rows that must carry at least 1 dB across every seam, in both detector stages
STILL = (VOWEL, ZERO)              # rows whose band never reaches the knee
SETTINGS = {
    "default_44k": (dr.SPEECH, 44100),
    "wide_16k": ((4000.0, -36.0, 10.0, 0.0, 0.1, 10.0, 24.0, "wide"), 16000),
    "slow_192k": ((8000.0, -30.0, 3.0, 12.0, 20.0, 300.0, 6.0, "split"), 192000),
}
FAST = ("default_44k", "wide_16k")
STATES = dr.BAND_STATES + dr.DET_STATES
REL = dr.BAND_STATES + ("h", "y")  # compared relative to the row's peak; the rest in dB


def widths():
    return [1, 31, 32, 33, SPAN - 1, SPAN + 1, TILE - dr.CHUNK, TILE + dr.CHUNK, W_MAX]


def seams(K):
    """the chunk indices at which a workgroup span or a scan tile begins, below K"""
    return sorted({k for k in range(dr.WG, K, dr.WG)} | {k for k in range(dr.SCAN, K, dr.SCAN)})


@functools.lru_cache(maxsize=None)
def rows(rate):
    rng = np.random.default_rng(23)
    n = np.arange(W_MAX)
    hiss = rng.standard_normal((4, W_MAX))
    vowel = np.sin(2 * np.pi * 180.0 / rate * n)
    x = np.zeros((8, W_MAX), np.float64)
    # a vowel with sibilance on top, the hiss almost gone over the first 500 samples and over 1500 samples of every workgroup span
    gap = (n < 500) | ((n % SPAN >= 3000) & (n % SPAN < 4500))
    x[ESS] = 0.4 * vowel + np.where(gap, 0.0005, 0.15) * hiss[0]
    x[NOISE] = 0.3 * hiss[1]
    x[NOISE, :300] *= 0.01
    # a carrier inside every band, +-9 dB round -30 dBFS: through every knee
    x[KNEE] = 0.3 * vowel + 10.0 ** ((-30.0 + 9.0 * np.sin(2 * np.pi * n / 20000.0)) / 20.0) * np.sign(np.sin(2 * np.pi * 0.31 * n))
    x[VOWEL] = 0.5 * vowel
    x[SPEECHLIKE] = 0.4 * vowel * (0.5 + 0.5 * np.sin(2 * np.pi * n / 11025.0)) ** 2 + 0.2 * hiss[2] * (0.5 + 0.5 * np.cos(2 * np.pi * n / 7000.0)) ** 4
    x[CLICKS] = 0.3 * vowel
    x[CLICKS, 700::5000] = 1.0
    x[RAMP] = 0.3 * hiss[3] * np.linspace(0.001, 1.0, W_MAX)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _deviation(got, ref):
    return np.abs(got.astype(np.float64) - ref).max(axis=tuple(range(1, got.ndim))) if got.size else np.zeros(got.shape[0])


@functools.lru_cache(maxsize=None)
def case(name):
    """the float64 reference, the float32 restatement's deviation from it and the bounds of one setting, computed once"""
    setting, rate = SETTINGS[name]
    f = dr.coefs(setting, rate)
    x = rows(rate)
    ref, f32 = dr.Ref(x, f, np.float64), dr.Ref(x, f, np.float32)
    st64, st32 = ref.states(f, W_MAX), f32.states(f, W_MAX)
    peak = np.abs(x.astype(np.float64)).max(axis=1)
    peak = np.where(peak > 0, peak, 1.0)
    dev = {k: _deviation(st32[k], st64[k]) for k in STATES}
    dev.update(h=_deviation(f32.h, ref.h), yl=_deviation(f32.yl, ref.yl), y=_deviation(f32.y, ref.y))
    for k in REL:
        dev[k] = dev[k] / peak
    bound = {k: np.full(8, 4 * d.max()) for k, d in dev.items()}
    still = dev["yl"] == 0  # the rows without an allowance in the detector and the output
    for k in dr.DET_STATES + ("yl",):
        bound[k] = np.where(still, 0.0, bound[k])
    bound["y"] = np.where(still, 0.0 if f["split"] else 4 * 2.0 ** -23, bound["y"])
    return SimpleNamespace(name=name, setting=setting, rate=rate, f=f, x=x, ref=ref, f32=f32, peak=peak, dev=dev, bound=bound, still=still)


def conditions(c):
    """what the inputs must show on the float64 reference alone, before anything is held against it"""
    K = dr.chunks(W_MAX)
    st = c.ref.states(c.f, W_MAX)
    R, T, Kn = float(c.f["R"]), float(c.f["T"]), float(c.f["K"])
    for r in LOUD:
        assert c.ref.yl[r].max() >= min(12.0, R) - 0.1, (c.name, NAMES[r], "the reduction must come within 0.1 dB of min(12, range_db)", c.ref.yl[r].max())
    assert (c.ref.yl[ESS] == 0).any(), (c.name, "the reduction must be exactly 0 somewhere")
    if c.name in ("default_44k", "slow_192k"):
        assert (c.ref.z[NOISE] == R).sum() > 1000, (c.name, "the range cap must bind", int((c.ref.z[NOISE] == R).sum()))
    if Kn > 0:
        hg = 20 * np.log10(np.maximum(np.abs(c.ref.h[KNEE]), 1e-6))
        assert (np.abs(2 * (hg - T)) <= Kn).sum() > 1000, (c.name, "band samples must fall in the knee")
    assert not c.ref.yl[list(STILL)].any() and not c.ref.y1[list(STILL)].any(), (c.name, "vowel and zero must never reduce")
    assert list(np.flatnonzero(c.still)) == list(STILL), (c.name, "exactly vowel and zero are without deviation in yL", c.dev["yl"])
    low = min(min(st["s1_start"][r, k], st["s2_start"][r, k]) for k in seams(K) for r in LOUD)
    assert low >= 1.0, (c.name, "a lost carry could hide: both stages must carry 1 dB into every seam", low)
    assert set(seams(K)) >= {dr.WG, dr.SCAN, 2 * dr.SCAN, 3 * dr.SCAN}
    return low


def over_bound(c, what, got, ref):
    """per row: the largest |got - ref| (relative to the row's peak where the bound is) over that row's bound; 0 where both are exactly
    equal, inf where there is no allowance and they are not"""
    d = _deviation(got, ref)
    if what in REL:
        d = d / c.peak
    b = c.bound[what]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / b)

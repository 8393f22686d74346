"""The inputs, settings, widths and bounds the compressor's kernel tests share (tests/test_compressor_cpu.py checks the model on them,
tests/test_gpu_compressor_kernels.py the GPU).  Every bound comes from the float32 sequential restatement's deviation from the float64
reference on the same input (tests/compressor_ref.py: the contract operation for operation, fma included), times 4: DESIGN.md section
18's convention.  None comes from a kernel.

States and yL are compared in dB, absolutely: per case the bound is 4 x the restatement's largest deviation over all rows.  y is
compared relative to the row's peak of |y|.  A row on which the restatement does not deviate at all (it stays under the threshold, so
every state is exactly 0 in both precisions; with no makeup its y is exactly x) gets the floor instead: 4 fp32 spacings at the row's
peak, for the division, the power of ten (2 ulp) and the product a sample goes through.  For the states of such a row that floor is 0:
they must be exactly 0."""
import functools
from types import SimpleNamespace

import numpy as np

import compressor_ref as cr

TILE = cr.SCAN * cr.CHUNK          # samples per scan tile
SPAN = cr.WG * cr.CHUNK            # samples a workgroup of the chunk passes owns
W_MAX = 3 * TILE + 40
NAMES = ["bursts", "noise", "knee", "quiet", "zero", "speechlike", "clicks", "ramp"]
BURSTS, NOISE, KNEE, QUIET, ZERO, SPEECHLIKE, CLICKS, RAMP = range(8)
LOUD = (BURSTS, NOISE)             # rows that must carry at least 1 dB across every seam, in both stages
SETTINGS = {
    "speech_44k": (cr.SPEECH, 44100),
    "hard_8k": ((-30.0, 20.0, 0.0, 0.1, 10.0, 6.0), 8000),
    "slow_192k": ((-20.0, 4.0, 12.0, 300.0, 3000.0, -3.0), 192000),
}
STATES = ("s1_end", "s1_start", "s2_end", "s2_start")


def widths():
    return [1, 31, 32, 33, SPAN - 1, SPAN + 1, TILE - cr.CHUNK, TILE + cr.CHUNK, W_MAX]


def seams(K):
    """the chunk indices at which a workgroup span or a scan tile begins, below K"""
    return sorted({k for k in range(cr.WG, K, cr.WG)} | {k for k in range(cr.SCAN, K, cr.SCAN)})


@functools.lru_cache(maxsize=None)
def rows():
    rng = np.random.default_rng(20)
    n = np.arange(W_MAX)
    x = np.zeros((8, W_MAX), np.float64)
    tone = np.sin(2 * np.pi * 0.055 * n)
    # 0.6 against 0.01: loud except for the first 500 samples and a gap of 1500 samples in the middle of every workgroup span
    loud = (n >= 500) & ~((n % SPAN >= 3000) & (n % SPAN < 4500))
    x[BURSTS] = np.where(loud, 0.6, 0.01) * tone
    x[NOISE] = 0.3 * rng.standard_normal(W_MAX)
    x[NOISE, :300] *= 0.01
    x[KNEE] = 10.0 ** ((-24.0 + 9.0 * np.sin(2 * np.pi * n / 20000.0)) / 20.0) * np.sign(tone)  # +-9 dB round -24 dBFS: through every knee
    x[QUIET] = 0.002 * rng.standard_normal(W_MAX).clip(-3, 3)                                      # under -44 dBFS: under every threshold's knee
    x[SPEECHLIKE] = 0.5 * rng.standard_normal(W_MAX) * (0.5 + 0.5 * np.sin(2 * np.pi * n / 11025.0)) ** 4
    x[CLICKS] = 0.02 * tone
    x[CLICKS, 700::5000] = 1.0
    x[RAMP] = np.linspace(0.001, 1.0, W_MAX) * tone
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _deviation(got, ref):
    return np.abs(got.astype(np.float64) - ref).max(axis=tuple(range(1, got.ndim))) if got.size else np.zeros(got.shape[0])


@functools.lru_cache(maxsize=None)
def case(name):
    """the float64 reference, the float32 restatement's deviation from it and the bounds of one setting, computed once"""
    setting, rate = SETTINGS[name]
    f = cr.coefs(setting, rate)
    x = rows()
    ref, f32 = cr.Ref(x, f, np.float64), cr.Ref(x, f, np.float32)
    st64, st32 = ref.states(f, W_MAX), f32.states(f, W_MAX, np.float32)
    peak = np.abs(ref.y).max(axis=1)
    dev = {k: _deviation(st32[k], st64[k]) for k in STATES}                      # per row, dB
    dev["yl"] = _deviation(f32.yl, ref.yl)
    dev["y"] = _deviation(f32.y, ref.y) / np.where(peak > 0, peak, 1.0)         # per row, relative to the row's peak
    bound = {}
    for k, d in dev.items():
        if k == "y":
            floor = np.full(8, 4 * 2.0 ** -23)                                   # 4 spacings at the peak, relative to it (at most)
        else:
            top = np.abs(ref.yl if k == "yl" else st64[k]).max(axis=1)
            floor = 4 * np.spacing(top.astype(np.float32)).astype(np.float64) * (top > 0)
        bound[k] = np.where(d > 0, 4 * d.max(), floor)
    return SimpleNamespace(name=name, setting=setting, rate=rate, f=f, x=x, ref=ref, f32=f32, peak=peak, dev=dev, bound=bound)


def conditions(c):
    """what the inputs must show on the float64 reference alone, before anything is held against it"""
    K = cr.chunks(W_MAX)
    st = c.ref.states(c.f, W_MAX)
    assert c.ref.yl.max() >= 6.0 and (c.ref.yl == 0).any(), (c.name, "the reduction must reach 6 dB somewhere and be exactly 0 somewhere")
    T, Kn = float(c.f["T"]), float(c.f["K"])
    if Kn > 0:
        xg = 20 * np.log10(np.maximum(np.abs(c.x.astype(np.float64)), 1e-6))
        assert (np.abs(2 * (xg - T)) <= Kn).sum() > 1000, (c.name, "samples must fall in the knee")
    assert not c.ref.yl[[QUIET, ZERO]].any(), (c.name, "the quiet rows must stay under the threshold")
    for k in seams(K):
        for r in LOUD:
            assert st["s1_start"][r, k] >= 1.0 and st["s2_start"][r, k] >= 1.0, (c.name, NAMES[r], f"chunk {k}", "a lost carry could hide",
                                                                                 st["s1_start"][r, k], st["s2_start"][r, k])
    assert set(seams(K)) >= {cr.WG, cr.SCAN, 2 * cr.SCAN, 3 * cr.SCAN}


def over_bound(c, what, got, ref):
    """per row: the largest |got - ref| (y: relative to the row's peak) over that row's bound; 0 where both are exactly equal"""
    d = _deviation(got, ref)
    if what == "y":
        d = d / np.where(c.peak > 0, c.peak, 1.0)
    b = c.bound[what]
    return np.where(d == 0, 0.0, d / np.where(b > 0, b, np.finfo(np.float64).tiny))

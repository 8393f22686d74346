"""The inputs, settings, widths and bounds the expander's kernel tests share (tests/test_expander_cpu.py checks the model on them,
tests/test_gpu_expander_kernels.py the GPU).  Every bound comes from the float32 sequential restatement's deviation from the float64
reference on the same input (tests/expander_ref.py: the contract operation for operation, fma included), times 4: DESIGN.md section
18's convention.  None comes from a kernel.

States and yL are compared in dB, absolutely: per case the bound is 4 x the restatement's largest deviation over all rows.  y is
compared relative to the row's peak of |y|.  A row on which the restatement's states do not deviate at all (it stays under the
threshold, so every state is exactly 0 in both precisions and y is x times one constant) gets the floor instead: its states must be
exactly 0, and y within 4 fp32 spacings at the row's peak, for the division, the power of ten (2 ulp) and the product a sample goes
through.

The loud stretches of the burst rows end 40 and 25 samples in front of every multiple of the workgroup span (8192 samples; every scan
tile's seam, 32768, is one of them), so every seam falls into the hold or the release: there a lost start value shows (a seam inside a
loud stretch hides it, since the detector re-acquires at once)."""
import functools
from types import SimpleNamespace

import numpy as np

import expander_ref as xr

TILE = xr.SCAN * xr.CHUNK          # samples per scan tile
SPAN = xr.WG * xr.CHUNK            # samples a workgroup of the chunk passes owns
W_MAX = 3 * TILE + 40
NAMES = ["bursts", "noise", "knee", "loud", "quiet", "zero", "clicks", "ramp"]
BURSTS, NOISE, KNEE, LOUD, QUIET, ZERO, CLICKS, RAMP = range(8)
BURST_ROWS = (BURSTS, NOISE)       # rows that must carry at least 1 dB across every seam, in both stages (the two fast settings)
SETTINGS = {
    "speech_44k": (xr.SPEECH, 44100),
    "gate_8k": ((-45.0, 20.0, 0.0, 60.0, 0.1, 0.0, 10.0), 8000),
    "slow_192k": ((-40.0, 2.0, 12.0, 12.0, 300.0, 500.0, 3000.0), 192000),
}
FAST = ("speech_44k", "gate_8k")
STATES = ("s1_end", "s1_start", "s2_end", "s2_start")


def widths():
    return [1, 31, 32, 33, SPAN - 1, SPAN + 1, TILE - xr.CHUNK, TILE + xr.CHUNK, W_MAX]


def seams(K):
    """the chunk indices at which a workgroup span or a scan tile begins, below K"""
    return sorted({k for k in range(xr.WG, K, xr.WG)} | {k for k in range(xr.SCAN, K, xr.SCAN)})


@functools.lru_cache(maxsize=None)
def rows(rate):
    rng = np.random.default_rng(25)
    n = np.arange(W_MAX)
    x = np.zeros((8, W_MAX), np.float64)
    tone = np.sin(2 * np.pi * 220.0 * n / rate + 0.3)
    m = n % SPAN
    x[BURSTS] = np.where((m >= 4000) & (m < SPAN - 40), 0.5, 0.0008) * tone                 # 220 Hz bursts of 0.5 against 0.0008
    x[NOISE] = np.where((m >= 2000) & (m < SPAN - 25), 0.1, 0.0005) * rng.standard_normal(W_MAX)
    x[KNEE] = 10.0 ** ((-47.0 + 12.0 * np.sin(2 * np.pi * n / 20000.0)) / 20.0) * np.where(tone >= 0, 1.0, -1.0)  # -59 .. -35 dBFS: through every knee
    x[LOUD] = 0.2 * np.where(tone >= 0, 1.0, -1.0) * (1.0 + 0.5 * rng.random(W_MAX))       # wholly above every threshold and knee
    x[QUIET] = 0.0002 * rng.standard_normal(W_MAX).clip(-3, 3)                              # under -64 dBFS: closed under every setting
    x[CLICKS, 700::5000] = 1.0                                                              # clicks in digital silence
    x[RAMP] = np.linspace(0.0001, 0.5, W_MAX) * tone
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _deviation(got, ref):
    return np.abs(got.astype(np.float64) - ref).max(axis=tuple(range(1, got.ndim))) if got.size else np.zeros(got.shape[0])


@functools.lru_cache(maxsize=None)
def case(name):
    """the float64 reference, the float32 restatement's deviation from it and the bounds of one setting, computed once"""
    setting, rate = SETTINGS[name]
    f = xr.coefs(setting, rate)
    x = rows(rate)
    ref, f32 = xr.Ref(x, f, np.float64), xr.Ref(x, f, np.float32)
    st64, st32 = ref.states(f, W_MAX), f32.states(f, W_MAX, np.float32)
    peak = np.abs(ref.y).max(axis=1)
    dev = {k: _deviation(st32[k], st64[k]) for k in STATES}                      # per row, dB
    dev["yl"] = _deviation(f32.yl, ref.yl)
    dev["y"] = _deviation(f32.y, ref.y) / np.where(peak > 0, peak, 1.0)         # per row, relative to the row's peak
    still = np.all([dev[k] == 0 for k in STATES + ("yl",)], axis=0)              # rows on which no state of the restatement deviates
    bound = {}
    for k, d in dev.items():
        if k == "y":
            floor = 4 * np.spacing(peak.astype(np.float32)).astype(np.float64) / np.where(peak > 0, peak, 1.0)  # 4 spacings at the peak, relative to it
        else:
            top = np.abs(ref.yl if k == "yl" else st64[k]).max(axis=1)
            floor = 4 * np.spacing(top.astype(np.float32)).astype(np.float64) * (top > 0)
        bound[k] = np.where(still, floor, 4 * d.max())
    return SimpleNamespace(name=name, setting=setting, rate=rate, f=f, x=x, ref=ref, f32=f32, peak=peak, dev=dev, bound=bound, still=still,
                           hold=xr.hold_samples(setting, rate))


def conditions(c):
    """what the inputs must show on the float64 reference alone, before anything is held against it"""
    K = xr.chunks(W_MAX)
    st = c.ref.states(c.f, W_MAX)
    R, kA = float(c.f["R"]), float(c.f["kA"])
    att = R - c.ref.yl
    assert att.max() == R, (c.name, "the attenuation must reach the range")
    if c.name in FAST:
        assert att.min() < 0.01, (c.name, "the attenuation must come under 0.01 dB somewhere", att.min())
    else:
        # a 300 ms attack cannot open the gate within W_MAX samples (0.51 s at 192 kHz): the one-pole's own limit R (1 - kA)^W_MAX is
        # what the wholly loud row must reach, and nothing can come under it
        limit = R * (1.0 - kA) ** W_MAX
        assert limit > 0.01 and abs(att[LOUD].min() - limit) < 1e-6 * R and att.min() >= limit - 1e-9, (c.name, att.min(), limit)
    T, Kn = float(c.f["T"]), float(c.f["K"])
    if Kn > 0:
        xg = 20 * np.log10(np.maximum(np.abs(c.x.astype(np.float64)), 1e-6))
        assert (np.abs(2 * (T - xg)) <= Kn).sum() > 1000, (c.name, "samples must fall in the knee")
    assert not c.ref.yl[[QUIET, ZERO]].any() and c.still[[QUIET, ZERO]].all(), (c.name, "the quiet rows must stay closed")
    assert (c.ref.z[LOUD] == 0).all(), (c.name, "the loud row must lie wholly above the threshold")
    if c.name in FAST:
        for k in seams(K):
            for r in BURST_ROWS:
                assert st["s1_start"][r, k] >= 1.0 and st["s2_start"][r, k] >= 1.0, (c.name, NAMES[r], f"chunk {k}", "a lost carry could hide",
                                                                                     st["s1_start"][r, k], st["s2_start"][r, k])
                # and the seam lies in the hold or the release: the sample in front of it is not fully open
                assert c.ref.z[r, k * xr.CHUNK - 1] > 0, (c.name, NAMES[r], f"chunk {k}", "the seam must not fall into a loud stretch")
    assert set(seams(K)) >= {xr.WG, xr.SCAN, 2 * xr.SCAN, 3 * xr.SCAN}


def over_bound(c, what, got, ref):
    """per row: the largest |got - ref| (y: relative to the row's peak) over that row's bound; 0 where both are exactly equal"""
    d = _deviation(got, ref)
    if what == "y":
        d = d / np.where(c.peak > 0, c.peak, 1.0)
    b = c.bound[what]
    return np.where(d == 0, 0.0, d / np.where(b > 0, b, np.finfo(np.float64).tiny))

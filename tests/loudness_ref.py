"""A float64 statement of ITU-R BS.1770-4 integrated loudness (one channel, weight 1.0), written from the standard's text and
independent of the engine's kernels: the K-weighting biquads derived at any rate from the analog prototypes of the standard's 48 kHz
table, filtered with scipy.signal.lfilter, then the 400 ms / 100 ms gating."""
import math

import numpy as np


def kweighting(hz):
    """(shelf_b, shelf_a, hp_b, hp_a) in float64 at hz."""
    fs = float(hz)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf_b = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    shelf_a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp_b = np.array([1.0, -2.0, 1.0])
    hp_a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf_b, shelf_a, hp_b, hp_a


def hop(hz):
    return (int(hz) + 5) // 10


def integrated_loudness(x, hz):
    """BS.1770-4 integrated loudness of x (1-D) in LUFS, -inf when x is shorter than one 400 ms block or every block is gated out."""
    from scipy.signal import lfilter
    x = np.asarray(x, np.float64)
    sb, sa, hb, ha = kweighting(hz)
    y = lfilter(hb, ha, lfilter(sb, sa, x))
    h = hop(hz)
    nseg = len(x) // h
    if nseg < 4:
        return -math.inf
    seg = (y[: nseg * h] ** 2).reshape(nseg, h).sum(axis=1)
    z = (seg[:-3] + seg[1:-2] + seg[2:-1] + seg[3:]) / (4 * h)
    with np.errstate(divide="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
    g = lj > -70.0
    if not g.any():
        return -math.inf
    rel = -0.691 + 10.0 * math.log10(z[g].mean()) - 10.0
    g &= lj > rel
    if not g.any():
        return -math.inf
    return -0.691 + 10.0 * math.log10(z[g].mean())


def pcm_rule(y):
    """writeWavFile's conversion in fp32: clamp to [-1, 1], * 32767, truncation toward zero."""
    return (np.clip(np.asarray(y, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int32).astype(np.int16)

"""A float64 statement of the loudness report (include/stn.h "loudness range"): maximum momentary loudness (400 ms), maximum short-term
loudness (3 s) and loudness range (EBU Tech 3342) of one channel, written from the definitions and independent of the engine: the
K-weighting of tests/loudness_ref.py (scipy.signal.lfilter), 100 ms segment sums, numpy reductions.

Below it, the rows the tests of the report share (case_rows): the CPU test proves that no 3 s window of any of them lies within
MARGIN of a gate, so a device rounding cannot flip a gate decision, and the GPU test measures exactly these rows."""
import math

import numpy as np

from loudness_ref import hop, kweighting

BLOCK, WINDOW = 4, 30   # segments of a momentary block and of a short-term window
MARGIN = 0.05           # LU: every window of every case row is at least this far from -70 and from its row's relative threshold
RATES = (8000, 44100, 48000)


def segment_sums(x, hz):
    """The sums of y^2 (y: x K-weighted) over the whole 100 ms segments of x, float64 [len(x) // hop]."""
    from scipy.signal import lfilter
    x = np.asarray(x, np.float64)
    h = hop(hz)
    nseg = len(x) // h
    if nseg == 0:
        return np.zeros(0)
    sb, sa, hb, ha = kweighting(hz)
    y = lfilter(hb, ha, lfilter(sb, sa, x))
    return (y[: nseg * h] ** 2).reshape(nseg, h).sum(axis=1)


def _level(z):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def range_from_segments(seg, h):
    """dict from 100 ms segment sums: m_max, s_max (LUFS, -inf without a block / a window), lra (LU), n_st (windows behind both gates),
    S (every window's level), rel (the relative threshold, None when no window passes the absolute gate) and margin (the distance in LU
    of the nearest window from -70 or, among the windows above it, from rel; inf without windows)."""
    seg = np.asarray(seg, np.float64)
    n = len(seg)
    out = dict(m_max=-math.inf, s_max=-math.inf, lra=0.0, n_st=0, S=np.zeros(0), rel=None, margin=math.inf)
    if n >= BLOCK:
        z = sum(seg[i: n - BLOCK + 1 + i] for i in range(BLOCK)) / (BLOCK * h)
        out["m_max"] = float(_level(z).max())
    if n < WINDOW:
        return out
    z = sum(seg[i: n - WINDOW + 1 + i] for i in range(WINDOW)) / (WINDOW * h)
    S = _level(z)
    out["S"], out["s_max"] = S, float(S.max())
    out["margin"] = float(np.abs(S + 70.0).min())
    g = S > -70.0
    if not g.any():
        return out
    rel = float(_level(z[g].mean())) - 20.0
    out["rel"] = rel
    out["margin"] = min(out["margin"], float(np.abs(S[g] - rel).min()))
    s = np.sort(S[g & (S > rel)])
    out["n_st"] = len(s)
    if len(s) >= 2:
        out["lra"] = float(s[int(math.floor((len(s) - 1) * 0.95 + 0.5))] - s[int(math.floor((len(s) - 1) * 0.10 + 0.5))])
    return out


def loudness_range(x, hz):
    """range_from_segments of x (1-D) at hz."""
    return range_from_segments(segment_sums(x, hz), hop(hz))


def three_level(hz, top=0.5, seconds=12.0, freq=1000.0, order=(1, 0, 2)):
    """A tone at three levels 15 dB apart in equal thirds (order: which third holds the loudest, the middle and the quietest level)."""
    t = np.arange(int(round(seconds * hz))) / hz
    third = np.minimum((t / (seconds / 3.0)).astype(int), 2)
    amp = top * 10.0 ** (-15.0 * np.asarray(order)[third] / 20.0)
    return amp * np.sin(2 * np.pi * freq * t)


_ROWS = {}


def case_rows(hz):
    """(x [9, W] float32, n [9] int64) at hz, built once per rate and shared (do not write to them): the spans of one launch.
    0: no samples; 1: under 0.4 s; 2: exactly 4 segments; 3: exactly 30 segments (one window); 4: 30 hop - 1 samples (no window);
    5: 31 segments (two windows, unlike); 6: 12 s at three levels 15 dB apart; 7: a row whose last third is digital silence (windows
    under the absolute gate); 8: noise under a slow envelope, a span that ends inside a segment."""
    if hz in _ROWS:
        return _ROWS[hz]
    h = hop(hz)
    W = 120 * h + 8
    rng = np.random.default_rng(1000 + hz)
    t = np.arange(W) / hz
    tone = 0.25 * np.sin(2 * np.pi * 440.0 * t)
    ramp = tone * (0.2 + 0.8 * np.minimum(t / 3.1, 1.0))  # rising: the two windows of row 5 differ
    levels = np.zeros(W)
    levels[: 120 * h] = three_level(hz)[: 120 * h]
    gone = 0.3 * np.sin(2 * np.pi * 700.0 * t) * (0.4 + 0.6 * (np.sin(2 * np.pi * 0.23 * t) ** 2))
    gone[80 * h:] = 0.0
    noise = 0.1 * rng.standard_normal(W) * (0.25 + 0.75 * np.sin(2 * np.pi * 0.11 * t) ** 2)
    x = np.stack([tone, tone, noise, ramp, ramp, ramp, levels, gone, noise]).astype(np.float32)
    n = np.array([0, int(0.35 * hz), 4 * h, 30 * h, 30 * h - 1, 31 * h, 120 * h, 120 * h, 117 * h + 123], np.int64)
    x.setflags(write=False)
    n.setflags(write=False)
    _ROWS[hz] = (x, n)
    return _ROWS[hz]


_REFS = {}


def case_refs(hz):
    """range_from_segments of every case row at hz over its span (the float32 samples in float64), computed once and shared."""
    if hz not in _REFS:
        x, n = case_rows(hz)
        _REFS[hz] = [loudness_range(x[r, : n[r]].astype(np.float64), hz) for r in range(len(n))]
    return _REFS[hz]

"""Silence trimming by level (include/stn.h "silence trimming") in float64 numpy, the fade in float32: the reference of
tests/test_silence_cpu.py and tests/test_gpu_silence.py.

A row's first n samples at rate hz are cut into frames of F = (hz + 50) // 100 samples from sample 0, the last one short; a frame's level is
the mean of x^2 over its own samples.  The margin of a row says how far the float64 decision is from flipping: the smallest
|10 log10(m_k / thr)| over its frames, and |10 log10(m_max / 1e-7)|, the distance of the loudest frame from the no-speech floor."""
import math

import numpy as np

FLOOR = 1e-7  # mean square, -70 dBFS


def frame(hz):
    return (int(hz) + 50) // 100


def samples(hz, ms):
    """(int64)(ms * hz / 1000 + 0.5) in double, ms as the float32 the ABI takes"""
    return int(float(np.float32(ms)) * float(hz) / 1000.0 + 0.5)


def levels(x, n, hz):
    """m_k [K] float64 of one row"""
    F = frame(hz)
    n = int(n)
    K = -(-n // F)
    xx = np.asarray(x[:n], np.float64) ** 2
    return np.array([xx[k * F:min((k + 1) * F, n)].mean() for k in range(K)], np.float64)


def edges(x, n, hz, top_db, keep_ms):
    """one row -> (start, end, margin in dB)"""
    n = int(n)
    m = levels(x, n, hz)
    if n == 0:
        return 0, 0, math.inf
    mx = float(m.max())
    floor_margin = math.inf if mx == 0.0 else abs(10.0 * math.log10(mx / FLOOR))
    if mx <= FLOOR:
        return 0, n, floor_margin
    F = frame(hz)
    thr = mx * 10.0 ** (-float(np.float32(top_db)) / 10.0)
    active = np.flatnonzero(m >= thr)
    with np.errstate(divide="ignore"):
        margin = min(float(np.min(np.abs(10.0 * np.log10(m / thr)))), floor_margin)
    keep = samples(hz, keep_ms)
    f0, f1 = int(active[0]), int(active[-1])
    return max(0, f0 * F - keep), min(n, (f1 + 1) * F + keep), margin


def batch_edges(x, n, hz, top_db, keep_ms):
    """rows -> (start [rows], end [rows] int64, margin [rows] float64)"""
    x = np.atleast_2d(x)
    n = np.broadcast_to(np.asarray(x.shape[1] if n is None else n, np.int64), (x.shape[0],))
    out = [edges(x[r], n[r], hz, top_db, keep_ms) for r in range(x.shape[0])]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.float64)


def fade_window(hz, fade_ms):
    """w[j] = float32(0.5 - 0.5 cos(pi (j + 0.5) / Fd)), j < Fd = samples(hz, fade_ms)"""
    fd = samples(hz, fade_ms)
    j = np.arange(fd, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (j + 0.5) / max(fd, 1))).astype(np.float32)


def trimmed_row(x, n, start, end, hz, fade_ms, gain=None):
    """the float32 segment a fetch delivers: ((x * g) * w_in) * w_out, three float32 multiplies in that order, each only where it applies"""
    seg = np.array(x[start:end], np.float32)
    if gain is not None:
        seg = seg * np.float32(gain)
    w = fade_window(hz, fade_ms)
    k = min(w.size, seg.size)
    if k and start > 0:
        seg[:k] = seg[:k] * w[:k]
    if k and end < int(n):
        seg[seg.size - k:] = seg[seg.size - k:] * w[:k][::-1]
    return seg


def trim_rows(x, n, hz, top_db, keep_ms, fade_ms, gain=None):
    """rows x W float32 -> (y [rows, W] float32 with each segment from column 0 and +0.0 behind it, start, end, margin)"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    nn = np.broadcast_to(np.asarray(x.shape[1] if n is None else n, np.int64), (x.shape[0],))
    start, end, margin = batch_edges(x, nn, hz, top_db, keep_ms)
    y = np.zeros_like(x)
    for r in range(x.shape[0]):
        seg = trimmed_row(x[r], nn[r], int(start[r]), int(end[r]), hz, fade_ms, None if gain is None else gain[r])
        y[r, :seg.size] = seg
    return y, start, end, margin


def speech_rows(hz, rows, seconds, seed, floor_db=-80.0):
    """Designed rows with known silences: a modulated tone plus noise between a lead and a tail of 0.05 - 0.6 s of noise at floor_db; row 0
    has no lead, row 1 no tail, row 2 a 250 ms pause inside.  n is a multiple of neither 32 nor the frame.  -> (x [rows, W] float32, n)"""
    rng = np.random.default_rng(seed)
    W = int(seconds * hz)
    W += (-W) % 4  # (rows 16-byte aligned: the vector path; an odd W runs the scalar one)
    x = np.zeros((rows, W), np.float32)
    n = np.zeros(rows, np.int64)
    F = frame(hz)
    fl = 10.0 ** (floor_db / 20.0)
    for r in range(rows):
        nr = int(W - rng.integers(0, W // 8))
        while nr % 32 == 0 or nr % F == 0:
            nr -= 1
        lead = 0 if r == 0 else int(rng.uniform(0.05, 0.6) * hz)
        tail = 0 if r == 1 else int(rng.uniform(0.05, 0.6) * hz)
        t = np.arange(nr) / hz
        tone = 0.3 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + r)) * np.sin(2 * np.pi * (180.0 + 40.0 * r) * t) + 0.01 * rng.standard_normal(nr)
        sig = fl * rng.standard_normal(nr)
        sig[lead:nr - tail] += tone[lead:nr - tail]
        if r == 2:
            p0 = (lead + nr - tail) // 2
            sig[p0:p0 + int(0.25 * hz)] = fl * rng.standard_normal(int(0.25 * hz))
        x[r, :nr] = sig
        x[r, nr:] = 0.25 * rng.standard_normal(W - nr)  # loud padding behind the span: never measured
        n[r] = nr
    return x, n

"""The pause limit (include/stn.h "pause limit") in float64 numpy, the delivered row in float32: the reference of
tests/test_pause_cpu.py and tests/test_gpu_pause.py.  Levels, edges and the fade window are silence_ref's.

A pause is a maximal run of inactive frames a .. b - 1 between two active ones inside [f0, f1]; longer than Mp samples it loses its
middle [aF + hl, bF - hr), hl = Mp - Mp // 2, hr = Mp // 2.  The first 255 such pauses of a row are cut."""
import math

import numpy as np

import silence_ref as ref

MAX_CUTS = 255
MARGIN_DB = 0.01  # section 14's bound on the distance of every frame from the threshold


def pause_samples(hz, max_pause_ms):
    """(int64)(max_pause_ms * hz / 1000 + 0.5) in double, max_pause_ms as the float32 the ABI takes"""
    return int(float(np.float32(max_pause_ms)) * float(hz) / 1000.0 + 0.5)


def plan_levels(m, n, hz, top_db, keep_ms, max_pause_ms):
    """frame levels m [K] float64 of a row of n samples -> (start, end, cuts [(lo, hi)], margin in dB)"""
    n = int(n)
    m = np.asarray(m, np.float64)
    if n == 0:
        return 0, 0, [], math.inf
    mx = float(m.max())
    floor_margin = math.inf if mx == 0.0 else abs(10.0 * math.log10(mx / ref.FLOOR))
    if mx <= ref.FLOOR:
        return 0, n, [], floor_margin
    F = ref.frame(hz)
    thr = mx * 10.0 ** (-float(np.float32(top_db)) / 10.0)
    act = m >= thr
    with np.errstate(divide="ignore"):
        margin = min(float(np.min(np.abs(10.0 * np.log10(m / thr)))), floor_margin)
    idx = np.flatnonzero(act)
    f0, f1 = int(idx[0]), int(idx[-1])
    keep = ref.samples(hz, keep_ms)
    start, end = max(0, f0 * F - keep), min(n, (f1 + 1) * F + keep)
    Mp = pause_samples(hz, max_pause_ms)
    hr = Mp // 2
    hl = Mp - hr
    cuts = []
    for p, b in zip(idx[:-1], idx[1:]):  # consecutive active frames: the frames between them are one pause
        a = int(p) + 1
        b = int(b)
        if (b - a) * F > Mp and len(cuts) < MAX_CUTS:
            cuts.append((a * F + hl, b * F - hr))
    return start, end, cuts, margin


def plan(x, n, hz, top_db, keep_ms, max_pause_ms):
    """one row -> (start, end, cuts, margin)"""
    return plan_levels(ref.levels(x, n, hz), n, hz, top_db, keep_ms, max_pause_ms)


def segments(start, end, cuts):
    """[(src, stop)]: [start, c_1.lo), [c_1.hi, c_2.lo), ..., [c_m.hi, end)"""
    lo = [start] + [c[1] for c in cuts]
    hi = [c[0] for c in cuts] + [end]
    return list(zip(lo, hi))


def delivered_row(x, n, start, end, cuts, hz, fade_ms, gain=None):
    """the float32 samples a fetch delivers from column 0: every segment ((x * g) * w_in) * w_out, three float32 multiplies in that order,
    each only where it applies; an edge made by a cut is faded, and start > 0 and end < n as under trimming"""
    w = ref.fade_window(hz, fade_ms)
    segs = segments(start, end, cuts)
    out = []
    for j, (a, b) in enumerate(segs):
        seg = np.array(x[a:b], np.float32)
        if gain is not None:
            seg = seg * np.float32(gain)
        k = min(w.size, seg.size)
        if k and (j > 0 or start > 0):
            seg[:k] = seg[:k] * w[:k]
        if k and (j < len(segs) - 1 or end < int(n)):
            seg[seg.size - k:] = seg[seg.size - k:] * w[:k][::-1]
        out.append(seg)
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def pause_rows(x, n, hz, top_db, keep_ms, fade_ms, max_pause_ms, gain=None):
    """rows x W float32 -> dict(y [rows, W] float32 with +0.0 behind len, start, end, len [rows] int64, n_cuts [rows], cuts (list of lists
    of (lo, hi)), margin [rows])"""
    x = np.atleast_2d(np.asarray(x, np.float32))
    nn = np.broadcast_to(np.asarray(x.shape[1] if n is None else n, np.int64), (x.shape[0],))
    y = np.zeros_like(x)
    o = dict(start=[], end=[], len=[], n_cuts=[], cuts=[], margin=[])
    for r in range(x.shape[0]):
        s, e, cuts, margin = plan(x[r], nn[r], hz, top_db, keep_ms, max_pause_ms)
        row = delivered_row(x[r], nn[r], s, e, cuts, hz, fade_ms, None if gain is None else gain[r])
        y[r, :row.size] = row
        o["start"].append(s); o["end"].append(e); o["len"].append(row.size); o["n_cuts"].append(len(cuts)); o["cuts"].append(cuts); o["margin"].append(margin)
    return dict(y=y, start=np.array(o["start"], np.int64), end=np.array(o["end"], np.int64), len=np.array(o["len"], np.int64),
                n_cuts=np.array(o["n_cuts"], np.int32), cuts=o["cuts"], margin=np.array(o["margin"], np.float64))


def cuts_array(cuts, cap):
    """[rows][cap][2] int64 as the ABI fills it over an array preset to -1"""
    a = np.full((len(cuts), cap, 2), -1, np.int64)
    for r, c in enumerate(cuts):
        for j, (lo, hi) in enumerate(c[:cap]):
            a[r, j] = (lo, hi)
    return a


def burst_row(hz, W, n, bursts, seed, floor_db=-80.0, amp=0.3):
    """One designed row: tone bursts [(first frame, frames)] over a noise floor at floor_db inside the span n, loud noise behind the span
    (never measured).  A burst covers whole frames, so every frame is either a full-scale tone (all bursts alike: within a fraction of a
    dB of the loudest) or floor noise (some 70 dB below): the 0.01 dB margin holds by construction.  -> x [W] float32"""
    rng = np.random.default_rng(seed)
    F = ref.frame(hz)
    x = np.zeros(W, np.float64)
    x[:n] = 10.0 ** (floor_db / 20.0) * rng.standard_normal(n)
    t = np.arange(W) / hz
    tone = amp * np.sin(2 * np.pi * 440.0 * t + 0.3)
    for f, k in bursts:
        lo, hi = f * F, min((f + k) * F, n)
        x[lo:hi] += tone[lo:hi]
    x[n:] = 0.25 * rng.standard_normal(W - n)
    return x.astype(np.float32)

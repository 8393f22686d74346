"""Float64 reference of the fetch-time pitch shift (include/stn.h "pitch"): the ratio of a shift, the stretcher's
geometry and window, WSOLA with a normalised search frame by frame, the overlap-add, the polyphase resample back, and the checks the GPU
tests apply to a device's table of offsets.  Written from the rule, not from the kernels: numpy only."""
import math

import numpy as np

MAX_TERM = 640
EPS = 1e-9


# ---- ratio ----------------------------------------------------------------------------------------------------------------------------------
def ratio_target(semitones):
    """r = pow(2, s / 12) in double, s rounded to float32 first (the ABI takes a float)"""
    return math.pow(2.0, float(np.float32(semitones)) / 12.0)


def ratio_error(a, b, r):
    """the larger of q / r and r / q for q = a / b: monotonic in |log q - log r|"""
    q = a / b
    return q / r if q > r else r / q


_FRACTIONS = None


def _fractions():
    """every reduced a / b with terms in [1, 640], sorted by value: (values, a, b)"""
    global _FRACTIONS
    if _FRACTIONS is None:
        a, b = np.meshgrid(np.arange(1, MAX_TERM + 1), np.arange(1, MAX_TERM + 1), indexing="ij")
        keep = np.gcd(a, b) == 1
        a, b = a[keep], b[keep]
        order = np.argsort(a / b, kind="stable")
        _FRACTIONS = ((a / b)[order], a[order], b[order])
    return _FRACTIONS


def ratio_brute(semitones):
    """the closest fraction by search over every fraction: only the two neighbours of r in the sorted list can be closest; of equals the
    smaller b"""
    r = ratio_target(semitones)
    v, a, b = _fractions()
    i = int(np.searchsorted(v, r))
    best = None
    for j in (i - 1, i):
        if 0 <= j < len(v):
            e = ratio_error(int(a[j]), int(b[j]), r)
            if best is None or e < best[0] or (e == best[0] and b[j] < best[2]):
                best = (e, int(a[j]), int(b[j]))
    return best[1], best[2]


def ratio_exhaustive(semitones):
    """the same by the full table of 640 x 640 pairs (slow: for a few values)"""
    r = ratio_target(semitones)
    a, b = np.meshgrid(np.arange(1, MAX_TERM + 1), np.arange(1, MAX_TERM + 1), indexing="ij")
    q = a / b
    e = np.where(q > r, q / r, r / q)
    m = e == e.min()
    bb = b[m].min()
    return int(a[m & (b == bb)][0]), int(bb)


def cents(a, b, semitones):
    return 1200.0 * math.log2((a / b) / ratio_target(semitones))


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------
def hop(hz):
    H = 1
    while 128 * H < hz:
        H *= 2
    return H


def plan(hz, W, a, b):
    H = hop(hz)
    Ws = -(-W * a // b)
    return dict(H=H, N=2 * H, delta=3 * H // 4, Ws=Ws, M=Ws // H + 2)


def window(hz):
    """the periodic Hann in double"""
    N = 2 * hop(hz)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N) / N))


def window32(hz):
    """... as the float32 table the device multiplies by, widened"""
    return window(hz).astype(np.float32).astype(np.float64)


def pos(m, H, a, b):
    return m * H * b // a


# ---- the stretch ------------------------------------------------------------------------------------------------------------------------------
class Row:
    """a row of span n: reads outside [0, n) are 0.0 whatever x holds there"""

    def __init__(self, x, n=None):
        x = np.asarray(x, np.float64)
        n = len(x) if n is None else max(0, min(int(n), len(x)))
        self.n = n
        self.x = x[:n].copy()

    def read(self, start, count):
        """x[start .. start + count) with zeros outside the span"""
        out = np.zeros(count)
        lo, hi = max(start, 0), min(start + count, self.n)
        if hi > lo:
            out[lo - start:hi - start] = self.x[lo:hi]
        return out


def frame_scores(row, H, a, b, m, d_prev):
    """frame m >= 1 given d_{m-1}: (score over d in [-D, D], ||t||_2): the target is the previous grain's continuation"""
    N, D = 2 * H, 3 * H // 4
    q_prev = pos(m - 1, H, a, b) + d_prev - H
    t = row.read(q_prev + H, N)
    region = row.read(pos(m, H, a, b) - D - H, N + 2 * D)
    cand = np.lib.stride_tricks.sliding_window_view(region, N)  # [2 D + 1][N]: row j is d = j - D
    c = cand @ t
    sq = np.concatenate(([0.0], np.cumsum(region * region)))
    E = np.maximum(sq[N:] - sq[:-N], 0.0)
    return c / np.sqrt(E + EPS), float(np.sqrt(t @ t))


def pick(score, D, allowed=None):
    """the d of the largest score; of equals the smallest |d|, of two such the negative one.  allowed: a mask over d = -D .. D"""
    d = np.arange(-D, D + 1)
    s = score if allowed is None else np.where(allowed, score, -np.inf)
    best = np.flatnonzero(s == s.max())
    key = np.abs(d[best]) * 2 + (d[best] > 0)
    return int(d[best[np.argmin(key)]])


def search(x, n, hz, a, b, allowed=None, zero=False):
    """-> (delta [M] int, score [M]): the chain of decisions.  allowed: a mask over the candidates (the mutated searches of the tests);
    zero: every offset 0 (plain overlap-add)"""
    p = plan(hz, len(x), a, b)
    row = Row(x, n)
    delta, score = np.zeros(p["M"], np.int64), np.zeros(p["M"])
    if zero:
        return delta, score
    for m in range(1, p["M"]):
        s, _ = frame_scores(row, p["H"], a, b, m, int(delta[m - 1]))
        delta[m] = pick(s, p["delta"], allowed)
        score[m] = s[delta[m] + p["delta"]]
    return delta, score


def ola(x, n, hz, a, b, delta, w=None):
    """the overlap-add of the grains at `delta` under w (window32 by default) -> y [Ws] float64, 0 from the end of the stretched span,
    ceil(n a / b), on"""
    p = plan(hz, len(x), a, b)
    H = p["H"]
    w = window32(hz) if w is None else w
    row = Row(x, n)
    y = np.zeros(p["M"] * H)
    for m in range(p["M"] - 1):
        q0 = pos(m, H, a, b) + int(delta[m]) - H
        q1 = pos(m + 1, H, a, b) + int(delta[m + 1]) - H
        y[m * H:(m + 1) * H] = w[H:] * row.read(q0 + H, H) + w[:H] * row.read(q1, H)
    y[-(-row.n * a // b):] = 0.0
    return y[:p["Ws"]]


def stretch(x, n, hz, a, b, **kw):
    delta, score = search(x, n, hz, a, b, **kw)
    return ola(x, n, hz, a, b, delta), delta, score


def decision_gaps(x, n, hz, a, b, delta):
    """A table of offsets judged frame by frame without cascades: for every m >= 1 the float64 scores given the table's own d_{m-1} ->
    (gap [M], margin [M]): gap = max score - score(d_m), margin = 4 (N + 8) 2^-24 ||t||_2, the worst-case fp32 error of two N-term dot
    products and their normalisation (Cauchy-Schwarz bounds every score by ||t||_2).  A table passes where gap <= margin."""
    p = plan(hz, len(x), a, b)
    row = Row(x, n)
    gap, margin = np.zeros(p["M"]), np.zeros(p["M"])
    for m in range(1, p["M"]):
        s, tn = frame_scores(row, p["H"], a, b, m, int(delta[m - 1]))
        gap[m] = s.max() - s[int(delta[m]) + p["delta"]]
        margin[m] = 4.0 * (p["N"] + 8) * 2.0 ** -24 * tn
    return gap, margin


def judge(x, n, hz, a, b, delta):
    """decision_gaps and tie_frames in one pass over the frames, and what settles a decision outright -> dict: gap [M], margin [M] (as
    decision_gaps), ties (as tie_frames), lead [M] (the best float64 score minus the best of every other candidate's; 0 where two share
    the top) and pick [M] (the rule's d_m given the table's own d_{m-1}).  Every fp32 score is within margin of its float64 value, so
    where lead > 2 margin no rounding puts another candidate in front of the best and d_m must be pick."""
    p = plan(hz, len(x), a, b)
    row = Row(x, n)
    out = dict(gap=np.zeros(p["M"]), margin=np.zeros(p["M"]), lead=np.zeros(p["M"]), pick=np.zeros(p["M"], np.int64), ties=[])
    for m in range(1, p["M"]):
        s, tn = frame_scores(row, p["H"], a, b, m, int(delta[m - 1]))
        out["gap"][m] = s.max() - s[int(delta[m]) + p["delta"]]
        out["margin"][m] = 4.0 * (p["N"] + 8) * 2.0 ** -24 * tn
        top = np.partition(s, -2)[-2:]
        out["lead"][m] = top[1] - top[0]
        out["pick"][m] = pick(s, p["delta"])
        if not np.any(s != 0.0):
            out["ties"].append(m)
    return out


def tie_frames(x, n, hz, a, b, delta):
    """the frames m >= 1 whose target or whose every candidate is all zero given the table's own d_{m-1}: every score is 0 there and the
    rule pins d_m = 0"""
    p = plan(hz, len(x), a, b)
    row = Row(x, n)
    out = []
    for m in range(1, p["M"]):
        s, _ = frame_scores(row, p["H"], a, b, m, int(delta[m - 1]))
        if not np.any(s != 0.0):
            out.append(m)
    return out


# ---- the resample back --------------------------------------------------------------------------------------------------------------------------
def rate_scale(a, b):
    """k: the table of the way back is the resampler's design for a k -> b k Hz, the smallest k with min(a, b) k >= 8000"""
    return -(-8000 // min(a, b))


def resample(ys, taps, P, Q, n_out):
    """rational polyphase resampling in float64 with the float32 table taps [P][T]: output j sums taps[(j Q) % P][t] x[j Q // P - off + t],
    off = T / 2 - 1, zeros outside the row"""
    T = taps.shape[1]
    off = T // 2 - 1
    xp = np.concatenate((np.zeros(T), np.asarray(ys, np.float64), np.zeros(T + Q)))
    j = np.arange(n_out)
    first = j * Q // P - off + T
    idx = first[:, None] + np.arange(T)[None, :]
    return np.sum(taps.astype(np.float64)[(j * Q) % P] * xp[idx], axis=1)


def pitch(x, n, hz, a, b, taps):
    """the whole shift: the stretch by a / b, then the resample by b / a, first len(x) samples"""
    ys, delta, _ = stretch(x, n, hz, a, b)
    return resample(ys, taps, b, a, len(x)), delta


# ---- properties ---------------------------------------------------------------------------------------------------------------------------------
def envelope_db(y, hz, lo, hi):
    """per-10-ms RMS of y[lo:hi) in dB relative to the median block -> (min, max)"""
    blk = hz // 100
    seg = np.asarray(y, np.float64)[lo:hi]
    k = len(seg) // blk
    rms = np.sqrt(np.mean(seg[:k * blk].reshape(k, blk) ** 2, axis=1))
    db = 20.0 * np.log10(rms / np.median(rms))
    return float(db.min()), float(db.max())


def autocorr_f0(y, hz, lo, hi, f_lo=80.0, f_hi=600.0):
    """the fundamental by the autocorrelation peak of y[lo:hi) over lags of hz / f_hi .. hz / f_lo -> (f0 in Hz, the lag)"""
    seg = np.asarray(y, np.float64)[lo:hi]
    seg = seg - seg.mean()
    lags = np.arange(int(hz / f_hi), int(hz / f_lo) + 1)
    L = len(seg) - lags.max()
    r = np.array([seg[:L] @ seg[k:k + L] for k in lags])
    k = int(lags[np.argmax(r)])
    return hz / k, k

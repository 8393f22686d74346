"""The look-ahead peak limiter's contract (include/stn.h "limiter") in numpy: v, r and every comparison in
float32 exactly as specified, the weighted sum in float64."""
import math

import numpy as np

F32 = np.float32
BELOW_ONE = 1.0 - 2.0 ** -24  # the largest float32 below 1


def samples(hz, ms):
    return int(float(F32(ms)) * float(hz) / 1000.0 + 0.5)


def window(hz, ms):
    """float32 [A + 1]: 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), normalized to sum 1 in float64"""
    A = samples(hz, ms)
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(A + 1, dtype=np.float64) + 1.0) / (A + 2.0))
    return (h / h.sum()).astype(F32)


def ceiling(ceiling_db):
    return F32(10.0 ** (float(F32(ceiling_db)) / 20.0))


def s_tol(hz, ms):
    """|s - s_ref|: sequential summation of A + 1 non-negative terms of total weight <= 1, plus the weight, divide and final roundings"""
    return (samples(hz, ms) + 8) * 2.0 ** -24


def limit_row(x, n, g, ceiling_db, hz, ms):
    """x [W] float32, span n, gain g -> dict(y, s float64 [W]; v, r, M float32 [W]; limited; reduction_db)"""
    x = np.asarray(x, F32)
    W = x.size
    n = int(n)
    A = samples(hz, ms)
    c = ceiling(ceiling_db)
    w = window(hz, ms).astype(np.float64)
    v = (x * F32(g)).astype(F32)
    a = np.abs(v)
    r = np.ones(W, F32)
    over = a[:n] > c
    r[:n][over] = (c / a[:n][over]).astype(F32)
    rp = np.concatenate([np.ones(A, F32), r, np.ones(A, F32)])  # rp[j + A] = r[j], j in [-A, W + A)
    # m[j] = min r[j .. j + A] for j in [-A, W): me[j + A]
    me = np.lib.stride_tricks.sliding_window_view(rp, A + 1).min(axis=1)
    assert me.size == W + A
    M = np.minimum(me[:W], me[A:])  # min(m[i - A], m[i])
    tot = np.convolve(me.astype(np.float64), w, mode="valid")  # tot[i] = sum_k w[k] m[i - k]
    assert tot.size == W
    s = np.where(M == 1.0, 1.0, np.minimum(np.minimum(tot, r.astype(np.float64)), BELOW_ONE))
    vd = v.astype(np.float64)
    y = np.clip(vd, -float(c), float(c))
    y[:n] = np.clip(vd[:n] * s[:n], -float(c), float(c))
    s_out = s.copy()
    s_out[n:] = 1.0  # (the padding has no curve)
    lim = int(np.count_nonzero(M[:n] < 1.0))
    smin = float(s[:n].min()) if n else 1.0
    return dict(y=y, s=s_out, v=v, r=r, M=M, limited=lim, reduction_db=(-20.0 * math.log10(smin) if smin < 1.0 else 0.0), c=c, A=A)


def limit_rows(x, n, g, ceiling_db, hz, ms):
    x = np.atleast_2d(np.asarray(x, F32))
    n = [x.shape[1]] * x.shape[0] if n is None else n
    g = [1.0] * x.shape[0] if g is None else g
    return [limit_row(x[b], n[b], g[b], ceiling_db, hz, ms) for b in range(x.shape[0])]


SPANS = lambda A, W: [0, 1, A, A + 1, 2 * A + 1, 4096, 4097, 8191, 16385, W, 12345, W - 1]  # noqa: E731
GAINS = np.array([1.0, 0.5, 2.0, 1.5, 0.75, 3.0], F32)


def peaky_row(W, n, g, c, A, seed):
    """a low-level sine (all of W) plus, inside the span, peaks of 2-6 x the ceiling after the gain: at sample 0, at n - 1, two A apart,
    two 2A + 1 apart, an isolated one, a 3A-long plateau, and at every multiple of 1024 +- 1 up to 16384 (whatever the tile length, a
    boundary is hit); in the padding one over-level sample (it must come out clamped)"""
    rng = np.random.default_rng(seed)
    t = np.arange(W)
    x = (0.05 * np.sin(2 * np.pi * t / 97.3 + seed)).astype(np.float64) / float(g)
    def put(i, mult=None):
        if 0 <= i < n:
            x[i] = (rng.uniform(2.0, 6.0) if mult is None else mult) * float(c) / float(g) * (1 if rng.random() < 0.5 else -1)
    put(0)
    put(n - 1)
    b = 300
    put(b); put(b + A)
    b = 300 + 4 * A + 7
    put(b); put(b + 2 * A + 1)
    put(b + 6 * A + 11)
    b = 300 + 16 * A + 50
    for i in range(b, b + 3 * A):
        put(i, 3.0)
    for k in range(1024, 16384 + 1, 1024):
        put(k - 1)
        put(k + 1)
        if k % 4096 == 0:
            put(k)
    if n + 5 < W:
        x[n + 5] = 4.0 * float(c) / float(g)
    return x.astype(F32)


def peaky_rows(hz, ms, ceiling_db, W, rep):
    """the 6 rows of repeat `rep` (0 or 1): spans SPANS[6 rep : 6 rep + 6]"""
    A, c = samples(hz, ms), ceiling(ceiling_db)
    n = np.array(SPANS(A, W)[6 * rep:6 * rep + 6], np.int64)
    x = np.stack([peaky_row(W, int(n[b]), GAINS[b], c, A, 100 * rep + b) for b in range(6)])
    return x, n, GAINS.copy()


# ---- rows that scale with the look-ahead (the rates above 48 kHz: A up to 1920, where peaky_row's layout no longer fits 20011 samples) ---
TILE = 2048  # LM_TILE: samples per workgroup of the limiter kernel
LONG_CASES = ((192000, 10.0), (96000, 10.0), (88200, 5.0), (176400, 0.5))  # A = 1920 (the maximum), 960, 441, 88


def long_width(A):
    return max(20011, 20 * A + 4096)


def long_layout(A):
    """where peaky_row_long puts its peaks: an isolated one (2A + 1 clear samples each side and more), two A apart, two 2A + 1 apart, a
    3A-long plateau, then a clear stretch that holds a whole tile with its look-ahead on both sides, then peaks at the tile multiples
    +- 1 (and on every other multiple) up to the row's end"""
    W = long_width(A)
    clear = (12 * A + 1000, 14 * A + 5100)  # no peak in [clear[0], clear[1]): plateau end + A rounded up to a tile, + TILE + A, fits
    return dict(W=W, iso=2 * A + 600, pair=(4 * A + 700, 5 * A + 700), wide=(6 * A + 900, 8 * A + 901), plateau=(9 * A + 1000, 12 * A + 1000),
                clear=clear, bounds=[k for k in range(TILE, W, TILE) if k - 1 >= clear[1] and k + 1 < W])


def long_spans(A):
    """12 spans: the set of SPANS with the tile multiples +- 1 that mean something at this A: around the first boundary behind the
    plateau's start (the span cuts the plateau or ends in the clear stretch) and around the last boundary with peaks"""
    lay = long_layout(A)
    W = lay["W"]
    ka = (lay["plateau"][0] + TILE - 1) // TILE * TILE
    kb = lay["bounds"][-1]
    return [0, 1, A, A + 1, 2 * A + 1, ka - 1, ka + 1, kb - 1, kb + 1, W, lay["bounds"][0] + 1, W - 1]


def peaky_row_long(n, g, c, A, seed):
    """peaky_row at the width long_width(A), laid out by long_layout(A); peaks at sample 0 and n - 1, one over-level sample in the padding"""
    lay = long_layout(A)
    W = lay["W"]
    rng = np.random.default_rng(seed)
    x = (0.05 * np.sin(2 * np.pi * np.arange(W) / 97.3 + seed)).astype(np.float64) / float(g)

    def put(i, mult=None):
        if 0 <= i < n:
            x[i] = (rng.uniform(2.0, 6.0) if mult is None else mult) * float(c) / float(g) * (1 if rng.random() < 0.5 else -1)
    put(0)
    put(lay["iso"])
    for p in lay["pair"] + lay["wide"]:
        put(p)
    for i in range(*lay["plateau"]):
        put(i, 3.0)
    for k in lay["bounds"]:
        put(k - 1)
        put(k + 1)
        if k % (2 * TILE) == 0:
            put(k)
    if n - 1 < lay["clear"][0] or n - 1 >= lay["clear"][1]:  # (a span that ends in the clear stretch keeps it clear)
        put(n - 1)
    if n + 5 < W:
        x[n + 5] = 4.0 * float(c) / float(g)
    return x.astype(F32)


_LONG = {}


def long_case(hz, ms, ceiling_db, rep):
    """(x [6, W], n, g, outs) of repeat rep (0 or 1) at the width long_width(A), computed once per process and read-only: the rows, their
    spans long_spans(A)[6 rep : 6 rep + 6], GAINS and the reference's results.  A row whose span is the whole row or one short of it
    must hold a tile the reference leaves untouched (M == 1 over the tile: r == 1 over the tile and A samples each side, the kernel's
    early exit) and a tile it limits in."""
    key = (hz, float(ms), float(ceiling_db), rep)
    if key not in _LONG:
        A, c = samples(hz, ms), ceiling(ceiling_db)
        W = long_width(A)
        n = np.array(long_spans(A)[6 * rep:6 * rep + 6], np.int64)
        x = np.stack([peaky_row_long(int(n[b]), GAINS[b], c, A, 1000 + 100 * rep + b) for b in range(6)])
        g = GAINS.copy()
        outs = limit_rows(x, n, g, ceiling_db, hz, ms)
        for b, o in enumerate(outs):
            if n[b] >= W - 1:
                whole = o["M"][:W // TILE * TILE].reshape(-1, TILE)
                assert np.any(np.all(whole == 1.0, axis=1)) and np.any(np.any(whole < 1.0, axis=1)), (hz, ms, b)
        for a in (x, n, g):
            a.setflags(write=False)
        _LONG[key] = (x, n, g, outs)
    return _LONG[key]
